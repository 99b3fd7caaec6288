"""GPU tests of lsm_lz4_compress_blocks (Block::write_into with CompressionType::Lz4,
src/table/block/mod.rs:60-74).  The stream's bytes are pinned by no reference test
(any valid LZ4 block reads back), so what is asserted is: the stream is a conforming
LZ4 block (tests/lz4_check.py), it decodes to the payload under three independent
decoders (the oracle's, liblz4 through pyarrow, the GPU decompressor), the header
around it is byte-exact (pyoracle.block_header), the stream is a pure function of
the payload, and its size stays close to liblz4's on the same payloads.

Ratio bound (test_ratio_against_liblz4): over the corpus members of >= 1 KiB the
total stored bytes are <= 1.05 x liblz4's total and each block is <= 1.10 x
liblz4's size for it.  Reference: liblz4 (pyarrow "lz4_raw"), not the code under test."""
import ctypes as C

import numpy as np
import pytest

import pyoracle
from helpers import random_sorted_items
from lz4_cases import lz4_compress
from lz4_check import lz4_check
from lz4_compress_corpus import corpus, frame, json_block, json_items, json_rows

pytestmark = pytest.mark.gpu

OK, BAD_MAGIC, PARSE, OVERFLOW, TRUNCATED, UNSUPPORTED = 0, 1, 5, 6, 8, 9
FIELDS = (("seqno", np.uint64), ("key_off", np.uint32), ("val_off", np.uint32), ("val_len", np.uint32),
          ("key_len", np.uint16), ("prefix_len", np.uint16), ("vtype", np.uint8))


def _offsets(blocks):
    off = np.zeros(len(blocks) + 1, np.int64)
    off[1:] = np.cumsum([len(b) for b in blocks])
    return off


def _compress(gpu, blocks, in_status=None, out_cap=None, fill=None):
    """blocks: framed uncompressed blocks -> (list of output blocks, statuses, offsets, whole buffer)."""
    import torch
    off = _offsets(blocks)
    buf = gpu.to_device_bytes(np.frombuffer(b"".join(blocks), np.uint8))
    st_in = None if in_status is None else torch.tensor(in_status, dtype=torch.int32).cuda()
    if fill is None:
        res = gpu.lz4_compress_blocks(buf, torch.from_numpy(off).cuda(), in_status=st_in, out_cap=out_cap)
        out = res["buf"]
    else:  # a caller-owned output buffer, pre-filled, with the library told only out_cap of it
        n = len(blocks)
        out = torch.full((fill[0],), fill[1], dtype=torch.uint8, device="cuda")
        d_off = torch.from_numpy(off).cuda()
        res = {"block_off": torch.zeros(n + 1, dtype=torch.int64, device="cuda"),
               "status": torch.empty(n, dtype=torch.int32, device="cuda")}
        nbytes = buf.numel()
        ws = torch.empty(gpu.lib().lsm_lz4_compress_workspace_size(n, nbytes), dtype=torch.uint8, device="cuda")
        rc = gpu.lib().lsm_lz4_compress_blocks(buf.data_ptr(), d_off.data_ptr(), n, None, out.data_ptr(), out_cap,
                                               res["block_off"].data_ptr(), res["status"].data_ptr(), ws.data_ptr(),
                                               ws.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
    torch.cuda.synchronize()
    o = out.cpu().numpy().tobytes()
    oo = res["block_off"].cpu().numpy()
    st = res["status"].cpu().numpy().tolist()
    got = [o[oo[i]:oo[i + 1]] if st[i] == OK else b"" for i in range(len(blocks))]
    return got, st, oo, o


def _check_block(name, payload, out_block):
    """Test 1's checks of one output block against its payload."""
    stored = out_block[33:]
    raw_len = len(payload)
    assert out_block[:33] == pyoracle.block_header(0, stored, raw_len), name
    assert lz4_check(stored, raw_len) == payload, name
    assert pyoracle.lz4_decompress(stored, raw_len) == payload, name
    import pyarrow as pa
    if raw_len:  # (pyarrow refuses a zero-size destination)
        assert pa.Codec("lz4_raw").decompress(stored, decompressed_size=raw_len, asbytes=True) == payload, name
    assert len(stored) <= raw_len + raw_len // 255 + 16, name


def _check_batch(names, payloads, got, st, oo):
    assert st == [OK] * len(payloads)
    assert oo[0] == 0 and list(np.diff(oo)) == [len(g) for g in got]  # contiguous from 0
    for name, p, g in zip(names, payloads, got):
        _check_block(name, p, g)


@pytest.fixture(scope="module")
def clean(gpu):
    """The corpus compressed once, in one batch, shared by the tests below."""
    names = [n for n, _ in corpus()]
    payloads = [p for _, p in corpus()]
    got, st, oo, _ = _compress(gpu, [frame(p) for p in payloads])
    return names, payloads, got, st, oo


def test_round_trip_corpus(clean):
    names, payloads, got, st, oo = clean
    sizes = sorted(len(p) for p in payloads)
    assert sizes[0] == 0 and any(5120 < s <= 65536 for s in sizes) and sizes[-1] > 65536  # every size class
    _check_batch(names, payloads, got, st, oo)
    assert got[names.index("pattern0")][33:] == b"\x00"


def test_gpu_chain_decodes_the_compressed_batch(gpu, clean):
    import torch
    names, payloads, got, st, oo = clean
    idx = [i for i, n in enumerate(names) if n.startswith(("counter", "random_sorted", "prefix", "json"))]
    comp = [got[i] for i in idx]
    plain = [frame(payloads[i]) for i in idx]
    out = gpu.decode_lz4_blocks(gpu.to_device_bytes(np.frombuffer(b"".join(comp), np.uint8)),
                                torch.from_numpy(_offsets(comp)).cuda(), expect_type=0)
    torch.cuda.synchronize()
    nb = len(idx)
    assert out["status"][:nb].cpu().tolist() == [OK] * nb
    parsed, item_start, status = pyoracle.decode_blocks(np.frombuffer(b"".join(plain), np.uint8),
                                                        _offsets(plain).astype(np.uint64), nthreads=2)
    assert (status == 0).all()
    n = int(item_start[-1])
    assert out["item_start"].cpu().numpy().tolist() == item_start.tolist()
    for f, dt in FIELDS:
        assert (out[f].cpu().numpy().view(dt)[:n] == parsed[f].astype(dt)[:n]).all(), f


def test_ratio_against_liblz4(clean):
    names, payloads, got, st, oo = clean
    total = ref_total = 0
    for name, p, g in zip(names, payloads, got):
        if len(p) < 1024:
            continue
        mine, ref = len(g) - 33, len(lz4_compress(p))
        print(f"{name}: raw {len(p)} stored {mine} liblz4 {ref} ratio {mine / ref:.4f}")
        total += mine
        ref_total += ref
        assert mine <= 1.10 * ref, name
    print(f"total: stored {total} liblz4 {ref_total} ratio {total / ref_total:.4f}")
    assert total <= 1.05 * ref_total


def test_far_offsets(gpu):
    rng = np.random.default_rng(5)
    body = rng.integers(0, 256, 70000, dtype=np.uint8).tobytes()
    beyond = body + body[:2000]                  # the only repeat lies 70,000 back: no match may use it
    exact = body[:65535] + body[:2000]           # the copy lies exactly 65,535 back
    # The same with a run of zeros in between: the run is one long match, whose inner positions
    # are not inserted, so the first copy's table entries are still there when the second copy
    # arrives and only the offset limit decides.  2000 random bytes do not compress: the second
    # copy costs ~2000 bytes as literals and a few bytes as a match.
    a = body[:2000]
    run_beyond = a + bytes(68000) + a            # 70,000 back: must stay literals
    run_exact = a + bytes(65535 - 2000) + a      # exactly 65,535 back: the longest offset there is
    names = ["beyond_window", "exactly_65535", "run_beyond_window", "run_exactly_65535"]
    payloads = [beyond, exact, run_beyond, run_exact]
    got, st, oo, _ = _compress(gpu, [frame(p) for p in payloads])
    _check_batch(names, payloads, got, st, oo)  # (lz4_check enforces the offset limit)
    assert len(got[2]) - 33 >= 4000
    assert len(got[3]) - 33 < 2600


def test_position_independence_reversed(gpu, clean):
    names, payloads, got, st, oo = clean
    rgot, rst, roo, _ = _compress(gpu, [frame(p) for p in reversed(payloads)])
    assert rst == [OK] * len(payloads)
    assert list(reversed(rgot)) == got


def test_position_independence_interleaved(gpu):
    kinds = [json_block(52), pyoracle.data_block_encode(random_sorted_items(52, seed=3), restart_interval=4),
             np.random.default_rng(2).integers(0, 256, 4000, dtype=np.uint8).tobytes()]
    assert all(len(k) <= 5120 for k in kinds)
    payloads = [kinds[i % 3] for i in range(203)]  # 203 = 50 workgroups of four waves and a partial one
    got, st, oo, _ = _compress(gpu, [frame(p) for p in payloads])
    assert st == [OK] * 203
    for i in range(3):
        _check_block(f"kind{i}", kinds[i], got[i])
    assert all(got[i] == got[i % 3] for i in range(203))


def test_many_small_blocks(gpu):
    payloads = [pyoracle.data_block_encode(random_sorted_items(52, seed=s), restart_interval=ri)
                for s, ri in enumerate([1, 2, 4, 8, 16] * 40 + [1, 2, 4])]
    assert len(payloads) == 203
    got, st, oo, _ = _compress(gpu, [frame(p) for p in payloads])
    _check_batch([f"small{i}" for i in range(203)], payloads, got, st, oo)


def test_statuses(gpu, clean):
    names, payloads, got, st, oo = clean
    pick = [names.index(n) for n in ("counter52", "json52", "json205", "random5000", "zeros9000", "fox", "pattern13",
                                     "json1300")]
    base = [frame(payloads[i]) for i in pick]
    want = [got[i] for i in pick]
    bad_magic = bytearray(base[1])
    bad_magic[0] ^= 1
    short = base[2][:20]
    off_by_one = bytearray(base[3])
    off_by_one[21:25] = (len(payloads[pick[3]]) + 1).to_bytes(4, "little")
    stored = lz4_compress(payloads[pick[4]])
    compressed = pyoracle.block_header(0, stored, len(payloads[pick[4]])) + stored
    blocks = [base[0], bytes(bad_magic), short, bytes(off_by_one), compressed, base[5], base[6], base[7]]
    in_status = [OK] * 8
    in_status[5] = PARSE
    g, s, o, _ = _compress(gpu, blocks, in_status=in_status)
    assert s == [OK, BAD_MAGIC, TRUNCATED, TRUNCATED, UNSUPPORTED, PARSE, OK, OK]
    sizes = list(np.diff(o))
    for i in range(1, 6):
        assert sizes[i] == 0, i
    for i in (0, 6, 7):
        assert g[i] == want[i] and sizes[i] == len(want[i]), i  # byte-identical to the clean batch's
    assert o[0] == 0 and o[-1] == sum(len(want[i]) for i in (0, 6, 7))


def test_out_cap_overflow(gpu, clean):
    names, payloads, got, st, oo = clean
    pick = [names.index(n) for n in ("json52", "counter52", "json205", "fox", "random5000")]
    blocks = [frame(payloads[i]) for i in pick]
    want = [got[i] for i in pick]
    ends = np.cumsum([len(w) for w in want])
    k = 2
    cap = int(ends[k]) - 7  # cuts block k in the middle
    size = int(ends[-1]) + 64
    g, s, o, raw = _compress(gpu, blocks, out_cap=cap, fill=(size, 0xA5))
    assert s == [OK] * k + [OVERFLOW] * (len(blocks) - k)
    assert list(o) == [0] + list(ends)  # the real offsets
    assert raw[:int(ends[k - 1])] == b"".join(want[:k])
    assert raw[int(ends[k - 1]):] == b"\xa5" * (size - int(ends[k - 1]))  # no byte of an overflowing block written


def test_workspace_sized_for_fewer_bytes(gpu, clean):
    """The call cannot see the input's size (it is in no argument), so a workspace sized for
    fewer bytes than the offsets span is caught per block: a block whose slot does not fit gets
    LSM_BAD_ARG and 0 bytes, the others are written as usual, nothing past the workspace changes."""
    import torch
    names, payloads, got, st, oo = clean
    i = names.index("json52")
    n, blk = 4, frame(payloads[i])
    off = torch.from_numpy(_offsets([blk] * n)).cuda()
    buf = gpu.to_device_bytes(np.frombuffer(blk * n, np.uint8))
    lib = gpu.lib()
    small = lib.lsm_lz4_compress_workspace_size(n, 2 * len(blk))  # room for two of the four
    assert small < lib.lsm_lz4_compress_workspace_size(n, n * len(blk))
    arena = torch.full((small + 65536,), 0xA5, dtype=torch.uint8, device="cuda")
    cap = int(lib.lsm_lz4_compress_bound(n * len(blk), n))
    out = gpu.padded_bytes(cap)
    out_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    status = torch.empty(n, dtype=torch.int32, device="cuda")
    rc = lib.lsm_lz4_compress_blocks(buf.data_ptr(), off.data_ptr(), n, None, out.data_ptr(), cap, out_off.data_ptr(),
                                     status.data_ptr(), arena.data_ptr(), small,
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [OK, OK, 10, 10]
    o = out_off.cpu().numpy()
    assert list(np.diff(o)) == [len(got[i]), len(got[i]), 0, 0]
    raw = out.cpu().numpy().tobytes()
    assert raw[:o[1]] == got[i] and raw[o[1]:o[2]] == got[i]
    assert bool((arena[small:] == 0xA5).all().item())


@pytest.mark.parametrize("two_level", [False, True], ids=["full", "two_level"])
def test_write_table_lz4(gpu, oracle, two_level):
    import torch
    import test_gpu_merge_pipeline as P
    items = json_items(600)
    kw = {"block_size": 1024, "two_level": two_level}
    if two_level:
        kw["partition_size"] = 256
    d = gpu.items_to_device(items)
    t = gpu.write_table(d, compression="lz4", **kw)
    assert t["compression"] == "lz4"
    nb = t["block_count"]
    boff = t["block_off"].cpu().numpy()
    assert nb > 30 and boff[0] == 0 and boff[nb] == t["data_len"] == t["index_off"] and (np.diff(boff) > 33).all()
    file = t["file"]
    # the index: TLI, and the partitions it points at when two-level
    fbytes = file.cpu().numpy()

    def index_handles(lo, hi):
        blk = gpu.to_device_bytes(fbytes[lo:hi])
        out = gpu.decode_blocks(blk, torch.tensor([0, hi - lo], dtype=torch.int64).cuda(), expect_type=1)
        torch.cuda.synchronize()
        assert out["status"].cpu().tolist()[:1] == [OK]
        n = int(out["item_start"][1].item())
        return out["handle_off"].cpu().numpy()[:n].tolist(), out["val_len"].cpu().numpy()[:n].tolist()

    h_off, h_size = index_handles(t["tli_off"], t["tli_off"] + t["tli_size"])
    if two_level:
        assert len(h_off) > 1 and h_off[0] == t["index_off"] and h_off[-1] + h_size[-1] == t["tli_off"]
        parts = [index_handles(o, o + s) for o, s in zip(h_off, h_size)]
        h_off = sum((p[0] for p in parts), [])
        h_size = sum((p[1] for p in parts), [])
    assert h_off == boff[:nb].tolist() and h_size == np.diff(boff[:nb + 1]).tolist()
    # the data region through the LZ4 read path
    out = gpu.decode_lz4_blocks(file, t["block_off"], nb, expect_type=0)
    assert out["status"][:nb].cpu().tolist() == [OK] * nb
    keys, key_off = gpu.materialize_keys(out["frames"], out["frame_off"], nb, out)
    part = gpu.decoded_to_items(out["frames"], out["frame_off"], nb, out, keys, key_off)
    kt, vt = int(part["key_off"][-1]), int(part["val_off"][-1])
    assert P._rows_of(dict(part, keys=part["keys"][:kt], vals=part["vals"][:vt])) == json_rows(600)
    # compression=None is what it was: the oracle's file
    ref = oracle.table_write(items, **kw)
    plain = gpu.write_table(d, compression=None, **kw)
    assert plain["compression"] is None
    assert plain["file"].cpu().numpy().tobytes() == bytes(ref["file"])
    assert (plain["tli_off"], plain["tli_size"]) == (ref["tli_off"], ref["tli_size"])


def test_graph_replay(gpu):
    """One call captured on one stream (a linear graph), replayed over two different batches
    copied into the same input buffers."""
    import torch
    from merge_gpu import capture
    batch_a = [json_block(52), bytes(3000), json_block(205), b"the quick brown fox " * 150, json_block(1300)]
    rng = np.random.default_rng(8)
    other = pyoracle.data_block_encode(random_sorted_items(820, seed=6), restart_interval=8) * 3
    batch_b = [rng.integers(0, 256, len(p), dtype=np.uint8).tobytes() if i % 2 else other[i:i + len(p)]
               for i, p in enumerate(batch_a)]
    assert [len(p) for p in batch_a] == [len(p) for p in batch_b]  # the same offsets: only the bytes change
    frames_a, frames_b = [frame(p) for p in batch_a], [frame(p) for p in batch_b]
    n = len(batch_a)
    off = _offsets(frames_a)
    d_in = gpu.to_device_bytes(np.frombuffer(b"".join(frames_a), np.uint8))
    d_off = torch.from_numpy(off).cuda()
    nbytes = d_in.numel()
    cap = int(gpu.lib().lsm_lz4_compress_bound(nbytes, n))
    d_out = gpu.padded_bytes(cap)
    d_out_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_st = torch.empty(n, dtype=torch.int32, device="cuda")
    ws = torch.empty(gpu.lib().lsm_lz4_compress_workspace_size(n, nbytes), dtype=torch.uint8, device="cuda")

    def call():
        rc = gpu.lib().lsm_lz4_compress_blocks(d_in.data_ptr(), d_off.data_ptr(), n, None, d_out.data_ptr(), cap,
                                               d_out_off.data_ptr(), d_st.data_ptr(), ws.data_ptr(), ws.numel(),
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0

    g = capture(call)
    for tag, payloads, frames in (("b", batch_b, frames_b), ("a", batch_a, frames_a)):
        src = torch.from_numpy(np.frombuffer(b"".join(frames), np.uint8).copy()).cuda()
        d_in[:src.numel()].copy_(src)
        d_out.fill_(0x5A)
        d_out_off.zero_()
        d_st.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        o, oo = d_out.cpu().numpy().tobytes(), d_out_off.cpu().numpy()
        got = [o[oo[i]:oo[i + 1]] for i in range(n)]
        _check_batch([f"{tag}{i}" for i in range(n)], payloads, got, d_st.cpu().tolist(), oo)
