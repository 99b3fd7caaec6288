"""lsm_materialize_items_plan / lsm_materialize_items: decoded blocks -> merge-ready item runs
(DataBlockParsedItem::materialize producing the owned key and value, data_block/mod.rs:296-315,
as Scanner::next yields it into Merger::new).  Expected rows come from pyoracle.materialize or
from the rows written, never from the code under test; decoded_to_items (torch ops) is a
second, independent path for the value arena and for the merge."""
import ctypes as C

import numpy as np
import pytest

import merge_model as M
import test_gpu_materialize as TM
import test_gpu_merge_pipeline as P
from helpers import pack
from lz4_cases import lz4_compress
from merge_gpu import capture

pytestmark = pytest.mark.gpu

CANARY = 0xA5
WORD = int.from_bytes(bytes([CANARY]) * 8, "little", signed=True)
OK, OVERFLOW = 0, 6
GATHER_BUF = 8192  # kGatherBuf (csrc/gather.hpp): a span of more bytes, alignment pad included, never goes through LDS
MI_BUF = 4096      # kMiBuf (csrc/materialize_items.hip): a span of at most that many goes through LDS at once
FIELDS = ("keys", "key_off", "vals", "val_off", "seqno", "vtype")


def _read_rows(items, r0, r1):
    """Rows [r0, r1) of a device lsm_items dict -> [(key, value, seqno, vtype)]; only those
    rows' bytes are downloaded.  Offsets must not decrease."""
    ko = items["key_off"][r0:r1 + 1].cpu().numpy()
    vo = items["val_off"][r0:r1 + 1].cpu().numpy()
    assert (np.diff(ko) >= 0).all() and (np.diff(vo) >= 0).all()
    keys = items["keys"][int(ko[0]):int(ko[-1])].cpu().numpy().tobytes()
    vals = items["vals"][int(vo[0]):int(vo[-1])].cpu().numpy().tobytes()
    seq = items["seqno"][r0:r1].cpu().numpy().view(np.uint64)
    vt = items["vtype"][r0:r1].cpu().numpy()
    ko, vo = ko - ko[0], vo - vo[0]
    return [(keys[ko[i]:ko[i + 1]], vals[vo[i]:vo[i + 1]], int(seq[i]), int(vt[i])) for i in range(r1 - r0)]


def _canary_dst(gpu, n, key_cap, val_cap):
    """Caller-owned outputs for n items, every byte CANARY."""
    import torch

    def full(nbytes):
        return torch.full((nbytes,), CANARY, dtype=torch.uint8, device="cuda")

    return {"keys": full(key_cap + gpu.LSM_INPUT_PADDING), "vals": full(val_cap + gpu.LSM_INPUT_PADDING),
            "key_off": full(8 * (n + 1)).view(torch.int64), "val_off": full(8 * (n + 1)).view(torch.int64),
            "seqno": full(8 * max(n, 1)).view(torch.int64), "vtype": full(max(n, 1))}


def _untouched(dst, fields=FIELDS):
    return all(bool((dst[f] == (CANARY if dst[f].element_size() == 1 else WORD)).all().item()) for f in fields)


def _decode(gpu, blocks):
    import torch
    buf, off = pack(blocks)
    d_blocks = gpu.to_device_bytes(buf)
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    return d_blocks, d_off, gpu.decode_blocks(d_blocks, d_off, len(blocks)), buf, off


def _shape_blocks(oracle):
    blocks = TM._blocks(oracle)
    bad = bytearray(blocks[2])
    bad[50] ^= 0x10  # payload bit flip: checksum mismatch
    blocks[2] = bytes(bad)
    return blocks


def _totals(rows):
    return [len(rows), sum(len(r[0]) for r in rows), sum(len(r[1]) for r in rows)]


# ------------------------------------------------------------------ 1. block shapes
def test_block_shapes_match_oracle(gpu, oracle):
    import torch
    blocks = _shape_blocks(oracle)
    n = len(blocks)
    d_blocks, d_off, out, buf, off = _decode(gpu, blocks)
    items = gpu.materialize_items(d_blocks, d_off, n, out)
    torch.cuda.synchronize()
    st = out["status"].cpu().numpy()[:n]
    assert st[2] == 4 and (np.delete(st, 2) == 0).all()
    item_start = out["item_start"].cpu().numpy().view(np.uint32)
    R = int(item_start[n])
    want = []
    for b in range(n):
        lo, hi = int(item_start[b]), int(item_start[b + 1])
        if st[b] != 0 or b == n - 1:  # the corrupt block and the index block: empty rows
            want += [(b"", b"", 0, 0)] * (hi - lo)
            continue
        payload = bytes(buf[int(off[b]) + 33:int(off[b + 1])])
        cnt, parsed = oracle.data_block_decode(payload)
        assert cnt == hi - lo
        want += oracle.materialize(payload, parsed, payload[-31])
    assert len(want) == R and sum(1 for w in want if w == (b"", b"", 0, 0)) >= 40
    assert items["result"].item() == OK and items["plan_result"].item() == OK
    assert items["end"].cpu().tolist() == _totals(want)
    assert items["seqno"].numel() == R and items["key_off"].numel() == items["val_off"].numel() == R + 1
    assert int(items["key_off"][0]) == 0 and int(items["val_off"][0]) == 0
    assert [int(items["key_off"][R]), int(items["val_off"][R])] == items["end"].cpu().tolist()[1:]
    assert _read_rows(items, 0, R) == want


# ------------------------------------------------------- 2. length and boundary edges
EDGE_VALUE_LENGTHS = (0, 1, 15, 16, 17, 127, 128, 255, 256, 257, 4000)
EDGE_BLOCKS = ((1, 16), (2, 16), (3, 2), (63, 16), (64, 1), (65, 5), (129, 3), (200, 16),  # boundaries inside tiles
               (len(EDGE_VALUE_LENGTHS), 16), (1, 16), (5000, 64), (300, 16))   # (rows, restart interval)
EDGE_TILE_SPANS = (GATHER_BUF - 1, GATHER_BUF, GATHER_BUF + 1, MI_BUF - 1, MI_BUF, MI_BUF + 1)


def _edge_rows():
    """Rows 0 .. 383 are six tiles whose value spans, alignment pad included, are
    EDGE_TILE_SPANS bytes (values of < 256 bytes, so the size alone decides between the LDS
    and the direct path; the halves of the first three lie around kMiBuf as well); then short
    random rows up to the end of the 200-row block, the edge value lengths, one 70 000-byte
    value alone in its block, a block of 5000 rows, and keys of 1 .. 300 bytes that share up
    to 288 bytes with their restart head."""
    rng = np.random.default_rng(20)
    rows = []

    def add(vlen, vt=0, key=None):
        i = len(rows)
        v = b"" if vt else rng.integers(0, 256, vlen, dtype=np.uint8).tobytes()
        rows.append((key if key is not None else b"k%07d" % i, v, 3 * i + 1, vt))

    for last in (127, 113, 129):
        for vlen in [128] * 63 + [last]:
            add(vlen)
    for last in (62, 49, 65):
        for vlen in [64] * 63 + [last]:
            add(vlen)
    while len(rows) < 1 + 2 + 3 + 63 + 64 + 65 + 129 + 200:
        vt = int(rng.choice((0, 0, 0, 1, 2, 4)))
        add(int(rng.integers(0, 91)), vt)
    for vlen in EDGE_VALUE_LENGTHS:
        add(vlen)
    add(70000)
    for j in range(5000):
        add(3, 1 if j % 11 == 0 else 0)
    for j in range(1, 301):
        add(j % 5, key=b"q" * j)
    assert len(rows) == sum(c for c, _ in EDGE_BLOCKS)
    return rows


def test_length_and_boundary_edges(gpu, oracle):
    import torch
    rows = _edge_rows()
    its = oracle.Items.from_list(rows)
    blocks, first = [], 0
    for count, ri in EDGE_BLOCKS:
        blocks.append(oracle.block_write(oracle.data_block_encode(its, first, count, restart_interval=ri)))
        first += count
    n = len(blocks)
    d_blocks, d_off, out, _, _ = _decode(gpu, blocks)
    items = gpu.materialize_items(d_blocks, d_off, n, out)
    torch.cuda.synchronize()
    assert (out["status"][:n] == 0).all().item()
    assert items["result"].item() == OK and items["end"].cpu().tolist() == _totals(rows)
    # the six tiles are what the docstring says, for the arena this call wrote
    assert items["vals"].data_ptr() % 16 == 0
    vo = items["val_off"].cpu().numpy()
    for t, span in enumerate(EDGE_TILE_SPANS):
        assert int(vo[64 * t + 64] - vo[64 * t]) + int(vo[64 * t]) % 16 == span
    assert _read_rows(items, 0, len(rows)) == rows
    keys, key_off = gpu.materialize_keys(d_blocks, d_off, n, out)
    ref = gpu.decoded_to_items(d_blocks, d_off, n, out, keys, key_off)
    vt = int(ref["val_off"][-1])
    assert torch.equal(items["val_off"], ref["val_off"]) and torch.equal(items["vals"][:vt], ref["vals"][:vt])
    kt = int(key_off[-1])
    assert torch.equal(items["key_off"], key_off) and torch.equal(items["keys"][:kt], keys[:kt])


# ------------------------------------------------------------------------ 3. append
def _three_tables():
    """[(rows, global seqno)], table_write arguments, gc threshold: table 0 has odd key and value
    totals (the next base is unaligned), table 1 a global seqno that wraps, table 2 a two-level
    index."""
    tables, _, thr = P._tables("wrapped_seqnos")
    rows0, g0 = tables[0]
    _, kt, vt = _totals(rows0)
    rows0 = rows0 + [(b"~" * (1 if kt % 2 == 0 else 2), b"x" * (1 if vt % 2 == 0 else 2), 1000, 0)]
    assert _totals(rows0)[1] % 2 == 1 and _totals(rows0)[2] % 2 == 1 and M.run_is_sorted(rows0)
    assert tables[1][1] > 2 ** 63
    kws = [{"block_size": 1024}, {"block_size": 1024}, {"block_size": 1024, "two_level": True, "partition_size": 256}]
    return [(rows0, g0), tables[1], tables[2]], kws, thr


def _scan_out(gpu, oracle, rows, g, kw):
    t = oracle.table_write(oracle.Items.from_list(rows), **kw)
    d_file = gpu.to_device_bytes(t["file"])
    out = gpu.scan_table(d_file, len(t["file"]), t["tli_off"], t["tli_size"], two_level=kw.get("two_level", False),
                         global_seqno=g, block_count=t["block_count"])
    assert out["table_status"] == 0 and out["n_blocks"] == t["block_count"] > 3
    return d_file, out, t


def _merged(gpu, items, run_start, thr):
    """merge_runs -> everything defined of its output, as host values."""
    import torch
    out = gpu.merge_runs(items, run_start, thr, evict_tombstones=True)
    torch.cuda.synchronize()
    n_out = int(out["n_out"].cpu()[0])
    ko, vo = out["key_off"][:n_out + 1].cpu().numpy(), out["val_off"][:n_out + 1].cpu().numpy()
    part = {"keys": out["keys"], "key_off": out["key_off"], "vals": out["vals"], "val_off": out["val_off"],
            "seqno": out["seqno"], "vtype": out["vtype"]}
    return (n_out, out["status"].cpu().tolist(), out["src"].cpu().numpy()[:n_out].tolist(), ko.tolist(), vo.tolist(),
            _read_rows(part, 0, n_out))


def test_append_tables_and_merge(gpu, oracle):
    import torch
    tables, kws, thr = _three_tables()
    want_parts = [P._shifted(rows, g) for rows, g in tables]
    scans = [_scan_out(gpu, oracle, rows, g, kw) for (rows, g), kw in zip(tables, kws)]
    N, KT, VT = (sum(_totals(w)[k] for w in want_parts) for k in range(3))
    dst = _canary_dst(gpu, N, KT, VT)
    cursor = torch.zeros((4, 3), dtype=torch.int64, device="cuda")
    for t, (d_file, out, _) in enumerate(scans):
        before = {f: dst[f].clone() for f in ("keys", "vals", "seqno", "vtype")}
        r = gpu.materialize_items(d_file, out["block_off"], out["n_blocks"], out, base=cursor[t], into=dst,
                                  caps=(N, KT, VT), end=cursor[t + 1])
        torch.cuda.synchronize()
        assert r["result"].item() == OK and r["plan_result"].item() == OK
        b, e = cursor[t].cpu().tolist(), cursor[t + 1].cpu().tolist()
        assert e == [x + y for x, y in zip(b, _totals(want_parts[t]))]
        for f, k in (("keys", 1), ("vals", 2), ("seqno", 0), ("vtype", 0)):  # nothing outside [base, end)
            assert torch.equal(dst[f][:b[k]], before[f][:b[k]]), (t, f)
            assert (dst[f][e[k]:] == (WORD if f == "seqno" else CANARY)).all().item(), (t, f)
        assert _read_rows(dst, b[0], e[0]) == want_parts[t]
    c = cursor.cpu().tolist()
    assert c[1][1] % 2 == 1 and c[1][2] % 2 == 1  # table 1 was appended at an unaligned base
    assert c[3] == [N, KT, VT]
    run_start = cursor[:, 0].contiguous()
    assert run_start.cpu().tolist() == [0] + list(np.cumsum([len(w) for w in want_parts]))
    assert _read_rows(dst, 0, N) == [r for w in want_parts for r in w]

    # the same through tables_to_runs
    items2, rs2 = gpu.tables_to_runs([(d_file, out["block_off"], out["n_blocks"], out) for d_file, out, _ in scans])
    torch.cuda.synchronize()
    assert items2["result"].cpu().tolist() == [OK] * 3 and torch.equal(rs2, run_start)
    for f, size in (("keys", KT), ("vals", VT), ("key_off", N + 1), ("val_off", N + 1), ("seqno", N), ("vtype", N)):
        assert items2[f].numel() == (size + gpu.LSM_INPUT_PADDING if f in ("keys", "vals") else size)
        assert torch.equal(items2[f][:size], dst[f][:size]), f

    # merge: the model, and the torch path (materialize_keys + decoded_to_items + torch.cat) bit for bit
    want, want_src, dropped = M.merge_runs(want_parts, thr, True, False)
    assert dropped and len(want) > 300
    got = _merged(gpu, {f: dst[f] for f in FIELDS}, run_start, thr)
    assert got[0] == len(want) and got[1] == [0, 0, 0] and got[2] == want_src and got[5] == want
    parts = []
    for d_file, out, _ in scans:
        keys, key_off = gpu.materialize_keys(d_file, out["block_off"], out["n_blocks"], out)
        parts.append(gpu.decoded_to_items(d_file, out["block_off"], out["n_blocks"], out, keys, key_off))
    ref_items, ref_rs = P._concat(gpu, parts)
    assert _merged(gpu, ref_items, ref_rs, thr) == got


# -------------------------------------------------------------------------- 4. caps
def test_caps_all_or_nothing(gpu, oracle):
    import torch
    blocks = _shape_blocks(oracle)
    n = len(blocks)
    d_blocks, d_off, out, _, _ = _decode(gpu, blocks)
    ref = gpu.materialize_items(d_blocks, d_off, n, out)
    torch.cuda.synchronize()
    totals = ref["end"].cpu().tolist()
    R, kt, vt = totals
    assert R > 1000 and kt > 0 and vt > 0
    sizes = {"keys": kt, "vals": vt, "key_off": R + 1, "val_off": R + 1, "seqno": R, "vtype": R}

    dst = _canary_dst(gpu, R, kt, vt)
    r = gpu.materialize_items(d_blocks, d_off, n, out, into=dst, caps=(R, kt, vt))
    torch.cuda.synchronize()
    assert r["result"].item() == OK and r["plan_result"].item() == OK and r["end"].cpu().tolist() == totals
    for f in FIELDS:
        assert torch.equal(dst[f][:sizes[f]], ref[f][:sizes[f]]), f
    assert (dst["keys"][kt:] == CANARY).all().item() and (dst["vals"][vt:] == CANARY).all().item()

    for short in range(3):
        caps = [R, kt, vt]
        caps[short] -= 1
        dst = _canary_dst(gpu, R, kt, vt)
        r = gpu.materialize_items(d_blocks, d_off, n, out, into=dst, caps=tuple(caps))
        torch.cuda.synchronize()
        assert r["result"].item() == OVERFLOW, short
        assert r["end"].cpu().tolist() == totals  # still the real totals
        assert _untouched(dst, ("keys", "vals", "seqno", "vtype")), short
        if short == 0:  # the plan reports it too and writes no offset
            assert r["plan_result"].item() == OVERFLOW and _untouched(dst, ("key_off", "val_off"))
        else:
            assert r["plan_result"].item() == OK
            assert torch.equal(dst["key_off"], ref["key_off"]) and torch.equal(dst["val_off"], ref["val_off"])


# ------------------------------------------------------------- 5. device block count
def test_device_block_count(gpu, oracle):
    import torch
    tables, kw, _ = P._tables("two_level")
    rows, g = tables[0][0], 5
    t = oracle.table_write(oracle.Items.from_list(rows), **kw)
    d_file = gpu.to_device_bytes(t["file"])
    args = (d_file, len(t["file"]), t["tli_off"], t["tli_size"])
    sync = gpu.scan_table(*args, two_level=True, global_seqno=g, block_count=t["block_count"])
    assert sync["table_status"] == 0 and sync["n_blocks"] == t["block_count"]
    a = gpu.materialize_items(d_file, sync["block_off"], sync["n_blocks"], sync)
    torch.cuda.synchronize()
    totals = a["end"].cpu().tolist()
    assert totals == _totals(rows)
    asy = gpu.scan_table(*args, two_level=True, global_seqno=g, block_count=t["block_count"], sync=False,
                         data_blocks_hint=t["block_count"] + 7)
    assert asy["item_start"].numel() - 1 > t["block_count"] + 7  # the host bound is not the count
    b = gpu.materialize_items(d_file, asy["block_off"], asy["n_blocks"], asy, caps=tuple(totals))
    torch.cuda.synchronize()
    assert asy["table_status"].item() == 0 and asy["n_blocks"].item() == t["block_count"]
    assert b["result"].item() == OK and b["plan_result"].item() == OK and b["end"].cpu().tolist() == totals
    sizes = {"keys": totals[1], "vals": totals[2], "key_off": totals[0] + 1, "val_off": totals[0] + 1,
             "seqno": totals[0], "vtype": totals[0]}
    for f in FIELDS:
        assert torch.equal(b[f][:sizes[f]], a[f][:sizes[f]]), f
    assert _read_rows(b, 0, totals[0]) == P._shifted(rows, g)


# ---------------------------------------------------------------------- 6. LZ4 frames
def test_lz4_frames_give_the_same_items(gpu, oracle):
    import torch
    tables, kw, _ = P._tables("big_values")
    rows = tables[0][0]
    d_file, out, t = _scan_out(gpu, oracle, rows, 0, kw)
    a = gpu.materialize_items(d_file, out["block_off"], out["n_blocks"], out)
    off = t["block_off"].astype(np.int64)
    blocks = []
    for b in range(t["block_count"]):
        payload = t["file"][int(off[b]) + 33:int(off[b + 1])]
        stored = lz4_compress(payload)
        blocks.append(oracle.block_header(0, stored, len(payload)) + stored)
    boff = np.concatenate([[0], np.cumsum([len(b) for b in blocks])]).astype(np.int64)
    nb = len(blocks)
    z = gpu.decode_lz4_blocks(gpu.to_device_bytes(b"".join(blocks)), torch.from_numpy(boff).cuda(), expect_type=0)
    assert (z["status"][:nb] == 0).all().item()
    b = gpu.materialize_items(z["frames"], z["frame_off"], nb, z)
    torch.cuda.synchronize()
    assert a["end"].cpu().tolist() == b["end"].cpu().tolist() == _totals(rows)
    for f in ("key_off", "val_off", "seqno", "vtype"):
        assert torch.equal(a[f], b[f]), f
    assert _read_rows(b, 0, len(rows)) == rows == _read_rows(a, 0, len(rows))


# ---------------------------------------------------------------------- 7. high bases
def test_bases_past_2gib_and_4gib(gpu, oracle):
    """A key arena of 2^31 + 64 KiB bytes and a value arena of 2^32 + 64 KiB bytes, really
    allocated; the table is appended at d_base = {5, 2^31 + 3, 2^32 + 9}.  Offsets with bit 31
    (keys) and bit 32 (values) set must survive the wave broadcasts, and nothing around the
    span may be touched."""
    import torch
    tables, kw, _ = P._tables("prefix_keys")
    rows = tables[0][0]
    R, kt, vt = _totals(rows)
    base = [5, 2 ** 31 + 3, 2 ** 32 + 9]
    guard = 4096
    try:
        keys = torch.empty(2 ** 31 + 65536, dtype=torch.uint8, device="cuda")
        vals = torch.empty(2 ** 32 + 65536, dtype=torch.uint8, device="cuda")
    except RuntimeError as e:  # (torch.cuda.OutOfMemoryError is one)
        pytest.skip(f"cannot allocate the 2 GiB + 4 GiB arenas: {e}")
    assert base[1] + kt + guard < keys.numel() and base[2] + vt + guard < vals.numel()
    keys[base[1] - guard:].fill_(CANARY)
    vals[base[2] - guard:].fill_(CANARY)
    dst = _canary_dst(gpu, base[0] + R, 0, 0)
    dst["keys"], dst["vals"] = keys, vals
    d_file, out, _ = _scan_out(gpu, oracle, rows, 0, kw)
    d_base = torch.tensor(base, dtype=torch.int64, device="cuda")
    r = gpu.materialize_items(d_file, out["block_off"], out["n_blocks"], out, base=d_base, into=dst,
                              caps=(base[0] + R, keys.numel() - gpu.LSM_INPUT_PADDING,
                                    vals.numel() - gpu.LSM_INPUT_PADDING))
    torch.cuda.synchronize()
    assert r["result"].item() == OK and r["plan_result"].item() == OK
    end = r["end"].cpu().tolist()
    assert end == [base[0] + R, base[1] + kt, base[2] + vt]
    ko, vo = dst["key_off"].cpu().numpy(), dst["val_off"].cpu().numpy()
    assert (ko[:5] == WORD).all() and (vo[:5] == WORD).all()
    assert ko[5] == base[1] and ko[-1] == end[1] and vo[5] == base[2] and vo[-1] == end[2]
    assert ((ko[5:] >> 31) == 1).all() and ((vo[5:] >> 32) == 1).all()
    assert _read_rows(dst, base[0], end[0]) == rows
    assert (keys[base[1] - guard:base[1]] == CANARY).all().item() and (keys[end[1]:] == CANARY).all().item()
    assert (vals[base[2] - guard:base[2]] == CANARY).all().item() and (vals[end[2]:] == CANARY).all().item()
    assert (dst["seqno"][:5] == WORD).all().item() and (dst["vtype"][:5] == CANARY).all().item()


# --------------------------------------------------------------------------- 8. graph
def test_graph_replay_over_overwritten_inputs(gpu, oracle):
    """Plan + gather captured on one stream; the replay reads whatever the input buffers hold
    then: a second table copied over the first (block count on the device), then the first
    again."""
    import torch
    tables, _, _ = P._tables("two_level")
    sets = [(tables[0][0], 3), (tables[1][0][:200], 11)]  # (fewer rows: another block count)
    written = [oracle.table_write(oracle.Items.from_list(rows), block_size=1024) for rows, _ in sets]
    flen = max(len(t["file"]) for t in written)
    cap_blocks = max(t["block_count"] for t in written) + 5
    item_cap = flen // 3 + 1
    src = []
    for (rows, g), t in zip(sets, written):
        d_file = gpu.to_device_bytes(bytes(t["file"]) + bytes(flen - len(t["file"])))
        out = gpu.scan_table(d_file, len(t["file"]), t["tli_off"], t["tli_size"], global_seqno=g,
                             block_count=t["block_count"], cap_blocks=cap_blocks, item_cap=item_cap, sync=False,
                             data_blocks_hint=cap_blocks)
        torch.cuda.synchronize()
        assert out["table_status"].item() == 0 and out["n_blocks"].item() == t["block_count"]
        src.append(dict(out, file=d_file))
    assert written[0]["block_count"] != written[1]["block_count"]
    live = {f: t.clone() for f, t in src[0].items()}
    assert all(s[f].shape == live[f].shape for s in src for f in live)
    want = [P._shifted(rows, g) for rows, g in sets]
    N, KT, VT = (max(_totals(w)[k] for w in want) for k in range(3))
    dst = _canary_dst(gpu, N, KT, VT)
    end = torch.zeros(3, dtype=torch.int64, device="cuda")
    res = torch.zeros(2, dtype=torch.int32, device="cuda")
    lib = gpu.lib()
    ws = torch.zeros(lib.lsm_materialize_items_workspace_size(item_cap), dtype=torch.uint8, device="cuda")
    args, ps = gpu._mi_args(live["file"], live["block_off"], live["n_blocks"], live)
    assert args[7] == item_cap and args[2] == cap_blocks
    p = lambda t: C.c_void_p(t.data_ptr())

    def launch():
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = lib.lsm_materialize_items_plan(*args, None, p(dst["key_off"]), p(dst["val_off"]), N, p(end), p(res[0:]),
                                            p(ws), ws.numel(), s)
        assert rc == 0, rc
        rc = lib.lsm_materialize_items(*args, None, p(end), p(dst["key_off"]), p(dst["val_off"]), p(dst["keys"]), KT,
                                       p(dst["vals"]), VT, p(dst["seqno"]), p(dst["vtype"]), N, p(res[1:]), s)
        assert rc == 0, rc

    graph = capture(launch)
    for which in (0, 1, 0):
        for f, t in live.items():
            t.copy_(src[which][f])
        for t in dst.values():
            t.view(torch.uint8).fill_(CANARY)
        end.fill_(-1)
        res.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert res.cpu().tolist() == [OK, OK]
        e = end.cpu().tolist()
        assert e == _totals(want[which])
        assert _read_rows(dst, 0, e[0]) == want[which]
        assert (dst["keys"][e[1]:] == CANARY).all().item() and (dst["vals"][e[2]:] == CANARY).all().item()
        assert (dst["seqno"][e[0]:] == WORD).all().item() and (dst["vtype"][e[0]:] == CANARY).all().item()
