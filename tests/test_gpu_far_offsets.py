"""Every 64-bit input offset of the C ABI with bit 31 or bit 32 set.

One 4 GiB + 16 MiB device buffer (tests/far_offsets.py) stands for every input arena: the batch
under test, a needle / bound / key / value arena or a table image is laid so that a line (2^31 or
2^32) falls strictly inside a block, exactly at a block's first byte, or wholly below the batch,
and the pointer the library gets is always the buffer's first byte.  The regions a truncated or
bit-31-dropped offset would reach hold 0xA5, so a kernel that loses a bit reads bytes that are no
block.  Every comparison is bit-exact against the oracle or the CPU model of the entry point, on
the compact batch (parsed fields are block-relative, so they are the same at any base)."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import far_offsets as F
import merge_read_model as R
import pyoracle
from helpers import compare_decode, prefix_items, random_sorted_items
from lz4_cases import lz4_compress

pytestmark = pytest.mark.gpu

PLACEMENTS = F.placements()
at_every_placement = pytest.mark.parametrize("pl", PLACEMENTS, ids=[p[0] for p in PLACEMENTS])
SENT = 0x5A
U63 = (1 << 63) - 1


@pytest.fixture(scope="module")
def arena(gpu):
    import torch
    a = F.allocate_arena()
    yield a
    del a
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def reference():
    """The oracle's decode of the compact batch (computed once, left unchanged)."""
    b = F.batch()
    parsed, item_start, status = pyoracle.decode_blocks(b["buf"], b["off"])
    return {"parsed": parsed, "item_start": item_start, "status": status, "n": len(b["blocks"]),
            "item_cap": int(item_start[-1]) + 64}


def _i64(a):
    import torch
    return torch.from_numpy(np.asarray(a, np.uint64).view(np.int64).copy()).cuda()


def lay_batch(arena, base, blocks=None):
    """The batch (or another list of blocks) laid back to back at `base` -> (device offsets,
    layout)."""
    blocks = F.batch()["blocks"] if blocks is None else blocks
    off = np.zeros(len(blocks) + 1, np.uint64)
    off[1:] = np.cumsum([len(b) for b in blocks])
    lay = F.place(arena, [(int(off[i]), blocks[i]) for i in range(len(blocks))], base)
    return _i64(off + np.uint64(base)), lay


def lay_arena(arena, parts, at):
    """Short pieces (needles, bounds, keys, values) packed back to back at `at` -> (device
    offsets [n + 1], layout)."""
    off = np.zeros(len(parts) + 1, np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts])
    lay = F.place(arena, [(0, b"".join(parts) or b"\0")], at)
    return _i64(off + np.uint64(at)), lay


def small_arena(gpu, parts):
    """The same pieces in a small buffer of their own, offsets from 0."""
    off = np.zeros(len(parts) + 1, np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts])
    return gpu.to_device_bytes(b"".join(parts)), _i64(off)


def disjoint(*layouts):
    """No alias region or guard of any layout overlaps a placed piece of any of them."""
    placed = [p for lay in layouts for p in lay["placed"]]
    for lay in layouts:
        assert F.overlaps(lay["aliases"], placed) == [] and F.overlaps(lay["guards"], placed) == []


def after(lay, skip=3 * F.GUARD + 7):
    """An offset past a layout's upper guard, for the next arena of the same test."""
    return max(o + n for o, n in lay["placed"]) + skip


def sentinel_outputs(gpu, item_cap, n, compact=False):
    import torch
    out = gpu.Decoder().alloc_outputs(item_cap, n, compact=compact)
    for t in out.values():
        t.view(torch.uint8).fill_(SENT)
    return out


def far_decode(gpu, arena, d_off, tuning=None, pool=False, compact=False):
    """lsm_decode_blocks / _tuned / 16 on the arena, outputs starting as sentinels -> numpy dict."""
    import torch
    ref = reference()
    n, cap = ref["n"], ref["item_cap"]
    out = sentinel_outputs(gpu, cap, n, compact)
    gpu.Decoder().decode(arena, d_off, n, out, cap, tuning=tuning, pool=pool, compact=compact,
                         blocks_bytes=len(F.batch()["buf"]))
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res["status"] = res["status"][:n]
    return res, out


# ---- decode ---------------------------------------------------------------------------------------
DECODE_VARIANTS = [("lsm_decode_blocks", None, False), ("pool", None, True)] + \
    [(f"{t}-{'pool' if p else 'no-pool'}", t, p) for t in ((1, 256, 64), (48, 65536, 1024)) for p in (True, False)]


@at_every_placement
def test_decode_blocks(gpu, arena, pl):
    """lsm_decode_blocks and lsm_decode_blocks_tuned (both tunings, pool on and off)."""
    ref = reference()
    d_off, lay = lay_batch(arena, pl[4])
    assert int(d_off[0]) != 0
    for name, tuning, pool in DECODE_VARIANTS:
        res, _ = far_decode(gpu, arena, d_off, tuning, pool)
        try:
            compare_decode(res, ref["parsed"], ref["item_start"], ref["status"])
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from e
    F.assert_untouched(arena, lay)


@at_every_placement
def test_decode_blocks16(gpu, arena, pl):
    """lsm_decode_blocks16, compared as tests/test_gpu_compact.py compares (index blocks and
    payloads above 65535 bytes report LSM_UNSUPPORTED)."""
    from test_gpu_compact import FIELD16, _compact_expected
    ref, b = reference(), F.batch()
    d_off, lay = lay_batch(arena, pl[4])
    exp = _compact_expected(b["buf"], b["off"], ref["status"])
    assert (exp == 0).sum() >= 23 and (exp == 9).sum() == 2
    for tuning in (None, (1, 256, 64), (48, 65536, 1024)):
        g, _ = far_decode(gpu, arena, d_off, tuning, compact=True)
        st = g["status"].astype(np.int32)
        assert (st == exp).all(), (tuning, np.nonzero(st != exp)[0][:10], st, exp)
        assert (g["item_start"].view(np.uint32) == ref["item_start"]).all()
        starts = ref["item_start"].astype(np.int64)
        mask = np.zeros(int(starts[-1]), bool)
        for blk in np.nonzero(exp == 0)[0]:
            mask[starts[blk]:starts[blk + 1]] = True
        for f, dt in FIELD16.items():
            o = ref["parsed"][f][:len(mask)]
            assert (o[mask] <= np.iinfo(dt).max).all(), f
            gv = g[f].view(dt)[:len(mask)]
            bad = np.nonzero((gv != o.astype(dt)) & mask)[0]
            assert len(bad) == 0, (tuning, f, bad[:10], gv[bad[:10]], o[bad[:10]])
    F.assert_untouched(arena, lay)


# ---- checksums and hashes -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def block_digests():
    return [pyoracle.xxh3_128(blk) for blk in F.batch()["blocks"]]


@at_every_placement
def test_xxh3_128_batch(gpu, arena, pl):
    import torch
    d_off, lay = lay_batch(arena, pl[4])
    n = reference()["n"]
    out = gpu.xxh3_128_batch(arena, d_off, n)
    torch.cuda.synchronize()
    v = out.cpu().numpy().view(np.uint64)
    got = [(int(v[2 * i + 1]) << 64) | int(v[2 * i]) for i in range(n)]
    assert got == block_digests()
    F.assert_untouched(arena, lay)


@functools.lru_cache(maxsize=None)
def hash_keys():
    """Keys of 1 .. 40 bytes and their xxh3_64: the 40-byte keys in the middle."""
    short = F.item_keys(random_sorted_items(150, seed=3, kmin=1, kmax=24))
    keys = short[:75] + F.item_keys(prefix_items(40, seed=5)) + short[75:]
    return keys, [pyoracle.xxh3_64(k) for k in keys]


KEY_ANCHORS = F.short_anchors(np.cumsum([0] + [len(k) for k in hash_keys()[0]]), 95)


@pytest.mark.parametrize("name,base", KEY_ANCHORS, ids=[a[0] for a in KEY_ANCHORS])
def test_hash64_keys(gpu, arena, name, base):
    import torch
    keys, want = hash_keys()
    assert len(keys[95]) == 40
    d_off, lay = lay_arena(arena, keys, base)
    out = gpu.hash64_keys(arena, d_off)
    torch.cuda.synchronize()
    assert out.cpu().numpy().view(np.uint64).tolist() == want
    F.assert_untouched(arena, lay)


# ---- lookups ----------------------------------------------------------------------------------------
def _data_blocks():
    """The batch's data blocks that decode: [(block index, keys, seqnos)]."""
    b, st = F.batch(), reference()["status"]
    return [(i, F.item_keys(b["items"][i]), b["items"][i].seqno) for i, c in enumerate(b["classes"])
            if c not in ("index", "cksum", "parse") and st[i] == 0]


def _payload(i):
    b = F.batch()
    return bytes(b["buf"][int(b["off"][i]) + 33:int(b["off"][i + 1])])


@functools.lru_cache(maxsize=None)
def point_queries():
    """[(block, needle, snapshot)] into every data block (so below, around and above every line),
    hits and misses, and the oracle's answers."""
    rng = random.Random(5)
    qs = []
    for i, keys, seq in _data_blocks():
        for j in sorted({0, len(keys) // 2, len(keys) - 1, rng.randrange(len(keys))}):
            s = int(seq[j])
            qs += [(i, keys[j], min(s + 1, U63)), (i, keys[j], s), (i, keys[j], U63)]
        qs += [(i, keys[0] + b"\0zz", U63), (i, b"", U63), (i, b"\xff" * 9, 5)]
    exp = [pyoracle.point_read(_payload(i), k, s) for i, k, s in qs]
    assert sum(e >= 0 for e in exp) > len(qs) // 3 and sum(e == -1 for e in exp) > len(qs) // 4
    return qs, exp


def _check_point(res, pl):
    qs, exp = point_queries()
    ref = reference()
    parsed, item_start = ref["parsed"], ref["item_start"]
    assert (res["status"] == 0).all()
    sides = set()
    for q, ((blk, needle, snap), e) in enumerate(zip(qs, exp)):
        assert int(res["item"][q]) == e, (q, blk, needle, snap)
        sides.add((blk > pl[2]) - (blk < pl[2]))
        if e >= 0:
            r = int(item_start[blk]) + e
            assert int(res["seqno"][q]) & (2 ** 64 - 1) == int(parsed["seqno"][r])
            assert int(res["val_off"][q]) == int(parsed["val_off"][r])
            assert int(res["val_len"][q]) == int(parsed["val_len"][r])
            assert int(res["vtype"][q]) == int(parsed["vtype"][r])
    if pl[3] != "above":
        assert sides == {-1, 0, 1}  # blocks below the line, the one at it and blocks above


@at_every_placement
@pytest.mark.parametrize("needles", ["near", "far"])
def test_point_read_blocks(gpu, arena, pl, needles):
    import torch
    qs, _ = point_queries()
    d_off, lay = lay_batch(arena, pl[4])
    lays = [lay]
    if needles == "far":
        d_needles = arena
        d_noff, nlay = lay_arena(arena, [q[1] for q in qs], after(lay))
        assert int(d_noff[0]) >= pl[1]
        lays.append(nlay)
        disjoint(*lays)
    else:
        d_needles, d_noff = small_arena(gpu, [q[1] for q in qs])
    out = gpu.point_read(arena, d_off, reference()["n"], torch.tensor([q[0] for q in qs], dtype=torch.int32).cuda(),
                         d_needles, d_noff, _i64([q[2] for q in qs]))
    torch.cuda.synchronize()
    _check_point({k: v.cpu().numpy()[:len(qs)] for k, v in out.items()}, pl)
    F.assert_untouched(arena, *lays)


@functools.lru_cache(maxsize=None)
def seek_queries():
    """[(block, lo, hi, flags)]: every data block under all 16 flag values, bounds that are keys of
    the block, keys between them and the empty key; and the oracle's answers."""
    rng = random.Random(6)
    qs = []
    for i, keys, _ in _data_blocks():
        def bound():
            r = rng.random()
            if r < 0.6:
                return rng.choice(keys)
            return rng.choice(keys) + b"\1" if r < 0.85 else bytes(rng.choice(b"abcdefgh") for _ in range(rng.randint(0, 4)))
        for fl in range(16):
            qs.append((i, bound(), bound(), fl))
            qs.append((i, bound(), bound(), fl))
    exp = [pyoracle.seek(_payload(i), lo if fl & 1 else None, hi if fl & 2 else None, bool(fl & 4), bool(fl & 8))
           for i, lo, hi, fl in qs]
    assert all(e is not None for e in exp) and sum(e[0] < e[1] for e in exp) > len(qs) // 4
    return qs, exp


@at_every_placement
def test_seek_blocks(gpu, arena, pl):
    """Blocks, lower bounds and upper bounds all far, every flag value."""
    import torch
    qs, exp = seek_queries()
    d_off, lay = lay_batch(arena, pl[4])
    d_lo_off, lo_lay = lay_arena(arena, [q[1] for q in qs], after(lay))
    d_hi_off, hi_lay = lay_arena(arena, [q[2] for q in qs], after(lo_lay))
    disjoint(lay, lo_lay, hi_lay)
    assert int(d_lo_off[0]) >= pl[1] and int(d_hi_off[0]) >= pl[1]
    out = gpu.seek(arena, d_off, reference()["n"], torch.tensor([q[0] for q in qs], dtype=torch.int32).cuda(),
                   arena, d_lo_off, arena, d_hi_off, torch.tensor([q[3] for q in qs], dtype=torch.uint8).cuda())
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    assert (res["status"][:len(qs)] == 0).all()
    for q, e in enumerate(exp):
        got = (int(res["first"][q]), int(res["end"][q]), bool(res["found"][q] & 1), bool(res["found"][q] & 2))
        assert got == e, (q, qs[q], got, e)
    F.assert_untouched(arena, lay, lo_lay, hi_lay)


# ---- materialize ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def materialized_rows():
    """The oracle's rows of every block: (keys as lsm_materialize_keys gives them, rows as
    lsm_materialize_items gives them), flat in batch order."""
    b, ref = F.batch(), reference()
    keys, rows = [], []
    for i, c in enumerate(b["classes"]):
        count = int(ref["item_start"][i + 1]) - int(ref["item_start"][i])
        if ref["status"][i] != 0:
            keys += [b""] * count
            rows += [(b"", b"", 0, 0)] * count
            continue
        payload = _payload(i)
        n, parsed = pyoracle.data_block_decode(payload, index=(c == "index"))
        assert n == count
        want = pyoracle.materialize(payload, parsed, payload[-31])
        keys += [w[0] for w in want]
        rows += want if c != "index" else [(b"", b"", 0, 0)] * count  # (an index block's rows are rejected)
    return keys, rows


@at_every_placement
def test_materialize_keys_and_items(gpu, arena, pl):
    """lsm_materialize_plan / _keys and lsm_materialize_items_plan / _items read the far blocks; the
    outputs lie at small bases."""
    import torch
    from test_gpu_materialize_items import _read_rows
    n = reference()["n"]
    want_keys, want_rows = materialized_rows()
    d_off, lay = lay_batch(arena, pl[4])
    _, out = far_decode(gpu, arena, d_off)
    keys, key_off = gpu.materialize_keys(arena, d_off, n, out)
    items = gpu.materialize_items(arena, d_off, n, out)
    torch.cuda.synchronize()
    ko = key_off.cpu().numpy()
    kb = keys.cpu().numpy().tobytes()
    assert len(ko) == len(want_keys) + 1
    assert [kb[ko[i]:ko[i + 1]] for i in range(len(want_keys))] == want_keys
    assert items["result"].item() == 0 and items["plan_result"].item() == 0
    total = [len(want_rows), sum(len(r[0]) for r in want_rows), sum(len(r[1]) for r in want_rows)]
    assert items["end"].cpu().tolist() == total
    assert _read_rows(items, 0, len(want_rows)) == want_rows
    F.assert_untouched(arena, lay)


# ---- LZ4 ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lz4_batch():
    """The payloads of the batch's blocks that decode, compressed by liblz4 and framed; one stored
    byte of block 2 flipped.  -> (blocks, raw payloads, expected statuses, k_small, k_largest)."""
    b, ref = F.batch(), reference()
    idx = [i for i in range(ref["n"]) if ref["status"][i] == 0]
    raws = [_payload(i) for i in idx]
    blocks = [pyoracle.block_header(b["blocks"][i][4], c, len(r)) + c
              for i, r, c in zip(idx, raws, [lz4_compress(r) for r in raws])]
    bad = bytearray(blocks[2])
    bad[40] ^= 1
    blocks[2] = bytes(bad)
    status = [0] * len(blocks)
    status[2] = 4
    for r, blk in zip(raws, blocks):
        assert pyoracle.lz4_decompress(blk[33:], len(r)) == r or blk is blocks[2]
    return blocks, raws, status, 5, int(np.argmax([len(x) for x in blocks]))


def _lz4_offsets():
    blocks = lz4_batch()[0]
    return np.concatenate([[0], np.cumsum([len(x) for x in blocks])]).astype(np.uint64)


LZ4_PLACEMENTS = F.placements_of(_lz4_offsets(), lz4_batch()[3], lz4_batch()[4])


def _lz4_run(gpu, d_blocks, d_off, n):
    import torch
    plain = gpu.lz4_decompress_blocks(d_blocks, d_off, n)
    framed = gpu.decode_lz4_blocks(d_blocks, d_off, n, item_cap=reference()["item_cap"])
    torch.cuda.synchronize()
    return {"out": plain[0].cpu().numpy(), "out_off": plain[1].cpu().numpy(), "status": plain[2].cpu().numpy(),
            "frames": framed["frames"].cpu().numpy(), "frame_off": framed["frame_off"].cpu().numpy(),
            "frame_status": framed["status"].cpu().numpy()[:n]}


@pytest.fixture(scope="module")
def lz4_base0(gpu):
    """The run at base 0 in a buffer of its own, checked against the oracle once."""
    blocks, raws, status, _, _ = lz4_batch()
    d_blocks, d_off = small_arena(gpu, blocks)
    g = _lz4_run(gpu, d_blocks, d_off, len(blocks))
    assert g["status"].tolist() == status
    oo, fo = g["out_off"], g["frame_off"]
    for i, r in enumerate(raws):
        if status[i] == 0:
            assert g["out"][oo[i]:oo[i + 1]].tobytes() == r
            assert g["frames"][fo[i] + 33:fo[i + 1]].tobytes() == r
    return g


@pytest.mark.parametrize("pl", LZ4_PLACEMENTS, ids=[p[0] for p in LZ4_PLACEMENTS])
def test_lz4_decompress(gpu, arena, lz4_base0, pl):
    """lsm_lz4_plan_output + lsm_lz4_decompress_blocks and lsm_lz4_plan_framed +
    lsm_lz4_decompress_framed with the compressed blocks far: bytes, offsets and statuses equal
    the base-0 run's (which equals the oracle's)."""
    blocks, raws, status, _, _ = lz4_batch()
    d_off, lay = lay_batch(arena, pl[4], blocks)
    g = _lz4_run(gpu, arena, d_off, len(blocks))
    assert g["status"].tolist() == status
    for f in ("out_off", "frame_off", "frame_status"):
        assert (g[f] == lz4_base0[f]).all(), f
    ok = np.array(status) == 0
    for i in np.nonzero(ok)[0]:
        for buf, off in (("out", "out_off"), ("frames", "frame_off")):
            lo, hi = int(g[off][i]), int(g[off][i + 1])
            assert (g[buf][lo:hi] == lz4_base0[buf][lo:hi]).all(), (buf, i)
    F.assert_untouched(arena, lay)


def _compress_run(gpu, d_blocks, d_off, n, nbytes):
    import torch
    res = gpu.lz4_compress_blocks(d_blocks, d_off, n, blocks_bytes=nbytes)
    torch.cuda.synchronize()
    return {"buf": res["buf"].cpu().numpy(), "off": res["block_off"].cpu().numpy(), "status": res["status"].cpu().numpy()}


@pytest.fixture(scope="module")
def compress_base0(gpu):
    """lsm_lz4_compress_blocks of the batch at base 0: Header' || stream decompresses (oracle) to
    the input payload."""
    from test_gpu_lz4_compress import _check_block
    b, ref = F.batch(), reference()
    d_blocks, d_off = small_arena(gpu, b["blocks"])
    g = _compress_run(gpu, d_blocks, d_off, ref["n"], len(b["buf"]))
    ok = 0
    for i in range(ref["n"]):
        if g["status"][i] == 0:
            out = g["buf"][int(g["off"][i]):int(g["off"][i + 1])].tobytes()
            if b["classes"][i] == "index":
                assert out[4] == 1 and pyoracle.lz4_decompress(out[33:], len(_payload(i))) == _payload(i)
            elif b["classes"][i] != "cksum":  # (its payload is not the one its header was made for)
                _check_block(b["classes"][i], _payload(i), out)
            ok += 1
    assert ok >= 24
    return g


@at_every_placement
def test_lz4_compress_blocks(gpu, arena, compress_base0, pl):
    b, ref = F.batch(), reference()
    d_off, lay = lay_batch(arena, pl[4])
    g = _compress_run(gpu, arena, d_off, ref["n"], len(b["buf"]))
    assert (g["status"] == compress_base0["status"]).all() and (g["off"] == compress_base0["off"]).all()
    total = int(g["off"][-1])
    assert (g["buf"][:total] == compress_base0["buf"][:total]).all()
    F.assert_untouched(arena, lay)


# ---- merges -------------------------------------------------------------------------------------------
def _lay_items(arena, flat, key_at, val_at):
    """Items (key, value, seqno, vtype) -> a device lsm_items dict whose key and value arenas are
    the far arena, plus the two layouts."""
    import torch
    key_off, klay = lay_arena(arena, [it[0] for it in flat], key_at)
    val_off, vlay = lay_arena(arena, [it[1] for it in flat], val_at)
    disjoint(klay, vlay)
    d = {"keys": arena, "key_off": key_off, "vals": arena, "val_off": val_off,
         "seqno": _i64([it[2] for it in flat]),
         "vtype": torch.from_numpy(np.array([it[3] for it in flat], np.uint8)).cuda()}
    return d, klay, vlay


def _merge_anchors(flat, item):
    """[(id, key base, value base)]: per line the keys straddling it (the line one byte into
    `item`'s key) with the values above them, then the values straddling it with the keys above
    them; and both above L32."""
    ko = np.cumsum([0] + [len(it[0]) for it in flat])
    vo = np.cumsum([0] + [len(it[1]) for it in flat])
    assert ko[item + 1] - ko[item] >= 2 and vo[item + 1] - vo[item] >= 2
    out = []
    for name, line in (("L31", F.L31), ("L32", F.L32)):
        kb, vb = line - int(ko[item]) - 1, line - int(vo[item]) - 1
        out.append((f"{name}-keys", kb, kb + int(ko[-1]) + 3 * F.GUARD + 5))
        out.append((f"{name}-values", vb + int(vo[-1]) + 3 * F.GUARD + 5, vb))
    out.append(("above", F.ABOVE, F.ABOVE + int(ko[-1]) + 3 * F.GUARD + 5))
    return out


@functools.lru_cache(maxsize=None)
def merge_case():
    """Four sorted runs of about 150 items and merge_model's answer; the anchor item lies in the
    middle of run 2, so that run straddles the line."""
    import merge_gpu as G
    rng = random.Random(11)
    runs = G.deal(rng, G.random_items(rng, 600, 90, key_len=(2, 24), val_len=(2, 80)), 4)
    flat = [it for r in runs for it in r]
    item = next(i for i in range(len(runs[0]) + len(runs[1]) + len(runs[2]) // 2, len(flat)) if len(flat[i][1]) >= 2)
    assert item < len(flat) - len(runs[3])
    return runs, flat, item


MERGE_ANCHORS = _merge_anchors(merge_case()[1], merge_case()[2])


@pytest.mark.parametrize("name,key_at,val_at", MERGE_ANCHORS, ids=[a[0] for a in MERGE_ANCHORS])
def test_merge_runs(gpu, arena, name, key_at, val_at):
    import merge_gpu as G
    import torch
    runs, flat, _ = merge_case()
    d, klay, vlay = _lay_items(arena, flat, key_at, val_at)
    kb, vb = G.input_bytes(runs)
    out = G.alloc_outputs(gpu, len(flat), kb, vb, len(runs))
    ws = G.alloc_workspace(gpu, len(flat), len(runs))
    rs = torch.tensor(np.cumsum([0] + [len(r) for r in runs]), dtype=torch.int64, device="cuda")
    G.MergeCall(gpu, d, rs, out, ws, thr=300, evict=True).launch()
    torch.cuda.synchronize()
    want = G.assert_extents(G.read_outputs(out, len(runs)), runs, 300, True, False)
    assert len(want) > 100
    F.assert_untouched(arena, klay, vlay)


@functools.lru_cache(maxsize=None)
def merge_read_case():
    """3 sources x 24 groups and merge_read_model's answer."""
    rng = random.Random(12)
    runs = R.random_grouped(rng, 3, 24, max_len=12, n_keys=7, max_seq=40)
    runs = [[[(k * 3, v * 2, s, t) for k, v, s, t in run] for run in src] for src in runs]
    flat = [it for run in R.flat_runs(runs) for it in run]
    item = next(i for i in range(len(flat) // 2, len(flat)) if len(flat[i][1]) >= 2)
    return runs, flat, item, R.merge_read(runs, 25)


READ_ANCHORS = _merge_anchors(merge_read_case()[1], merge_read_case()[2])


@pytest.mark.parametrize("name,key_at,val_at", READ_ANCHORS, ids=[a[0] for a in READ_ANCHORS])
def test_merge_read(gpu, arena, name, key_at, val_at):
    import torch
    import test_gpu_merge_read as T
    runs, flat, _, ans = merge_read_case()
    assert len(ans["items"]) > 30 and ans["status"] == [0] * 24
    d, klay, vlay = _lay_items(arena, flat, key_at, val_at)
    n, kb, vb = T.sizes_of(runs)
    out = T.alloc_outputs(n, kb, vb, 24)
    ws = torch.zeros(gpu.lib().lsm_merge_read_workspace_size(n, 24, 3), dtype=torch.uint8, device="cuda")
    rs = torch.tensor(np.cumsum([0] + [len(r) for r in R.flat_runs(runs)]), dtype=torch.int64, device="cuda")
    T.ReadCall(gpu, d, rs, 24, 3, out, ws, 25).launch()
    torch.cuda.synchronize()
    T.assert_answer(T.read_outputs(out), ans)
    F.assert_untouched(arena, klay, vlay)


# ---- index entries ------------------------------------------------------------------------------------
@pytest.mark.parametrize("first,base_offset", [(F.L31 - 20000, F.L31), (F.L32 - 20000, 0), (F.L32 - 20000, 4096),
                                               (0, F.L32 - 20000), (F.L32 + 5, F.L32 + 7)],
                         ids=["off-L31+base-L31", "off-L32", "off-L32+base", "base-L32", "both-above"])
def test_index_entries(gpu, first, base_offset):
    """block_off far (no big buffer: the offsets are only numbers here) and base_offset chosen so
    that the handle offsets straddle L32: handles = block_off + base_offset, end keys and seqnos
    the last item's of each block."""
    import torch
    items = random_sorted_items(900, seed=21, kmin=3, kmax=30, vmax=50, big_seq=True)
    starts = pyoracle.cut_blocks(items, 512)
    nb = len(starts) - 1
    _, off = pyoracle.encode_blocks(items, starts)
    off = off + np.uint64(first)
    handles = off[:-1].astype(object) + base_offset
    if first != F.L32 + 5:
        assert int(handles[0]) < F.L32 < int(handles[-1]) and nb > 30
    d = gpu.items_to_device(items)
    out = gpu.index_entries(d, torch.from_numpy(starts.astype(np.int32)).cuda(), _i64(off), nb, base_offset=base_offset)
    torch.cuda.synchronize()
    assert int(out["result"].item()) == 0
    assert out["handle_off"].cpu().numpy().view(np.uint64).tolist() == [int(h) for h in handles]
    assert out["handle_size"].cpu().numpy().tolist() == np.diff(off).astype(np.int64).tolist()
    keys = F.item_keys(items)
    last = starts[1:].astype(np.int64) - 1
    ko = out["key_off"].cpu().numpy()
    kb = out["keys"].cpu().numpy().tobytes()
    assert [kb[ko[i]:ko[i + 1]] for i in range(nb)] == [keys[j] for j in last]
    assert out["seqno"].cpu().numpy().view(np.uint64).tolist() == [int(items.seqno[j]) for j in last]


# ---- a table image larger than 4 GiB --------------------------------------------------------------
TABLE_CASES = [(tl, where) for tl in (False, True) for where in ("data", "index")]
table_cases = pytest.mark.parametrize("two_level,where", TABLE_CASES,
                                      ids=[f"{'two_level' if tl else 'full'}-L32-in-{w}" for tl, w in TABLE_CASES])
TRUNCATED = 8


@functools.lru_cache(maxsize=None)
def far_table(two_level, where):
    """The MVCC table of the table tests laid D bytes into a file so that 2^32 falls inside a data
    block or inside an index block, with a filter block after the TLI.  -> (items, compact table,
    relocation, pieces, the wrappers' table dict, filter handle)."""
    from table_get_model import filter_block, mvcc_table
    items, t = mvcc_table(1, two_level)
    r = F.relocate_table(t["file"], t, F.table_shift(t["file"], t, where), two_level)
    held = F.block_holding(r, F.L32)
    assert held is not None and (held[0] < int(r["block_off"][-1])) == (where == "data")
    flt = filter_block(items)
    pieces = r["pieces"] + [(r["file_len"], flt)]
    table = {"tli_off": r["tli_off"], "tli_size": r["tli_size"], "two_level": two_level,
             "file_len": r["file_len"] + len(flt)}
    assert F.L32 < table["file_len"] < F.L32 + (4 << 20)
    return items, t, r, pieces, table, (r["file_len"], len(flt))


def lay_table(arena, two_level, where):
    items, t, r, pieces, table, flt = far_table(two_level, where)
    return F.place(arena, pieces, 0)


@table_cases
@pytest.mark.parametrize("filtered", [False, True], ids=["no-filter", "filter"])
def test_table_get(gpu, arena, two_level, where, filtered):
    """lsm_table_get: the answers of table_get_model on the compact table, the hit's block offset
    passed through the relocation map; the filter block lies past 2^32."""
    import test_gpu_table_get as T
    from table_get_model import GET_FILTERED, GET_HIT, GET_MISS
    _, _, r, _, table, flt = far_table(two_level, where)
    lay = lay_table(arena, two_level, where)
    _, _, _, _, queries, expected = T.mvcc_case(1, two_level, filtered)
    mapped = [(st, (e[0], r["map"][e[1]]) + e[2:] if e[0] == GET_HIT else e) for st, e in expected]
    assert flt[0] > F.L32
    res = T.run(gpu, arena, table, queries, filter=flt if filtered else None, hashes=filtered)
    outcomes = T.compare(res, queries, mapped)
    assert outcomes[GET_HIT] > 600 and outcomes[GET_MISS] > 0 and (not filtered or outcomes[GET_FILTERED] > 0)
    hit_blocks = {int(res["block_off"][q]) for q, (_, e) in enumerate(expected) if e[0] == GET_HIT}
    if where == "data":  # hits on both sides of the line
        assert min(hit_blocks) < F.L32 - 1000 and max(hit_blocks) > F.L32
    F.assert_untouched(arena, lay)


@table_cases
def test_table_range(gpu, arena, two_level, where):
    """lsm_table_range: table_range_model's positions on the compact table, block offsets mapped,
    ordinals against the relocated block offsets."""
    import torch
    import test_gpu_table_range as T
    from table_range_model import RANGE_ROWS
    _, t, r, _, table, _ = far_table(two_level, where)
    lay = lay_table(arena, two_level, where)
    _, _, queries, expected = T.mvcc_case(1, two_level)
    mapped = [(st, (e[0], r["map"][e[1]], e[2], e[3], r["map"][e[4]], e[5], e[6]) if e[0] == RANGE_ROWS else e)
              for st, e in expected]
    scan = {"block_off": _i64(r["block_off"]), "item_start": torch.from_numpy(t["starts"].astype(np.int32)).cuda()}
    res = T.run(gpu, arena, table, queries, scan=scan)
    outcomes = T.compare(res, queries, mapped, ordinal=T.ordinals(r["block_off"]))
    assert outcomes[RANGE_ROWS] >= 600
    F.assert_untouched(arena, lay)


@table_cases
def test_table_range_rows(gpu, arena, two_level, where):
    """table_block_offsets -> lsm_table_range_rows_plan / lsm_table_range_rows: the rows
    table_range_rows_model gives on the compact table (every fifth query)."""
    import torch
    import test_gpu_table_range_rows as T
    from table_range_rows_model import RowsModel, mvcc_rows_case
    _, t, r, _, table, _ = far_table(two_level, where)
    lay = lay_table(arena, two_level, where)
    d_off = gpu.table_block_offsets(arena, table, data_off=int(r["block_off"][0]))
    assert d_off.cpu().numpy().view(np.uint64).tolist() == r["block_off"].tolist()
    positions = mvcc_rows_case(1, two_level)[3][::5]
    base = (3, 37, 41)
    ans = RowsModel(t["file"], t["block_off"], 5).answer(positions, base)
    assert ans["need"][1] > 20000
    into = T.sentinel_items(ans["end"][0] + 3, ans["end"][1] + 29, ans["end"][2] + 31)
    res = gpu.table_range_rows(arena, dict(table, global_seqno=5), T.device_positions(positions), d_off,
                               base=torch.tensor(base, dtype=torch.int64, device="cuda"), into=into,
                               caps=(ans["need"][0], ans["need"][1], ans["end"][1], ans["end"][2]),
                               n_queries=len(positions))
    T.assert_rows(T.read(res), ans, base)
    F.assert_untouched(arena, lay)


@table_cases
def test_scan_table_needs_data_from_offset_zero(gpu, arena, two_level, where):
    """lsm_scan_table and lsm_scan_table_async read a table whose data blocks lie back to back
    from file offset 0 (include/lsmgpu.h); the relocated table's start at D > 2^31, so both report
    LSM_TRUNCATED and no block, after decoding the far index blocks."""
    import torch
    _, t, r, _, table, _ = far_table(two_level, where)
    lay = lay_table(arena, two_level, where)
    kw = dict(two_level=two_level, block_count=t["block_count"], cap_blocks=t["block_count"] + 8, item_cap=4096)
    out = gpu.scan_table(arena, table["file_len"], table["tli_off"], table["tli_size"], **kw)
    assert (out["table_status"], out["n_blocks"]) == (TRUNCATED, 0)
    out = gpu.scan_table(arena, table["file_len"], table["tli_off"], table["tli_size"], sync=False,
                         data_blocks_hint=t["block_count"], index_blocks_hint=t["block_count"] + 8, **kw)
    torch.cuda.synchronize()
    assert (int(out["table_status"].item()), int(out["n_blocks"].item())) == (TRUNCATED, 0)
    F.assert_untouched(arena, lay)


def test_range_read_over_a_far_table(gpu, arena):
    """range_read (table_range -> table_range_rows -> merge_read) once, the one source a two-level
    table with 2^32 inside a data block: merge_read_model over the rows model's runs."""
    import test_gpu_merge_read as T
    from table_range_model import mvcc_range_queries
    from table_range_rows_model import RowsModel, mvcc_rows_case
    _, t, r, _, table, _ = far_table(True, "data")
    lay = lay_table(arena, True, "data")
    queries = mvcc_range_queries(1, True)[::10]
    positions = mvcc_rows_case(1, True)[3][::10]
    runs = RowsModel(t["file"], t["block_off"], 0).answer(positions)["runs"]
    snapshot = 500
    ans = R.merge_read([runs], snapshot)
    assert sum(1 for g in range(len(runs)) if ans["group_start"][g + 1] > ans["group_start"][g]) > 40
    src = dict(table, file=arena, block_off=_i64(r["block_off"]))
    got, status = T._rows_of(gpu.range_read([src], *T._device_queries(gpu, queries), snapshot))
    assert status == ans["status"] == [0] * len(queries)
    gs = ans["group_start"]
    assert got == [ans["items"][gs[g]:gs[g + 1]] for g in range(len(queries))]
    F.assert_untouched(arena, lay)


# ---- the file checksum past 4 GiB -------------------------------------------------------------------
def test_file_checksum_past_4gib(gpu):
    """lsm_xxh3_128_file with len = 2^32 + 1025, and the same bytes as a stream: one update of
    2^32 - 512 bytes, then one of 1537, a digest after each.  The data is a 1 MiB random block
    tiled; the oracle's two digests are computed once."""
    import torch
    total, first = F.L32 + 1025, F.L32 - 512
    tile = np.random.default_rng(99).integers(0, 256, 1 << 20, dtype=np.uint8)
    host = np.tile(tile, total // len(tile) + 1)[:total]
    try:
        data = torch.empty(total + 64, dtype=torch.uint8, device="cuda")
    except RuntimeError as e:
        pytest.skip(f"cannot allocate {total >> 20} MiB: {e}")
    data[:total].copy_(torch.from_numpy(host))
    L = pyoracle.lib()
    want = []
    for n in (first, total):
        lo, hi = C.c_uint64(), C.c_uint64()
        L.orc_xxh3_128(C.c_void_p(host.ctypes.data), n, C.byref(lo), C.byref(hi))
        want.append((lo.value, hi.value))
    assert want[0] != want[1]
    assert gpu.xxh3_128_file(data, total) == want[1]
    assert gpu.xxh3_128_file(data, first) == want[0]
    w = gpu.ChecksummedWriter()
    w.write(data, first)
    assert w.checksum() == want[0]
    w.write(data, total - first, offset=first)
    assert w.checksum() == want[1] and w.bytes_written == total
