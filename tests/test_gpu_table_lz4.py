"""GPU parity of the framed readers (lsm_table_get_framed, lsm_table_range_framed,
lsm_table_range_rows_plan_framed / lsm_table_range_rows_framed) on LZ4 tables against the models
in tests/table_lz4_model.py, never against the library's own plain path except where a test says
so (the identity view, and the block cut of the uncompressed original)."""
import functools
import random

import numpy as np
import pytest

import long_key_cases as LK
import pyoracle
import test_gpu_merge_read as MR
import test_gpu_table_get as TG
import test_gpu_table_range as TR
import test_gpu_table_range_rows as RR
from table_get_model import (GET_FILTERED, GET_HIT, GET_MISS, GET_NO_BLOCK, GET_NONE, GET_SEQNO_SKIP, TRUNCATED,
                             TYPE_MISMATCH, item_key, mvcc_queries, mvcc_table, with_filter)
from table_lz4_model import (BAD_ARG, CKSUM, DECOMPRESS, FramesModel, FramesRangeModel, FramesRowsModel,
                             LZ4RangeModel, LZ4RowsModel, LZ4TableModel, View, lz4_twin)
from table_range_model import RANGE_EMPTY, RANGE_NO_BLOCK, RANGE_NONE, RANGE_ROWS, mvcc_range_queries
from table_range_rows_model import RowsModel, mvcc_rows_case, positions_of

pytestmark = pytest.mark.gpu

CASES = [(1, False), (1, True), (2, False), (2, True)]
ROW_STEP = 5  # every fifth range query goes through the rows calls (300 of 1,500)


# ---------------------------------------------------------------- device helpers
def i64(values):
    import torch
    return torch.from_numpy(np.asarray([int(v) for v in values], np.int64)).cuda()


def make_view(gpu, frames, stored_off, frame_off, status=None, frames_len=None, n_blocks=None):
    """A view dict from host lists and a padded device arena (or bytes)."""
    import torch
    if isinstance(frames, (bytes, bytearray)):
        frames_len = len(frames) if frames_len is None else frames_len
        frames = gpu.to_device_bytes(frames)
    return {"stored_off": i64(stored_off), "frames": frames, "frame_off": i64(frame_off),
            "status": None if status is None else torch.tensor(list(status), dtype=torch.int32).cuda(),
            "n_blocks": len(stored_off) - 1 if n_blocks is None else n_blocks, "frames_len": frames_len}


def host_view(v, **change):
    """The device view dict -> the model's View, with fields replaced."""
    import torch
    torch.cuda.synchronize()
    frames = v["frames"].cpu().numpy().tobytes()
    h = View(v["stored_off"].cpu().tolist(), frames[:v["frames_len"]], v["frame_off"].cpu().tolist(),
             None if v["status"] is None else v["status"].cpu().tolist(), v["frames_len"], v["n_blocks"])
    h.frames = frames  # (the padding too: frames_len bounds what is read)
    for k, x in change.items():
        setattr(h, k, x)
    return h


def run_get(gpu, d_file, table, queries, view, filter=None, hashes=False, lowest_seqno=0, global_seqno=0):
    import torch
    needles = b"".join(q[0] for q in queries)
    noff = np.concatenate([[0], np.cumsum([len(q[0]) for q in queries])]).astype(np.int64)
    kw = dict(key_hash=TG._i64(pyoracle.xxh3_64(q[0]) for q in queries) if hashes else None, filter=filter,
              lowest_seqno=lowest_seqno, global_seqno=global_seqno)
    res = gpu.table_get(d_file, table, gpu.to_device_bytes(needles), torch.from_numpy(noff).cuda(),
                        TG._i64(q[1] for q in queries), frames=view, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy()[:len(queries)] for k, v in res.items()}


def device_bounds(gpu, queries):
    return MR._device_queries(gpu, queries)


def run_range(gpu, d_file, table, queries, view=None, scan=None):
    import torch
    out = {f: torch.full((len(queries),), TR.SENTINEL, dtype=getattr(torch, dt), device="cuda")
           for f, dt in gpu.TABLE_RANGE_FIELDS}
    res = gpu.table_range(d_file, table, *device_bounds(gpu, queries), scan=scan, out=out, frames=view)
    torch.cuda.synchronize()
    return res, {k: v.cpu().numpy()[:len(queries)] for k, v in res.items()}


def run_rows(gpu, d_file, table, positions, ans, view=None, block_off=None, base=(3, 37, 41), d_pos=None):
    """One rows call on sentinel outputs with caps from the model's answer, everything compared."""
    import torch
    into = RR.sentinel_items(ans["end"][0] + 3, ans["end"][1] + 29, ans["end"][2] + 31)
    res = gpu.table_range_rows(d_file, table, d_pos or RR.device_positions(positions), block_off,
                               base=torch.tensor(base, dtype=torch.int64, device="cuda"), into=into,
                               caps=(ans["need"][0], ans["need"][1], ans["end"][1], ans["end"][2]),
                               n_queries=len(positions), frames=view)
    g = RR.read(res)
    RR.assert_rows(g, ans, base)
    return g


def check_blocks(res, expected, ordinal):
    for q, (st, e) in enumerate(expected):
        if st == 0 and e[0] == GET_HIT:
            assert int(res["block"][q]) == ordinal[e[1:3]], q


def check_values(res, expected, model, view_h):
    """For every hit, the value bytes read from the frames are the item's."""
    hits = 0
    for q, (st, e) in enumerate(expected):
        if st == 0 and e[0] == GET_HIT:
            payload, _ = model.data_block(e[1], e[2])
            at = view_h.frame_off[int(res["block"][q])] + 33 + int(res["val_off"][q])
            assert view_h.frames[at:at + int(res["val_len"][q])] == payload[e[5]:e[5] + e[6]], q
            hits += 1
    return hits


# ---------------------------------------------------------------- shared cases
@functools.lru_cache(maxsize=None)
def twin_case(seed, two_level):
    items, t = mvcc_table(seed, two_level)
    return items, t, lz4_twin(t, two_level)


@functools.lru_cache(maxsize=None)
def twin_get_expected(seed, two_level):
    items, _, twin = twin_case(seed, two_level)
    model = LZ4TableModel(twin["file"], twin["tli_off"], twin["tli_size"], two_level)
    queries = mvcc_queries(items, seed)
    return model, queries, [model.lookup(k, s) for k, s in queries]


@functools.lru_cache(maxsize=None)
def twin_range_expected(seed, two_level):
    _, _, twin = twin_case(seed, two_level)
    model = LZ4RangeModel(twin["file"], twin["tli_off"], twin["tli_size"], two_level)
    queries = mvcc_range_queries(seed, two_level)
    return queries, [model.answer(*q) for q in queries]


def twin_on_device(gpu, twin, two_level, file=None):
    file = twin["file"] if file is None else file
    table = dict(twin, two_level=two_level, file_len=len(file))
    d_file = gpu.to_device_bytes(file)
    return d_file, table, gpu.table_frames(d_file, table, block_off=i64(twin["block_off"]))


# ---------------------------------------------------------------- 1. the identity view
@pytest.mark.parametrize("seed,two_level", CASES)
def test_identity_view(gpu, seed, two_level):
    """frames = the file, frame_off = stored_off, no statuses, over the uncompressed table: the
    plain models' answers, and the plain entry points' outputs on the same inputs."""
    import torch
    file, table, _, _, queries, expected = TG.mvcc_case(seed, two_level, False)
    d_file = gpu.to_device_bytes(file)
    table = dict(table, file_len=len(file))
    off = [int(o) for o in table["block_off"]]
    view = make_view(gpu, d_file, off, off, frames_len=len(file))
    ordinal = TR.ordinals(off)
    # get
    res = run_get(gpu, d_file, table, queries, view)
    TG.compare(res, queries, expected)
    check_blocks(res, expected, ordinal)
    plain = TG.run(gpu, d_file, table, queries)
    for f, _ in gpu.TABLE_GET_FIELDS:
        assert (res[f] == plain[f]).all(), f
    # range
    _, _, rq, rexp = TR.mvcc_case(seed, two_level)
    d_res, res = run_range(gpu, d_file, table, rq, view)
    TR.compare(res, rq, rexp, ordinal=ordinal)
    _, plain = run_range(gpu, d_file, table, rq, scan={"block_off": view["stored_off"],
                         "item_start": torch.zeros(len(off), dtype=torch.int32, device="cuda")})
    for f, _ in gpu.TABLE_RANGE_FIELDS:
        assert (res[f] == plain[f]).all(), f
    # rows
    positions = mvcc_rows_case(seed, two_level)[3][::ROW_STEP]
    ans = RowsModel(file, off, 5).answer(positions, (3, 37, 41))
    table5 = dict(table, global_seqno=5)
    d_pos = {k: v[::ROW_STEP].contiguous() for k, v in d_res.items()}
    g = run_rows(gpu, d_file, table5, positions, ans, view=view, d_pos=d_pos)
    p = run_rows(gpu, d_file, table5, positions, ans, block_off=view["stored_off"], d_pos=d_pos)
    for f in g:
        assert (g[f] == p[f]).all(), f
    assert ans["need"][1] >= 20_000


# ---------------------------------------------------------------- 2. the LZ4 twin, get
@pytest.mark.parametrize("seed,two_level", CASES)
def test_twin_get(gpu, seed, two_level):
    _, _, twin = twin_case(seed, two_level)
    model, queries, expected = twin_get_expected(seed, two_level)
    d_file = gpu.to_device_bytes(twin["file"])
    table = dict(twin, two_level=two_level, file_len=len(twin["file"]))
    view = gpu.table_frames(d_file, table)  # (the stored offsets from the index alone)
    assert view["stored_off"].cpu().tolist() == [int(o) for o in twin["block_off"]]
    assert view["n_blocks"] == twin["block_count"] and not view["status"].any().item()
    res = run_get(gpu, d_file, table, queries, view)
    outcomes = TG.compare(res, queries, expected)  # (block_off / block_size: the stored handle)
    assert outcomes[GET_HIT] > 600 and outcomes[GET_MISS] > 0 and outcomes[GET_NO_BLOCK] > 0
    check_blocks(res, expected, TR.ordinals(twin["block_off"]))
    view_h = host_view(view)
    assert check_values(res, expected, model, view_h) == outcomes[GET_HIT]


@pytest.mark.parametrize("hashes", [False, True])
@pytest.mark.parametrize("seed,two_level", [(1, True), (2, False)])
def test_twin_get_with_filter(gpu, seed, two_level, hashes):
    items, _, twin = twin_case(seed, two_level)
    file, flt = with_filter(twin, items)
    model = LZ4TableModel(file, twin["tli_off"], twin["tli_size"], two_level, filter=flt)
    queries = mvcc_queries(items, seed)[::2]
    expected = [model.lookup(k, s) for k, s in queries]
    d_file, table, view = twin_on_device(gpu, twin, two_level, file)
    res = run_get(gpu, d_file, table, queries, view, filter=flt, hashes=hashes)
    outcomes = TG.compare(res, queries, expected)
    assert outcomes[GET_FILTERED] > 0 and outcomes[GET_HIT] > 300
    check_blocks(res, expected, TR.ordinals(twin["block_off"]))


def test_twin_get_global_and_lowest_seqno(gpu):
    items, _, twin = twin_case(1, True)
    lowest = int(items.seqno.min())
    model = LZ4TableModel(twin["file"], twin["tli_off"], twin["tli_size"], True, lowest_seqno=lowest, global_seqno=7)
    queries = []
    for i in range(0, items.n, 3):
        k, s = item_key(items, i), int(items.seqno[i])
        queries += [(k, s + 8), (k, s + 7), (k, s + 1)]
    queries += [(item_key(items, 0), s) for s in (0, 1, 6, 7, 8, lowest + 6, lowest + 7, lowest + 8, TG.U64, 1 << 63)]
    expected = [model.lookup(k, s) for k, s in queries]
    d_file, table, view = twin_on_device(gpu, twin, True)
    res = run_get(gpu, d_file, table, queries, view, lowest_seqno=lowest, global_seqno=7)
    outcomes = TG.compare(res, queries, expected)
    assert outcomes[GET_SEQNO_SKIP] >= 6 and outcomes[GET_HIT] > 150
    assert check_values(res, expected, model, host_view(view)) == outcomes[GET_HIT]


# ---------------------------------------------------------------- 3. the LZ4 twin, range and rows
@pytest.mark.parametrize("seed,two_level", CASES)
def test_twin_range_and_rows(gpu, seed, two_level):
    import torch
    _, t, twin = twin_case(seed, two_level)
    queries, expected = twin_range_expected(seed, two_level)
    d_file, table, view = twin_on_device(gpu, twin, two_level)
    d_res, res = run_range(gpu, d_file, table, queries, view)
    outcomes = TR.compare(res, queries, expected, ordinal=TR.ordinals(twin["block_off"]))  # (the stored handles)
    assert outcomes[RANGE_ROWS] >= 600 and outcomes[RANGE_EMPTY] >= 50 and outcomes[RANGE_NO_BLOCK] >= 500
    # compression does not move the block cut: the plain call on the uncompressed original
    d_orig = gpu.to_device_bytes(t["file"])
    orig = dict(t, two_level=two_level, file_len=len(t["file"]))
    _, plain = run_range(gpu, d_orig, orig, queries, scan={"block_off": i64(t["block_off"]),
                         "item_start": torch.zeros(len(t["block_off"]), dtype=torch.int32, device="cuda")})
    for f in ("status", "outcome", "first_item", "last_item", "first_block", "last_block"):
        assert (res[f] == plain[f]).all(), f
    # the rows are the original's, byte for byte
    positions = positions_of(expected, twin["block_off"])[::ROW_STEP]
    assert positions == mvcc_rows_case(seed, two_level)[3][::ROW_STEP]
    ans = RowsModel(t["file"], t["block_off"], 5).answer(positions, (3, 37, 41))
    d_pos = {k: v[::ROW_STEP].contiguous() for k, v in d_res.items()}
    run_rows(gpu, d_file, dict(table, global_seqno=5), positions, ans, view=view, d_pos=d_pos)
    assert ans["need"][1] >= 20_000 and ans["need"][0] >= 1_000


# ---------------------------------------------------------------- 4. faults stay local
def _faulted(twin, b, fault):
    """The twin's file with data block b damaged, same length."""
    off = [int(o) for o in twin["block_off"]]
    blk = bytearray(twin["file"][off[b]:off[b + 1]])
    if fault == CKSUM:  # one stored payload byte flipped
        blk[33 + (len(blk) - 33) // 2] ^= 0x04
    elif fault == DECOMPRESS:  # a literal run longer than the stream, the checksum resealed
        blk[33:36] = b"\xff\xff\xff"
        raw = int.from_bytes(blk[25:29], "little")
        blk = pyoracle.block_header(0, bytes(blk[33:]), raw) + bytes(blk[33:])
    else:  # TYPE_MISMATCH: the header says Index
        blk = pyoracle.block_header(1, bytes(blk[33:]), int.from_bytes(blk[25:29], "little")) + bytes(blk[33:])
    assert len(blk) == off[b + 1] - off[b]
    return twin["file"][:off[b]] + bytes(blk) + twin["file"][off[b + 1]:]


@pytest.mark.parametrize("fault", [CKSUM, DECOMPRESS, TYPE_MISMATCH])
@pytest.mark.parametrize("two_level", [False, True])
def test_faults_stay_local(gpu, two_level, fault):
    items, _, twin = twin_case(1, two_level)
    b = twin["block_count"] // 2
    file = _faulted(twin, b, fault)
    d_file, table, view = twin_on_device(gpu, twin, two_level, file)
    status = view["status"].cpu().tolist()
    assert status == [0 if i != b or fault == TYPE_MISMATCH else fault for i in range(twin["block_count"])]
    # get
    _, queries, clean = twin_get_expected(1, two_level)
    queries, clean = queries[::2], clean[::2]
    model = LZ4TableModel(file, twin["tli_off"], twin["tli_size"], two_level)
    expected = [model.lookup(k, s) for k, s in queries]
    bad = [q for q, e in enumerate(expected) if e[0] != 0]
    assert bad and all(expected[q] == (fault, (GET_NONE, 0, 0, -1, 0, 0, 0, 0)) for q in bad)
    assert all(e == c for e, c in zip(expected, clean) if e[0] == 0) and len(bad) < len(queries) // 4
    TG.compare(run_get(gpu, d_file, table, queries, view), queries, expected)
    # range
    rq, rclean = twin_range_expected(1, two_level)
    rmodel = LZ4RangeModel(file, twin["tli_off"], twin["tli_size"], two_level)
    rexp = [rmodel.answer(*q) for q in rq]
    rbad = [q for q, e in enumerate(rexp) if e[0] != 0]
    assert rbad and all(rexp[q] == (fault, (RANGE_NONE, 0, 0, 0, 0, 0, 0)) for q in rbad)
    assert all(e == c for e, c in zip(rexp, rclean) if e[0] == 0)
    _, res = run_range(gpu, d_file, table, rq, view)
    TR.compare(res, rq, rexp, ordinal=TR.ordinals(twin["block_off"]))
    # rows, from the clean twin's positions: a run that touches block b is empty, the status is
    # that of the lowest-ordinal faulted block (there is one)
    positions = positions_of(rclean, twin["block_off"])[::ROW_STEP]
    ans = LZ4RowsModel(file, twin["block_off"], 5).answer(positions, (3, 37, 41))
    touched = [q for q, p in enumerate(positions) if p[1] == RANGE_ROWS and p[2] <= b <= p[4]]
    assert touched and all(ans["row_status"][q] == fault and ans["runs"][q] == [] for q in touched)
    assert sum(1 for s in ans["row_status"] if s) == len(touched)
    run_rows(gpu, d_file, dict(table, global_seqno=5), positions, ans, view=view)


# ---------------------------------------------------------------- 5. a wrong view
def _reaches_block(e):
    return e[1][0] in (GET_HIT, GET_MISS)


@pytest.mark.parametrize("wrong", ["other_table", "off_by_one", "frame_off_decreasing", "frames_len_short",
                                   "no_blocks"])
def test_wrong_view(gpu, wrong):
    """The view's own faults, against the model of the five steps over the same view."""
    import torch
    two_level = True
    _, t, twin = twin_case(2, two_level)
    d_file, table, view = twin_on_device(gpu, twin, two_level)
    nb = twin["block_count"]
    stored, frame_off = view["stored_off"].cpu().tolist(), view["frame_off"].cpu().tolist()
    change, hit_by = {}, None  # hit_by: the ordinals whose queries change (None: every data block)
    if wrong == "other_table":  # the uncompressed original's offsets: no handle is the twin's
        change["stored_off"] = [int(o) for o in t["block_off"]]
        assert not set(zip(change["stored_off"], change["stored_off"][1:])) & set(zip(stored, stored[1:]))
        want = BAD_ARG
    elif wrong == "off_by_one":
        k = nb // 2
        change["stored_off"] = stored[:k] + [stored[k] + 1] + stored[k + 1:]
        want, hit_by = BAD_ARG, {k - 1, k}
    elif wrong == "frame_off_decreasing":
        change["frame_off"] = frame_off[:nb] + [frame_off[nb - 1] - 1]
        want, hit_by = TRUNCATED, {nb - 1}
    elif wrong == "frames_len_short":  # (the tensor stays allocated)
        change["frames_len"] = view["frames_len"] - 1
        want, hit_by = TRUNCATED, {nb - 1}
    else:
        change["n_blocks"] = 0
        want = BAD_ARG
    bad_view = dict(view)
    for k, v in change.items():
        bad_view[k] = i64(v) if isinstance(v, list) else v
    view_h = host_view(view, **change)
    ordinal = TR.ordinals(twin["block_off"])
    # get
    _, queries, clean = twin_get_expected(2, two_level)
    queries, clean = queries[::2], clean[::2]
    model = FramesModel(view_h, twin["file"], twin["tli_off"], twin["tli_size"], two_level)
    expected = [model.lookup(k, s) for k, s in queries]
    for e, c in zip(expected, clean):
        if e != c:
            assert e == (want, (GET_NONE, 0, 0, -1, 0, 0, 0, 0)) and _reaches_block(c)
        elif hit_by is None:
            assert not _reaches_block(c)  # SEQNO_SKIP / FILTERED / NO_BLOCK queries are unchanged
        elif c[1][0] == GET_HIT:
            assert ordinal[c[1][1:3]] not in hit_by
    assert sum(e != c for e, c in zip(expected, clean)) >= 5
    TG.compare(run_get(gpu, d_file, table, queries, bad_view), queries, expected)
    # range
    rq, rclean = twin_range_expected(2, two_level)
    rq, rclean = rq[::2], rclean[::2]
    rmodel = FramesRangeModel(view_h, twin["file"], twin["tli_off"], twin["tli_size"], two_level)
    rexp = [rmodel.answer(*q) for q in rq]
    for e, c in zip(rexp, rclean):
        if e != c:
            assert e == (want, (RANGE_NONE, 0, 0, 0, 0, 0, 0)) and c[1][0] in (RANGE_ROWS, RANGE_EMPTY)
        elif hit_by is None:
            assert c[1][0] == RANGE_NO_BLOCK
    assert sum(e != c for e, c in zip(rexp, rclean)) >= 5
    _, res = run_range(gpu, d_file, table, rq, bad_view)
    TR.compare(res, rq, rexp, ordinal=ordinal)
    # rows (block b is frame b: stored_off is not read), from the clean positions
    positions = positions_of(rclean, twin["block_off"])[::ROW_STEP]
    ans = FramesRowsModel(view_h, 5).answer(positions, (3, 37, 41))
    clean_ans = LZ4RowsModel(twin["file"], twin["block_off"], 5).answer(positions, (3, 37, 41))
    if wrong in ("other_table", "off_by_one"):
        assert ans == clean_ans
    else:
        rows_want = BAD_ARG if wrong == "no_blocks" else TRUNCATED
        changed = [q for q in range(len(positions)) if ans["row_status"][q] != clean_ans["row_status"][q]]
        assert changed and all(ans["row_status"][q] == rows_want and ans["runs"][q] == [] for q in changed)
        assert all(positions[q][4] == nb - 1 for q in changed) or wrong == "no_blocks"
    run_rows(gpu, d_file, dict(table, global_seqno=5), positions, ans, view=bad_view)


def test_view_argument_errors(gpu):
    import torch
    _, _, twin = twin_case(1, False)
    d_file, table, view = twin_on_device(gpu, twin, False)
    queries = [(b"a", 1 << 62)]
    for field in ("stored_off", "frames", "frame_off"):
        with pytest.raises(gpu.LsmError, match="BAD_ARG"):
            run_get(gpu, d_file, table, queries, dict(view, **{field: None}))
        with pytest.raises(gpu.LsmError, match="BAD_ARG"):
            run_range(gpu, d_file, table, [(None, None, False, False)], dict(view, **{field: None}))
    with pytest.raises(gpu.LsmError, match="BAD_ARG"):
        run_get(gpu, d_file, table, queries, dict(view, frames=view["frames"][8:]))
    ans = {"end": [3, 37, 41], "need": [1, 1, 1, 1]}
    with pytest.raises(gpu.LsmError, match="BAD_ARG"):
        run_rows(gpu, d_file, table, [(0, RANGE_ROWS, 0, 0, 0, 0)], ans, view=dict(view, frame_off=None))
    with pytest.raises(gpu.LsmError, match="BAD_ARG"):
        run_rows(gpu, d_file, table, [(0, RANGE_ROWS, 0, 0, 0, 0)], ans, view=dict(view, frames=view["frames"][8:]))


# ---------------------------------------------------------------- 6. smallest shapes
def _check_table(gpu, items, t, two_level, queries, rq):
    """Get, range and rows of a small table's twin against the LZ4 models."""
    twin = lz4_twin(t, two_level)
    d_file, table, view = twin_on_device(gpu, twin, two_level)
    assert not view["status"].any().item()
    model = LZ4TableModel(twin["file"], twin["tli_off"], twin["tli_size"], two_level)
    expected = [model.lookup(k, s) for k, s in queries]
    res = run_get(gpu, d_file, table, queries, view)
    outcomes = TG.compare(res, queries, expected)
    ordinal = TR.ordinals(twin["block_off"])
    check_blocks(res, expected, ordinal)
    view_h = host_view(view)
    assert check_values(res, expected, model, view_h) == outcomes.get(GET_HIT, 0)
    residues = {view_h.frame_off[int(b)] % 16 for q, b in enumerate(res["block"]) if expected[q][1][0] == GET_HIT}
    rmodel = LZ4RangeModel(twin["file"], twin["tli_off"], twin["tli_size"], two_level)
    rexp = [rmodel.answer(*q) for q in rq]
    d_res, rres = run_range(gpu, d_file, table, rq, view)
    TR.compare(rres, rq, rexp, ordinal=ordinal)
    positions = positions_of(rexp, twin["block_off"])
    ans = RowsModel(t["file"], t["block_off"], 0).answer(positions, (3, 37, 41))
    run_rows(gpu, d_file, table, positions, ans, view=view, d_pos=d_res)
    return twin, outcomes, ans, residues


@pytest.mark.parametrize("two_level", [False, True])
def test_one_block_table(gpu, two_level):
    items = pyoracle.Items.from_list([(b"k%02d" % i, b"v" * i, 9, 0) for i in range(1, 20)])
    t = pyoracle.table_write(items, block_size=1 << 16, two_level=two_level)
    assert t["block_count"] == 1
    queries = [(b"a", 10), (b"k00", 10), (b"k19\0", 10), (b"z", 10), (b"", 10), (b"k05", 10), (b"k05", 9),
               (b"k055", 10), (b"k19", 10), (b"k01", 10)]
    rq = [(None, None, False, False), (b"", b"k05", False, True), (b"k05", b"k05", False, False),
          (b"k19", None, True, False), (b"z", None, False, False), (b"k03", b"k10", True, False)]
    _, outcomes, ans, _ = _check_table(gpu, items, t, two_level, queries, rq)
    assert outcomes[GET_HIT] == 3 and ans["need"][1] == 19 + 4 + 1 + 0 + 0 + 7


def test_incompressible_values(gpu):
    """Random values: the LZ4 stream is longer than the payload it stores."""
    rng = random.Random(77)
    rows = [(b"r%05d" % i, bytes(rng.getrandbits(8) for _ in range(500)), 50, 0) for i in range(120)]
    items = pyoracle.Items.from_list(rows)
    t = pyoracle.table_write(items, block_size=4096, two_level=True, partition_size=128)
    queries = [(r[0], 51) for r in rows] + [(b"", 51), (b"r00007x", 51), (b"s", 51)]
    rq = [(None, None, False, False), (b"r00010", b"r00050", False, False), (b"r00033", b"r00034", True, True),
          (b"", b"r00000", False, False)]
    twin, outcomes, ans, _ = _check_table(gpu, items, t, True, queries, rq)
    longer = sum(1 for (o, z), (_, nz) in twin["handle_map"].items() if nz > z)
    assert longer == twin["block_count"] >= 10 and outcomes[GET_HIT] == 120 and ans["need"][1] == 120 + 41 + 1


@pytest.mark.parametrize("two_level", [False, True])
def test_long_keys(gpu, two_level):
    """Keys longer than one 16-byte compare window (tests/long_key_cases.py), every seventh query.
    The batch's hits lie in frames on every residue mod 16 (the 33-byte headers see to that)."""
    _, t, _ = LK.table(two_level, False)
    twin, outcomes, _, residues = _check_table(gpu, LK.items(), t, two_level, LK.get_queries()[::7],
                                               LK.range_queries()[::7])
    assert twin["block_count"] >= 200 and outcomes[GET_HIT] >= 200 and residues == set(range(16))


# ---------------------------------------------------------------- 7. the device round trip
@pytest.mark.parametrize("two_level", [False, True])
def test_device_round_trip(gpu, two_level):
    """write_table(compression="lz4") -> table_frames -> a get of every item's key at seqno + 1."""
    items, _ = mvcc_table(2, two_level)
    wt = gpu.write_table(gpu.items_to_device(items), block_size=256, restart_interval=4, hash_ratio=1.33,
                         two_level=two_level, partition_size=128, compression="lz4")
    table = dict(wt, two_level=two_level, file_len=int(wt["file"].numel()))
    view = gpu.table_frames(wt["file"], table, block_off=wt["block_off"] if two_level else None)
    assert view["n_blocks"] == wt["block_count"] and not view["status"].any().item()
    queries = [(item_key(items, i), int(items.seqno[i]) + 1) for i in range(items.n)]
    res = run_get(gpu, wt["file"], table, queries, view)
    assert (res["status"] == 0).all() and (res["outcome"] == GET_HIT).all()
    v = host_view(view)
    stored = v.stored_off
    for i in range(items.n):
        b = int(res["block"][i])
        assert (int(res["block_off"][i]), int(res["block_size"][i])) == (stored[b], stored[b + 1] - stored[b])
        assert int(res["seqno"][i]) == int(items.seqno[i]) and int(res["vtype"][i]) == int(items.vtype[i])
        at = v.frame_off[b] + 33 + int(res["val_off"][i])
        want = b"" if int(items.vtype[i]) in (1, 2) else bytes(items.vals[int(items.val_off[i]):int(items.val_off[i + 1])])
        assert v.frames[at:at + int(res["val_len"][i])] == want, i


# ---------------------------------------------------------------- 8. the mixed read
def test_mixed_range_read(gpu):
    """range_read over tables that overlap in keys, the middle one LZ4, against the read with
    every table plain."""
    lists, qs = MR._tables(), MR._queries()
    plain, mixed = [], []
    for s, (items, gseq) in enumerate(zip(lists, MR.GLOBAL_SEQNOS)):
        d, _ = MR.to_device(gpu, [items])
        t = dict(gpu.write_table(d, block_size=4096), two_level=False, global_seqno=gseq)
        plain.append(t)
        if s == 1:
            z = dict(gpu.write_table(d, block_size=4096, compression="lz4"), two_level=False, global_seqno=gseq)
            z["frames"] = gpu.table_frames(z["file"], z, block_off=z["block_off"])
            assert z["block_count"] == t["block_count"] >= 3 and z["compression"] == "lz4"
            assert z["data_len"] != t["data_len"] and not z["frames"]["status"].any().item()
            t = z
        mixed.append(t)
    bounds = device_bounds(gpu, qs)
    want, wstatus = MR._rows_of(gpu.range_read(plain, *bounds, MR.PIPE_SNAP))
    got, status = MR._rows_of(gpu.range_read(mixed, *bounds, MR.PIPE_SNAP))
    assert status == wstatus == [0] * len(qs)
    assert got == want and sum(1 for w in want if w) >= 25


# ---------------------------------------------------------------- 9. graph capture
def test_framed_calls_in_one_graph(gpu):
    """Framed get + range + rows plan + rows captured on one stream and replayed."""
    import torch
    from test_gpu_graphs import _capture
    items, t, twin = twin_case(1, True)
    d_file, table, view = twin_on_device(gpu, twin, True)
    table = dict(table, global_seqno=5)
    _, queries, expected = twin_get_expected(1, True)
    queries, expected = queries[:600], expected[:600]
    rq, rexp = twin_range_expected(1, True)
    rq, rexp = rq[:200], rexp[:200]
    positions = positions_of(rexp, twin["block_off"])
    ans = RowsModel(t["file"], t["block_off"], 5).answer(positions, (0, 0, 0))
    needles = gpu.to_device_bytes(b"".join(q[0] for q in queries))
    noff = torch.from_numpy(np.concatenate([[0], np.cumsum([len(q[0]) for q in queries])]).astype(np.int64)).cuda()
    snaps = TG._i64(q[1] for q in queries)
    bounds = device_bounds(gpu, rq)
    n, m = len(queries), len(rq)
    get_out = {f: torch.zeros(n, dtype=getattr(torch, dt), device="cuda") for f, dt in gpu.TABLE_GET_FIELDS}
    get_out["block"] = torch.zeros(n, dtype=torch.int32, device="cuda")
    rng_out = {f: torch.zeros(m, dtype=getattr(torch, dt), device="cuda") for f, dt in gpu.TABLE_RANGE_FIELDS}
    into = RR.sentinel_items(ans["end"][0] + 3, ans["end"][1] + 29, ans["end"][2] + 31)
    base = torch.zeros(3, dtype=torch.int64, device="cuda")
    caps = (ans["need"][0], ans["need"][1], ans["end"][1], ans["end"][2])
    held = {}

    def step():
        gpu.table_get(d_file, table, needles, noff, snaps, out=get_out, frames=view)
        gpu.table_range(d_file, table, *bounds, out=rng_out, frames=view)
        held["rows"] = gpu.table_range_rows(d_file, table, rng_out, None, base=base, into=into, caps=caps,
                                            n_queries=m, frames=view)

    graph = _capture(step)
    for _ in range(2):
        for d in (get_out, rng_out, into, {k: held["rows"][k] for k in ("run_start", "row_status", "end", "need",
                                                                        "result", "plan_result")}):
            for k, v in d.items():
                v.fill_(TR.SENTINEL if d is rng_out or d is into else 0)
        graph.replay()
        torch.cuda.synchronize()
        TG.compare({k: v.cpu().numpy() for k, v in get_out.items()}, queries, expected)
        TR.compare({k: v.cpu().numpy() for k, v in rng_out.items()}, rq, rexp, ordinal=TR.ordinals(twin["block_off"]))
        g = RR.read(held["rows"])
        assert g["run_start"].tolist() == ans["run_start"] and g["row_status"].tolist() == ans["row_status"]
        assert g["end"].tolist() == ans["end"] and int(g["result"][0]) == 0
        flat = [r for run in ans["runs"] for r in run]
        assert g["keys"][:ans["end"][1]].tobytes() == b"".join(r[0] for r in flat)
        assert g["vals"][:ans["end"][2]].tobytes() == b"".join(r[1] for r in flat)
