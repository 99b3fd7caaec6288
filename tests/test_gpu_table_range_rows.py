"""GPU parity of lsm_table_range_rows_plan / lsm_table_range_rows (the rows of batched
Table::range as item runs) against tests/table_range_rows_model.py, never against the library
itself.  Bar: keys, values, both offset arrays, seqno, vtype, run_start, row_status, end and need
are bit-exact, and no output byte outside [base, end) differs from the sentinel it held."""
import random

import numpy as np
import pytest

import merge_model
import pyoracle
from helpers import counter_items
from table_get_model import index_block, item_key, reseal_header
from table_range_model import RANGE_EMPTY, RANGE_NO_BLOCK, RANGE_ROWS, RangeModel, brute_force, flags_of
from table_range_rows_model import BAD_ARG, OVERFLOW, RowsModel, item_rows, mvcc_rows_case, positions_of

pytestmark = pytest.mark.gpu

SENT = 0x5A
SENT64 = 0x5A5A5A5A5A5A5A5A
POS_FIELDS = (("status", "int32"), ("outcome", "uint8"), ("first_block", "int32"), ("first_item", "int32"),
              ("last_block", "int32"), ("last_item", "int32"))
ROWS = RANGE_ROWS


def device_positions(positions):
    """[(status, outcome, first_block, first_item, last_block, last_item)] -> the dict table_range returns."""
    import torch
    cols = list(zip(*positions)) if positions else [[]] * 6
    return {f: torch.from_numpy(np.array([c & 0xFFFFFFFF for c in col], np.uint32 if dt == "int32" else np.uint8)
                                .view(getattr(np, dt))).cuda() if positions
            else torch.zeros(1, dtype=getattr(torch, dt), device="cuda") for (f, dt), col in zip(POS_FIELDS, cols)}


def sentinel_items(item_cap, key_cap, val_cap):
    """An items dict as table_range_rows appends to, every byte a sentinel."""
    import torch
    pad = 64
    return {"keys": torch.full((key_cap + pad,), SENT, dtype=torch.uint8, device="cuda"),
            "vals": torch.full((val_cap + pad,), SENT, dtype=torch.uint8, device="cuda"),
            "key_off": torch.full((item_cap + 1,), SENT64, dtype=torch.int64, device="cuda"),
            "val_off": torch.full((item_cap + 1,), SENT64, dtype=torch.int64, device="cuda"),
            "seqno": torch.full((max(item_cap, 1),), SENT64, dtype=torch.int64, device="cuda"),
            "vtype": torch.full((max(item_cap, 1),), SENT, dtype=torch.uint8, device="cuda")}


def read(res):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def assert_untouched(g, lo=None, hi=None):
    """Nothing outside rows [lo[0], hi[0]), key bytes [lo[1], hi[1]), value bytes [lo[2], hi[2])
    and offset entries [lo[0], hi[0]] differs from its sentinel; without lo / hi: nothing at all."""
    def outside(a, a0, a1):
        return np.concatenate([a[:a0], a[a1:]])
    closing = 0 if lo is None else 1
    lo, hi = lo or (0, 0, 0), hi or (0, 0, 0)
    assert (outside(g["keys"], lo[1], hi[1]) == SENT).all() and (outside(g["vals"], lo[2], hi[2]) == SENT).all()
    assert (outside(g["seqno"], lo[0], hi[0]) == SENT64).all() and (outside(g["vtype"], lo[0], hi[0]) == SENT).all()
    for f in ("key_off", "val_off"):
        assert (outside(g[f], lo[0], hi[0] + closing) == SENT64).all(), f


def assert_rows(g, ans, base):
    """Every output of a call against the model's answer (computed for the same base)."""
    b0, b1, b2 = base
    e0, e1, e2 = ans["end"]
    assert int(g["plan_result"][0]) == 0 and int(g["result"][0]) == 0
    assert g["need"].tolist() == ans["need"] and g["end"].tolist() == ans["end"]
    assert g["run_start"].tolist() == ans["run_start"]
    assert g["row_status"].tolist() == ans["row_status"]
    flat = [r for run in ans["runs"] for r in run]
    assert len(flat) == e0 - b0
    key_off = np.cumsum([b1] + [len(r[0]) for r in flat])
    val_off = np.cumsum([b2] + [len(r[1]) for r in flat])
    assert (g["key_off"][b0:e0 + 1] == key_off).all() and (g["val_off"][b0:e0 + 1] == val_off).all()
    assert g["keys"][b1:e1].tobytes() == b"".join(r[0] for r in flat)
    assert g["vals"][b2:e2].tobytes() == b"".join(r[1] for r in flat)
    assert (g["seqno"][b0:e0].view(np.uint64) == np.array([r[2] for r in flat], np.uint64)).all()
    assert (g["vtype"][b0:e0] == np.array([r[3] for r in flat], np.uint8)).all()
    assert_untouched(g, (b0, b1, b2), (e0, e1, e2))


def setup(gpu, file, block_off, global_seqno=0):
    """-> (padded device file, the table dict of the wrappers, device offsets)."""
    import torch
    table = {"tli_off": 0, "tli_size": 33, "two_level": False, "file_len": len(file), "global_seqno": global_seqno}
    return gpu.to_device_bytes(file), table, torch.from_numpy(np.asarray(block_off, np.int64)).cuda()


def run_and_check(gpu, file, block_off, positions, base=(3, 37, 41), global_seqno=0, d_pos=None):
    """One call on sentinel outputs with caps taken from the model's need, everything compared."""
    import torch
    ans = RowsModel(file, block_off, global_seqno).answer(positions, base)
    d_file, table, d_off = setup(gpu, file, block_off, global_seqno)
    into = sentinel_items(ans["end"][0] + 3, ans["end"][1] + 29, ans["end"][2] + 31)
    res = gpu.table_range_rows(d_file, table, d_pos or device_positions(positions), d_off,
                               base=torch.tensor(base, dtype=torch.int64, device="cuda"), into=into,
                               caps=(ans["need"][0], ans["need"][1], ans["end"][1], ans["end"][2]),
                               n_queries=len(positions))
    assert_rows(read(res), ans, base)
    return ans


# ---- 1. the four MVCC tables
@pytest.mark.parametrize("global_seqno", [5, 2 ** 64 - 3])
@pytest.mark.parametrize("two_level", [False, True])
@pytest.mark.parametrize("seed", [1, 2])
def test_rows_mvcc_tables(gpu, seed, two_level, global_seqno):
    """All 1,500 queries: table_range gives the positions, table_block_offsets the offsets."""
    import torch
    items, t, queries, positions = mvcc_rows_case(seed, two_level)
    d_file = gpu.to_device_bytes(t["file"])
    table = dict(t, file_len=len(t["file"]), global_seqno=global_seqno)
    d_off = gpu.table_block_offsets(d_file, table)
    assert d_off.cpu().numpy().tolist() == [int(o) for o in t["block_off"]]

    def arena(which):
        parts = [q[which] or b"" for q in queries]
        off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
        return gpu.to_device_bytes(b"".join(parts)), torch.from_numpy(off).cuda()

    (lo, lo_off), (hi, hi_off) = arena(0), arena(1)
    flags = torch.tensor([flags_of(*q) for q in queries], dtype=torch.uint8).cuda()
    d_pos = gpu.table_range(d_file, table, lo, lo_off, hi, hi_off, flags, scan={"block_off": d_off,
                            "item_start": torch.from_numpy(np.asarray(t["starts"], np.int32)).cuda()})
    ans = run_and_check(gpu, t["file"], t["block_off"], positions, global_seqno=global_seqno, d_pos=d_pos)
    keys = [item_key(items, i) for i in range(items.n)]
    rows = item_rows(items, global_seqno)
    for q in (0, 1, 700, 1499):  # (the model itself is checked on every query by the CPU test)
        assert ans["runs"][q] == [rows[i] for i in brute_force(keys, *queries[q])]
    assert ans["need"][1] >= 150_000 and ans["need"][0] >= 7_000


# ---- 2. record shapes
def _rng_val(rng, n):
    return bytes(rng.getrandbits(8) for _ in range(n))


def _shape_items(shape):
    rng = random.Random(len(shape))
    if shape == "interval1":  # 200 items, one block, restart interval 1: more intervals than a group is wide
        rows = [(b"k%05d" % i, _rng_val(rng, i % 7), 1000 - i, 0) for i in range(200)]
        return rows, dict(block_size=1 << 20, restart_interval=1)
    if shape == "interval16":
        rows = [(b"key-%06d" % i, _rng_val(rng, 20 + i % 50), 7, 0) for i in range(700)]
        return rows, dict(block_size=4096, restart_interval=16)
    if shape == "one_item_blocks":
        rows = [(b"solo%04d" % i, _rng_val(rng, 9), i, 0) for i in range(90)]
        return rows, dict(block_size=1, restart_interval=16)
    if shape == "long_prefix":  # 300-byte keys, 280 shared: the prefix is at least 256 bytes
        rows = [(b"P" * 280 + b"%020d" % i, _rng_val(rng, 5), 3, 0) for i in range(120)]
        return rows, dict(block_size=8192, restart_interval=16)
    if shape == "values":  # 0, 255, 256 and 20,000 bytes, tombstones between
        sizes = [0, 255, 256, 20000, 1, 256, 0, 255, 300, 20000, 17]
        rows = []
        for i in range(66):
            vt = (0, 1, 0, 2, 0, 4)[i % 6]
            rows.append((b"v%04d" % i, b"" if vt in (1, 2) else _rng_val(rng, sizes[i % len(sizes)]), 50 + i, vt))
        return rows, dict(block_size=32768, restart_interval=4)
    if shape == "cursor_path":  # seqnos >= 2^49 and keys of 128 bytes or more leave the fast parse
        rows = [(b"%04d" % (i // 3) + b"x" * (124 + i % 40), _rng_val(rng, 30), (1 << 62) - i, 0) for i in range(150)]
        return rows, dict(block_size=4096, restart_interval=16)
    raise AssertionError(shape)


@pytest.mark.parametrize("shape", ["interval1", "interval16", "one_item_blocks", "long_prefix", "values",
                                   "cursor_path"])
def test_rows_record_shapes(gpu, shape):
    rows, kw = _shape_items(shape)
    rows = sorted(rows, key=lambda r: (r[0], -r[2]))
    items = pyoracle.Items.from_list(rows)
    t = pyoracle.table_write(items, **kw)
    starts = [int(s) for s in t["starts"]]
    nb, ri = t["block_count"], kw["restart_interval"]
    count = [starts[b + 1] - starts[b] for b in range(nb)]
    if shape == "interval1":
        assert nb == 1 and count[0] == 200
    rng = random.Random(nb)
    positions = [(0, ROWS, 0, 0, nb - 1, count[-1] - 1)]  # unbounded
    for _ in range(40):  # a single row
        b = rng.randrange(nb)
        i = rng.randrange(count[b])
        positions.append((0, ROWS, b, i, b, i))
    for _ in range(60):  # edges on and off restart heads
        fb = rng.randrange(nb)
        lb = min(nb - 1, fb + rng.choice([0, 0, 1, 2, 5]))
        fi, li = rng.randrange(count[fb]), rng.randrange(count[lb])
        if rng.random() < 0.4:
            fi -= fi % ri
        if rng.random() < 0.3:
            li = min(count[lb] - 1, li - li % ri + ri - 1)
        if fb == lb and fi > li:
            fi, li = li, fi
        positions.append((0, ROWS, fb, fi, lb, li))
    positions += [(0, RANGE_EMPTY, 0, 0, 0, 0), (0, RANGE_NO_BLOCK, 9, 9, 9, 9), (5, 0, 0, 0, 0, 0)]
    ans = run_and_check(gpu, t["file"], t["block_off"], positions)
    want = [(k, b"" if vt in (1, 2) else v, s, vt) for k, v, s, vt in rows]
    assert ans["runs"][0] == want and ans["row_status"][-1] == 5
    for pos, run in zip(positions[1:101], ans["runs"][1:101]):
        assert run == want[starts[pos[2]] + pos[3]:starts[pos[4]] + pos[5] + 1]


# ---- 3. one fault per file, in a block strictly between the two rows; positions that do not fit
def _five_blocks():
    items = counter_items(100, key_len=8, val_len=20, seed=4)
    blocks = [pyoracle.block_write(pyoracle.data_block_encode(pyoracle.Items.from_list(
        [(item_key(items, i), b"v" * 20, 63, 0) for i in range(b, b + 20)]), restart_interval=4))
        for b in range(0, 100, 20)]
    return blocks


def _fault(kind, blocks):
    """Damages block 2 (or the offsets) -> (blocks, offsets' last entry delta, expected status)."""
    b = bytearray(blocks[2])
    if kind == "magic":
        b[1] ^= 0x20
        return bytes(b), 0, 1
    if kind == "index_block":
        return index_block([(b"zz", 1, 0, 100)]), 0, 7
    if kind == "compressed":  # resealed with uncompressed_length != data_length
        payload = bytes(b[33:])
        return pyoracle.block_header(0, payload, len(payload) + 5) + payload, 0, 9
    if kind == "record":  # the seventh record's value claims 127 bytes: the records no longer end at the marker
        n, p = pyoracle.data_block_decode(bytes(b[33:]))
        assert n == 20 and b[33 + int(p["val_off"][7]) - 1] == 20
        b[33 + int(p["val_off"][7]) - 1] = 127
        return bytes(b), 0, 5
    if kind == "offsets":
        return bytes(b), 1000, 8
    raise AssertionError(kind)


@pytest.mark.parametrize("kind", ["magic", "index_block", "compressed", "record", "offsets"])
def test_rows_fault_between_the_rows(gpu, kind):
    blocks = _five_blocks()
    damaged, delta, status = _fault(kind, blocks)
    faulted = 4 if kind == "offsets" else 2
    blocks[2] = damaged
    file = b"".join(blocks)
    off = np.concatenate([[0], np.cumsum([len(x) for x in blocks])]).astype(np.int64)
    off[-1] += delta
    positions = [(0, ROWS, 0, 3, 4 if kind != "offsets" else 3, 11), (0, ROWS, 1, 0, 3, 19), (0, ROWS, 0, 0, 1, 19),
                 (0, ROWS, 3, 2, 3, 17), (0, ROWS, 0, 5, 4, 2), (0, ROWS, 1, 7, 4, 0), (0, ROWS, 3, 0, 4, 19),
                 (0, ROWS, 0, 0, 0, 0),
                 (0, ROWS, 0, 20, 1, 3), (0, ROWS, 0, 0, 1, 20), (0, ROWS, 3, 9, 3, 8),   # an item past the count
                 (0, ROWS, 3, 0, 1, 0), (0, ROWS, 0, 0, 5, 0), (0, ROWS, 7, 0, 7, 0)]     # ordinals that do not fit
    ans = run_and_check(gpu, file, off, positions)
    touches = [p[2] <= faulted <= p[4] for p in positions[:8]]
    assert 2 <= sum(touches) < 8
    assert ans["row_status"][:8] == [status if hit else 0 for hit in touches]
    assert [len(r) > 0 for r in ans["runs"][:8]] == [not hit for hit in touches]
    assert ans["row_status"][8:] == [BAD_ARG] * 6 and not any(ans["runs"][8:])


# ---- 4. caps
def test_rows_caps(gpu):
    import torch
    items, t, queries, positions = mvcc_rows_case(1, True)
    positions = positions[:300] + [(7, 0, 0, 0, 0, 0)]  # (ROWS, EMPTY and NO_BLOCK queries, and a failed one)
    assert {p[1] for p in positions} >= {RANGE_ROWS, RANGE_EMPTY, RANGE_NO_BLOCK}
    base = (2, 10, 20)
    ans = RowsModel(t["file"], t["block_off"], 9).answer(positions, base)
    assert all(not r for p, r in zip(positions, ans["runs"]) if p[1] != RANGE_ROWS) and ans["row_status"][-1] == 7
    d_file, table, d_off = setup(gpu, t["file"], t["block_off"], 9)
    d_pos = device_positions(positions)
    d_base = torch.tensor(base, dtype=torch.int64, device="cuda")
    pairs, rows, kb, vb = ans["need"]
    e0, e1, e2 = ans["end"]
    good = (pairs, rows, e1, e2, e0)  # (pairs, rows, key bytes, value bytes, items): capacities of the outputs

    def call(caps):
        into = sentinel_items(e0 + 3, e1 + 29, e2 + 31)
        return read(gpu.table_range_rows(d_file, table, d_pos, d_off, base=d_base, into=into, caps=caps))

    for k, name in enumerate(("block_cap", "row_cap", "key_cap", "val_cap", "out_item_cap")):
        caps = tuple(c - (i == k) for i, c in enumerate(good))
        g = call(caps)
        assert int(g["result"][0]) == OVERFLOW, name
        assert_untouched(g)
        assert int(g["plan_result"][0]) == (OVERFLOW if k < 2 else 0), name
        if k == 0:  # only the pair count is meaningful; the cursor does not move, every run is empty
            assert int(g["need"][0]) == pairs and g["end"].tolist() == list(base)
            assert g["run_start"].tolist() == [base[0]] * (len(positions) + 1)
        else:
            assert g["need"].tolist() == ans["need"] and g["end"].tolist() == ans["end"]
            assert g["run_start"].tolist() == ans["run_start"]
    need = [int(x) for x in g["need"]]  # caps taken from need: the call succeeds
    g = call((need[0], need[1], base[1] + need[2], base[2] + need[3], base[0] + need[1]))
    assert_rows(g, ans, base)


def test_rows_no_queries(gpu):
    import torch
    _, t, _, _ = mvcc_rows_case(1, False)
    d_file, table, d_off = setup(gpu, t["file"], t["block_off"])
    base = (4, 5, 6)
    into = sentinel_items(8, 16, 16)
    g = read(gpu.table_range_rows(d_file, table, device_positions([]), d_off,
                                  base=torch.tensor(base, dtype=torch.int64, device="cuda"), into=into,
                                  caps=(0, 0, 16, 16), n_queries=0))
    assert int(g["result"][0]) == 0 and int(g["plan_result"][0]) == 0
    assert g["end"].tolist() == list(base) and g["need"].tolist() == [0] * 4 and g["run_start"].tolist() == [4]
    assert_untouched(g)


def test_rows_sized_by_read_back(gpu):
    """caps=None: the wrapper sizes the outputs from need; the trimmed items are the rows."""
    _, t, _, positions = mvcc_rows_case(2, False)
    positions = positions[:200]
    ans = RowsModel(t["file"], t["block_off"], 0).answer(positions)
    d_file, table, d_off = setup(gpu, t["file"], t["block_off"])
    g = read(gpu.table_range_rows(d_file, table, device_positions(positions), d_off))
    flat = [r for run in ans["runs"] for r in run]
    assert int(g["result"][0]) == 0 and g["need"].tolist() == ans["need"] and len(g["seqno"]) == len(flat)
    assert g["run_start"].tolist() == ans["run_start"] and len(g["key_off"]) == len(flat) + 1
    assert g["keys"][:ans["end"][1]].tobytes() == b"".join(r[0] for r in flat)
    assert g["vals"][:ans["end"][2]].tobytes() == b"".join(r[1] for r in flat)
    assert g["seqno"].view(np.uint64).tolist() == [r[2] for r in flat]


# ---- 5. cursor and pipeline: one range over two tables, then the merge
def test_rows_two_tables_then_merge(gpu):
    import torch
    bounds = (b"ab", b"c", False, True)
    runs, calls = [], []
    for seed in (1, 2):
        items, t = mvcc_rows_case(seed, True)[:2]
        model = RangeModel(t["file"], t["tli_off"], t["tli_size"], True)
        positions = positions_of([model.answer(*bounds)], t["block_off"])
        assert positions[0][1] == RANGE_ROWS and positions[0][4] - positions[0][2] >= 2
        keys = [item_key(items, i) for i in range(items.n)]
        rows = item_rows(items)
        runs.append([rows[i] for i in brute_force(keys, *bounds)])
        calls.append((t, positions))
    total = [sum(len(r) for r in runs), sum(len(x[0]) for r in runs for x in r), sum(len(x[1]) for r in runs for x in r)]
    into = sentinel_items(total[0], total[1], total[2])
    cursor = torch.zeros(3, dtype=torch.int64, device="cuda")
    starts = [0]
    for (t, positions), run in zip(calls, runs):
        d_file, table, d_off = setup(gpu, t["file"], t["block_off"])
        res = gpu.table_range_rows(d_file, table, device_positions(positions), d_off, base=cursor, into=into,
                                   caps=(64, len(run), total[1], total[2]))
        cursor = res["end"]
        g = read(res)
        assert int(g["result"][0]) == 0 and g["run_start"].tolist() == [starts[-1], starts[-1] + len(run)]
        starts.append(starts[-1] + len(run))
    assert cursor.cpu().tolist() == total
    merged = gpu.merge_runs({f: into[f] for f in ("keys", "key_off", "vals", "val_off", "seqno", "vtype")}, starts)
    torch.cuda.synchronize()
    want, _, _ = merge_model.merge_runs(runs)
    n_out = int(merged["n_out"].cpu()[0])
    assert merged["status"].cpu().tolist()[:2] == [0, 0] and n_out == len(want)
    ko, vo = merged["key_off"].cpu().numpy(), merged["val_off"].cpu().numpy()
    keys, vals = merged["keys"].cpu().numpy().tobytes(), merged["vals"].cpu().numpy().tobytes()
    seq, vt = merged["seqno"].cpu().numpy().view(np.uint64), merged["vtype"].cpu().numpy()
    got = [(keys[ko[j]:ko[j + 1]], vals[vo[j]:vo[j + 1]], int(seq[j]), int(vt[j])) for j in range(n_out)]
    assert got == want


# ---- 6. graph: table_range + plan + rows captured on one stream, replayed after the bounds changed in place
def test_rows_graph_replay(gpu):
    import torch
    items, t, queries, _ = mvcc_rows_case(2, True)
    sets = [queries[:64], queries[64:128]]
    d_file = gpu.to_device_bytes(t["file"])
    table = dict(t, file_len=len(t["file"]), global_seqno=11)
    d_off = torch.from_numpy(np.asarray(t["block_off"], np.int64)).cuda()
    scan = {"block_off": d_off, "item_start": torch.from_numpy(np.asarray(t["starts"], np.int32)).cuda()}
    model = RangeModel(t["file"], t["tli_off"], t["tli_size"], True)
    answers = [RowsModel(t["file"], t["block_off"], 11).answer(
        positions_of([model.answer(*q) for q in qs], t["block_off"])) for qs in sets]
    caps = tuple(max(a["need"][k] for a in answers) + 1 for k in range(4))

    def bounds(qs):
        out = []
        for which in (0, 1):
            parts = [q[which] or b"" for q in qs]
            out += [np.frombuffer(b"".join(parts).ljust(512, b"\0"), np.uint8),
                    np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)]
        return out + [np.array([flags_of(*q) for q in qs], np.uint8)]

    bound = [torch.from_numpy(a.copy()).cuda() for a in bounds(sets[0])]
    bound[0], bound[2] = gpu.to_device_bytes(bound[0].cpu().numpy()), gpu.to_device_bytes(bound[2].cpu().numpy())
    pos = {f: torch.zeros(64, dtype=getattr(torch, dt), device="cuda") for f, dt in gpu.TABLE_RANGE_FIELDS}
    into = sentinel_items(caps[1] + 2, caps[2] + 8, caps[3] + 8)
    held = {}

    def step():
        gpu.table_range(d_file, table, bound[0], bound[1], bound[2], bound[3], bound[4], scan=scan, out=pos)
        held["res"] = gpu.table_range_rows(d_file, table, pos, d_off, into=into, caps=caps)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for which in (0, 1, 0):
        for dst, src in zip(bound, bounds(sets[which])):
            dst[:len(src)].copy_(torch.from_numpy(src.copy()))
        for v in into.values():
            v.fill_(SENT if v.dtype == torch.uint8 else SENT64)
        graph.replay()
        assert_rows(read(dict(into, **{k: held["res"][k] for k in ("run_start", "row_status", "end", "need",
                                                                   "result", "plan_result")})),
                    answers[which], (0, 0, 0))
