"""lsm_merge_read on the device against tests/merge_read_model.py, straight through the C ABI
with caller-owned outputs that start as sentinels: offsets, arenas, seqno, vtype, src,
group_start and status are compared exactly, and every byte, row and offset entry past the
defined extents must still hold the sentinel.  Then the pipeline: write_table -> range_read
(table_range -> table_range_rows -> merge_read) against a brute-force dict over the raw items."""
import ctypes as C
import random

import numpy as np
import pytest

import merge_read_cases as Cs
import merge_read_model as R
from merge_gpu import capture, to_device
from table_range_model import brute_force, flags_of

pytestmark = pytest.mark.gpu

SENT = 0xA5
OUT_FIELDS = ("keys", "key_off", "vals", "val_off", "seqno", "vtype", "src", "group_start", "status")
VIEWS = {"key_off": np.uint64, "val_off": np.uint64, "seqno": np.uint64, "src": np.uint32, "group_start": np.uint64,
         "status": np.int32}


def sizes_of(runs):
    flat = [it for src in runs for run in src for it in run]
    return len(flat), sum(len(it[0]) for it in flat), sum(len(it[1]) for it in flat)


def alloc_outputs(n, key_bytes, val_bytes, n_groups, key_skew=0, val_skew=0, fill=SENT):
    """Caller-owned outputs sized as include/lsmgpu.h asks, every byte `fill`; skew: the arena
    starts that many bytes into its allocation."""
    import torch
    sizes = {"keys": key_bytes + 64 + key_skew, "vals": val_bytes + 64 + val_skew, "key_off": 8 * (n + 1),
             "val_off": 8 * (n + 1), "seqno": 8 * max(n, 1), "vtype": max(n, 1), "src": 4 * max(n, 1),
             "group_start": 8 * (n_groups + 1), "status": 4 * max(n_groups, 1)}
    out = {f: torch.full((sizes[f],), fill, dtype=torch.uint8, device="cuda") for f in OUT_FIELDS}
    out["keys"], out["vals"] = out["keys"][key_skew:], out["vals"][val_skew:]
    return out


class ReadCall:
    """One lsm_merge_read call with every argument fixed: launch() only goes through ctypes."""

    def __init__(self, L, d, run_start, n_groups, n_sources, out, ws, snapshot, group_seqno=None, in_status=None,
                 keep=False, with_src=True):
        import torch
        self.L = L
        self.it = L.LsmItems()
        self.held = [d, run_start, out, ws, group_seqno, in_status]
        for f in ("keys", "key_off", "vals", "val_off", "seqno", "vtype"):
            t = d[f]
            if t.numel() == 0:
                t = torch.zeros(1, dtype=t.dtype, device="cuda")
                self.held.append(t)
            setattr(self.it, f, t.data_ptr())
        self.it.n_items = d["seqno"].numel()
        assert ws.numel() >= L.lib().lsm_merge_read_workspace_size(self.it.n_items, n_groups, n_sources)
        assert ws.data_ptr() % 256 == 0
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        self.args = (C.byref(self.it), p(run_start), n_groups, n_sources, snapshot & (2 ** 64 - 1), p(group_seqno),
                     p(in_status), L.MERGE_READ_KEEP_TOMBSTONES if keep else 0, p(out["keys"]), p(out["key_off"]),
                     p(out["vals"]), p(out["val_off"]), p(out["seqno"]), p(out["vtype"]),
                     p(out["src"]) if with_src else None, p(out["group_start"]), p(out["status"]), p(ws), ws.numel())

    def launch(self, stream=None):
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        rc = self.L.lib().lsm_merge_read(*self.args, C.c_void_p(s.cuda_stream))
        assert rc == 0, rc


def read_outputs(out):
    g = {f: out[f].cpu().numpy() for f in OUT_FIELDS}
    return {f: g[f].view(VIEWS[f]) if f in VIEWS else g[f] for f in OUT_FIELDS}


def assert_answer(g, ans, with_src=True, fill=SENT):
    """Every output against the model's answer, and nothing stored past the defined extents."""
    word = int.from_bytes(bytes([fill]) * 8, "little")
    items, total = ans["items"], len(ans["items"])
    assert g["status"].tolist() == ans["status"]
    assert g["group_start"].tolist() == ans["group_start"]
    key_off = np.cumsum([0] + [len(it[0]) for it in items])
    val_off = np.cumsum([0] + [len(it[1]) for it in items])
    assert (g["key_off"][:total + 1] == key_off).all() and (g["val_off"][:total + 1] == val_off).all()
    kt, vt = int(key_off[-1]), int(val_off[-1])
    assert g["keys"][:kt].tobytes() == b"".join(it[0] for it in items)
    assert g["vals"][:vt].tobytes() == b"".join(it[1] for it in items)
    assert g["seqno"][:total].tolist() == [it[2] for it in items]
    assert g["vtype"][:total].tolist() == [it[3] for it in items]
    assert g["src"][:total if with_src else 0].tolist() == (ans["src"] if with_src else [])
    assert (g["keys"][kt:] == fill).all() and (g["vals"][vt:] == fill).all()
    assert (g["key_off"][total + 1:] == word).all() and (g["val_off"][total + 1:] == word).all()
    assert (g["seqno"][total:] == word).all() and (g["vtype"][total:] == fill).all()
    assert (g["src"][total if with_src else 0:] == word & 0xFFFFFFFF).all()


def run_call(L, runs, snapshot=Cs.SNAP, keep=False, group_seqno=None, in_status=None, run_start=None, ws=None,
             with_src=True, skews=(0, 0, 0, 0), fill=SENT):
    """One call on fresh sentinel outputs; returns read_outputs()."""
    import torch
    n_src, n_groups = len(runs), len(runs[0])
    d, rs = to_device(L, R.flat_runs(runs), skews[0], skews[1])
    n, kb, vb = sizes_of(runs)
    out = alloc_outputs(n, kb, vb, n_groups, skews[2], skews[3], fill)
    if ws is None:
        ws = torch.zeros(L.lib().lsm_merge_read_workspace_size(n, n_groups, n_src), dtype=torch.uint8, device="cuda")
    d_rs = torch.tensor(rs if run_start is None else run_start, dtype=torch.int64, device="cuda")
    d_gs = None if group_seqno is None else torch.from_numpy(np.array(group_seqno, np.uint64).view(np.int64)).cuda()
    d_st = None if in_status is None else torch.tensor(in_status, dtype=torch.int32, device="cuda")
    ReadCall(L, d, d_rs, n_groups, n_src, out, ws, snapshot, d_gs, d_st, keep, with_src).launch()
    torch.cuda.synchronize()
    return read_outputs(out)


@pytest.fixture(scope="module")
def mid():
    """The 3 x 65 case and its answer at the case's snapshot, shared and left unchanged."""
    runs = Cs.grouped_case(3, 65)
    return runs, R.merge_read(runs, Cs.SNAP)


# ---- 1. every case of merge_read_cases.py, both flag values
@pytest.mark.parametrize("keep", [False, True], ids=["drop-tombstones", "keep-tombstones"])
@pytest.mark.parametrize("shape", Cs.SHAPES, ids=["%dx%d" % s for s in Cs.SHAPES])
def test_cases(gpu, shape, keep):
    runs = Cs.grouped_case(*shape)
    ans = R.merge_read(runs, Cs.SNAP, keep)
    assert 0 < len(ans["items"])
    assert_answer(run_call(gpu, runs, keep=keep), ans)


# ---- 2. snapshots
def test_snapshot_zero_and_max(gpu, mid):
    runs, _ = mid
    nothing = R.merge_read(runs, 0)
    assert nothing["items"] == [] and nothing["group_start"] == [0] * 66
    assert_answer(run_call(gpu, runs, snapshot=0), nothing)
    for keep in (False, True):
        everything = R.merge_read(runs, 2 ** 64 - 1, keep)
        assert any(it[2] >= 2 ** 63 for it in everything["items"])
        assert_answer(run_call(gpu, runs, snapshot=2 ** 64 - 1, keep=keep), everything)


def test_group_seqno(gpu, mid):
    """A snapshot per group (the scalar is then ignored), from below to above the seqno range."""
    runs, _ = mid
    gs = [Cs.SNAP - 9 + (5 * g) % 19 for g in range(65)]
    ans = R.merge_read(runs, 0, group_seqno=gs)
    assert len({ans["group_start"][g + 1] - ans["group_start"][g] for g in range(65)}) > 3
    assert ans != R.merge_read(runs, Cs.SNAP)
    assert_answer(run_call(gpu, runs, snapshot=0, group_seqno=gs), ans)


# ---- 3. per-group faults
def test_unsorted_group(gpu, mid):
    runs, good = mid
    b = Cs.group_between_neighbours(runs, good["group_start"])
    bad, _ = Cs.unsorted_group(runs, b)
    ans = R.merge_read(bad, Cs.SNAP)
    assert ans["status"] == [0] * b + [10] + [0] * (64 - b)
    assert_answer(run_call(gpu, bad), ans)


def test_in_status(gpu, mid):
    runs, good = mid
    b = Cs.group_between_neighbours(runs, good["group_start"])
    st = [0] * (3 * 65)
    st[1 * 65 + b] = 5            # one source of one group
    st[2 * 65 + b + 1] = 8        # two sources of the next: the lowest source's entry
    st[1 * 65 + b + 1] = 4
    ans = R.merge_read(runs, Cs.SNAP, in_status=st)
    assert ans["status"][b:b + 2] == [5, 4] and sum(ans["status"]) == 9
    assert ans["group_start"][b] == ans["group_start"][b + 2] and len(ans["items"]) < len(good["items"])
    assert_answer(run_call(gpu, runs, in_status=st), ans)
    both, _ = Cs.unsorted_group(runs, b)  # an input status stands before the order check
    assert_answer(run_call(gpu, both, in_status=st), R.merge_read(both, Cs.SNAP, in_status=st))


def _malformed(runs):
    rs = np.concatenate([[0], np.cumsum([len(r) for r in R.flat_runs(runs)])]).tolist()
    k = next(i for i in range(1, len(rs) - 1) if rs[i] < rs[i + 1])
    return {"decreasing": rs[:k] + [rs[k + 1], rs[k]] + rs[k + 2:], "short_of_n_items": rs[:-1] + [rs[-1] - 1],
            "past_n_items": rs[:-1] + [rs[-1] + 3], "first_not_zero": [1] + rs[1:]}


@pytest.mark.parametrize("form", ["decreasing", "short_of_n_items", "past_n_items", "first_not_zero"])
def test_malformed_run_start(gpu, mid, form):
    runs, _ = mid
    rejected = {"items": [], "src": [], "group_start": [0] * 66, "status": [10] * 65}
    assert_answer(run_call(gpu, runs, run_start=_malformed(runs)[form]), rejected)


# ---- 4. arguments and state
def test_null_out_src(gpu, mid):
    runs, ans = mid
    assert_answer(run_call(gpu, runs, with_src=False), ans, with_src=False)


@pytest.mark.parametrize("fill_ff", [False, True], ids=["as-left", "0xFF-before-every-call"])
def test_reused_workspace(gpu, mid, fill_ff):
    import torch
    runs, _ = mid
    b = Cs.group_between_neighbours(runs, mid[1]["group_start"])
    unsorted, _ = Cs.unsorted_group(runs, b)
    small, empty = Cs.grouped_case(2, 1), [[[], []], [[], []]]
    need = max(gpu.lib().lsm_merge_read_workspace_size(sizes_of(r)[0], len(r[0]), len(r)) for r in (runs, small, empty))
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    steps = [(runs, None), (unsorted, None), (runs, _malformed(runs)["decreasing"]), (runs, None), (small, None),
             (empty, None), (runs, None)]
    for case, run_start in steps:
        if fill_ff:
            ws.fill_(0xFF)
        g = run_call(gpu, case, ws=ws, run_start=run_start)
        if run_start is not None:
            assert_answer(g, {"items": [], "src": [], "group_start": [0] * 66, "status": [10] * 65})
        else:
            assert_answer(g, R.merge_read(case, Cs.SNAP))


def test_odd_addresses(gpu, mid):
    runs, ans = mid
    assert_answer(run_call(gpu, runs, skews=(3, 5, 1, 7)), ans)
    big = Cs.grouped_case(2, 1)  # (the long gather path at odd source and destination addresses)
    assert_answer(run_call(gpu, big, skews=(1, 3, 5, 9)), R.merge_read(big, Cs.SNAP))


def test_no_groups_and_no_items(gpu):
    import torch
    g = run_call(gpu, [[[], [], []], [[], [], []]])
    assert_answer(g, {"items": [], "src": [], "group_start": [0, 0, 0, 0], "status": [0, 0, 0]})
    d, _ = to_device(gpu, [])
    out = alloc_outputs(0, 0, 0, 0)
    ws = torch.zeros(gpu.lib().lsm_merge_read_workspace_size(0, 0, 1), dtype=torch.uint8, device="cuda")
    ReadCall(gpu, d, torch.zeros(1, dtype=torch.int64, device="cuda"), 0, 1, out, ws, 5).launch()
    torch.cuda.synchronize()
    g = read_outputs(out)
    assert g["group_start"].tolist() == [0] and (g["status"].view(np.uint8) == SENT).all()


def test_wrapper(gpu):
    """lsmgpu.merge_read (allocates outputs and workspace per call)."""
    import torch
    runs = Cs.grouped_case(2, 1)
    d, rs = to_device(gpu, R.flat_runs(runs))
    out = gpu.merge_read(d, rs, 1, 2, Cs.SNAP, keep_tombstones=True)
    torch.cuda.synchronize()
    ans = R.merge_read(runs, Cs.SNAP, True)
    total = len(ans["items"])
    assert out["group_start"].cpu().tolist() == [0, total] and out["status"].cpu().tolist() == [0]
    assert out["src"].cpu().numpy().view(np.uint32)[:total].tolist() == ans["src"]
    assert out["seqno"].cpu().numpy().view(np.uint64)[:total].tolist() == [it[2] for it in ans["items"]]


# ---- 5. a captured graph replayed after the inputs changed in place
def _reseq(runs):
    """The same keys, values and run lengths with other seqnos (every run sorted again)."""
    out = []
    for src in runs:
        out.append([sorted([(k, v, Cs.SNAP - 8 + ((s - (Cs.SNAP - 8)) * 7 + 3) % 16, t) for k, v, s, t in run],
                           key=lambda it: (it[0], -it[2])) for run in src])
    return out


def test_graph_replay(gpu, mid):
    import torch
    first, _ = mid
    second = _reseq(first)
    assert R.merge_read(second, Cs.SNAP) != R.merge_read(first, Cs.SNAP)
    d, rs = to_device(gpu, R.flat_runs(first))
    n, kb, vb = sizes_of(first)
    out = alloc_outputs(n, kb, vb, 65)
    ws = torch.zeros(gpu.lib().lsm_merge_read_workspace_size(n, 65, 3), dtype=torch.uint8, device="cuda")
    d_rs = torch.tensor(rs, dtype=torch.int64, device="cuda")
    call = ReadCall(gpu, d, d_rs, 65, 3, out, ws, Cs.SNAP)
    graph = capture(call.launch)
    for runs in (first, second, first):
        src, _ = to_device(gpu, R.flat_runs(runs))
        for f in ("keys", "key_off", "vals", "val_off", "seqno", "vtype"):
            assert d[f].shape == src[f].shape
            d[f].copy_(src[f])
        for t in out.values():
            t.fill_(SENT)
        graph.replay()
        torch.cuda.synchronize()
        assert_answer(read_outputs(out), R.merge_read(runs, Cs.SNAP))


# ---- 6. the pipeline: three tables, a batch of ranges, one snapshot
GLOBAL_SEQNOS = (200, 100, 0)  # tables[0] is the newest
PIPE_SNAP = 260


def _tables():
    """Three item lists over one key space, newest first; tombstones in the two newer ones."""
    rng = random.Random(6001)
    out = []
    for t in range(3):
        seen, items = set(), []
        while len(items) < 420:
            k, s = b"key%04d" % rng.randrange(220), rng.randrange(100)
            if (k, s) in seen:
                continue
            seen.add((k, s))
            vt = rng.choice((0, 0, 0, 1, 2, 4) if t < 2 else (0, 0, 4))
            items.append((k, b"" if vt in (1, 2) else bytes(rng.getrandbits(8) for _ in range(rng.randrange(200))), s, vt))
        out.append(sorted(items, key=lambda it: (it[0], -it[2])))
    return out


def _queries():
    rng = random.Random(6002)
    qs = [(None, None, False, False), (b"zzz", None, False, False), (None, b"a", False, False),   # all, outside x 2
          (b"key0010a", b"key0010b", False, False), (b"key0050", b"key0050", True, True),        # empty x 2
          (b"key0100", b"key0102", False, False), (b"key0007", b"key0008", True, False)]        # inside one block x 2
    while len(qs) < 40:
        a, b = sorted((rng.randrange(230), rng.randrange(230)))
        if len(qs) % 2:  # every other range is narrow: a few keys, mostly inside one block
            b = a + rng.randrange(8)
        lo = None if rng.random() < 0.1 else b"key%04d" % a + (b"x" if rng.random() < 0.2 else b"")
        hi = None if rng.random() < 0.1 else b"key%04d" % b
        qs.append((lo, hi, rng.random() < 0.3, rng.random() < 0.3))
    return qs


def _device_queries(gpu, qs):
    import torch

    def arena(which):
        parts = [q[which] or b"" for q in qs]
        off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
        return gpu.to_device_bytes(b"".join(parts)), torch.from_numpy(off).cuda()

    (lo, lo_off), (hi, hi_off) = arena(0), arena(1)
    return lo, lo_off, hi, hi_off, torch.tensor([flags_of(*q) for q in qs], dtype=torch.uint8).cuda()


def _rows_of(out):
    """range_read's dict -> (per-query item lists, status list)."""
    gs = out["group_start"].cpu().numpy().tolist()
    ko, vo = out["key_off"].cpu().numpy(), out["val_off"].cpu().numpy()
    keys, vals = out["keys"].cpu().numpy().tobytes(), out["vals"].cpu().numpy().tobytes()
    seq, vt = out["seqno"].cpu().numpy().view(np.uint64), out["vtype"].cpu().numpy()
    rows = [[(keys[ko[j]:ko[j + 1]], vals[vo[j]:vo[j + 1]], int(seq[j]), int(vt[j])) for j in range(gs[q], gs[q + 1])]
            for q in range(len(gs) - 1)]
    return rows, out["status"].cpu().numpy().tolist()


def test_pipeline_range_read(gpu):
    import torch
    lists, qs = _tables(), _queries()
    tables = []
    for items, gseq in zip(lists, GLOBAL_SEQNOS):
        d, _ = to_device(gpu, [items])
        t = gpu.write_table(d, block_size=4096)
        assert t["block_count"] >= 3
        tables.append(dict(t, two_level=False, global_seqno=gseq))
    bounds = _device_queries(gpu, qs)
    want = []
    for q in qs:
        sources = [[(it[0], it[1], it[2] + gseq, it[3]) for it in (items[i] for i in brute_force([x[0] for x in items], *q))]
                   for items, gseq in zip(lists, GLOBAL_SEQNOS)]
        want.append(R.brute_group(sources, PIPE_SNAP))
    assert sum(1 for w in want if not w) >= 4 and sum(1 for w in want if w) >= 25
    assert len(want[0]) < len({it[0] for items in lists for it in items})  # tombstones and the snapshot hide keys
    got, status = _rows_of(gpu.range_read(tables, *bounds, PIPE_SNAP))
    assert status == [0] * len(qs)
    assert got == want
    kept, _ = _rows_of(gpu.range_read(tables, *bounds, PIPE_SNAP, keep_tombstones=True))
    assert kept == [R.brute_group(
        [[(it[0], it[1], it[2] + gseq, it[3]) for it in (items[i] for i in brute_force([x[0] for x in items], *q))]
         for items, gseq in zip(lists, GLOBAL_SEQNOS)], PIPE_SNAP, True) for q in qs]

    # one data block of the middle table damaged (its magic): the queries that read it carry
    # LSM_BAD_MAGIC and no rows, the others are unchanged
    t = tables[1]
    b = t["block_count"] // 2
    starts = t["starts"].cpu().numpy().tolist()
    file = t["file"].clone()
    file[int(t["block_off"][b].item())] ^= 0xFF
    padded = gpu.padded_bytes(file.numel())
    padded[:file.numel()] = file
    damaged = [tables[0], dict(t, file=padded[:file.numel()]), tables[2]]
    got2, status2 = _rows_of(gpu.range_read(damaged, *bounds, PIPE_SNAP))
    block_of = lambda i: next(k for k in range(len(starts) - 1) if starts[k] <= i < starts[k + 1])
    must_fault = must_pass = 0
    for q, query in enumerate(qs):
        idx = brute_force([x[0] for x in lists[1]], *query)
        if idx and block_of(idx[0]) <= b <= block_of(idx[-1]):    # the block holds rows of the query
            assert status2[q] == 1 and got2[q] == [], q
            must_fault += 1
        elif idx and (block_of(idx[-1]) < b - 1 or block_of(idx[0]) > b + 1):  # its rows lie well away from it
            assert status2[q] == 0 and got2[q] == want[q], q
            must_pass += 1
        else:  # (a seek may or may not have walked through the block)
            assert (status2[q], got2[q]) in ((0, want[q]), (1, [])), q
    assert must_fault >= 5 and must_pass >= 5, (must_fault, must_pass)
    torch.cuda.synchronize()
