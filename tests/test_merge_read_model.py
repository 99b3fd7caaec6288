"""CPU side of lsm_merge_read: the Python model (tests/merge_read_model.py) reproduces the
reference's MvccStream unit tests (transcribed as data in tests/golden/mvcc_stream_cases.json),
its per-position rule agrees with the reference loop and with a brute-force dict, the case
generator (tests/merge_read_cases.py) holds every edge it was built for, and the C entry point
rejects bad arguments before any device call."""
import ctypes as C
import json
import random
import re
from pathlib import Path

import pytest

import merge_model as M
import merge_read_cases as Cs
import merge_read_model as R

ROOT = Path(__file__).resolve().parent.parent
CASES = json.loads((ROOT / "tests" / "golden" / "mvcc_stream_cases.json").read_text())["cases"]


def case_rows(rows):
    return [(bytes.fromhex(k), bytes.fromhex(v), int(s), int(t)) for k, v, s, t in rows]


@pytest.fixture(scope="module")
def L():
    import lsmgpu
    if not lsmgpu.LIB_PATH.exists():
        lsmgpu.build()
    return lsmgpu


# ------------------------------------------------------------------ the model
def test_golden_file_shape():
    names = [c["name"] for c in CASES]
    assert len(names) == len(set(names)) == 14
    assert sum(n.startswith("mvcc_stream_") for n in names) == 8 and sum(n.startswith("mvcc_queue") for n in names) == 6


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_model_reproduces_reference_case(case):
    """MvccStream filters neither by seqno nor by type: every item visible, tombstones kept."""
    rows = case_rows(case["input"])
    assert M.run_is_sorted(rows)
    for fn in (R.read_group, R.rule_group):
        got = fn([rows], 2 ** 64 - 1, keep_tombstones=True)
        assert [it for it, _ in got] == case_rows(case["expect"])
        assert all(rows[i] == it for it, i in got)
    assert [it for it, _ in R.mvcc_stream([(it, i) for i, it in enumerate(rows)])] == case_rows(case["expect"])


def test_rule_equals_reference_loop():
    assert R.cross_check(1500, seed=11) == 12000


def test_model_equals_brute_force():
    """Per group, a dict of the newest visible version of each key, tombstones dropped."""
    rng = random.Random(12)
    for _ in range(600):
        max_seq = rng.randrange(1, 10)
        runs = R.random_grouped(rng, rng.randrange(1, 5), rng.randrange(1, 4), n_keys=rng.randrange(1, 4),
                                max_seq=max_seq)
        for snap in (0, rng.randrange(0, max_seq + 1), max_seq + 1):
            for keep in (False, True):
                ans = R.merge_read(runs, snap, keep)
                assert ans["status"] == [0] * len(runs[0])
                for g in range(len(runs[0])):
                    got = ans["items"][ans["group_start"][g]:ans["group_start"][g + 1]]
                    want = R.brute_group([src[g] for src in runs], snap, keep)
                    # (of equal (key, seqno) the dict keeps the first it met, lowest source first, as the merge)
                    assert got == want


def test_model_statuses_and_indices():
    a = [(b"k", b"new", 7, 0), (b"k", b"old", 3, 0)]
    b = [(b"j", b"", 9, 1), (b"k", b"tie", 7, 0)]
    runs = [[a, []], [b, [(b"k", b"g1", 1, 0)]]]  # 2 sources x 2 groups: flat order a, [], b, [k g1]
    ans = R.merge_read(runs, 8)
    assert ans == {"items": [a[0], (b"k", b"g1", 1, 0)], "src": [0, 4], "group_start": [0, 1, 2], "status": [0, 0]}
    assert R.merge_read(runs, 10, True)["src"] == [2, 0, 4]       # the tombstone kept, the tie lower source first
    assert R.merge_read(runs, 7)["items"] == [a[1], (b"k", b"g1", 1, 0)]  # seqno == snapshot is not visible
    assert R.merge_read(runs, 8, group_seqno=[8, 1])["group_start"] == [0, 1, 1]
    assert R.merge_read(runs, 8, in_status=[0, 0, 5, 0]) == {"items": [(b"k", b"g1", 1, 0)], "src": [4],
                                                             "group_start": [0, 0, 1], "status": [5, 0]}
    assert R.merge_read(runs, 8, in_status=[4, 0, 5, 0])["status"] == [4, 0]  # the lowest source's
    bad = [[a[::-1], []], [b, [(b"k", b"g1", 1, 0)]]]
    assert R.merge_read(bad, 8)["status"] == [R.BAD_ARG, 0] and R.merge_read(bad, 8)["group_start"] == [0, 0, 1]
    assert R.merge_read(bad, 8, in_status=[0, 0, 5, 0])["status"] == [5, 0]   # an input status before the order


# ------------------------------------------------------- the case generator
@pytest.mark.parametrize("shape", Cs.SHAPES, ids=["%dx%d" % s for s in Cs.SHAPES])
def test_case_holds_its_edges(shape):
    runs = Cs.grouped_case(*shape)
    assert len(runs) == shape[0] and all(len(src) == shape[1] for src in runs)
    assert all(M.run_is_sorted(r) for src in runs for r in src)
    assert {len(r) for src in runs for r in src} <= set(Cs.RUN_LENS)
    found = Cs.edges_of(runs)
    for edge in sorted(Cs.expected_edges(*shape)):
        assert edge in found, edge
    assert sum(len(r) for src in runs for r in src) <= 3000
    ans = R.merge_read(runs, Cs.SNAP)
    assert 0 < len(ans["items"]) < sum(len(r) for src in runs for r in src) and ans["status"] == [0] * shape[1]
    assert R.merge_read(runs, Cs.SNAP, fn=R.rule_group) == ans


def test_edge_detectors_are_not_trivial():
    """Each planted edge disappears when its plant does (one source, one group)."""
    assert Cs.edges_of([[[(b"k", b"v", 1, 0)]]], snap=5) == {"run_len_1"}
    assert "seqno_equals_snapshot" in Cs.edges_of([[[(b"k", b"v", 5, 0)]]], snap=5)
    two = [[[(b"k", b"v", 1, 0)], [(b"k", b"w", 2, 0)]]]
    assert "group_boundary" in Cs.edges_of(two, snap=5) and "group_boundary" not in Cs.edges_of(two, snap=2)
    assert len(set(Cs.EDGES)) == len(Cs.EDGES) >= 9 + len(Cs.RUN_LENS)


def test_unsorted_group_breaks_one_run_only():
    runs = Cs.grouped_case(3, 65)
    good = R.merge_read(runs, Cs.SNAP)
    b = Cs.group_between_neighbours(runs, good["group_start"])
    bad, s = Cs.unsorted_group(runs, b)
    assert not M.run_is_sorted(bad[s][b])
    assert all(M.run_is_sorted(bad[q][g]) for q in range(3) for g in range(65) if (q, g) != (s, b))
    ans = R.merge_read(bad, Cs.SNAP)
    for g in (b - 1, b, b + 1):  # all three groups emit rows while the input is sorted
        assert good["group_start"][g] < good["group_start"][g + 1]
    assert ans["status"] == [0] * b + [R.BAD_ARG] + [0] * (64 - b) and ans["group_start"][b] == ans["group_start"][b + 1]
    assert len(ans["items"]) == len(good["items"]) - (good["group_start"][b + 1] - good["group_start"][b])


# --------------------------------------------------- the C ABI without a device
def test_header_declares_merge_read(L):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "lsmgpu.h").read_text(), flags=re.S)
    for f in ("lsm_merge_read", "lsm_merge_read_workspace_size"):
        assert re.search(r"\b%s\s*\(" % f, text), f
        assert f in L.EXPORTED_SYMBOLS and hasattr(L.lib(), f)
    assert "#define LSM_MERGE_READ_KEEP_TOMBSTONES 1u" in text
    assert L.MERGE_READ_KEEP_TOMBSTONES == 1
    assert L.lib().lsm_abi_version() == 7 and L.ABI_VERSION == 7


def _call(L, it, n_groups=3, n_sources=2, flags=0, run_start=0x2000, group_start=0x9000, status=0xA000, ws=0xB000,
          ws_bytes=None, d_in=True, outs=None):
    lib = L.lib()
    if ws_bytes is None:
        ws_bytes = lib.lsm_merge_read_workspace_size(it.n_items, n_groups, n_sources)
    p = lambda v: C.c_void_p(v) if v else None
    o = dict(keys=0x3000, key_off=0x4000, vals=0x5000, val_off=0x6000, seqno=0x7000, vtype=0x8000)
    o.update(outs or {})
    return lib.lsm_merge_read(C.byref(it) if d_in else None, p(run_start), n_groups, n_sources, 0, None, None, flags,
                              p(o["keys"]), p(o["key_off"]), p(o["vals"]), p(o["val_off"]), p(o["seqno"]),
                              p(o["vtype"]), None, p(group_start), p(status), p(ws), ws_bytes, None)


def test_merge_read_bad_args_rejected_without_device(L):
    """Every host-side LSM_BAD_ARG of include/lsmgpu.h: the checks happen before any HIP call (the
    pointers are not addresses of anything)."""
    it = L.LsmItems(0x100, 0x200, 0x300, 0x400, 0x500, 0x600, None, None, 1000)
    for n_sources in (0, 65, 2 ** 32 - 1):
        assert _call(L, it, n_sources=n_sources) == 10
    assert _call(L, it, n_groups=0) == 10                                   # no group, but items
    assert _call(L, it, n_groups=2 ** 31, n_sources=2, ws_bytes=1 << 62) == 10  # 2^32 runs
    assert _call(L, it, n_groups=2 ** 32 - 1, n_sources=1, ws_bytes=1 << 62) == 10
    for flags in (2, 4, 1 << 31, 3):
        assert _call(L, it, flags=flags) == 10
    assert _call(L, it, d_in=False) == 10
    for kw in ({"run_start": 0}, {"group_start": 0}, {"status": 0}, {"ws": 0}):
        assert _call(L, it, **kw) == 10, kw
    for f in ("keys", "key_off", "vals", "val_off", "seqno", "vtype"):
        assert _call(L, it, outs={f: 0}) == 10, f
        miss = L.LsmItems(0x100, 0x200, 0x300, 0x400, 0x500, 0x600, None, None, 1000)
        setattr(miss, f, None)
        assert _call(L, miss) == 10, f
    need = L.lib().lsm_merge_read_workspace_size(1000, 3, 2)
    assert _call(L, it, ws_bytes=need - 1) == 10
    big = L.LsmItems(0x100, 0x200, 0x300, 0x400, 0x500, 0x600, None, None, 2 ** 32 - 1)
    assert _call(L, big, ws_bytes=1 << 62) == 10


def test_merge_read_workspace_size_monotone(L):
    lib = L.lib()
    sizes_n = [lib.lsm_merge_read_workspace_size(n, 7, 4) for n in (0, 1, 63, 2048, 2049, 1 << 20, 2 ** 32 - 2)]
    assert sizes_n == sorted(sizes_n) and sizes_n[0] > 0
    sizes_g = [lib.lsm_merge_read_workspace_size(1 << 12, g, 4) for g in (0, 1, 65, 4096, 1 << 20, 2 ** 32 - 2)]
    assert sizes_g == sorted(sizes_g) and sizes_g[-1] > sizes_g[0]
