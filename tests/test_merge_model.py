"""CPU side of lsm_merge_runs: the Python model (tests/merge_model.py) reproduces
the reference's CompactionStream / Merger unit tests (transcribed as data in
tests/golden/compaction_stream_cases.json), its per-item GC rule agrees with
the reference loop, and the C entry point rejects bad arguments before any
device call."""
import ctypes as C
import json
import re
from pathlib import Path

import pytest

import merge_model as M

ROOT = Path(__file__).resolve().parent.parent
CASES = json.loads((ROOT / "tests" / "golden" / "compaction_stream_cases.json").read_text())["cases"]


def case_rows(rows):
    return [(bytes.fromhex(k), bytes.fromhex(v), int(s), int(t)) for k, v, s, t in rows]


@pytest.fixture(scope="module")
def L():
    import lsmgpu
    if not lsmgpu.LIB_PATH.exists():
        lsmgpu.build()
    return lsmgpu


def test_golden_file_shape():
    names = [c["name"] for c in CASES]
    assert len(names) == len(set(names)) == 14
    assert sum(n.startswith("compaction_stream_") for n in names) == 12 and sum(n.startswith("merge_") for n in names) == 2


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_model_reproduces_reference_case(case):
    runs = [case_rows(r) for r in case["runs"]]
    flat = [it for r in runs for it in r]
    items, src, dropped = M.merge_runs(runs, case["gc_seqno_threshold"], case["evict_tombstones"], case["zero_seqnos"])
    assert items == case_rows(case["expect"])
    assert [flat[i] for i in dropped] == case_rows(case["dropped"])
    assert sorted(src + dropped) == list(range(len(flat)))
    for it, i in zip(items, src):  # an emitted item is its input item, but for a zeroed seqno
        assert (it[0], it[1], it[3]) == (flat[i][0], flat[i][1], flat[i][3])
        assert it[2] == flat[i][2] or (case["zero_seqnos"] and it[2] == 0)


def test_expired_callback_is_the_drained_tail():
    """compaction_stream_expired_callback_1: the callback receives the drained versions in order."""
    case = CASES[0]
    stream = M.merge([case_rows(r) for r in case["runs"]])
    _, drained = M.compaction_stream(stream, case["gc_seqno_threshold"])
    assert [stream[i][0] for i in drained] == case_rows(case["dropped"])


def test_per_item_rule_equals_reference_loop():
    assert M.cross_check(4000, seed=7) == 16000


def test_merge_tie_order_and_stability():
    a = [(b"k", b"r0", 5, 0), (b"k", b"r0b", 5, 0)]
    b = [(b"j", b"", 1, 0), (b"k", b"r1", 5, 0), (b"k\x00", b"", 9, 0)]
    got = M.merge([a, b])
    assert [i for _, i in got] == [2, 0, 1, 3, 4]
    assert M.run_is_sorted(a) and M.run_is_sorted(b) and not M.run_is_sorted(b[::-1])


def test_header_declares_merge_entry_points(L):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "lsmgpu.h").read_text(), flags=re.S)
    for f in ("lsm_merge_runs", "lsm_merge_workspace_size"):
        assert re.search(r"\b%s\s*\(" % f, text), f
        assert f in L.EXPORTED_SYMBOLS and hasattr(L.lib(), f)
    assert "#define LSM_MERGE_MAX_RUNS 64" in text
    assert L.MERGE_MAX_RUNS == 64 and L.MERGE_EVICT_TOMBSTONES == 1 and L.MERGE_ZERO_SEQNOS == 2


def _call(L, it, n_runs=2, flags=0, run_start=0x2000, n_out=0x9000, status=0xA000, ws=0xB000, ws_bytes=None,
          d_in=True):
    lib = L.lib()
    if ws_bytes is None:
        ws_bytes = lib.lsm_merge_workspace_size(it.n_items, max(n_runs, 1))
    p = lambda v: C.c_void_p(v) if v else None
    return lib.lsm_merge_runs(C.byref(it) if d_in else None, p(run_start), n_runs, 0, flags, p(0x3000), p(0x4000),
                              p(0x5000), p(0x6000), p(0x7000), p(0x8000), None, p(n_out), p(status), p(ws),
                              ws_bytes, None)


def test_merge_bad_args_rejected_without_device(L):
    """As test_bad_args_rejected_without_device: every check happens before any HIP call."""
    it = L.LsmItems(0x100, 0x200, 0x300, 0x400, 0x500, 0x600, None, None, 1000)
    for n_runs in (0, 65):
        assert _call(L, it, n_runs=n_runs) == 10
    for flags in (4, 1 << 31, 7):
        assert _call(L, it, flags=flags) == 10
    assert _call(L, it, d_in=False) == 10
    for kw in ({"run_start": 0}, {"n_out": 0}, {"status": 0}, {"ws": 0}):
        assert _call(L, it, **kw) == 10, kw
    need = L.lib().lsm_merge_workspace_size(1000, 2)
    assert _call(L, it, ws_bytes=need - 1) == 10
    big = L.LsmItems(0x100, 0x200, 0x300, 0x400, 0x500, 0x600, None, None, 2 ** 32 - 1)
    assert _call(L, big, ws_bytes=1 << 60) == 10
    for f in ("keys", "key_off", "vals", "val_off", "seqno", "vtype"):  # the input arrays the merge reads
        miss = L.LsmItems(0x100, 0x200, 0x300, 0x400, 0x500, 0x600, None, None, 1000)
        setattr(miss, f, None)
        assert _call(L, miss) == 10, f


def test_merge_workspace_size_monotone(L):
    lib = L.lib()
    sizes_n = [lib.lsm_merge_workspace_size(n, 4) for n in (0, 1, 63, 64, 65, 2048, 2049, 1 << 20, 2 ** 32 - 2)]
    assert sizes_n == sorted(sizes_n) and sizes_n[0] > 0
    sizes_r = [lib.lsm_merge_workspace_size(1 << 20, r) for r in (1, 2, 3, 8, 63, 64)]
    assert sizes_r == sorted(sizes_r)
    assert lib.lsm_merge_workspace_size(1 << 20, 64) > lib.lsm_merge_workspace_size(1 << 20, 1)
