"""lsm_merge_runs, ordering: seqnos over the whole u64 range (cmp_probe, the GC threshold
compares and the zero_seqnos store), long stretches of equal (key, seqno) items across
segment boundaries of several runs (the tie rule of merge_split_kernel and
merge_rank_kernel), and keys that share their first 16 or 32 bytes (cmp_key_tail in the
binary searches).  Inputs from tests/merge_cases.py, run through the C ABI with a zeroed
workspace and canary outputs (merge_gpu.check_call); the expected result is
merge_model.merge_runs, bit for bit."""
import pytest

import merge_cases as MC
from merge_gpu import check_call as check

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("evict", [False, True])
@pytest.mark.parametrize("thr", MC.WIDE_THRESHOLDS, ids=["0", "2^32", "2^63-1", "2^63", "2^64-1"])
def test_full_width_seqnos(gpu, thr, evict):
    runs = MC.wide_seqnos()
    want, _ = check(gpu, runs, thr, evict, zero=True)
    if thr == 0 and not evict:
        assert len(want) == sum(len(r) for r in runs)
        for key, pair in ((b"x-high-dword", MC.HIGH_DWORD_PAIR), (b"y-bit-63", MC.BIT63_PAIR)):
            assert tuple(it[2] for it in want if it[0] == key) == pair


def test_long_ties(gpu):
    runs = MC.long_ties()
    want, _ = check(gpu, runs, thr=0)
    assert [it[1] for it in want] == [it[1] for r in runs for it in r]  # src == 0 .. 394: lower run first
    want, _ = check(gpu, runs, thr=MC.TIE_SEQ + 1)
    assert want == [runs[0][0]]
    check(gpu, runs, thr=MC.TIE_SEQ)  # the threshold equal to the seqno drains nothing
    check(gpu, [runs[0], [], runs[1], [], runs[2], []], thr=0)  # empty runs between them


@pytest.mark.parametrize("order", range(6))
def test_long_ties_in_every_run_order(gpu, order):
    runs = MC.long_ties_orders()[order]
    want, _ = check(gpu, runs, thr=0)
    assert len(want) == 395
    check(gpu, runs, thr=MC.TIE_SEQ + 1, evict=True)


def test_long_ties_between_ordinary_keys(gpu):
    runs = MC.long_ties_embedded()
    want, dropped = check(gpu, runs, thr=0)
    assert not dropped
    check(gpu, runs, thr=50, zero=True)
    want, _ = check(gpu, runs, thr=MC.TIE_SEQ + 1)
    assert [it for it in want if it[0] == MC.TIE_KEY] == [next(it for it in runs[0] if it[0] == MC.TIE_KEY)]
    check(gpu, [runs[2], runs[0], runs[1]], thr=0)


def test_long_ties_in_64_runs(gpu):
    runs = MC.long_ties_64_runs()
    want, _ = check(gpu, runs, thr=0)
    assert [it[1] for it in want] == [it[1] for r in runs for it in r]
    check(gpu, runs, thr=MC.TIE_SEQ + 1)


@pytest.mark.parametrize("head_len", [16, 32])
def test_shared_heads(gpu, head_len):
    runs = MC.shared_heads(head_len)
    want, dropped = check(gpu, runs, thr=500, evict=True)
    assert want and dropped
    check(gpu, runs, thr=0)
