"""lsm_merge_runs, output extents (merge_gather_kernel, gather_field, wave_copy): outputs
that start as canaries keep every byte past the defined ones, a gather step's span on both
sides of the LDS limit at several output alignments, and long keys next to short ones in
one step with some of them dropped.  Through the C ABI with caller-owned outputs
(merge_gpu.MergeCall); expected: merge_model.merge_runs, bit for bit."""
import pytest

import merge_cases as MC
import merge_model as M
from merge_gpu import (MergeCall, alloc_outputs, alloc_workspace, assert_extents, input_bytes, read_outputs,
                       run_call, to_device)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", ["nothing_dropped", "half_dropped"])
def test_canaries(gpu, case):
    runs, thr = {"nothing_dropped": (MC.nothing_dropped(), 0),
                 "half_dropped": (MC.half_dropped(), MC.HALF_DROPPED_THR)}[case]
    g = run_call(gpu, runs, thr)
    want = assert_extents(g, runs, thr)
    kb, vb = input_bytes(runs)
    assert len(g["keys"]) == kb + gpu.LSM_INPUT_PADDING and len(g["vals"]) == vb + gpu.LSM_INPUT_PADDING
    if case == "nothing_dropped":  # the output fills the arenas up to their padding
        assert sum(len(it[0]) for it in want) == kb and sum(len(it[1]) for it in want) == vb
    else:
        n = sum(len(r) for r in runs)
        assert 0.35 * n < len(want) < 0.65 * n
    for evict, zero in MC.FLAG_PAIRS[1:]:
        assert_extents(run_call(gpu, runs, thr, evict, zero), runs, thr, evict, zero)


@pytest.mark.parametrize("field", ["vals", "keys"])
@pytest.mark.parametrize("pad", [0, 1, 15])
@pytest.mark.parametrize("total", [MC.MERGE_BUF - 1, MC.MERGE_BUF, MC.MERGE_BUF + 1], ids=["buf-1", "buf", "buf+1"])
def test_span_limit(gpu, total, pad, field):
    """Step 1 (merged positions 64 .. 127) has `total` value (or key) bytes and its first output
    byte is `pad` bytes past a 16-byte boundary: gather_field assembles it in LDS up to
    total + pad == kMergeBuf and writes it straight to global memory above."""
    import torch
    runs = MC.span_limit(total, pad, field)
    want, _, dropped = M.merge_runs(runs, 0)
    assert not dropped
    off = [0]
    for it in want:
        off.append(off[-1] + len(it[0 if field == "keys" else 1]))
    assert off[MC.SEG] % 16 == pad and off[2 * MC.SEG] - off[MC.SEG] == total  # (the model's own offsets)
    d, rs = to_device(gpu, runs)
    n = sum(len(r) for r in runs)
    out = alloc_outputs(gpu, n, *input_bytes(runs), len(runs))
    assert out["vals"].data_ptr() % 16 == 0 and out["keys"].data_ptr() % 16 == 0
    MergeCall(gpu, d, torch.tensor(rs, dtype=torch.int64, device="cuda"), out, alloc_workspace(gpu, n, len(runs))).launch()
    torch.cuda.synchronize()
    assert_extents(read_outputs(out, len(runs)), runs)


@pytest.mark.parametrize("skew", [0, 1, 7])
def test_long_and_short_keys_in_one_step(gpu, skew):
    import torch
    runs = MC.mixed_keys()
    d, rs = to_device(gpu, runs, key_skew=skew, val_skew=skew)
    n = sum(len(r) for r in runs)
    d_rs = torch.tensor(rs, dtype=torch.int64, device="cuda")
    for evict in (False, True):
        out = alloc_outputs(gpu, n, *input_bytes(runs), len(runs))
        MergeCall(gpu, d, d_rs, out, alloc_workspace(gpu, n, len(runs)), MC.MIXED_KEYS_THR, evict).launch()
        torch.cuda.synchronize()
        want = assert_extents(read_outputs(out, len(runs)), runs, MC.MIXED_KEYS_THR, evict)
        assert any(len(it[0]) >= MC.MERGE_LONG for it in want) and any(len(it[0]) <= 20 for it in want)
