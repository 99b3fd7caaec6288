"""lsm_merge_runs, state and arguments, straight through the C ABI (merge_gpu.MergeCall):
one workspace reused by merges of other shapes and outcomes (MergeHdr.bad / .unsorted, perm,
keep and the splitter table live there), a workspace of 0xFF bytes, every malformed
d_run_start form merge_setup_kernel rejects, d_out_src == NULL, and two merges in flight
on two streams.  Expected: merge_model.merge_runs bit for bit, or the documented rejection
(include/lsmgpu.h: the rejected runs' status LSM_BAD_ARG, *d_n_out = 0)."""
import pytest

import merge_cases as MC
from merge_gpu import (MergeCall, alloc_outputs, alloc_workspace, assert_model, assert_rejected, input_bytes,
                       read_outputs, run_call, to_device)

pytestmark = pytest.mark.gpu

THR = 400


def _run_start(runs):
    out = [0]
    for r in runs:
        out.append(out[-1] + len(r))
    return out


@pytest.mark.parametrize("fill_ff", [False, True], ids=["as-left", "0xFF-before-every-call"])
def test_reused_workspace(gpu, fill_ff):
    import torch
    first, unsorted, one, empty = MC.state_sorted(), MC.state_unsorted(), MC.state_one_run(), [[], []]
    rs = _run_start(first)
    malformed, malformed_status = MC.malformed_run_starts(rs)["decreasing_pair"]
    need = max(gpu.lib().lsm_merge_workspace_size(sum(len(r) for r in runs), len(runs))
               for runs in (first, unsorted, one, empty))
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    steps = [("sorted", first, None, None), ("unsorted", unsorted, None, [0, 10, 0]),
             ("malformed run_start", first, malformed, malformed_status), ("sorted again", first, None, None),
             ("one shorter run", one, None, None), ("no items", empty, None, None),
             ("sorted a third time", first, None, None)]
    for name, runs, run_start, rejected in steps:
        if fill_ff:
            ws.fill_(0xFF)
        g = run_call(gpu, runs, THR, evict=True, ws=ws, run_start=run_start)
        if rejected:
            assert_rejected(g, rejected)
        else:
            want, _ = assert_model(g, runs, THR, evict=True)
            assert bool(want) == (runs is not empty), name


@pytest.mark.parametrize("form", ["first_not_zero", "last_not_n_items", "last_above_n_items", "decreasing_pair",
                                  "entry_above_n_items"])
def test_malformed_run_start(gpu, form):
    """merge_setup_kernel: run r = [s, e) is rejected unless s <= e <= n_items, s == 0 for the
    first run and e == n_items for the last; the statuses of every form are written out in
    merge_cases.malformed_run_starts.  Nothing is emitted."""
    runs = MC.state_sorted()
    run_start, status = MC.malformed_run_starts(_run_start(runs))[form]
    assert status == {"first_not_zero": [10, 0, 0], "last_not_n_items": [0, 0, 10], "last_above_n_items": [0, 0, 10],
                      "decreasing_pair": [0, 10, 0], "entry_above_n_items": [0, 10, 10]}[form]
    g = run_call(gpu, runs, THR, run_start=run_start)
    assert_rejected(g, status)
    assert int(g["key_off"][0]) == 0 and int(g["val_off"][0]) == 0  # entries 0 .. n_out of the offsets are written


def test_null_out_src(gpu):
    runs = MC.state_sorted()
    a = run_call(gpu, runs, THR, evict=True, zero=True)
    b = run_call(gpu, runs, THR, evict=True, zero=True, with_src=False)
    assert_model(a, runs, THR, True, True)
    assert_model(b, runs, THR, True, True, with_src=False)
    assert (b["src"] == 0xA5A5A5A5).all()  # never touched
    for f in ("keys", "vals", "key_off", "val_off", "seqno", "vtype"):
        assert (a[f] == b[f]).all(), f


def test_two_streams(gpu):
    """Two different merges on two non-default streams, each with its own workspace, in
    flight together: both correct after one synchronise."""
    import torch
    sets = [(MC.state_sorted(), THR, True), (MC.state_second(), 300, False)]
    calls = []
    for runs, thr, evict in sets:
        d, rs = to_device(gpu, runs)
        n = sum(len(r) for r in runs)
        out = alloc_outputs(gpu, n, *input_bytes(runs), len(runs))
        call = MergeCall(gpu, d, torch.tensor(rs, dtype=torch.int64, device="cuda"), out,
                         alloc_workspace(gpu, n, len(runs)), thr, evict)
        calls.append((call, out, torch.cuda.Stream()))
    torch.cuda.synchronize()  # the inputs and canaries were written on the default stream
    for call, _, stream in calls:
        call.launch(stream)
    torch.cuda.synchronize()
    for (runs, thr, evict), (_, out, _) in zip(sets, calls):
        assert_model(read_outputs(out, len(runs)), runs, thr, evict)
