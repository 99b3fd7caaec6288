"""lsm_merge_runs captured into a HIP graph (torch.cuda.CUDAGraph over one stream, as
tests/test_gpu_graphs.py captures the encoder) and replayed: the call makes no host
synchronisation and keeps no per-call state on the host, so a replay over inputs that
were overwritten in place must give the model's result for the new inputs, and an
unsorted input the documented rejection.  The n_items == 0 path (memset nodes) is a
second capture.  Expected: merge_model.merge_runs, bit for bit."""
import pytest

import merge_cases as MC
from merge_gpu import (MergeCall, alloc_outputs, alloc_workspace, assert_model, assert_rejected, capture, input_bytes,
                       read_outputs, to_device)

pytestmark = pytest.mark.gpu

IN_FIELDS = ("keys", "key_off", "vals", "val_off", "seqno", "vtype")


def _replay(graph, out, n_runs):
    import torch
    for t in out.values():
        t.fill_(0xFF)  # -1 in every output
    graph.replay()
    torch.cuda.synchronize()
    return read_outputs(out, n_runs)


def test_merge_graph_replay(gpu):
    import torch
    first, second, unsorted = MC.graph_sets()
    n = sum(len(r) for r in first)
    dev = {}
    for name, runs in (("first", first), ("second", second), ("unsorted", unsorted)):
        d, rs = to_device(gpu, runs)
        d["run_start"] = torch.tensor(rs, dtype=torch.int64, device="cuda")
        dev[name] = d
    live = {f: t.clone() for f, t in dev["first"].items()}  # the buffers the graph reads
    for d in dev.values():
        assert all(d[f].shape == live[f].shape for f in live)
    out = alloc_outputs(gpu, n, *input_bytes(first), len(first))
    call = MergeCall(gpu, live, live["run_start"], out, alloc_workspace(gpu, n, len(first)), MC.GRAPH_THR, evict=True,
                     zero=True)
    graph = capture(call.launch)
    for _ in range(3):
        assert_model(_replay(graph, out, 3), first, MC.GRAPH_THR, True, True)
    for name, runs in (("second", second), ("unsorted", None), ("first", first)):
        for f, t in live.items():
            t.copy_(dev[name][f])
        g = _replay(graph, out, 3)
        if runs is None:
            assert_rejected(g, [0, 0, 10])
        else:
            assert_model(g, runs, MC.GRAPH_THR, True, True)


def test_merge_graph_replay_no_items(gpu):
    import torch
    d, rs = to_device(gpu, [[], []])
    out = alloc_outputs(gpu, 0, 0, 0, 2)
    call = MergeCall(gpu, d, torch.tensor(rs, dtype=torch.int64, device="cuda"), out, alloc_workspace(gpu, 0, 2))
    graph = capture(call.launch)
    for _ in range(2):
        g = _replay(graph, out, 2)
        assert_model(g, [[], []])
        assert int(g["key_off"][0]) == 0 and int(g["val_off"][0]) == 0
