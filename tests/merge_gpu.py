"""Device helpers of the lsm_merge_runs tests (a plain module, imported by the
test_gpu_merge*.py files).  Two entries: gpu_merge goes through the wrapper
(lsmgpu.merge_runs, which allocates outputs and workspace per call), MergeCall
straight through the C ABI with caller-owned outputs and workspace, an optional
NULL d_out_src and a stream, so that one workspace can be reused, the outputs
can start as canaries and the call can be captured into a graph."""
import ctypes as C

import numpy as np

import merge_model as M

CANARY = 0xA5
BAD_ARG = 10


def to_device(L, runs, key_skew=0, val_skew=0):
    """Runs -> (device lsm_items dict, run_start list).  skew: the arena tensor starts that
    many bytes into its allocation and the first item another skew bytes into the arena."""
    import torch
    flat = [it for r in runs for it in r]
    n = len(flat)

    def arena(parts, skew):
        data = b"\xa5" * (2 * skew) + b"".join(parts)
        off = np.concatenate([[0], np.cumsum([len(p) for p in parts], dtype=np.int64)]).astype(np.int64) + skew
        return L.to_device_bytes(data)[skew:], torch.from_numpy(off).cuda()

    keys, key_off = arena([it[0] for it in flat], key_skew)
    vals, val_off = arena([it[1] for it in flat], val_skew)
    d = {"keys": keys, "key_off": key_off, "vals": vals, "val_off": val_off,
         "seqno": torch.from_numpy(np.array([it[2] for it in flat], np.uint64).view(np.int64)).cuda(),
         "vtype": torch.from_numpy(np.array([it[3] for it in flat], np.uint8)).cuda()}
    if n == 0:
        d["seqno"] = torch.zeros(0, dtype=torch.int64).cuda()
        d["vtype"] = torch.zeros(0, dtype=torch.uint8).cuda()
    run_start = np.concatenate([[0], np.cumsum([len(r) for r in runs])]).astype(np.int64)
    return d, run_start.tolist()


def gpu_merge(L, runs, thr=0, evict=False, zero=False, key_skew=0, val_skew=0):
    """Runs the merge; returns (items, src, status) read back from the device."""
    import torch
    d, run_start = to_device(L, runs, key_skew, val_skew)
    out = L.merge_runs(d, run_start, thr, evict, zero)
    torch.cuda.synchronize()
    n_out = int(out["n_out"].cpu()[0])
    status = out["status"].cpu().numpy()[:len(runs)].tolist()
    ko = out["key_off"].cpu().numpy()[:n_out + 1]
    vo = out["val_off"].cpu().numpy()[:n_out + 1]
    assert ko[0] == 0 and vo[0] == 0
    keys = out["keys"].cpu().numpy()[:int(ko[-1])].tobytes()
    vals = out["vals"].cpu().numpy()[:int(vo[-1])].tobytes()
    seq = out["seqno"].cpu().numpy().view(np.uint64)[:n_out]
    vt = out["vtype"].cpu().numpy()[:n_out]
    src = out["src"].cpu().numpy().view(np.uint32)[:n_out].tolist()
    items = [(keys[int(ko[j]):int(ko[j + 1])], vals[int(vo[j]):int(vo[j + 1])], int(seq[j]), int(vt[j]))
             for j in range(n_out)]
    return items, src, status


def check(L, runs, thr=0, evict=False, zero=False, **kw):
    assert all(M.run_is_sorted(r) for r in runs)
    want, want_src, dropped = M.merge_runs(runs, thr, evict, zero)
    got, src, status = gpu_merge(L, runs, thr, evict, zero, **kw)
    assert status == [0] * len(runs)
    assert len(got) == len(want)
    assert src == want_src
    assert got == want
    return want, dropped


def sort_run(items):
    return sorted(items, key=lambda it: (it[0], -it[2]))


def random_items(rng, n, n_keys, key_len=(1, 24), val_len=(0, 80), max_seq=1000, vtypes=(0, 0, 0, 1, 2, 4)):
    keys = set()
    while len(keys) < n_keys:
        keys.add(bytes(rng.choice(b"abcdefg\x00\xff") for _ in range(rng.randint(*key_len))))
    keys = sorted(keys)
    out = []
    for _ in range(n):
        t = rng.choice(vtypes)
        v = b"" if t in (1, 2) else bytes(rng.getrandbits(8) for _ in range(rng.randint(*val_len)))
        out.append((rng.choice(keys), v, rng.randrange(max_seq), t))
    return out


def deal(rng, items, n_runs):
    runs = [[] for _ in range(n_runs)]
    for it in items:
        runs[rng.randrange(n_runs)].append(it)
    return [sort_run(r) for r in runs]


# ------------------------------------------------------------- the C ABI entry
OUT_FIELDS = ("keys", "key_off", "vals", "val_off", "seqno", "vtype", "src", "n_out", "status")


def input_bytes(runs):
    """(key bytes, value bytes) of the runs: what the output arenas are sized from."""
    return sum(len(it[0]) for r in runs for it in r), sum(len(it[1]) for r in runs for it in r)


def alloc_outputs(L, n, key_bytes, val_bytes, n_runs, fill=CANARY):
    """Caller-owned outputs sized as include/lsmgpu.h asks (n entries, n + 1 offsets, the
    input arenas' bytes + LSM_INPUT_PADDING), as uint8 tensors so that every byte starts as
    `fill`."""
    import torch
    sizes = {"keys": key_bytes + L.LSM_INPUT_PADDING, "vals": val_bytes + L.LSM_INPUT_PADDING,
             "key_off": 8 * (n + 1), "val_off": 8 * (n + 1), "seqno": 8 * max(n, 1), "vtype": max(n, 1),
             "src": 4 * max(n, 1), "n_out": 8, "status": 4 * max(n_runs, 1)}
    return {f: torch.full((sizes[f],), fill, dtype=torch.uint8, device="cuda") for f in OUT_FIELDS}


def alloc_workspace(L, n, n_runs):
    import torch
    return torch.zeros(L.lib().lsm_merge_workspace_size(n, n_runs), dtype=torch.uint8, device="cuda")


class MergeCall:
    """One lsm_merge_runs call with every argument fixed: launch() only goes through ctypes
    (no allocation, no copy), on the given stream or the current one, and may be repeated
    or captured.  d: device lsm_items dict; run_start: int64 cuda tensor [n_runs + 1];
    out: alloc_outputs(); ws: uint8 cuda tensor of at least the workspace size."""

    def __init__(self, L, d, run_start, out, ws, thr=0, evict=False, zero=False, with_src=True):
        import torch
        self.L = L
        self.n_runs = run_start.numel() - 1
        self.it = L.LsmItems()
        self.held = [d, run_start, out, ws]
        for f in ("keys", "key_off", "vals", "val_off", "seqno", "vtype"):
            t = d[f]
            if t.numel() == 0:  # (an empty tensor has no address; the library wants every array non-NULL)
                t = torch.zeros(1, dtype=t.dtype, device="cuda")
                self.held.append(t)
            setattr(self.it, f, t.data_ptr())
        self.it.n_items = d["seqno"].numel()
        self.need = L.lib().lsm_merge_workspace_size(self.it.n_items, self.n_runs)
        assert ws.numel() >= self.need and ws.data_ptr() % 256 == 0
        flags = (L.MERGE_EVICT_TOMBSTONES if evict else 0) | (L.MERGE_ZERO_SEQNOS if zero else 0)
        p = lambda t: C.c_void_p(t.data_ptr())
        self.args = (C.byref(self.it), p(run_start), self.n_runs, thr & (2 ** 64 - 1), flags, p(out["keys"]),
                     p(out["key_off"]), p(out["vals"]), p(out["val_off"]), p(out["seqno"]), p(out["vtype"]),
                     p(out["src"]) if with_src else None, p(out["n_out"]), p(out["status"]), p(ws), ws.numel())

    def launch(self, stream=None):
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        rc = self.L.lib().lsm_merge_runs(*self.args, C.c_void_p(s.cuda_stream))
        assert rc == 0, rc


def read_outputs(out, n_runs):
    """Every output as numpy, whole (the caller has synchronised)."""
    g = {f: out[f].cpu().numpy() for f in OUT_FIELDS}
    return {"keys": g["keys"], "vals": g["vals"], "key_off": g["key_off"].view(np.uint64),
            "val_off": g["val_off"].view(np.uint64), "seqno": g["seqno"].view(np.uint64), "vtype": g["vtype"],
            "src": g["src"].view(np.uint32), "n_out": int(g["n_out"].view(np.uint64)[0]),
            "status": g["status"].view(np.int32)[:n_runs].tolist()}


def items_of(g):
    """read_outputs() -> (items, src) of the first n_out entries."""
    n_out = g["n_out"]
    ko, vo = g["key_off"][:n_out + 1], g["val_off"][:n_out + 1]
    assert ko[0] == 0 and vo[0] == 0
    keys, vals = g["keys"][:int(ko[-1])].tobytes(), g["vals"][:int(vo[-1])].tobytes()
    items = [(keys[int(ko[j]):int(ko[j + 1])], vals[int(vo[j]):int(vo[j + 1])], int(g["seqno"][j]), int(g["vtype"][j]))
             for j in range(n_out)]
    return items, g["src"][:n_out].tolist()


def assert_model(g, runs, thr=0, evict=False, zero=False, with_src=True):
    """read_outputs() == merge_model.merge_runs: statuses, n_out, items and src."""
    want, want_src, _ = M.merge_runs(runs, thr, evict, zero)
    assert g["status"] == [0] * len(runs)
    assert g["n_out"] == len(want)
    got, src = items_of(g)
    if with_src:
        assert src == want_src
    assert got == want
    return want, want_src


def assert_rejected(g, status):
    """The documented rejection: the given per-run statuses and n_out == 0."""
    assert g["status"] == status and BAD_ARG in status
    assert g["n_out"] == 0


def assert_extents(g, runs, thr=0, evict=False, zero=False, fill=CANARY):
    """assert_model, and nothing outside the defined outputs was written: the arenas from
    their last byte on, seqno / vtype / src from entry n_out on, the offsets past entry
    n_out."""
    want, _ = assert_model(g, runs, thr, evict, zero)
    n_out = len(want)
    kt, vt = sum(len(it[0]) for it in want), sum(len(it[1]) for it in want)
    assert int(g["key_off"][n_out]) == kt and int(g["val_off"][n_out]) == vt
    assert (g["keys"][kt:] == fill).all() and (g["vals"][vt:] == fill).all()
    word = int.from_bytes(bytes([fill]) * 8, "little")
    n = sum(len(r) for r in runs)
    assert len(g["key_off"]) == n + 1 and len(g["seqno"]) == max(n, 1)
    assert (g["seqno"][n_out:] == word).all() and (g["vtype"][n_out:] == fill).all()
    assert (g["src"][n_out:] == word & 0xFFFFFFFF).all()
    assert (g["key_off"][n_out + 1:] == word).all() and (g["val_off"][n_out + 1:] == word).all()
    return want


def run_call(L, runs, thr=0, evict=False, zero=False, ws=None, run_start=None, with_src=True, fill=CANARY):
    """One call through the C ABI with fresh canary outputs; ws: the workspace to use (default:
    a fresh one); run_start: the list handed to the device instead of the runs' own.
    Returns read_outputs()."""
    import torch
    d, rs = to_device(L, runs)
    n = sum(len(r) for r in runs)
    kb, vb = input_bytes(runs)
    out = alloc_outputs(L, n, kb, vb, len(runs), fill)
    if ws is None:
        ws = alloc_workspace(L, n, len(runs))
    d_rs = torch.tensor(rs if run_start is None else run_start, dtype=torch.int64, device="cuda")
    MergeCall(L, d, d_rs, out, ws, thr, evict, zero, with_src).launch()
    torch.cuda.synchronize()
    return read_outputs(out, len(runs))


def check_call(L, runs, thr=0, evict=False, zero=False):
    """check() through the C ABI: a zeroed workspace of its own (so a position of perm that a
    wrong kernel leaves unwritten reads as item 0, whatever ran before) and canary outputs."""
    assert all(M.run_is_sorted(r) for r in runs)
    want = assert_extents(run_call(L, runs, thr, evict, zero), runs, thr, evict, zero)
    return want, M.merge_runs(runs, thr, evict, zero)[2]


def capture(fn):
    """fn() once on a side stream, then captured on a single stream: a linear graph."""
    import torch
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g
