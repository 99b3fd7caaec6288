#!/usr/bin/env python3
"""Device-event time of lsm_merge_runs beside the encode of its own output and
the copy ceiling (diagnostic; results in profiles/merge_timing.txt).

    python scripts/merge_timing.py [--leg N] [--reps R] [--items M] [--no-ceiling]

Legs: 4 runs and 16 runs of the configs[1] item shape (16-byte keys, 64-byte
values), and 4 runs of 40 / 256-byte items (32-byte shared prefix + counter),
about 1 M items each, random interleave, 10 % of the keys present in two runs,
GC threshold in the middle of the seqno range.  The time per kernel comes from
a separate run under `rocprofv3 --kernel-trace --stats` with --leg and a small
--reps (scripts/kstats.py prints its CSV)."""
import argparse
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT / "lsm-tree_amd", ROOT / "oracle", ROOT):
    sys.path.insert(0, str(p))

LEGS = [("4 runs 16/64", 4, 16, 64, 4096), ("16 runs 16/64", 16, 16, 64, 4096), ("4 runs 40/256", 4, 40, 256, 16384)]
MAX_SEQ = 1000


def make_runs(n_target, n_runs, key_len, val_len, seed):
    """Numpy SoA of all runs back to back (each run sorted by key; a key is in at most two runs)."""
    rng = np.random.default_rng(seed)
    n_keys = int(n_target / 1.1)
    ctr = np.arange(n_keys, dtype=np.uint64)
    run = rng.integers(0, n_runs, n_keys)
    dup = rng.random(n_keys) < 0.10
    run2 = (run[dup] + 1 + rng.integers(0, n_runs - 1, int(dup.sum()))) % n_runs
    ctr = np.concatenate([ctr, ctr[dup]])
    run = np.concatenate([run, run2])
    order = np.lexsort((ctr, run))
    ctr, run = ctr[order], run[order]
    n = len(ctr)
    keys = np.zeros((n, key_len), np.uint8)
    if key_len > 16:
        keys[:, :key_len - 8] = rng.integers(0, 256, key_len - 8, dtype=np.uint8)  # shared prefix
    for b in range(8):
        keys[:, key_len - 1 - b] = ((ctr >> np.uint64(8 * b)) & np.uint64(0xFF)).astype(np.uint8)
    vtype = np.where(rng.random(n) < 0.05, 1, 0).astype(np.uint8)
    vlen = np.where(vtype == 1, 0, val_len).astype(np.int64)
    val_off = np.concatenate([[0], np.cumsum(vlen)]).astype(np.int64)
    vals = rng.integers(0, 256, int(val_off[-1]), dtype=np.uint8)
    seqno = rng.integers(0, MAX_SEQ, n).astype(np.int64)
    run_start = np.searchsorted(run, np.arange(n_runs + 1)).astype(np.int64)
    return {"keys": keys.reshape(-1), "key_off": np.arange(n + 1, dtype=np.int64) * key_len, "vals": vals,
            "val_off": val_off, "seqno": seqno, "vtype": vtype}, run_start


def timed(torch, fn, reps):
    fn()
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def copy_ceiling(torch, nbytes=1 << 30, reps=5):
    lib = C.CDLL(str(ROOT / "lsm-tree_amd" / "ceiling" / "liblsmceiling.so"))
    lib.lsm_ceiling_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    src.random_(0, 256)
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ms = timed(torch, lambda: lib.lsm_ceiling_copy(src.data_ptr(), dst.data_ptr(), nbytes, s), reps)
    return 2 * nbytes / (ms * 1e-3) / 1e9


def run_leg(torch, L, leg, n_items, reps, out):
    name, n_runs, key_len, val_len, block_size = LEGS[leg]
    host, run_start = make_runs(n_items, n_runs, key_len, val_len, seed=leg + 1)
    n = len(host["seqno"])
    d = {f: (L.to_device_bytes(a) if f in ("keys", "vals") else torch.from_numpy(a).cuda()) for f, a in host.items()}
    d_rs = torch.from_numpy(run_start).cuda()
    thr = MAX_SEQ // 2
    res = L.merge_runs(d, d_rs, thr, evict_tombstones=True)
    torch.cuda.synchronize()
    assert (res["status"] == 0).all().item()
    n_out = int(res["n_out"].cpu()[0])
    # the same call with every buffer allocated once
    it = L.LsmItems()
    for f in ("keys", "key_off", "vals", "val_off", "seqno", "vtype"):
        setattr(it, f, d[f].data_ptr())
    it.n_items = n
    ws = torch.empty(L.lib().lsm_merge_workspace_size(n, n_runs), dtype=torch.uint8, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())

    def merge():
        rc = L.lib().lsm_merge_runs(C.byref(it), p(d_rs), n_runs, thr, L.MERGE_EVICT_TOMBSTONES, p(res["keys"]),
                                    p(res["key_off"]), p(res["vals"]), p(res["val_off"]), p(res["seqno"]),
                                    p(res["vtype"]), p(res["src"]), p(res["n_out"]), p(res["status"]), p(ws),
                                    ws.numel(), s)
        assert rc == 0, rc

    merge_ms = timed(torch, merge, reps)
    ko = res["key_off"][:n_out + 1].cpu().numpy().view(np.uint64)
    vo = res["val_off"][:n_out + 1].cpu().numpy().view(np.uint64)
    in_bytes = int(host["key_off"][-1]) + int(host["val_off"][-1]) + 25 * n + 8 * (n_runs + 1)
    out_bytes = int(ko[-1]) + int(vo[-1]) + 25 * n_out + 16 + 4 * n_out + 8
    starts = L.cut_blocks(ko, vo, block_size)
    nb = len(starts) - 1
    merged = {"keys": res["keys"], "key_off": res["key_off"][:n_out + 1], "vals": res["vals"],
              "val_off": res["val_off"][:n_out + 1], "seqno": res["seqno"][:n_out], "vtype": res["vtype"][:n_out]}
    d_starts = torch.from_numpy(starts.astype(np.int32)).cuda()
    enc = L.Encoder()
    eout = enc.encode(merged, d_starts, nb)
    torch.cuda.synchronize()
    assert (eout["status"][:nb] == 0).all().item()
    enc_ms = timed(torch, lambda: enc.encode(merged, d_starts, nb, out=eout), reps)
    gbps = (in_bytes + out_bytes) / (merge_ms * 1e-3) / 1e9
    out(f"{name}: {n} items in, {n_out} out ({nb} blocks of {block_size}); merge {merge_ms * 1e3:.1f} us "
        f"({n / merge_ms / 1e3:.1f} M items/s), bytes read {in_bytes} + written {out_bytes} -> {gbps:.1f} GB/s; "
        f"encode of the output {enc_ms * 1e3:.1f} us; merge / encode = {merge_ms / enc_ms:.2f}")
    return gbps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", type=int, default=None)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--items", type=int, default=1 << 20)
    ap.add_argument("--no-ceiling", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import lsmgpu as L
    assert torch.cuda.is_available(), "needs a GPU"
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out(f"merge_timing {time.strftime('%Y-%m-%d')} {torch.cuda.get_device_name(0)}: reps {a.reps}, device events")
    ceil = None if a.no_ceiling else copy_ceiling(torch)
    if ceil:
        out(f"copy ceiling (lsm_ceiling_copy, 1 GiB, read + write): {ceil:.0f} GB/s")
    for leg in ([a.leg] if a.leg is not None else range(len(LEGS))):
        g = run_leg(torch, L, leg, a.items, a.reps, out)
        if ceil:
            out(f"    = {100 * g / ceil:.1f} % of the copy ceiling")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
