#!/usr/bin/env python3
"""First numbers of lsm_merge_read (diagnostic; results in profiles/merge_read_first.txt).

    python scripts/merge_read_first.py [--leg N] [--reps R] [--no-baseline] [--out FILE]

Leg 0: 4096 groups x 4 sources, runs of 48..80 rows (about 1 M items), 16-byte keys, 64-byte
values, a key of a group in about every fourth run of it, 5 % tombstones, the snapshot in the
middle of the seqno range.  Leg 1: one group, four runs of 256 Ki rows (the shape at which the
rank kernel's full-run binary search is the weak spot).
Both are timed with device events after a warm-up, every buffer allocated once.  The
baseline is the only route without the call: one lsm_merge_runs per group over that group's
runs copied contiguous (the copies are made beforehand and not timed); 64 of the groups are
timed and the result is scaled to all of them.  For leg 1 it is one lsm_merge_runs over the
same input.  The time per kernel comes from a separate run under
`rocprofv3 --kernel-trace --stats` with --leg, --no-baseline and a small --reps
(scripts/kstats.py prints its CSV)."""
import argparse
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT / "lsm-tree_amd", ROOT / "oracle", ROOT):
    sys.path.insert(0, str(p))

LEGS = [("4096 groups x 4 sources, ~64 rows", 4096, 4, (48, 81), 512), ("1 group x 4 sources, 256 Ki rows", 1, 4, (1 << 18, (1 << 18) + 1), 1 << 21)]
KEY_LEN, VAL_LEN, MAX_SEQ = 16, 64, 1000
BASE_GROUPS = 64


def make_input(n_groups, n_src, len_range, key_space, seed):
    """Numpy SoA of every run back to back, source-major (run s * n_groups + g), each run sorted
    by key (distinct keys inside a run: the group id, then a counter below key_space)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(len_range[0], len_range[1], n_src * n_groups)
    run_start = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(run_start[-1])
    ctr = np.empty(n, np.uint64)
    grp = np.empty(n, np.uint64)
    for r in range(n_src * n_groups):
        a, b = run_start[r], run_start[r + 1]
        ctr[a:b] = np.sort(rng.choice(key_space, int(b - a), replace=False))
        grp[a:b] = r % n_groups
    keys = np.zeros((n, KEY_LEN), np.uint8)
    for b in range(8):
        keys[:, 7 - b] = ((grp >> np.uint64(8 * b)) & np.uint64(0xFF)).astype(np.uint8)
        keys[:, 15 - b] = ((ctr >> np.uint64(8 * b)) & np.uint64(0xFF)).astype(np.uint8)
    vtype = np.where(rng.random(n) < 0.05, 1, 0).astype(np.uint8)
    vlen = np.where(vtype == 1, 0, VAL_LEN).astype(np.int64)
    val_off = np.concatenate([[0], np.cumsum(vlen)]).astype(np.int64)
    return {"keys": keys.reshape(-1), "key_off": np.arange(n + 1, dtype=np.int64) * KEY_LEN,
            "vals": rng.integers(0, 256, int(val_off[-1]), dtype=np.uint8), "val_off": val_off,
            "seqno": rng.integers(0, MAX_SEQ, n).astype(np.int64), "vtype": vtype}, run_start


def group_input(host, run_start, n_groups, n_src, g):
    """The runs of group g copied contiguous: (SoA, run_start) as lsm_merge_runs takes them."""
    spans = [(int(run_start[s * n_groups + g]), int(run_start[s * n_groups + g + 1])) for s in range(n_src)]
    idx = np.concatenate([np.arange(a, b) for a, b in spans])
    vo = host["val_off"]
    vlen = (vo[idx + 1] - vo[idx]).astype(np.int64)
    vals = np.concatenate([host["vals"][vo[a]:vo[b]] for a, b in spans]) if len(idx) else np.zeros(0, np.uint8)
    return {"keys": host["keys"].reshape(-1, KEY_LEN)[idx].reshape(-1),
            "key_off": np.arange(len(idx) + 1, dtype=np.int64) * KEY_LEN, "vals": vals,
            "val_off": np.concatenate([[0], np.cumsum(vlen)]).astype(np.int64), "seqno": host["seqno"][idx],
            "vtype": host["vtype"][idx]}, np.concatenate([[0], np.cumsum([b - a for a, b in spans])]).astype(np.int64)


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


def to_device(torch, L, host):
    return {f: (L.to_device_bytes(a) if f in ("keys", "vals") else torch.from_numpy(a).cuda()) for f, a in host.items()}


def items_struct(L, d):
    it = L.LsmItems()
    for f in ("keys", "key_off", "vals", "val_off", "seqno", "vtype"):
        setattr(it, f, d[f].data_ptr())
    it.n_items = d["seqno"].numel()
    return it


def runs_call(torch, L, d, run_start):
    """-> a closure launching lsm_merge_runs (thr 0, no flag) with every buffer allocated once."""
    d_rs = torch.from_numpy(run_start).cuda()
    res = L.merge_runs(d, d_rs)
    it = items_struct(L, d)
    n_runs = len(run_start) - 1
    ws = torch.empty(L.lib().lsm_merge_workspace_size(it.n_items, n_runs), dtype=torch.uint8, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    held = (d, d_rs, res, ws, it)

    def launch():
        rc = L.lib().lsm_merge_runs(C.byref(it), p(d_rs), n_runs, 0, 0, p(res["keys"]), p(res["key_off"]),
                                    p(res["vals"]), p(res["val_off"]), p(res["seqno"]), p(res["vtype"]), p(res["src"]),
                                    p(res["n_out"]), p(res["status"]), p(ws), ws.numel(), s)
        assert rc == 0 and held, rc
    return launch, res


def run_leg(torch, L, leg, reps, baseline, out):
    name, n_groups, n_src, len_range, key_space = LEGS[leg]
    host, run_start = make_input(n_groups, n_src, len_range, key_space, seed=leg + 1)
    n = len(host["seqno"])
    d = to_device(torch, L, host)
    d_rs = torch.from_numpy(run_start).cuda()
    snap = MAX_SEQ // 2
    res = L.merge_read(d, d_rs, n_groups, n_src, snap)
    torch.cuda.synchronize()
    assert (res["status"] == 0).all().item()
    n_out = int(res["group_start"][n_groups].item())
    it = items_struct(L, d)
    ws = torch.empty(L.lib().lsm_merge_read_workspace_size(n, n_groups, n_src), dtype=torch.uint8, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())

    def read():
        rc = L.lib().lsm_merge_read(C.byref(it), p(d_rs), n_groups, n_src, snap, None, None, 0, p(res["keys"]),
                                    p(res["key_off"]), p(res["vals"]), p(res["val_off"]), p(res["seqno"]),
                                    p(res["vtype"]), p(res["src"]), p(res["group_start"]), p(res["status"]), p(ws),
                                    ws.numel(), s)
        assert rc == 0, rc

    read_ms = timed(torch, read, reps)
    out(f"{name}: {n} items in {n_src * n_groups} runs, {n_out} rows out; lsm_merge_read {read_ms * 1e3:.1f} us "
        f"({n / read_ms / 1e3:.1f} M items/s)")
    if not baseline:
        return
    if n_groups == 1:
        launch, r = runs_call(torch, L, d, run_start)
        base_ms = timed(torch, launch, reps)
        out(f"    lsm_merge_runs over the same input (thr 0, {int(r['n_out'].item())} items out): {base_ms * 1e3:.1f} us; "
            f"merge_read / merge_runs = {read_ms / base_ms:.2f}")
        return
    groups = np.linspace(0, n_groups - 1, BASE_GROUPS).astype(int)
    calls = [runs_call(torch, L, to_device(torch, L, gi), rs)[0]
             for gi, rs in (group_input(host, run_start, n_groups, n_src, int(g)) for g in groups)]

    def all_groups():
        for launch in calls:
            launch()

    base_ms = timed(torch, all_groups, max(reps // 4, 3))
    scaled = base_ms * n_groups / BASE_GROUPS
    out(f"    one lsm_merge_runs per group, {BASE_GROUPS} groups timed: {base_ms * 1e3:.1f} us = {base_ms * 1e3 / BASE_GROUPS:.1f} us "
        f"per group; scaled to {n_groups} groups {scaled * 1e3:.0f} us; per-group route / merge_read = {scaled / read_ms:.1f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", type=int, default=None)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import lsmgpu as L
    assert torch.cuda.is_available(), "needs a GPU"
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out(f"merge_read_first {time.strftime('%Y-%m-%d')} {torch.cuda.get_device_name(0)}: reps {a.reps}, device events")
    for leg in ([a.leg] if a.leg is not None else range(len(LEGS))):
        run_leg(torch, L, leg, a.reps, not a.no_baseline, out)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
