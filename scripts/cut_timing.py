#!/usr/bin/env python3
"""Device-event time of the device block cut beside what it replaces (diagnostic;
results in profiles/cut_timing.txt).

    python scripts/cut_timing.py [--blocks N] [--reps R] [--only LEG] [--out FILE]

The headline batch: 52 items per block x 1 Mi blocks of 16-byte keys and 64-byte
values (bench.make_workload).  Legs, all in this process:
  (a) lsm_cut_blocks_device over the device offsets;
  (b) what a caller had to do without it: both offset arrays to the host (pinned
      buffers), the host lsm_cut_blocks loop, the starts back to the device;
  (c) lsm_index_entries for the batch (after one encode, for the block offsets);
  (d) the lsm_encode_blocks call of the same batch, for scale.
Each leg: two warm-up calls, then R timed calls between two device events
(legs with host work end in a synchronise inside the window), repeated 3 times:
the minimum, the median and the spread are printed.  The time per kernel of (a)
comes from a separate run under `rocprofv3 --kernel-trace --stats` with
--only a and a small --reps (scripts/kstats.py prints its CSV); the tile walk's
hop time is cut_walk_kernel's time over the number of tiles."""
import argparse
import ctypes as C
import statistics
import sys
import time
from pathlib import Path


ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT / "lsm-tree_amd", ROOT / "oracle", ROOT):
    sys.path.insert(0, str(p))


def timed(torch, fn, reps, rounds=3):
    fn()
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", choices="abcd", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bench
    import lsmgpu as L
    assert torch.cuda.is_available(), "needs a GPU"
    lib = L.lib()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    def report(name, ms, reps=None):
        out(f"{name}: min {min(ms) * 1e3:.1f} us, median {statistics.median(ms) * 1e3:.1f} us, "
            f"spread {(max(ms) - min(ms)) * 1e3:.1f} us over {len(ms)} rounds of {reps or a.reps}")
        return statistics.median(ms)

    items, ref_starts, n = bench.make_workload(torch, L, a.blocks)
    nb = a.blocks
    tiles = -(-n // L.CUT_TILE_ITEMS)
    out(f"cut_timing {time.strftime('%Y-%m-%d')} {torch.cuda.get_device_name(0)}: {n} items of 16 / 64 bytes, "
        f"{nb} blocks of 52 (block_size 4096), {tiles} tiles of {L.CUT_TILE_ITEMS}; device events")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    want = lambda leg: a.only in (None, leg)
    res = {}

    starts = torch.empty(nb + 1, dtype=torch.int32, device="cuda")
    if want("a"):
        ws = torch.empty(lib.lsm_cut_workspace_size(n), dtype=torch.uint8, device="cuda")
        d_nb = torch.zeros(1, dtype=torch.int64, device="cuda")
        d_st = torch.zeros(1, dtype=torch.int32, device="cuda")

        def cut():
            rc = lib.lsm_cut_blocks_device(p(items["key_off"]), p(items["val_off"]), n, None, 0, 4096, p(starts), nb,
                                           p(d_nb), p(d_st), p(ws), ws.numel(), s)
            assert rc == 0, rc

        cut()
        torch.cuda.synchronize()
        assert int(d_nb.item()) == nb and int(d_st.item()) == 0 and bool((starts == ref_starts).all().item())
        res["a"] = report(f"(a) lsm_cut_blocks_device (workspace {ws.numel() >> 20} MiB)", timed(torch, cut, a.reps))
        del ws

    if want("b"):
        h_ko = torch.empty(n + 1, dtype=torch.int64).pin_memory()
        h_vo = torch.empty(n + 1, dtype=torch.int64).pin_memory()
        h_st = torch.empty(nb + 1, dtype=torch.int32).pin_memory()
        parts = {"d2h": [], "loop": [], "h2d": []}

        def host_path():
            t0 = time.perf_counter()
            h_ko.copy_(items["key_off"], non_blocking=True)
            h_vo.copy_(items["val_off"], non_blocking=True)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            got = lib.lsm_cut_blocks(h_ko.data_ptr(), h_vo.data_ptr(), n, 4096, h_st.data_ptr(), nb)
            assert got == nb
            t2 = time.perf_counter()
            starts.copy_(h_st, non_blocking=True)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            for k, v in zip(("d2h", "loop", "h2d"), (t1 - t0, t2 - t1, t3 - t2)):
                parts[k].append(v * 1e3)

        reps_b = max(1, min(a.reps, 3))  # (each call takes a large fraction of a second)
        res["b"] = report("(b) offsets D2H + host lsm_cut_blocks + starts H2D", timed(torch, host_path, reps_b), reps_b)
        assert bool((starts == ref_starts).all().item())
        out("    host clock, median per call: " + ", ".join(
            f"{k} {statistics.median(v[2:]):.1f} ms" for k, v in parts.items()) +
            f" ({16 * (n + 1) / 1e6:.0f} MB down, {4 * (nb + 1) / 1e6:.1f} MB up, pinned)")
        del h_ko, h_vo, h_st

    if want("c") or want("d"):
        enc = L.Encoder()
        eout = enc.encode(items, ref_starts, nb)
        torch.cuda.synchronize()
        assert bool((eout["status"][:nb] == 0).all().item())
    if want("c"):
        it = L.LsmItems()
        it.keys, it.key_off, it.seqno, it.n_items = items["keys"].data_ptr(), items["key_off"].data_ptr(), \
            items["seqno"].data_ptr(), n
        cap = 16 * nb
        o = {"keys": torch.empty(cap + 64, dtype=torch.uint8, device="cuda"),
             "key_off": torch.empty(nb + 1, dtype=torch.int64, device="cuda"),
             "seqno": torch.empty(nb, dtype=torch.int64, device="cuda"),
             "hoff": torch.empty(nb, dtype=torch.int64, device="cuda"),
             "hsize": torch.empty(nb, dtype=torch.int32, device="cuda"),
             "res": torch.empty(1, dtype=torch.int32, device="cuda")}
        iws = torch.empty(lib.lsm_index_entries_workspace_size(nb), dtype=torch.uint8, device="cuda")

        def index():
            rc = lib.lsm_index_entries(C.byref(it), p(ref_starts), p(eout["block_off"]), nb, 0, p(o["keys"]), cap,
                                       p(o["key_off"]), p(o["seqno"]), p(o["hoff"]), p(o["hsize"]), p(o["res"]), p(iws),
                                       iws.numel(), s)
            assert rc == 0, rc

        index()
        torch.cuda.synchronize()
        assert int(o["res"].item()) == 0 and int(o["key_off"][-1].item()) == cap
        res["c"] = report("(c) lsm_index_entries", timed(torch, index, a.reps))
    if want("d"):
        res["d"] = report("(d) lsm_encode_blocks of the batch",
                          timed(torch, lambda: enc.encode(items, ref_starts, nb, out=eout), a.reps))
    if "a" in res and "b" in res:
        out(f"(a) / (b) = {res['a'] / res['b']:.4f}")
    if "a" in res and "d" in res:
        out(f"(a) / (d) = {res['a'] / res['d']:.3f}")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
