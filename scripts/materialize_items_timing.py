#!/usr/bin/env python3
"""Device-event time of lsm_materialize_items_plan / lsm_materialize_items beside the copy
ceiling and beside the torch path they replace (diagnostic; results in
profiles/materialize_items_timing.txt).

    python scripts/materialize_items_timing.py [--scale S] [--reps R] [--compare-blocks N] [--out FILE]

Shapes (bench.make_workload, seeded; encoded with lsm_encode_blocks, decoded with
lsm_decode_blocks, then timed):
  headline   16-byte keys / 64-byte values, 52 rows per 4 KiB block, 2^20 blocks
  prefix16k  40-byte keys (32-byte shared prefix) / 256-byte values, 56 rows per 16 KiB
             block, 2^18 blocks
  block1m    16 / 64-byte rows, 13108 rows per 1 MiB block, 4096 blocks
(--scale divides the block counts).  Per shape: the outputs are checked against the items
that were encoded, then plan and gather are timed separately: two warm-up calls, R calls
between two device events, three rounds; minimum, median and spread.  Bytes moved come
from the shape: 25 B of parsed row read, key and value bytes read and written, 16 B of
offsets and 9 B of seqno / vtype per row.  The copy ceiling is lsm-tree_amd/ceiling's
streaming copy, measured in the same run (bench.ceilings).
Comparison: at --compare-blocks headline blocks (the torch path builds >= 24 B of int64
index tensors per value byte, so it cannot hold the full shape) the wrapper's
materialize_items is timed against materialize_keys + decoded_to_items on the same
input, the two alternating, after their outputs were checked equal; both include their
allocations and their one read-back."""
import argparse
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT / "lsm-tree_amd", ROOT / "oracle", ROOT):
    sys.path.insert(0, str(p))

SHAPES = (("headline", 1 << 20, 52, 16, 64, "counter"),
          ("prefix16k", 1 << 18, 56, 40, 256, "prefix"),
          ("block1m", 1 << 12, 13108, 16, 64, "counter"))


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


def decoded(torch, bench, L, nb, per_block, key_len, val_len, kind):
    """One shape encoded and decoded: (items, blocks, block_off, decode output, rows)."""
    items, starts, n = bench.make_workload(torch, L, nb, per_block, key_len, val_len, kind=kind)
    enc = L.Encoder().encode(items, starts, nb)
    torch.cuda.synchronize()
    assert bool((enc["status"][:nb] == 0).all().item())
    out = L.decode_blocks(enc["buf"], enc["block_off"], nb, item_cap=n)
    torch.cuda.synchronize()
    assert bool((out["status"][:nb] == 0).all().item())
    return items, enc["buf"], enc["block_off"], out, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--compare-blocks", type=int, default=1 << 16)
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

    def stats(ms):
        return f"min {min(ms) * 1e3:.1f} us, median {statistics.median(ms) * 1e3:.1f} us, " \
               f"spread {(max(ms) - min(ms)) * 1e3:.1f} us"

    out(f"materialize_items_timing {time.strftime('%Y-%m-%d')} {torch.cuda.get_device_name(0)}; device events, "
        f"3 rounds of {a.reps}")
    ceil = bench.ceilings(torch)["copy_GBps"]
    out(f"copy ceiling (16 B/lane streaming copy, read + write): {ceil:.0f} GB/s")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())

    for name, nb, per_block, key_len, val_len, kind in SHAPES:
        nb = max(1, nb // a.scale)
        items, blocks, block_off, dec, n = decoded(torch, bench, L, nb, per_block, key_len, val_len, kind)
        kb, vb = n * key_len, n * val_len
        args, ps = L._mi_args(blocks, block_off, nb, dec)
        dst = L._mi_alloc("cuda", n, kb, vb)
        end = torch.zeros(3, dtype=torch.int64, device="cuda")
        res = torch.zeros(2, dtype=torch.int32, device="cuda")
        ws = torch.empty(lib.lsm_materialize_items_workspace_size(n), dtype=torch.uint8, device="cuda")

        def plan():
            rc = lib.lsm_materialize_items_plan(*args, None, p(dst["key_off"]), p(dst["val_off"]), n, p(end),
                                                p(res[0:]), p(ws), ws.numel(), s)
            assert rc == 0, rc

        def gather():
            rc = lib.lsm_materialize_items(*args, None, p(end), p(dst["key_off"]), p(dst["val_off"]), p(dst["keys"]),
                                           kb, p(dst["vals"]), vb, p(dst["seqno"]), p(dst["vtype"]), n, p(res[1:]), s)
            assert rc == 0, rc

        plan()
        gather()
        torch.cuda.synchronize()
        assert res.cpu().tolist() == [0, 0] and end.cpu().tolist() == [n, kb, vb]
        for f, size in (("keys", kb), ("vals", vb), ("key_off", n + 1), ("val_off", n + 1), ("seqno", n), ("vtype", n)):
            assert torch.equal(dst[f][:size], items[f][:size]), (name, f)
        del items
        moved = 25 * n + 2 * (kb + vb) + 16 * n + 9 * n
        pm, gm = timed(torch, plan, a.reps), timed(torch, gather, a.reps)
        rate = moved / (statistics.median(gm) * 1e-3) / 1e9
        out(f"{name}: {n} rows of {key_len} / {val_len} bytes, {nb} blocks of {per_block}; "
            f"{(kb + vb) / 1e9:.2f} GB of keys and values, {moved / 1e9:.2f} GB moved by the gather")
        out(f"    plan:   {stats(pm)}")
        out(f"    gather: {stats(gm)}: {rate:.0f} GB/s = {rate / ceil:.2f} of the copy ceiling")
        del dst, ws, blocks, block_off, dec, args, ps
        torch.cuda.empty_cache()

    nb = max(1, a.compare_blocks // a.scale)
    _, nb0, per_block, key_len, val_len, kind = SHAPES[0]
    items, blocks, block_off, dec, n = decoded(torch, bench, L, nb, per_block, key_len, val_len, kind)
    del items

    def torch_path():
        keys, key_off = L.materialize_keys(blocks, block_off, nb, dec, n)
        return L.decoded_to_items(blocks, block_off, nb, dec, keys, key_off)

    def hip_path():
        return L.materialize_items(blocks, block_off, nb, dec)

    x, y = torch_path(), hip_path()
    torch.cuda.synchronize()
    kb, vb = n * key_len, n * val_len
    for f, size in (("keys", kb), ("vals", vb), ("key_off", n + 1), ("val_off", n + 1), ("seqno", n), ("vtype", n)):
        assert torch.equal(x[f][:size], y[f][:size]), f
    del x, y
    old, new = [], []
    for _ in range(3):  # the two paths alternate
        old += timed(torch, torch_path, 3, rounds=1)
        new += timed(torch, hip_path, 3, rounds=1)
    out(f"comparison at {nb} headline blocks ({n} rows, {vb / 1e6:.0f} MB of values; the torch path's index "
        f"tensors are >= {24 * vb / 1e9:.1f} GB), wrappers with their allocations and read-back, alternating:")
    out(f"    materialize_keys + decoded_to_items: {stats(old)}")
    out(f"    materialize_items:                   {stats(new)}")
    out(f"    ratio of medians: {statistics.median(old) / statistics.median(new):.1f}x")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
