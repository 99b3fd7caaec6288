#!/usr/bin/env python3
"""Device-event time of lsm_lz4_compress_blocks alone (diagnostic; results in
profiles/lz4_compress.txt).

    python scripts/lz4_compress_rate.py [--blocks N] [--reps R] [--out FILE]

Two batches of N (default 65,536) 4 KiB-class data blocks, encoded on the device:
  (a) 52 rows per block of 12-byte keys and JSON-like values (compresses ~3x);
  (b) the configs[1] shape of bench.py: 52 items of 16-byte counter keys and
      64-byte random values per block (nearly incompressible).
Batch (a) is a tile of 1,024 distinct blocks' items repeated over the batch (the
rows are built on the host; the compressor's work per block depends on the block's
bytes alone).  Per batch: the compress call (two warm-up calls, then R timed calls
between two device events, 3 rounds: minimum, median, spread) as GiB/s of input
(header + payload bytes read), the stored size, the lsm_encode_blocks call of the
same blocks timed the same way as the yardstick, and single-thread liblz4
(pyarrow "lz4_raw") on the host over the first 2,048 payloads, host clock."""
import argparse
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT / "lsm-tree_amd", ROOT / "oracle", ROOT / "tests", ROOT):
    sys.path.insert(0, str(p))

TILE = 1024
ROWS = 52


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


def json_batch(torch, L, nb):
    """Device lsm_items of nb blocks x ROWS JSON rows: a TILE-block tile of rows, repeated."""
    import pyoracle
    from lz4_compress_corpus import json_rows  # (the tests' JSON-valued rows)
    assert nb % TILE == 0
    tile = L.items_to_device(pyoracle.Items.from_list(json_rows(TILE * ROWS)))
    reps, n1 = nb // TILE, TILE * ROWS
    items = {}
    for f, off in (("keys", "key_off"), ("vals", "val_off")):
        size = int(tile[off][n1].item())
        items[f] = L.padded_bytes(size * reps)
        items[f][:size * reps].copy_(tile[f][:size].repeat(reps))
        base = torch.arange(reps, dtype=torch.int64, device="cuda")[:, None] * size
        items[off] = torch.cat([(tile[off][:n1][None, :] + base).reshape(-1),
                                torch.tensor([size * reps], dtype=torch.int64, device="cuda")])
    items["seqno"] = tile["seqno"][:n1].repeat(reps)
    items["vtype"] = tile["vtype"][:n1].repeat(reps)
    starts = (torch.arange(nb + 1, dtype=torch.int64, device="cuda") * ROWS).to(torch.int32)
    return items, starts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import pyarrow as pa
    import torch
    import bench
    import lsmgpu as L
    from lz4_check import lz4_check
    assert torch.cuda.is_available(), "needs a GPU"
    lib = L.lib()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    nb = a.blocks
    out(f"lz4_compress_rate {time.strftime('%Y-%m-%d')} {torch.cuda.get_device_name(0)}: {nb} blocks per batch; "
        f"device events, 3 rounds of {a.reps} calls after 2 warm-up calls")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    codec = pa.Codec("lz4_raw")

    def batch(name, items, starts):
        enc_ctx = L.Encoder()
        enc = enc_ctx.encode(items, starts, nb)
        torch.cuda.synchronize()
        assert bool((enc["status"][:nb] == 0).all().item())
        in_bytes = int(enc["block_off"][nb].item())
        d_in = enc["buf"][:in_bytes + L.LSM_INPUT_PADDING]
        cap = int(lib.lsm_lz4_compress_bound(in_bytes, nb))
        d_out = L.padded_bytes(cap)
        d_off = torch.zeros(nb + 1, dtype=torch.int64, device="cuda")
        d_st = torch.empty(nb, dtype=torch.int32, device="cuda")
        ws = torch.empty(lib.lsm_lz4_compress_workspace_size(nb, in_bytes), dtype=torch.uint8, device="cuda")

        def compress():
            rc = lib.lsm_lz4_compress_blocks(p(d_in), p(enc["block_off"]), nb, p(enc["status"]), p(d_out), cap, p(d_off),
                                             p(d_st), p(ws), ws.numel(), s)
            assert rc == 0, rc

        compress()
        torch.cuda.synchronize()
        assert bool((d_st == 0).all().item())
        stored = int(d_off[nb].item())
        # spot check: the first and last blocks read back
        h_in, h_off = enc["buf"][:in_bytes].cpu().numpy(), enc["block_off"][:nb + 1].cpu().numpy()
        h_out, h_oo = d_out[:stored].cpu().numpy(), d_off.cpu().numpy()
        for b in (0, nb - 1):
            payload = h_in[h_off[b] + 33:h_off[b + 1]].tobytes()
            assert lz4_check(h_out[h_oo[b] + 33:h_oo[b + 1]].tobytes(), len(payload)) == payload
        ms = timed(torch, compress, a.reps)
        med = statistics.median(ms)
        out(f"({name}) lsm_lz4_compress_blocks: {in_bytes} B in ({in_bytes / nb:.0f} B per block), {stored} B stored "
            f"(x{stored / in_bytes:.3f}); min {min(ms):.3f} ms, median {med:.3f} ms, spread {max(ms) - min(ms):.3f} ms; "
            f"{in_bytes / (med * 1e-3) / 2 ** 30:.1f} GiB/s of input")
        ems = timed(torch, lambda: enc_ctx.encode(items, starts, nb, out=enc), a.reps)
        emed = statistics.median(ems)
        out(f"({name}) lsm_encode_blocks of the same blocks: min {min(ems):.3f} ms, median {emed:.3f} ms; "
            f"{in_bytes / (emed * 1e-3) / 2 ** 30:.1f} GiB/s of output; compress / encode = {med / emed:.1f}")
        k = min(nb, 2048)
        payloads = [h_in[h_off[b] + 33:h_off[b + 1]].tobytes() for b in range(k)]
        t0 = time.perf_counter()
        host = sum(len(codec.compress(x, asbytes=True)) for x in payloads)
        dt = time.perf_counter() - t0
        raw = sum(len(x) for x in payloads)
        gpu_stored = int(h_oo[k]) - 33 * k
        out(f"({name}) liblz4 on one host thread, first {k} payloads: {raw / dt / 2 ** 30:.2f} GiB/s, {host} B "
            f"(device streams of the same payloads: {gpu_stored} B, x{gpu_stored / host:.4f})")

    items, starts = json_batch(torch, L, nb)
    batch("a: JSON values", items, starts)
    del items, starts
    items, starts, _ = bench.make_workload(torch, L, nb)
    batch("b: configs[1], random values", items, starts)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
