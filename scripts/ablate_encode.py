#!/usr/bin/env python3
"""Encode ablations on a diagnostic build (LSMGPU_LIB=...libdiag.so): kernel
time with phases of the group kernel's group loop dropped (outputs invalid).
Bits (lsm_block_params.reserved, u8; the table is in csrc/encode_common.hpp):
1 no record stores, 2 no hash / header, 4 no copy-out, 8 no records and no
tails, 16 no next-group DMA, 0x20 the group loop only (no wave-per-block loop;
in the fused instantiation: the look-back gives up), 0x40 / 0x80 phase timers.
Any ablation bit keeps a run off the wave-per-block loop, so the ablations are
compared with the 0x20 run, not with the full one."""
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "lsm-tree_amd", ROOT / "oracle", ROOT / "tests"):
    sys.path.insert(0, str(p))
import torch  # noqa: E402
import bench  # noqa: E402
import lsmgpu  # noqa: E402

# csrc/encode_common.hpp, mirrored
DIAG_NO_RECORD_STORES, DIAG_NO_HASH, DIAG_NO_COPY_OUT, DIAG_NO_RECORDS_TAILS, DIAG_NO_NEXT_DMA = 1, 2, 4, 8, 16
DIAG_NO_WAVE_BLOCKS = 0x20


def main():
    torch.cuda.set_device(0)
    which = sys.argv[1] if len(sys.argv) > 1 else "c1"
    if which == "c1":
        nb = 1 << 20
        items, starts, n = bench.make_workload(torch, lsmgpu, nb)
    else:
        nb = 262144
        items, starts, n = bench.make_workload(torch, lsmgpu, nb, items_per_block=56, key_len=40, val_len=256,
                                               kind="prefix")
    lsmgpu.lib()
    orig = lsmgpu.LsmBlockParams
    enc_ctx = lsmgpu.Encoder()
    enc = enc_ctx.encode(items, starts, nb)
    torch.cuda.synchronize()
    bits_list = [(0, "full"), (DIAG_NO_WAVE_BLOCKS, "group loop only"), (DIAG_NO_RECORD_STORES, "no record stores"),
                 (DIAG_NO_HASH, "no hash/header"), (DIAG_NO_COPY_OUT, "no copy-out"),
                 (DIAG_NO_RECORD_STORES | DIAG_NO_HASH | DIAG_NO_COPY_OUT, "none of records/hash/copy-out"),
                 (DIAG_NO_RECORDS_TAILS, "no records and no tails"), (DIAG_NO_NEXT_DMA, "no next-group DMA")]
    res = {b: [] for b, _ in bits_list}
    for r in range(3):
        for bits, name in bits_list:
            lsmgpu.LsmBlockParams = lambda ri, bt, c, rr, hr, bits=bits: orig(ri, bt, c, bits, hr)
            enc_ctx.encode(items, starts, nb, out=enc)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                enc_ctx.encode(items, starts, nb, out=enc)
            e1.record()
            torch.cuda.synchronize()
            res[bits].append(e0.elapsed_time(e1) / 5)
    lsmgpu.LsmBlockParams = orig
    base = sorted(res[DIAG_NO_WAVE_BLOCKS])[1]
    for bits, name in bits_list:
        v = sorted(res[bits])[1]
        print(f"{which} {name:32s} {v:.4f} ms  (delta vs the group loop {v - base:+.4f})")


if __name__ == "__main__":
    main()
