#!/usr/bin/env python3
"""A/B timing of two library builds on the lookup side: bench.py's point_read extra (point read
and seek), its table-scan extra (lsm_scan_table, sync and async) and the legs of
scripts/bench_table_get.py.

usage: scripts/ab_block_reader.py PARENT_LIB RESULT_LIB [--rounds 3] [--out FILE]

Each round runs every library in fresh child processes (LSMGPU_LIB), the libraries alternating:
one child for the two bench.py extras on the configs[1] batch (2^20 blocks), one for
bench_table_get.py (its medians over its own three rounds).  Per figure: each library's median
and spread (max - min) over the rounds, and whether the second library's median is within the
first's spread of the first's median."""
import json
import os
import re
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def child():
    for p in (ROOT, ROOT / "lsm-tree_amd", ROOT / "oracle", ROOT / "tests"):
        sys.path.insert(0, str(p))
    import torch
    import bench
    import lsmgpu
    torch.cuda.set_device(0)
    nb = 1 << 20
    items, starts, n = bench.make_workload(torch, lsmgpu, nb)
    enc = lsmgpu.Encoder().encode(items, starts, nb)
    dec = lsmgpu.Decoder()
    out = dec.alloc_outputs(n, nb, fields=bench.DATA_FIELDS)
    dec.decode(enc["buf"], enc["block_off"], nb, out, n)
    torch.cuda.synchronize()
    pr = bench.bench_point_read(torch, lsmgpu, items, enc, nb, n, reps=20)
    ts = bench.bench_table_scan(torch, lsmgpu, items, enc, nb, n, out, reps=5)
    print(json.dumps({"point_read ms": pr["ms"], "seek ms": pr["seek_ms"], "scan_table ms": ts["ms"],
                      "scan_table_async ms": ts["async_ms"]}), flush=True)


def run(cmd, lib):
    env = dict(os.environ, LSMGPU_LIB=str(Path(lib).resolve()))
    p = subprocess.run([sys.executable] + cmd, env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        print(lib, "FAILED", p.stdout[-1000:], p.stderr[-2000:], flush=True)
        sys.exit(1)
    return p.stdout


def main():
    if sys.argv[1] == "--child":
        return child()
    a, libs, rounds, out_path = sys.argv[1:], [], 3, None
    while a:
        x = a.pop(0)
        if x == "--rounds":
            rounds = int(a.pop(0))
        elif x == "--out":
            out_path = a.pop(0)
        else:
            libs.append(x)
    lines, res = [], {l: {} for l in libs}

    def out(s):
        print(s, flush=True)
        lines.append(s)

    for r in range(rounds):
        for l in libs:
            d = json.loads(run([__file__, "--child"], l).strip().splitlines()[-1])
            for m in re.finditer(r"^\s+(\S.*?)\s+min .*? median\s+([\d.]+) us", run(
                    [str(ROOT / "scripts" / "bench_table_get.py"), "--reps", "20"], l), re.M):
                d[m.group(1) + " us"] = float(m.group(2))
            for k, v in d.items():
                res[l].setdefault(k, []).append(v)
            out(f"round {r} {l}: " + "  ".join(f"{k} {v}" for k, v in d.items()))
    out(f"{'figure':52s} " + " ".join(f"{'median':>10s} {'spread':>8s}" for _ in libs) + "  verdict")
    for k in res[libs[0]]:
        med = [statistics.median(res[l][k]) for l in libs]
        spread = [max(res[l][k]) - min(res[l][k]) for l in libs]
        ok = med[-1] <= med[0] + spread[0]
        out(f"{k:52s} " + " ".join(f"{m:10.4f} {s:8.4f}" for m, s in zip(med, spread)) +
            ("  within the first's spread" if ok else "  SLOWER"))
    if out_path:
        Path(out_path).parent.mkdir(parents=True, exist_ok=True)
        Path(out_path).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
