#!/usr/bin/env python3
"""Device-event time of lsm_table_range_rows_plan and lsm_table_range_rows beside the route that
existed before them, a scan and a materialize of the whole table (diagnostic; the first
measurement is in DESIGN.md §6.11).

    python scripts/bench_table_range_rows.py [--blocks N] [--queries Q] [--variant LABEL=LIB] [--out FILE]

Table: config-2 shape (16-byte keys / 64-byte values, 52 items per 4 KiB block, --blocks blocks,
65536 by default), built on the device by write_table under a full and under a two-level index;
the keys are the even big-endian counters.
Ranges: --queries (65536 by default) inclusive bound pairs at random places, of 10, 100 and
1,000 rows.  lsm_table_range gives the positions (not timed here: DESIGN.md §6.10).  Each leg's
rows are checked first against the item list: every key, value, seqno and offset of every run.
Legs: the plan call and the rows call of each batch, each timed by itself (the rows call on the
workspace the plan left), and the whole-table route: scan_table(sync=False) and
materialize_items of every block into preallocated outputs, which yields the rows of any range
as a slice.  --variant times the same two calls of another build of the library (e.g. one
compiled with -DLSM_RR_GROUP=64) beside the product's.
Timing: two warm-up calls, then per leg `reps` calls between two device events, three rounds,
the legs alternating within a round; minimum, median and spread.  Bytes of a batch: the touched
blocks (every (query, block) pair's block, once) plus the output (keys, values, two 8-byte
offsets, seqno and vtype of every row); the rate over plan + rows is held against the 16 B/lane
copy ceiling measured in the same run."""
import argparse
import ctypes as C
import hashlib
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT / "lsm-tree_amd", ROOT / "oracle", ROOT):
    sys.path.insert(0, str(p))

ROWS_PER_RANGE = {10: 20, 100: 10, 1000: 3}  # rows per range -> calls per timed window


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=1 << 16)
    ap.add_argument("--queries", type=int, default=1 << 16)
    ap.add_argument("--variant", default=None, help="LABEL=path of another liblsmgpu.so to time beside the product")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bench
    import lsmgpu as L
    assert torch.cuda.is_available(), "needs a GPU"
    libs = {"": L.lib()}
    if a.variant:
        label, path = a.variant.split("=", 1)
        v = C.CDLL(path)
        for fn in ("lsm_table_range_rows_workspace_size", "lsm_table_range_rows_plan", "lsm_table_range_rows"):
            getattr(v, fn).restype = getattr(libs[""], fn).restype
            getattr(v, fn).argtypes = getattr(libs[""], fn).argtypes
        libs[f" [{label}]"] = v
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    digest = hashlib.sha256(Path(L.LIB_PATH).read_bytes()).hexdigest()[:12]
    out(f"bench_table_range_rows {time.strftime('%Y-%m-%d')} {torch.cuda.get_device_name(0)}; liblsmgpu.so sha256 "
        f"{digest}; device events, 3 rounds")
    per_block, key_len, val_len = 52, 16, 64
    items, _, n = bench.make_workload(torch, L, a.blocks, per_block, key_len, val_len)
    ctr = torch.arange(n, dtype=torch.int64, device="cuda")
    items["keys"][:n * key_len].view(n, key_len)[:, 8:] = (2 * ctr).view(torch.uint8).view(n, 8).flip(1)
    item_keys = items["keys"][:n * key_len].view(n, key_len)
    item_vals = items["vals"][:n * val_len].view(n, val_len)
    nq = a.queries
    g = torch.Generator(device="cuda")
    g.manual_seed(13)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())

    def arena(counters):
        m = counters.numel()
        buf = L.padded_bytes(m * key_len)
        buf[:m * key_len].view(m, key_len)[:, 8:] = counters.contiguous().view(torch.uint8).view(m, 8).flip(1)
        return buf

    off = torch.arange(nq + 1, dtype=torch.int64, device="cuda") * key_len
    flags = torch.full((nq,), L.SEEK_LO | L.SEEK_HI, dtype=torch.uint8, device="cuda")
    ceiling = bench.ceilings(torch, nbytes=1 << 30)["copy_GBps"]
    out(f"copy ceiling (16 B/lane, read + write counted): {ceiling:.0f} GB/s")

    legs, info = {}, {}
    for two_level in (False, True):
        wt = L.write_table(items, block_size=4096, two_level=two_level)
        assert wt["block_count"] == a.blocks
        file, total, block_off = wt["file"], wt["file"].numel(), wt["block_off"]
        table = {"tli_off": wt["tli_off"], "tli_size": wt["tli_size"], "two_level": two_level, "file_len": total,
                 "global_seqno": 7}
        t = L.LsmTableScan(wt["tli_off"], wt["tli_size"], int(two_level), 7, 0)
        name = "two-level" if two_level else "full"
        sizes = (block_off[1:] - block_off[:-1])
        out(f"{name} index: {n} items, {a.blocks} data blocks, file {total} bytes")
        assert torch.equal(L.table_block_offsets(file, table), block_off), "table_block_offsets"

        # the route without this change: the whole table, scanned and materialized
        whole = L._mi_alloc("cuda", n, n * key_len, n * val_len)

        def whole_table(file=file, total=total, wt=wt, two_level=two_level, whole=whole):
            sc = L.scan_table(file, total, wt["tli_off"], wt["tli_size"], two_level=two_level, global_seqno=7,
                              cap_blocks=a.blocks, item_cap=n, sync=False, data_blocks_hint=a.blocks,
                              index_blocks_hint=min(wt["tli_size"] // 4, a.blocks) if two_level else 0)
            return L.materialize_items(file, sc["block_off"], sc["n_blocks"], sc, into=whole)
        r = whole_table()
        torch.cuda.synchronize()
        assert r["end"].cpu().tolist() == [n, n * key_len, n * val_len] and int(r["result"].cpu()[0]) == 0
        assert torch.equal(whole["keys"][:n * key_len].view(n, key_len), item_keys)
        legs[f"{name}: scan_table + materialize_items, whole table"] = (whole_table, 3)
        info[f"{name}: scan_table + materialize_items, whole table"] = (n, total + n * (key_len + val_len + 25), None)

        for rows, reps in ROWS_PER_RANGE.items():
            first = torch.randint(0, n - rows, (nq,), dtype=torch.int64, device="cuda", generator=g)
            last = first + rows - 1
            pos = L.table_range(file, table, arena(2 * first), off, arena(2 * last), off, flags,
                                scan={"block_off": block_off, "item_start": wt["starts"], "n_blocks": a.blocks})
            assert bool((pos["outcome"] == L.RANGE_ROWS).all().item()) and torch.equal(pos["row_first"], first)
            n_pairs = int((last // per_block - first // per_block + 1).sum().item())
            n_rows = nq * rows
            ps = L.LsmRangePositions(*(pos[f].data_ptr() for f in ("outcome", "status", "first_block", "first_item",
                                                                   "last_block", "last_item")))
            dst = L._mi_alloc("cuda", n_rows, n_rows * key_len, n_rows * val_len)
            st = {"run_start": torch.zeros(nq + 1, dtype=torch.int64, device="cuda"),
                  "end": torch.zeros(3, dtype=torch.int64, device="cuda"),
                  "need": torch.zeros(4, dtype=torch.int64, device="cuda"),
                  "row_status": torch.zeros(nq, dtype=torch.int32, device="cuda"),
                  "plan_result": torch.zeros(1, dtype=torch.int32, device="cuda"),
                  "result": torch.zeros(1, dtype=torch.int32, device="cuda")}
            fb, lb = (first // per_block), (last // per_block)
            csum = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), sizes.cumsum(0)])
            touched = int((csum[lb + 1] - csum[fb]).sum().item())
            out_bytes = n_rows * (key_len + val_len + 25)
            for tag, lib in libs.items():
                ws = torch.empty(lib.lsm_table_range_rows_workspace_size(nq, n_pairs, n_rows), dtype=torch.uint8,
                                 device="cuda")
                head = (p(file), total, C.byref(t), p(block_off), a.blocks, C.byref(ps), nq, n_pairs, n_rows, None)

                def plan(lib=lib, head=head, st=st, ws=ws, keep=(file, pos, ps)):
                    rc = lib.lsm_table_range_rows_plan(*head, p(st["run_start"]), p(st["end"]), p(st["need"]),
                                                       p(st["row_status"]), p(st["plan_result"]), p(ws), ws.numel(), s)
                    assert rc == 0, rc

                def rows_call(lib=lib, head=head, st=st, ws=ws, dst=dst, n_rows=n_rows, keep=(file, pos, ps)):
                    rc = lib.lsm_table_range_rows(*head, p(st["end"]), p(ws), ws.numel(), p(dst["key_off"]),
                                                  p(dst["val_off"]), p(dst["keys"]), n_rows * key_len, p(dst["vals"]),
                                                  n_rows * val_len, p(dst["seqno"]), p(dst["vtype"]), n_rows,
                                                  p(st["result"]), s)
                    assert rc == 0, rc
                for v in dst.values():
                    v.zero_()
                plan()
                rows_call()
                torch.cuda.synchronize()
                # every row of every run against the item list
                assert int(st["plan_result"].cpu()[0]) == 0 and int(st["result"].cpu()[0]) == 0
                assert st["need"].cpu().tolist() == [n_pairs, n_rows, n_rows * key_len, n_rows * val_len]
                assert bool((st["row_status"] == 0).all().item())
                assert torch.equal(st["run_start"], torch.arange(nq + 1, dtype=torch.int64, device="cuda") * rows)
                idx = (first[:, None] + torch.arange(rows, dtype=torch.int64, device="cuda")[None, :]).reshape(-1)
                assert torch.equal(dst["keys"][:n_rows * key_len].view(n_rows, key_len), item_keys[idx]), "keys"
                assert torch.equal(dst["vals"][:n_rows * val_len].view(n_rows, val_len), item_vals[idx]), "values"
                assert bool((dst["seqno"] == 63 + 7).all().item()) and bool((dst["vtype"] == 0).all().item())
                assert torch.equal(dst["key_off"], torch.arange(n_rows + 1, dtype=torch.int64, device="cuda") * key_len)
                assert torch.equal(dst["val_off"], torch.arange(n_rows + 1, dtype=torch.int64, device="cuda") * val_len)
                del idx
                leg = f"{name}, {rows} rows per range{tag}"
                out(f"    {leg}: {nq} runs of {rows} rows equal the item list; {n_pairs} (query, block) pairs, "
                    f"{n_pairs / a.blocks:.3f} of the table's blocks per batch")
                legs[f"{leg}: plan"] = (plan, reps)
                legs[f"{leg}: rows"] = (rows_call, reps)
                info[leg] = (n_rows, touched + out_bytes, n_pairs)

    ms = {name: [] for name in legs}
    for fn, _ in legs.values():
        fn()
        fn()
    torch.cuda.synchronize()
    for _ in range(3):
        for name, (fn, reps) in legs.items():  # the legs alternate within a round
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / reps)
    out(f"{nq} ranges per batch; per call, three rounds:")
    for name, v in ms.items():
        out(f"    {name:62s} min {min(v):9.3f} ms, median {statistics.median(v):9.3f} ms, spread "
            f"{max(v) - min(v):7.3f} ms")
    out("plan + rows (medians) against the whole-table route of the same index kind:")
    for leg, (n_rows, nbytes, n_pairs) in info.items():
        if n_pairs is None:
            med = statistics.median(ms[leg])
            out(f"    {leg:62s} {med:9.3f} ms: {n_rows / med / 1e3:8.1f} M rows/s, {nbytes / med / 1e6:7.1f} GB/s "
                f"(file + output) = {nbytes / med / 1e6 / ceiling:.3f} of the copy ceiling")
            continue
        med = statistics.median(ms[f"{leg}: plan"]) + statistics.median(ms[f"{leg}: rows"])
        whole = statistics.median(ms[f"{leg.split(',')[0]}: scan_table + materialize_items, whole table"])
        out(f"    {leg:62s} {med:9.3f} ms: {n_rows / med / 1e3:8.1f} M rows/s, {nbytes / med / 1e6:7.1f} GB/s "
            f"(touched blocks + output) = {nbytes / med / 1e6 / ceiling:.3f} of the copy ceiling; "
            f"{med / whole:.2f}x the whole-table route, touching {n_pairs / a.blocks:.3f} of its blocks")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
