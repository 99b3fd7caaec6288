#!/usr/bin/env python3
"""Device-event time of lsm_table_range beside what the library could do before it for the
same ranges (diagnostic; the first measurement is in DESIGN.md §6.10).

    python scripts/bench_table_range.py [--blocks N] [--queries Q] [--reps R] [--out FILE]

Table: config-2 shape (16-byte keys / 64-byte values, 52 items per 4 KiB block, --blocks
blocks, 65536 by default), built on the device by write_table; the keys are the even
big-endian counters, so the odd ones are absent keys that fall inside blocks.
Ranges: --queries (2^20 by default) bound pairs at random places, both bounds inclusive.
Legs, under a full and under a two-level index: short scans (10 rows), scans of two blocks'
worth (104 rows), bounds on absent keys (odd counters, 9 rows between them).  Each leg's
outputs are checked first against the row window computed from the counters: both
positions, both ordinals, every outcome ROWS.
Yardstick: lsm_seek_blocks over the same file with the first and the last block of every
range resolved beforehand (two block queries per range in one call), which leaves out the
host's index searches and the upload of the block ids: a lower bound on what the parent
needed, not a fair race.  The expectation to hold the call against is that yardstick plus
two index searches (2 x 0.33 ms per Mi queries).
Timing: the C entry points on preallocated outputs, two warm-up calls, --reps calls
between two device events, three rounds, the legs alternating within a round; minimum,
median and spread per leg."""
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

INDEX_SEARCH_MS_PER_MI = 0.33  # one index search on this table, per Mi queries


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=1 << 16)
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=50)
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

    digest = hashlib.sha256(Path(L.LIB_PATH).read_bytes()).hexdigest()[:12]
    out(f"bench_table_range {time.strftime('%Y-%m-%d')} {torch.cuda.get_device_name(0)}; liblsmgpu.so sha256 {digest}; "
        f"device events, 3 rounds of {a.reps}")
    per_block, key_len = 52, 16
    items, _, n = bench.make_workload(torch, L, a.blocks, per_block, key_len, 64)
    ctr = torch.arange(n, dtype=torch.int64, device="cuda")
    items["keys"][:n * key_len].view(n, key_len)[:, 8:] = (2 * ctr).view(torch.uint8).view(n, 8).flip(1)

    nq = a.queries
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())

    def arena(counters):
        """Big-endian 16-byte keys of the counters, as a padded arena."""
        m = counters.numel()
        buf = L.padded_bytes(m * key_len)
        buf[:m * key_len].view(m, key_len)[:, 8:] = counters.contiguous().view(torch.uint8).view(m, 8).flip(1)
        return buf

    # name -> (rows per range, 1 if the bounds are the odd counters after the rows' ends)
    shapes = {"short scans, 10 rows": (10, 0), "two blocks, 104 rows": (104, 0), "absent bounds, 9 rows": (10, 1)}
    ranges = {}
    for leg, (rows, odd) in shapes.items():
        r = torch.randint(0, n - rows, (nq,), dtype=torch.int64, device="cuda", generator=g)
        lo_c, hi_c = 2 * r + odd, 2 * (r + rows - 1) + odd
        first, last = r + odd, r + rows - 1  # rows [first, last] of the table lie inside the bounds
        ranges[leg] = {"lo": arena(lo_c), "hi": arena(hi_c), "first": first, "last": last,
                       # the yardstick's queries: the first block of every range, then the last
                       "lo2": arena(torch.cat([lo_c, lo_c])), "hi2": arena(torch.cat([hi_c, hi_c])),
                       "q_block": torch.cat([first // per_block, last // per_block]).to(torch.int32)}
    off = torch.arange(2 * nq + 1, dtype=torch.int64, device="cuda") * key_len
    flags = torch.full((2 * nq,), L.SEEK_LO | L.SEEK_HI, dtype=torch.uint8, device="cuda")

    res = {f: torch.zeros(nq, dtype=getattr(torch, dt), device="cuda") for f, dt in L.TABLE_RANGE_FIELDS}
    soa = L.LsmRangeResult(*(res[f].data_ptr() for f, _ in L.TABLE_RANGE_FIELDS[:8]))
    seek = {f: torch.zeros(2 * nq, dtype=getattr(torch, dt), device="cuda")
            for f, dt in (("first", "int32"), ("end", "int32"), ("found", "uint8"), ("status", "int32"))}
    legs, yard_of = {}, {}
    for two_level in (False, True):
        wt = L.write_table(items, block_size=4096, two_level=two_level)
        assert wt["block_count"] == a.blocks
        file, total, block_off = wt["file"], wt["file"].numel(), wt["block_off"]
        t = L.LsmTableScan(wt["tli_off"], wt["tli_size"], int(two_level), 0, 0)
        name = "two-level" if two_level else "full"
        out(f"{name} index: {n} items, {a.blocks} data blocks, file {total} bytes, TLI {wt['tli_size']} bytes")
        for leg, rg in ranges.items():
            def call(file=file, t=t, total=total, block_off=block_off, rg=rg):  # (the closures keep the file alive)
                rc = lib.lsm_table_range(p(file), total, C.byref(t), p(rg["lo"]), p(off), p(rg["hi"]), p(off),
                                         p(flags), nq, p(block_off), a.blocks, C.byref(soa), p(res["outcome"]),
                                         p(res["status"]), s)
                assert rc == 0, rc
            for v in res.values():
                v.fill_(0x5A)
            call()
            torch.cuda.synchronize()
            assert bool((res["status"] == 0).all().item()) and bool((res["outcome"] == L.RANGE_ROWS).all().item())
            for side in ("first", "last"):
                row = rg[side]
                assert torch.equal(res[f"{side}_block"].long(), row // per_block), f"{leg}: {side} block"
                assert torch.equal(res[f"{side}_item"].long(), row % per_block), f"{leg}: {side} item"
                assert torch.equal(res[f"{side}_block_off"], block_off[row // per_block]), f"{leg}: {side} handle"
            out(f"    {name}, {leg}: {nq} ranges answered at their row windows")
            legs[f"table_range {name}, {leg}"] = call
            yard_of[f"table_range {name}, {leg}"] = f"seek_blocks, blocks resolved beforehand, {leg}"
            if not two_level:
                def yardstick(file=file, block_off=block_off, rg=rg):
                    rc = lib.lsm_seek_blocks(p(file), p(block_off), a.blocks, p(rg["q_block"]), p(rg["lo2"]), p(off),
                                             p(rg["hi2"]), p(off), p(flags), 2 * nq, p(seek["first"]), p(seek["end"]),
                                             p(seek["found"]), p(seek["status"]), s)
                    assert rc == 0, rc
                yardstick()
                torch.cuda.synchronize()
                assert bool((seek["status"] == 0).all().item())
                assert torch.equal(seek["first"][:nq].long(), rg["first"] % per_block)
                assert torch.equal(seek["end"][nq:].long() - 1, rg["last"] % per_block)
                legs[f"seek_blocks, blocks resolved beforehand, {leg}"] = yardstick

    ms = {name: [] for name in legs}
    for fn in legs.values():
        fn()
        fn()
    torch.cuda.synchronize()
    for _ in range(3):
        for name, fn in legs.items():  # the legs alternate within a round
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.reps)
    searches = 2 * INDEX_SEARCH_MS_PER_MI * nq / (1 << 20)
    out(f"{nq} ranges per call (a yardstick call holds {2 * nq} block queries); expectation = yardstick + "
        f"{searches * 1e3:.0f} us (two index searches, §6.9):")
    for name, v in ms.items():
        med = statistics.median(v)
        line = (f"    {name:58s} min {min(v) * 1e3:8.1f} us, median {med * 1e3:8.1f} us, spread "
                f"{(max(v) - min(v)) * 1e3:6.1f} us: {nq / med / 1e3:7.1f} M ranges/s")
        if name in yard_of:
            base = statistics.median(ms[yard_of[name]])
            line += f", {med / base:.2f}x the yardstick, {med / (base + searches):.2f}x the expectation"
        out(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
