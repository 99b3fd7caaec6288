"""lsm_merge_runs on the GPU == Merger + CompactionStream as restated by
tests/merge_model.py (src/merge.rs:34-100, src/compaction/stream.rs:46-221):
every output field and n_out, bit for bit.  Cases of a few thousand items at
most; the shapes sit on either side of the splitter stride (64 items of a run),
the scan tile (2048), the 16-byte key head and the long-value cut-over (256)."""
import json
import random
from pathlib import Path

import numpy as np
import pytest

import merge_model as M
from merge_gpu import check, deal, gpu_merge, random_items, sort_run

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
CASES = json.loads((ROOT / "tests" / "golden" / "compaction_stream_cases.json").read_text())["cases"]
LONG_VALUE = 256  # kMergeLong (csrc/merge.hip): values from this length on are copied by the whole wave


def case_rows(rows):
    return [(bytes.fromhex(k), bytes.fromhex(v), int(s), int(t)) for k, v, s, t in rows]


# ------------------------------------------------------------------- golden
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_cases(gpu, case):
    runs = [case_rows(r) for r in case["runs"]]
    flat = [it for r in runs for it in r]
    layouts = [runs] + [[flat[k::n] for k in range(n)] for n in (2, 3)]  # (a sorted stream dealt round-robin stays sorted)
    for layout in layouts:
        got, src, status = gpu_merge(gpu, layout, case["gc_seqno_threshold"], case["evict_tombstones"],
                                     case["zero_seqnos"])
        assert status == [0] * len(layout)
        assert got == case_rows(case["expect"])
        dealt = [it for r in layout for it in r]
        kept = set(src)
        assert len(kept) == len(src)
        dropped = [dealt[i] for i in range(len(dealt)) if i not in kept]
        assert sorted(dropped) == sorted(case_rows(case["dropped"]))
        check(gpu, layout, case["gc_seqno_threshold"], case["evict_tombstones"], case["zero_seqnos"])


# --------------------------------------------------------------- run shapes
@pytest.mark.parametrize("n_runs", [1, 2, 3, 8, 64])
def test_run_counts(gpu, n_runs):
    rng = random.Random(100 + n_runs)
    runs = deal(rng, random_items(rng, 1500, 400), n_runs)
    check(gpu, runs, thr=500, evict=bool(n_runs & 1), zero=bool(n_runs & 2))


def test_empty_and_one_item_runs(gpu):
    rng = random.Random(5)
    a, b, c = deal(rng, random_items(rng, 300, 80), 3)
    for runs in ([[], a, b], [a, b, []], [a, [], [], b, c], [[], [], []], [[]], [a[:1]], [[], a[:1], []]):
        check(gpu, runs, thr=400)
    ones = [[it] for it in random_items(rng, 64, 20)]
    check(gpu, ones, thr=500, evict=True)
    got, src, status = gpu_merge(gpu, [[]])
    assert got == [] and src == [] and status == [0]


def test_disjoint_and_interleaved_runs(gpu):
    lo = sort_run([(b"a%04d" % i, b"v%d" % i, 7, 0) for i in range(200)])
    hi = sort_run([(b"b%04d" % i, b"w%d" % i, 9, 0) for i in range(300)])
    check(gpu, [lo, hi])
    check(gpu, [hi, lo])
    check(gpu, [hi, lo, hi[:10]], thr=8)
    every = sort_run([(b"k%05d" % i, b"x" * (i % 5), i % 3, 0) for i in range(900)])
    check(gpu, [every[0::3], every[1::3], every[2::3]])
    check(gpu, [every[1::2], every[0::2]], thr=1, zero=True)


@pytest.mark.parametrize("lens", [(63, 64, 65, 128, 129), (64, 64), (65, 1), (129, 63, 0, 64)])
def test_run_lengths_around_the_splitter_stride(gpu, lens):
    rng = random.Random(sum(lens))
    pool = random_items(rng, sum(lens), 150)
    runs, at = [], 0
    for n in lens:
        runs.append(sort_run(pool[at:at + n]))
        at += n
    check(gpu, runs, thr=300, evict=True)


@pytest.mark.parametrize("total", [2047, 2048, 2049])
def test_outputs_around_the_scan_tile(gpu, total):
    rng = random.Random(total)
    items = [(b"%06d" % rng.randrange(700), b"v", s, 0) for s in range(total)]
    want, dropped = check(gpu, deal(rng, items, 3), thr=0)
    assert len(want) == total and not dropped


# ------------------------------------------------------------ key comparison
def test_key_comparison_edges(gpu):
    rng = random.Random(9)
    keys = set()
    for n in (1, 7, 8, 9, 15, 16, 17, 33, 300):
        base = bytes((37 * i + 11) % 251 + 1 for i in range(n))
        keys.add(base)
        keys.add(base[:-1])                       # a key that is a prefix of the next
        keys.add(base + b"\x00")                  # ... extended by a zero byte (the head's fill)
        for p in {0, 6, 7, 8, 14, 15, 16, 17, 32, n - 1}:
            if p < n:
                for b in (0x00, 0x7f, 0x80, 0xff):  # signed / little-endian compares order these wrongly
                    keys.add(base[:p] + bytes([b]) + base[p + 1:])
    keys.discard(b"")
    keys = sorted(keys)
    assert any(a[:16] == b[:16] and a != b and len(a) > 16 for a, b in zip(keys, keys[1:]))  # differ only past byte 16
    items = [(k, b"v" + bytes([i & 0xff]), rng.randrange(4), 0) for i, k in enumerate(keys) for _ in range(2)]
    items.append((b"", b"empty key", 1, 0))
    check(gpu, deal(rng, items, 3), thr=2)
    check(gpu, deal(rng, items, 5), thr=0)


# ----------------------------------------------------------------------- GC
def gc_runs():
    rng = random.Random(21)
    runs = []
    for r in range(8):
        run = [(b"shared", b"r%d" % r, 10 * r + 5, rng.choice((0, 1, 2, 4)))]  # one key in every run
        run += random_items(rng, 70, 12, key_len=(1, 3), max_seq=80, vtypes=(0, 1, 2, 4))
        runs.append(sort_run(run))
    # equal (key, seqno) in two runs, told apart by their values and types
    runs[2] = sort_run(runs[2] + [(b"tie", b"from run 2", 40, 0), (b"tie", b"", 39, 2)])
    runs[6] = sort_run(runs[6] + [(b"tie", b"from run 6", 40, 4), (b"tie", b"old", 39, 0)])
    return runs


@pytest.mark.parametrize("thr", [0, 40, 1000])
@pytest.mark.parametrize("evict,zero", [(False, False), (True, False), (False, True), (True, True)])
def test_gc_rule(gpu, thr, evict, zero):
    want, _ = check(gpu, gc_runs(), thr, evict, zero)
    if thr == 0:
        ties = [it for it in want if it[0] == b"tie" and it[2] == 40]
        assert [it[1] for it in ties] == [b"from run 2", b"from run 6"]


# ------------------------------------------------------------------- values
@pytest.mark.parametrize("skew", [0, 1, 7])
def test_value_lengths_and_odd_arenas(gpu, skew):
    rng = random.Random(skew)
    lens = [0, 1, 15, 16, 17, 255, LONG_VALUE - 1, LONG_VALUE, LONG_VALUE + 1, 4000, 9000]
    items = []
    for i in range(260):
        n = rng.choice(lens) if i % 4 else rng.choice(lens[:5])
        items.append((b"key%04d" % (i // 2), rng.randbytes(n), rng.randrange(50), 0))
    check(gpu, deal(rng, items, 3), thr=25, key_skew=skew, val_skew=skew + (2 if skew else 0))
    # steps of short values only (assembled in LDS), of mid-size values that overflow the step
    # buffer, and of long keys
    short = [(b"s%05d" % i, rng.randbytes(i % 100), 3, 0) for i in range(400)]
    check(gpu, deal(rng, short, 2), key_skew=skew, val_skew=skew)
    mid = [(b"m%05d" % i, bytes([i & 0xff]) * (200 + i % 56), 3, 0) for i in range(200)]
    check(gpu, deal(rng, mid, 2), key_skew=skew, val_skew=skew)
    longk = [(bytes([65 + i % 7]) * (250 + i % 60) + b"%03d" % i, b"v", 3, 0) for i in range(150)]
    check(gpu, deal(rng, longk, 2), key_skew=skew, val_skew=skew)


# ----------------------------------------------------------- unsorted input
def test_unsorted_run_rejected(gpu):
    rng = random.Random(33)
    runs = deal(rng, random_items(rng, 600, 200), 3)
    bad = [list(r) for r in runs]
    k = next(i for i in range(len(bad[1]) - 1) if (bad[1][i][0], -bad[1][i][2]) != (bad[1][i + 1][0], -bad[1][i + 1][2]))
    bad[1][k], bad[1][k + 1] = bad[1][k + 1], bad[1][k]
    got, src, status = gpu_merge(gpu, bad, thr=100)
    assert status == [0, 10, 0] and got == []
    bad[2] = bad[2][::-1]
    got, src, status = gpu_merge(gpu, bad, thr=100)
    assert status == [0, 10, 10] and got == []
    # seqno ascending inside a key is unsorted too; equal neighbours are fine
    got, src, status = gpu_merge(gpu, [[(b"a", b"", 1, 0), (b"a", b"", 2, 0)]])
    assert status == [10] and got == []
    check(gpu, [[(b"a", b"x", 2, 0), (b"a", b"y", 2, 0)], [(b"a", b"z", 2, 0)]])
    check(gpu, runs, thr=100)


# --------------------------------------------------------------- end to end
def test_scan_merge_encode_end_to_end(gpu, oracle):
    """scan_table -> materialize_keys -> decoded_to_items -> merge_runs -> cut_blocks -> Encoder.encode
    over three small tables == pyoracle.encode_blocks of the model's output cut the same way."""
    import torch
    rng = random.Random(77)
    universe = [b"user%06d" % i for i in range(1500)]
    tables = []
    for t in range(3):
        rows = []
        for k in rng.sample(universe, 700):
            vt = rng.choice((0, 0, 0, 1, 2))
            v = b"" if vt else bytes(rng.getrandbits(8) for _ in range(rng.randint(0, 90)))
            rows.append((k, v, 100 * (t + 1) + rng.randrange(50), vt))
        tables.append(sort_run(rows))
    parts = []
    for rows in tables:
        t = oracle.table_write(oracle.Items.from_list(rows), block_size=1024)
        d_file = gpu.to_device_bytes(t["file"])
        out = gpu.scan_table(d_file, len(t["file"]), t["tli_off"], t["tli_size"], block_count=t["block_count"])
        assert out["table_status"] == 0 and out["n_blocks"] == t["block_count"]
        nb = out["n_blocks"]
        keys, key_off = gpu.materialize_keys(d_file, out["block_off"], nb, out)
        parts.append(gpu.decoded_to_items(d_file, out["block_off"], nb, out, keys, key_off))
        assert parts[-1]["seqno"].numel() == len(rows)
    items = {}
    for f in ("keys", "vals"):
        off = "key_off" if f == "keys" else "val_off"
        sizes = [int(p[off][-1]) for p in parts]
        items[f] = gpu.padded_bytes(sum(sizes))
        items[f][:sum(sizes)] = torch.cat([p[f][:s] for p, s in zip(parts, sizes)])
        bases = np.concatenate([[0], np.cumsum(sizes)])
        items[off] = torch.cat([parts[0][off]] + [p[off][1:] + int(b) for p, b in zip(parts[1:], bases[1:])])
    for f in ("seqno", "vtype"):
        items[f] = torch.cat([p[f] for p in parts])
    run_start = np.concatenate([[0], np.cumsum([len(r) for r in tables])]).tolist()
    thr = 180
    out = gpu.merge_runs(items, run_start, thr, evict_tombstones=True)
    torch.cuda.synchronize()
    want, want_src, _ = M.merge_runs(tables, thr, True, False)
    n_out = int(out["n_out"].cpu()[0])
    assert n_out == len(want) and out["status"].cpu().tolist() == [0, 0, 0]
    assert out["src"].cpu().numpy()[:n_out].tolist() == want_src
    ko = out["key_off"][:n_out + 1].cpu().numpy().view(np.uint64)
    vo = out["val_off"][:n_out + 1].cpu().numpy().view(np.uint64)
    starts = gpu.cut_blocks(ko, vo, 4096)
    ref_items = oracle.Items.from_list(want)
    assert list(starts) == list(oracle.cut_blocks(ref_items, 4096))
    merged = {"keys": out["keys"], "key_off": out["key_off"][:n_out + 1], "vals": out["vals"],
              "val_off": out["val_off"][:n_out + 1], "seqno": out["seqno"][:n_out], "vtype": out["vtype"][:n_out]}
    nb = len(starts) - 1
    enc = gpu.Encoder().encode(merged, torch.from_numpy(starts.astype(np.int32)).cuda(), nb)
    torch.cuda.synchronize()
    ref_buf, ref_off = oracle.encode_blocks(ref_items, starts, nthreads=2)
    assert (enc["status"][:nb] == 0).all().item()
    off = enc["block_off"].cpu().numpy().view(np.uint64)
    assert (off == ref_off).all()
    assert enc["buf"].cpu().numpy()[:int(off[-1])].tobytes() == ref_buf.tobytes()
