"""The compaction read side in front of lsm_merge_runs, in more than one shape:
scan_table -> materialize_keys -> decoded_to_items -> merge_runs -> cut_blocks ->
Encoder.encode over three small tables with a two-level index, global seqnos that wrap,
values of up to 4000 bytes and 40-byte keys with a shared 32-byte prefix; decoded_to_items
checked on its own against the rows written; and the same tables read from LZ4-compressed
data blocks (decode_lz4_blocks, then materialize_keys and decoded_to_items over the
frames).  Expected: merge_model.merge_runs on the rows with each table's global seqno added
(mod 2^64), bit for bit, and pyoracle.encode_blocks of that for the encoded bytes."""
import random

import numpy as np
import pytest

import merge_model as M
from lz4_cases import lz4_compress
from merge_gpu import sort_run

pytestmark = pytest.mark.gpu

MASK = 2 ** 64 - 1
PREFIX = bytes(range(200, 232))  # 32 bytes shared by every key of the "prefix_keys" variant


def _tables(variant):
    """Three tables of 300 rows (one version per key in a table, keys shared between the
    tables) -> [(rows as written, global_seqno)], table_write arguments, gc threshold."""
    rng = random.Random({"two_level": 1, "wrapped_seqnos": 2, "big_values": 3, "prefix_keys": 4}[variant])
    if variant == "prefix_keys":
        universe = [PREFIX + b"%08d" % i for i in range(600)]
    else:
        universe = [b"user%06d" % i for i in range(600)]
    vmax = 4000 if variant == "big_values" else 90
    # written seqnos 1000 .. 1049 everywhere; the global seqnos put table 1 (wrapped to 990 .. 1039)
    # below table 2 (1000 ..) below table 0 (1007 ..) in the "wrapped_seqnos" variant
    gseq = (7, 2 ** 64 - 10, 0) if variant == "wrapped_seqnos" else (0, 0, 0)
    tables = []
    for t in range(3):
        rows = []
        for k in rng.sample(universe, 300):
            vt = rng.choice((0, 0, 0, 1, 2))
            n = rng.choice((0, 5, 90, vmax)) if rng.random() < 0.1 else rng.randint(0, 90)
            v = b"" if vt else rng.randbytes(n)
            base = 1000 if variant == "wrapped_seqnos" else 100 * (t + 1)
            rows.append((k, v, base + rng.randrange(50), vt))
        tables.append((sort_run(rows), gseq[t]))
    kw = {"block_size": 1024}
    if variant == "two_level":
        kw.update(two_level=True, partition_size=256)
    thr = 1010 if variant == "wrapped_seqnos" else 180
    return tables, kw, thr


def _shifted(rows, g):
    return [(k, v, (s + g) & MASK, t) for k, v, s, t in rows]


def _scan(gpu, oracle, rows, g, kw):
    """One table written by the oracle and read back on the device -> device lsm_items dict."""
    t = oracle.table_write(oracle.Items.from_list(rows), **kw)
    d_file = gpu.to_device_bytes(t["file"])
    out = gpu.scan_table(d_file, len(t["file"]), t["tli_off"], t["tli_size"], two_level=kw.get("two_level", False),
                         global_seqno=g, block_count=t["block_count"])
    assert out["table_status"] == 0 and out["n_blocks"] == t["block_count"] > 3
    nb = out["n_blocks"]
    keys, key_off = gpu.materialize_keys(d_file, out["block_off"], nb, out)
    return gpu.decoded_to_items(d_file, out["block_off"], nb, out, keys, key_off), t


def _scan_lz4(gpu, oracle, t, g):
    """The table's data blocks LZ4-compressed and framed, read through decode_lz4_blocks; the
    table's global seqno is added as the scan adds it (wrapping)."""
    import torch
    off = t["block_off"].astype(np.int64)
    blocks = []
    for b in range(t["block_count"]):
        payload = t["file"][int(off[b]) + 33:int(off[b + 1])]
        stored = lz4_compress(payload)
        blocks.append(oracle.block_header(0, stored, len(payload)) + stored)
    boff = np.concatenate([[0], np.cumsum([len(b) for b in blocks])]).astype(np.int64)
    nb = len(blocks)
    out = gpu.decode_lz4_blocks(gpu.to_device_bytes(b"".join(blocks)), torch.from_numpy(boff).cuda(), expect_type=0)
    assert (out["status"][:nb] == 0).all().item()
    keys, key_off = gpu.materialize_keys(out["frames"], out["frame_off"], nb, out)
    items = gpu.decoded_to_items(out["frames"], out["frame_off"], nb, out, keys, key_off)
    items["seqno"] = items["seqno"] + torch.tensor(g - 2 ** 64 if g >= 2 ** 63 else g, dtype=torch.int64).cuda()
    return items


def _rows_of(part):
    """A device lsm_items dict -> [(key, value, seqno, vtype)]."""
    ko, vo = part["key_off"].cpu().numpy(), part["val_off"].cpu().numpy()
    keys, vals = part["keys"].cpu().numpy().tobytes(), part["vals"].cpu().numpy().tobytes()
    seq, vt = part["seqno"].cpu().numpy().view(np.uint64), part["vtype"].cpu().numpy()
    assert ko[0] == 0 and vo[0] == 0 and len(ko) == len(vo) == len(seq) + 1 == len(vt) + 1
    return [(keys[ko[i]:ko[i + 1]], vals[vo[i]:vo[i + 1]], int(seq[i]), int(vt[i])) for i in range(len(seq))]


def _concat(gpu, parts):
    """The tables' items back to back: one lsm_items dict and run_start."""
    import torch
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
    return items, np.concatenate([[0], np.cumsum([p["seqno"].numel() for p in parts])]).tolist()


def _merge(gpu, parts, thr):
    """merge_runs over the parts -> (device output dict, n_out, src, statuses, items)."""
    import torch
    items, run_start = _concat(gpu, parts)
    out = gpu.merge_runs(items, run_start, thr, evict_tombstones=True)
    torch.cuda.synchronize()
    n_out = int(out["n_out"].cpu()[0])
    merged = {"keys": out["keys"], "key_off": out["key_off"][:n_out + 1], "vals": out["vals"],
              "val_off": out["val_off"][:n_out + 1], "seqno": out["seqno"][:n_out], "vtype": out["vtype"][:n_out]}
    ko, vo = int(merged["key_off"][-1]), int(merged["val_off"][-1])
    rows = _rows_of(dict(merged, keys=out["keys"][:ko], vals=out["vals"][:vo]))
    return merged, n_out, out["src"].cpu().numpy()[:n_out].tolist(), out["status"].cpu().tolist(), rows


VARIANTS = ["two_level", "wrapped_seqnos", "big_values", "prefix_keys"]


@pytest.mark.parametrize("variant", VARIANTS)
def test_decoded_to_items_equals_the_rows_written(gpu, oracle, variant):
    tables, kw, _ = _tables(variant)
    for rows, g in tables:
        part, _ = _scan(gpu, oracle, rows, g, kw)
        n = len(rows)
        kt, vt = sum(len(r[0]) for r in rows), sum(len(r[1]) for r in rows)
        assert part["seqno"].numel() == n and int(part["key_off"][-1]) == kt and int(part["val_off"][-1]) == vt
        got = _rows_of(dict(part, keys=part["keys"][:kt], vals=part["vals"][:vt]))
        assert got == _shifted(rows, g)


@pytest.mark.parametrize("variant", VARIANTS)
def test_scan_merge_encode_variants(gpu, oracle, variant):
    import torch
    tables, kw, thr = _tables(variant)
    runs = [_shifted(rows, g) for rows, g in tables]
    assert all(M.run_is_sorted(r) for r in runs)
    want, want_src, dropped = M.merge_runs(runs, thr, True, False)
    assert dropped and len(want) > 300
    if variant == "wrapped_seqnos":  # the wrap decides the order: without it table 1's versions would be the newest
        unwrapped = [[(k, v, s + g, t) for k, v, s, t in rows] for rows, g in tables]
        assert [i for _, i in M.merge(unwrapped)] != [i for _, i in M.merge(runs)]
        assert max(r[2] for r in runs[1]) < 1040 < 2 ** 64 - 10 + 1000
    parts = [_scan(gpu, oracle, rows, g, kw)[0] for rows, g in tables]
    merged, n_out, src, status, got = _merge(gpu, parts, thr)
    assert status == [0, 0, 0] and n_out == len(want)
    assert src == want_src
    assert got == want
    ko = merged["key_off"].cpu().numpy().view(np.uint64)
    vo = merged["val_off"].cpu().numpy().view(np.uint64)
    starts = gpu.cut_blocks(ko, vo, 4096)
    ref_items = oracle.Items.from_list(want)
    assert list(starts) == list(oracle.cut_blocks(ref_items, 4096))
    nb = len(starts) - 1
    enc = gpu.Encoder().encode(merged, torch.from_numpy(starts.astype(np.int32)).cuda(), nb)
    torch.cuda.synchronize()
    ref_buf, ref_off = oracle.encode_blocks(ref_items, starts, nthreads=2)
    assert (enc["status"][:nb] == 0).all().item()
    off = enc["block_off"].cpu().numpy().view(np.uint64)
    assert (off == ref_off).all()
    assert enc["buf"].cpu().numpy()[:int(off[-1])].tobytes() == ref_buf.tobytes()


@pytest.mark.parametrize("variant", ["wrapped_seqnos", "big_values"])
def test_lz4_read_side(gpu, oracle, variant):
    """The same tables with LZ4-compressed data blocks give the same items and the same merge."""
    tables, kw, thr = _tables(variant)
    runs = [_shifted(rows, g) for rows, g in tables]
    want, want_src, _ = M.merge_runs(runs, thr, True, False)
    plain, packed = [], []
    for rows, g in tables:
        part, t = _scan(gpu, oracle, rows, g, kw)
        plain.append(part)
        packed.append(_scan_lz4(gpu, oracle, t, g))
        for f in ("key_off", "val_off", "seqno", "vtype"):
            assert (packed[-1][f] == part[f]).all().item(), f
        for f, off in (("keys", "key_off"), ("vals", "val_off")):
            n = int(part[off][-1])
            assert (packed[-1][f][:n] == part[f][:n]).all().item(), f
    a = _merge(gpu, plain, thr)
    b = _merge(gpu, packed, thr)
    assert b[1:] == a[1:]
    assert b[3] == [0, 0, 0] and b[2] == want_src and b[4] == want
