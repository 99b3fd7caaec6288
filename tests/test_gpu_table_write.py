"""The table write side on the device: cut_blocks_device -> Encoder.encode -> index_entries ->
index blocks (lsmgpu.write_table) against pyoracle.table_write, byte for byte, with a full and a
two-level (partitioned) block index; the GPU-written file read back with lsm_scan_table;
lsm_index_entries on its own with a key arena one byte short; and the whole chain behind a
merge, where the item count stays on the device."""
import random

import numpy as np
import pytest

import merge_model as M
import test_gpu_merge_pipeline as P

pytestmark = pytest.mark.gpu

PREFIX = bytes(range(100, 132))  # 32 bytes shared by every key of "prefix_keys": 40-byte keys


def _rows(variant):
    """About 900 rows in key order: (key, value, seqno, vtype), tombstones without a value."""
    rng = random.Random({"plain": 1, "prefix_keys": 2, "big_values": 3, "hash_index": 4, "single_block": 5}[variant])
    n = 6 if variant == "single_block" else 900
    ids = sorted(rng.sample(range(100000), n))
    rows = []
    for i in ids:
        key = PREFIX + b"%08d" % i if variant == "prefix_keys" else b"user%06d" % i + b"x" * rng.randrange(4)
        vt = rng.choice((0, 0, 0, 0, 1, 2))
        vmax = 4000 if variant == "big_values" and rng.random() < 0.1 else 90
        rows.append((key, b"" if vt else rng.randbytes(rng.randint(0, vmax)), rng.getrandbits(40), vt))
    return rows


def _kw(variant, two_level):
    kw = {"block_size": 1024}
    if variant == "hash_index":
        kw["hash_ratio"] = 1.33
    if two_level:
        kw.update(two_level=True, partition_size=256)
    return kw


def _assert_same_table(got, ref):
    for f in ("tli_off", "tli_size", "index_off", "data_len", "block_count"):
        assert got[f] == ref[f], f
    assert got["starts"].cpu().numpy().view(np.uint32).tolist() == ref["starts"].tolist()
    assert got["block_off"].cpu().numpy().view(np.uint64).tolist() == ref["block_off"].tolist()
    assert got["file"].numel() == len(ref["file"])
    assert got["file"].cpu().numpy().tobytes() == ref["file"]


VARIANTS = ["plain", "prefix_keys", "big_values", "hash_index", "single_block"]


@pytest.mark.parametrize("two_level", [False, True], ids=["full", "two_level"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_write_table_equals_the_oracle(gpu, oracle, variant, two_level):
    rows = _rows(variant)
    items = oracle.Items.from_list(rows)
    kw = _kw(variant, two_level)
    ref = oracle.table_write(items, **kw)
    assert ref["block_count"] == 1 if variant == "single_block" else ref["block_count"] > 30
    if two_level and variant != "single_block":
        assert ref["tli_off"] > ref["index_off"] + 5 * 256  # several partitions
    got = gpu.write_table(gpu.items_to_device(items), **kw)
    _assert_same_table(got, ref)


@pytest.mark.parametrize("two_level", [False, True], ids=["full", "two_level"])
def test_scan_reads_back_the_rows_written(gpu, oracle, two_level):
    rows = _rows("plain")
    t = gpu.write_table(gpu.items_to_device(oracle.Items.from_list(rows)), **_kw("plain", two_level))
    out = gpu.scan_table(t["file"], t["file"].numel(), t["tli_off"], t["tli_size"], two_level=two_level,
                         block_count=t["block_count"])
    assert out["table_status"] == 0 and out["n_blocks"] == t["block_count"]
    nb = out["n_blocks"]
    assert (out["block_off"] == t["block_off"]).all().item()
    keys, key_off = gpu.materialize_keys(t["file"], out["block_off"], nb, out)
    part = gpu.decoded_to_items(t["file"], out["block_off"], nb, out, keys, key_off)
    kt, vt = int(part["key_off"][-1]), int(part["val_off"][-1])
    assert P._rows_of(dict(part, keys=part["keys"][:kt], vals=part["vals"][:vt])) == rows


def test_index_entries_with_a_short_key_arena(gpu, oracle):
    import ctypes as C
    import torch
    rows = _rows("prefix_keys")
    items = oracle.Items.from_list(rows)
    d = gpu.items_to_device(items)
    starts = gpu.cut_blocks_device(d, 1024)
    nb = starts.numel() - 1
    ref_starts = oracle.cut_blocks(items, 1024)
    assert starts.cpu().numpy().view(np.uint32).tolist() == ref_starts.tolist() and nb > 40
    enc = gpu.Encoder().encode(d, starts, nb)
    last = ref_starts[1:].astype(np.int64) - 1
    want_keys = b"".join(rows[j][0] for j in last)
    total = len(want_keys)
    assert total == 40 * nb
    it = gpu.LsmItems()
    it.keys, it.key_off, it.seqno, it.n_items = d["keys"].data_ptr(), d["key_off"].data_ptr(), d["seqno"].data_ptr(), len(rows)
    ws = torch.empty(gpu.lib().lsm_index_entries_workspace_size(nb), dtype=torch.uint8, device="cuda")
    for cap, want in ((total - 1, 6), (total, 0), (0, 6), (total + 5, 0)):
        keys = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        key_off = torch.full((nb + 1,), -1, dtype=torch.int64, device="cuda")
        seqno = torch.full((nb,), -1, dtype=torch.int64, device="cuda")
        hoff = torch.full((nb,), -1, dtype=torch.int64, device="cuda")
        hsize = torch.full((nb,), -1, dtype=torch.int32, device="cuda")
        result = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        rc = gpu.lib().lsm_index_entries(C.byref(it), gpu._ptr(starts), gpu._ptr(enc["block_off"]), nb, 1000,
                                         gpu._ptr(keys), cap, gpu._ptr(key_off), gpu._ptr(seqno), gpu._ptr(hoff),
                                         gpu._ptr(hsize), gpu._ptr(result), gpu._ptr(ws), ws.numel(), gpu._stream(None))
        torch.cuda.synchronize()
        assert rc == 0 and int(result.item()) == want
        assert key_off.cpu().tolist() == list(range(0, total + 1, 40))
        if want:
            assert (keys == 0xA5).all().item() and (seqno == -1).all().item()
            assert (hoff == -1).all().item() and (hsize == -1).all().item()
            continue
        assert keys[:total].cpu().numpy().tobytes() == want_keys and (keys[total:] == 0xA5).all().item()
        assert seqno.cpu().tolist() == [rows[j][2] for j in last]
        off = enc["block_off"].cpu().numpy()[:nb + 1]
        assert hoff.cpu().tolist() == (off[:-1] + 1000).tolist()
        assert hsize.cpu().tolist() == np.diff(off).tolist()


@pytest.mark.parametrize("two_level", [False, True], ids=["full", "two_level"])
def test_scan_merge_write_table(gpu, oracle, two_level):
    """scan -> merge_runs -> write_table(n_items = the merge's device count): no offset array
    leaves the device.  Expected: the oracle's table of merge_model.merge_runs' rows."""
    tables, kw, thr = P._tables("two_level" if two_level else "big_values")
    runs = [P._shifted(rows, g) for rows, g in tables]
    want, _, dropped = M.merge_runs(runs, thr, True, False)
    assert dropped and len(want) > 300
    parts = [P._scan(gpu, oracle, rows, g, kw)[0] for rows, g in tables]
    items, run_start = P._concat(gpu, parts)
    out = gpu.merge_runs(items, run_start, thr, evict_tombstones=True)
    got = gpu.write_table(out, n_items=out["n_out"], **kw)
    assert out["status"].cpu().tolist() == [0, 0, 0] and int(out["n_out"].item()) == len(want)
    assert out["key_off"].numel() - 1 == 900 > len(want)  # the arrays are the capacity
    ref = oracle.table_write(oracle.Items.from_list(want), **kw)
    _assert_same_table(got, ref)
