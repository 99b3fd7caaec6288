"""GPU parity of lsm_table_range (batched Table::range bounds, src/table/mod.rs:391-422,
src/table/iter.rs:94-293) against the literal drain in tests/table_range_model.py, never
against the library itself.  Bar: for every query the status, the outcome and every result
field equal the model's; the fields of a query whose outcome is not ROWS keep what the
output held before."""
import functools
import random

import numpy as np
import pytest

import pyoracle
from helpers import counter_items
from table_get_model import (BAD_MAGIC, TRUNCATED, TYPE_MISMATCH, UNSUPPORTED, index_block, item_key, mvcc_table,
                             reseal_header)
from table_range_model import (RANGE_EMPTY, RANGE_NO_BLOCK, RANGE_NONE, RANGE_ROWS, RangeModel, brute_force, flags_of,
                               mvcc_range_queries)

pytestmark = pytest.mark.gpu

POSITION = ("first_block_off", "first_block_size", "first_item", "last_block_off", "last_block_size", "last_item")
BAD_ARG = 10
SENTINEL = 0x5A


def run(gpu, file, table, queries, scan=None):
    """queries: [(lo, hi, lo_excl, hi_excl)], None = unbounded -> result dict of numpy arrays,
    every output filled with SENTINEL before the call.  file: bytes (uploaded with padding) or a
    padded cuda tensor."""
    import torch

    def arena(which):
        parts = [q[which] or b"" for q in queries]
        off = np.zeros(len(queries) + 1, np.int64)
        off[1:] = np.cumsum([len(p) for p in parts])
        return gpu.to_device_bytes(b"".join(parts)), torch.from_numpy(off).cuda()

    (lo, lo_off), (hi, hi_off) = arena(0), arena(1)
    flags = torch.tensor([flags_of(*q) for q in queries], dtype=torch.uint8).cuda()
    if isinstance(file, (bytes, bytearray)):
        table = dict(table, file_len=len(file))
        file = gpu.to_device_bytes(file)
    out = {f: torch.full((len(queries),), SENTINEL, dtype=getattr(torch, dt), device="cuda")
           for f, dt in gpu.TABLE_RANGE_FIELDS}
    res = gpu.table_range(file, table, lo, lo_off, hi, hi_off, flags, scan=scan, out=out)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy()[:len(queries)] for k, v in res.items()}


def expect(model, queries):
    """[(status, (outcome, first off, size, item, last off, size, item))] of the model."""
    return [model.answer(*q) for q in queries]


def compare(res, queries, expected, ordinal=None):
    """Every output of every query against the model.  ordinal: {(block off, size): ordinal}
    of the offsets the call was given, None if it was given none."""
    outcomes = {}
    for q, (st, exp) in enumerate(expected):
        got = (int(res["status"][q]), int(res["outcome"][q]))
        assert got == (st, exp[0]), (q, queries[q], got, st, exp[0])
        outcomes[exp[0]] = outcomes.get(exp[0], 0) + 1
        rows = exp[0] == RANGE_ROWS
        for f, want in zip(POSITION, exp[1:]):
            assert int(res[f][q]) == (want if rows else SENTINEL), (q, queries[q], f, int(res[f][q]), want)
        for f, handle in (("first_block", exp[1:3]), ("last_block", exp[4:6])):
            want = ordinal[handle] if rows and ordinal is not None else SENTINEL
            assert int(res[f][q]) == want, (q, queries[q], f, int(res[f][q]), want)
    return outcomes


def ordinals(block_off):
    off = [int(o) for o in block_off]
    return {(off[i], off[i + 1] - off[i]): i for i in range(len(off) - 1)}


def check(gpu, file, table, queries, **kw):
    """Model and kernel on one table -> (expected, outcomes)."""
    model = RangeModel(file, table["tli_off"], table["tli_size"], table["two_level"])
    expected = expect(model, queries)
    return expected, compare(run(gpu, file, table, queries, **kw), queries, expected)


@functools.lru_cache(maxsize=None)
def mvcc_case(seed, two_level):
    """Table, queries and the model's answers, computed once per table."""
    items, t = mvcc_table(seed, two_level)
    model = RangeModel(t["file"], t["tli_off"], t["tli_size"], two_level)
    queries = mvcc_range_queries(seed, two_level)
    return items, dict(t, two_level=two_level), queries, expect(model, queries)


@pytest.mark.parametrize("two_level", [False, True])
@pytest.mark.parametrize("seed", [1, 2])
def test_table_range_mvcc_tables(gpu, seed, two_level):
    _, t, queries, expected = mvcc_case(seed, two_level)
    outcomes = compare(run(gpu, t["file"], t, queries), queries, expected)
    assert outcomes[RANGE_ROWS] >= 600 and outcomes[RANGE_EMPTY] >= 50 and outcomes[RANGE_NO_BLOCK] >= 500


@pytest.mark.parametrize("two_level", [False, True])
@pytest.mark.parametrize("seed", [1, 2])
def test_table_range_row_windows(gpu, seed, two_level):
    """With a scan of the table, [row_first, row_end) is the brute-force window over the item
    list (row index = item index), and the ordinals are the blocks' places in the scan."""
    items, t, queries, expected = mvcc_case(seed, two_level)
    file = gpu.to_device_bytes(t["file"])
    scan = gpu.scan_table(file, len(t["file"]), t["tli_off"], t["tli_size"], two_level=two_level)
    assert scan["table_status"] == 0 and scan["n_blocks"] == t["block_count"]
    res = run(gpu, file, dict(t, file_len=len(t["file"])), queries, scan=scan)
    compare(res, queries, expected, ordinal=ordinals(t["block_off"]))
    keys = [item_key(items, i) for i in range(items.n)]
    for q, bounds in enumerate(queries):
        want = brute_force(keys, *bounds)
        window = (want[0], want[-1] + 1) if want else (0, 0)
        assert (int(res["row_first"][q]), int(res["row_end"][q])) == window, (q, bounds, window)
        assert want == list(range(*window))


def _key16(c):
    return int(c).to_bytes(16, "big")


@pytest.mark.parametrize("n,step", [(4000, 4), (2500, 2)])
def test_table_range_binary_index_step(gpu, n, step):
    """One-item blocks under a full index: 4000 entries need a 4-byte binary-index step in the
    TLI, 2500 still fit 2 bytes.  Mostly short spans (the model drains every block of a span),
    every 25th pair unrelated."""
    items = counter_items(n, key_len=16, val_len=8, seed=3)
    t = pyoracle.table_write(items, block_size=1, two_level=False)
    assert t["block_count"] == n
    tli = t["file"][t["tli_off"]:t["tli_off"] + t["tli_size"]]
    assert tli[len(tli) - 31 + 1] == step, (t["tli_size"], tli[len(tli) - 31 + 1])
    rng = random.Random(n)

    def bound(c):  # a present key, the gap after it, or a key above the last
        return rng.choice([_key16(c), _key16(c) + b"\0", _key16(n + c)])

    queries = []
    for j in range(400):
        a = rng.randrange(n)
        b = rng.randrange(n) if j % 25 == 0 else min(n - 1, a + rng.choice([0, 1, 2, 7, 40]))
        queries.append((bound(a), bound(b), rng.random() < 0.5, rng.random() < 0.5))
    expected, outcomes = check(gpu, t["file"], dict(t, two_level=False), queries)
    assert outcomes[RANGE_ROWS] >= 100 and outcomes[RANGE_NO_BLOCK] >= 100, outcomes


def test_table_range_restart_interval_16(gpu):
    """4 KiB blocks with restart interval 16 under a two-level index of several partitions;
    even counters only, so odd ones are absent keys."""
    rng = random.Random(16)
    n = 2000
    items = pyoracle.Items.from_list([(_key16(2 * i), bytes(rng.getrandbits(8) for _ in range(64)), 63, 0)
                                      for i in range(n)])
    t = pyoracle.table_write(items, block_size=4096, two_level=True, partition_size=256)
    table = dict(t, two_level=True)
    model = RangeModel(t["file"], t["tli_off"], t["tli_size"], True)
    parts = model.table.index_entries(*model.table.tli)
    assert t["block_count"] >= 30 and len(parts) >= 5, (t["block_count"], len(parts))
    queries = []
    for _ in range(250):  # short scans
        lo = rng.randrange(2 * n)
        queries.append((_key16(lo), _key16(lo + rng.randint(2, 40)), rng.random() < 0.5, rng.random() < 0.5))
    for _ in range(100):  # bounds on odd (absent) counters
        lo = 2 * rng.randrange(n) + 1
        queries.append((_key16(lo), _key16(lo + 2 * rng.randint(0, 60)), rng.random() < 0.5, rng.random() < 0.5))
    last = [int(s) - 1 for s in t["starts"][1:]]  # each block's last item
    for i in last:  # bounds equal to a block's last key, each inclusivity
        k = item_key(items, i)
        for excl in (False, True):
            queries += [(k, _key16(2 * i + 10), excl, False), (_key16(max(0, 2 * i - 10)), k, False, excl),
                        (k, k, excl, excl)]
    for p in parts[:-1]:  # spans that cross a partition edge: around the partition's end key
        c = int.from_bytes(p[0], "big")
        for width in (1, 2, 30, 200):
            queries.append((_key16(max(0, c - width)), _key16(c + width), rng.random() < 0.5, rng.random() < 0.5))
    while len(queries) < 600:
        a, b = rng.randrange(2 * n + 20), rng.randrange(2 * n + 20)
        queries.append((_key16(a), _key16(b), rng.random() < 0.5, rng.random() < 0.5))
    queries = queries[:600]
    expected = expect(model, queries)
    compare(run(gpu, t["file"], table, queries), queries, expected)
    crossing = sum(1 for _, e in expected if e[0] == RANGE_ROWS and e[1] != e[4])
    assert crossing >= 50, crossing  # (first and last row in different blocks)


def test_table_range_one_block(gpu):
    items = pyoracle.Items.from_list([(b"k%02d" % i, b"v" * i, 9, 0) for i in range(1, 20)])
    for two_level in (False, True):
        t = pyoracle.table_write(items, block_size=1 << 16, two_level=two_level)
        assert t["block_count"] == 1
        size = int(t["block_off"][1])
        queries = [(None, None, False, False), (b"a", b"b", False, False), (b"a", b"k05", False, False),
                   (b"k05", b"k07", True, True), (b"k05", b"k05", False, False), (b"k05", b"k05", True, False),
                   (b"k055", b"k056", False, False), (b"k19", None, False, False), (b"k19", None, True, False),
                   (b"k19\0", None, False, False), (b"z", None, False, False), (None, b"", False, False),
                   (None, b"k01", False, True), (b"k10", b"k03", False, False)]
        expected, _ = check(gpu, t["file"], dict(t, two_level=two_level), queries)
        assert expected[0] == (0, (RANGE_ROWS, 0, size, 0, 0, size, 18))
        assert expected[3][1] == (RANGE_ROWS, 0, size, 5, 0, size, 5)
        assert [e[1][0] for e in expected[8:11]] == [RANGE_EMPTY, RANGE_NO_BLOCK, RANGE_NO_BLOCK]


def _data_block(rows, **kw):
    return pyoracle.block_write(pyoracle.data_block_encode(pyoracle.Items.from_list(rows), **kw))


def _hand_table(blocks, entries_of):
    """blocks back to back, then the TLI entries_of([(off, size)]) builds -> (file, table)."""
    off, handles = 0, []
    for b in blocks:
        handles.append((off, len(b)))
        off += len(b)
    tli = index_block(entries_of(handles))
    return b"".join(blocks) + tli, {"tli_off": off, "tli_size": len(tli), "two_level": False}


def test_table_range_index_disagrees_with_blocks(gpu):
    """Block 0 is indexed under b"b" but holds a0, a1: the lower bound b"b" names it and must
    walk on to block 1.  Mirrored: the last block is indexed under b"c" but holds d0, d1, so the
    upper bound b"c" names it and the walk must go back to the block before."""
    b0 = _data_block([(b"a0", b"x", 5, 0), (b"a1", b"y", 4, 0)])
    b1 = _data_block([(b"b", b"value", 3, 0)])
    file, table = _hand_table([b0, b1], lambda h: [(b"b", 5) + h[0], (b"c", 1) + h[1]])
    queries = [(b"b", None, False, False), (b"b", b"b", False, False), (b"a1", b"b", True, False),
               (b"b", None, True, False), (None, None, False, False), (b"a00", b"a1", False, False)]
    expected, _ = check(gpu, file, table, queries)
    assert expected[0] == (0, (RANGE_ROWS, len(b0), len(b1), 0, len(b0), len(b1), 0))
    assert expected[3][1][0] == RANGE_EMPTY and expected[5][1] == (RANGE_ROWS, 0, len(b0), 1, 0, len(b0), 1)

    c0 = _data_block([(b"a", b"x", 5, 0), (b"b", b"y", 4, 0)])
    c1 = _data_block([(b"d0", b"value", 3, 0), (b"d1", b"value", 3, 0)])
    file, table = _hand_table([c0, c1], lambda h: [(b"b", 4) + h[0], (b"c", 3) + h[1]])
    queries = [(None, b"c", False, False), (b"a", b"c", True, False), (b"b", b"c", True, False),
               (None, None, False, False), (None, b"d0", False, False)]
    expected, _ = check(gpu, file, table, queries)
    assert expected[0] == (0, (RANGE_ROWS, 0, len(c0), 0, 0, len(c0), 1))
    assert expected[1][1] == (RANGE_ROWS, 0, len(c0), 1, 0, len(c0), 1) and expected[2][1][0] == RANGE_EMPTY


# ---- statuses: one fault per file, answers from the model
def _three_blocks():
    items = counter_items(60, key_len=8, val_len=20, seed=4)
    blocks = [_data_block([(item_key(items, i), b"v" * 20, 63, 0) for i in range(b, b + 20)]) for b in (0, 20, 40)]
    ends = [item_key(items, i) for i in (19, 39, 59)]
    keys = [item_key(items, i) for i in range(60)]
    queries = [(None, None, False, False)] + [(k, k, False, False) for k in keys[::3]]
    queries += [(keys[a], keys[b], False, True) for a, b in ((0, 59), (5, 25), (25, 45), (21, 38), (0, 19), (40, 59))]
    queries += [(None, keys[30], False, False), (keys[30], None, False, False)]
    return blocks, ends, queries


def _check_status(gpu, file, table, queries, want_status, some_ok=False):
    model = RangeModel(file, table["tli_off"], table["tli_size"], table["two_level"])
    expected = expect(model, queries)
    bad = [e for e in expected if e[0] != 0]
    assert bad and all(e[0] == want_status and e[1][0] == RANGE_NONE for e in bad)
    assert (len(bad) < len(expected)) == some_ok
    compare(run(gpu, file, table, queries), queries, expected)
    return expected


def _small_table():
    items = counter_items(120, key_len=8, val_len=20, seed=4)
    t = pyoracle.table_write(items, block_size=512, two_level=False)
    keys = [item_key(items, i) for i in range(items.n)]
    return t, [(None, None, False, False), (keys[3], keys[90], False, False), (keys[119], None, True, False)]


def test_table_range_status_tli_magic(gpu):
    t, queries = _small_table()
    file = bytearray(t["file"])
    file[t["tli_off"] + 1] ^= 0x20
    _check_status(gpu, bytes(file), dict(t, two_level=False), queries, BAD_MAGIC)


def test_table_range_status_tli_type(gpu):
    t, queries = _small_table()
    tli = bytearray(t["file"][t["tli_off"]:])
    tli[4] = 0  # BlockType::Data
    file = t["file"][:t["tli_off"]] + reseal_header(tli)
    _check_status(gpu, file, dict(t, two_level=False), queries, TYPE_MISMATCH)


def test_table_range_status_first_block_past_file(gpu):
    blocks, ends, queries = _three_blocks()
    file, table = _hand_table(blocks, lambda h: [(ends[0], 63, h[0][0], h[0][1] + 100000), (ends[1], 63) + h[1],
                                                 (ends[2], 63) + h[2]])
    expected = _check_status(gpu, file, table, queries, TRUNCATED, some_ok=True)
    assert expected[0][0] == TRUNCATED  # (the unbounded range starts in it)


def test_table_range_status_last_block_short_handle(gpu):
    blocks, ends, queries = _three_blocks()
    file, table = _hand_table(blocks, lambda h: [(ends[0], 63) + h[0], (ends[1], 63) + h[1],
                                                 (ends[2], 63, h[2][0], 32)])
    expected = _check_status(gpu, file, table, queries, TRUNCATED, some_ok=True)
    assert expected[0][0] == TRUNCATED  # (the unbounded range ends in it: found by the upper walk)


def test_table_range_status_partition_past_file(gpu):
    blocks, ends, queries = _three_blocks()
    part = index_block([(ends[0], 63, 0, len(blocks[0]))])
    body = blocks[0] + part
    tli = index_block([(ends[0], 63, len(blocks[0]), len(part)), (ends[2], 63, len(body), 1 << 20)])
    table = {"tli_off": len(body), "tli_size": len(tli), "two_level": True}
    _check_status(gpu, body + tli, table, queries, TRUNCATED, some_ok=True)


def test_table_range_status_compressed_block(gpu):
    """A data block whose header says it is compressed (uncompressed_length != data_length),
    as every data block of an LZ4 table: UNSUPPORTED for the ranges that begin or end in it."""
    blocks, ends, queries = _three_blocks()
    payload = blocks[2][33:]
    blocks[2] = pyoracle.block_header(0, payload, len(payload) + 5) + payload
    file, table = _hand_table(blocks, lambda h: [(ends[i], 63) + h[i] for i in range(3)])
    _check_status(gpu, file, table, queries, UNSUPPORTED, some_ok=True)


def test_table_range_middle_block_not_read(gpu):
    """A damaged block strictly between the two rows is never read: the range is answered."""
    blocks, ends, queries = _three_blocks()
    middle = bytearray(blocks[1])
    middle[1] ^= 0x20
    blocks[1] = bytes(middle)
    file, table = _hand_table(blocks, lambda h: [(ends[i], 63) + h[i] for i in range(3)])
    expected = _check_status(gpu, file, table, queries, BAD_MAGIC, some_ok=True)
    size = [len(b) for b in blocks]
    assert expected[0] == (0, (RANGE_ROWS, 0, size[0], 0, size[0] + size[1], size[2], 19))


def test_table_range_offsets_of_another_table(gpu):
    """d_data_block_off of a shorter table (this one's first blocks only): BAD_ARG and NONE for
    the ranges with a handle that is not in it, the rest answered with their ordinals."""
    import torch
    _, t, queries, expected = mvcc_case(1, True)
    queries, expected = queries[:500], expected[:500]
    kept = t["block_count"] // 2
    known = ordinals(t["block_off"][:kept + 1])
    scan = {"block_off": torch.from_numpy(np.asarray(t["block_off"][:kept + 1], np.int64)).cuda(), "n_blocks": kept,
            "item_start": torch.from_numpy(np.asarray(t["starts"][:kept + 1], np.int32)).cuda()}
    want = [(BAD_ARG, (RANGE_NONE,) + e[1:]) if e[0] == RANGE_ROWS and not (e[1:3] in known and e[4:6] in known)
            else (st, e) for st, e in expected]
    outcomes = compare(run(gpu, t["file"], t, queries, scan=scan), queries, want, ordinal=known)
    assert outcomes[RANGE_NONE] >= 50 and outcomes[RANGE_ROWS] >= 50, outcomes


def test_table_range_after_write_table(gpu):
    """A two-level table built on the device by write_table, queried where it lies with the
    offsets the writer left; the model runs on the downloaded bytes."""
    items, _ = mvcc_table(2, True)
    wt = gpu.write_table(gpu.items_to_device(items), block_size=256, restart_interval=4, hash_ratio=1.33,
                         two_level=True, partition_size=128)
    queries = mvcc_range_queries(2, True)[::3]
    scan = {"block_off": wt["block_off"], "item_start": wt["starts"], "n_blocks": wt["block_count"]}
    res = run(gpu, wt["file"], dict(wt, two_level=True), queries, scan=scan)
    file = wt["file"].cpu().numpy().tobytes()
    model = RangeModel(file, wt["tli_off"], wt["tli_size"], True)
    outcomes = compare(res, queries, expect(model, queries), ordinal=ordinals(wt["block_off"].cpu().numpy()))
    assert outcomes[RANGE_ROWS] > 200
    keys = [item_key(items, i) for i in range(items.n)]
    for q, bounds in enumerate(queries):
        want = brute_force(keys, *bounds)
        window = (want[0], want[-1] + 1) if want else (0, 0)
        assert (int(res["row_first"][q]), int(res["row_end"][q])) == window, (q, bounds)
