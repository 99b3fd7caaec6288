"""GPU parity of lsm_table_get (batched Table::get, src/table/mod.rs:229-340) against the
Python model in tests/table_get_model.py, never against the library itself.  Bar: for
every query the status, the outcome and every result field equal the model's (rows the
kernel does not write, i.e. the fields of a non-hit, keep what the output held before)."""
import functools
import random

import numpy as np
import pytest

import pyoracle
from helpers import counter_items
from table_get_model import (BAD_MAGIC, GET_FILTERED, GET_HIT, GET_MISS, GET_NO_BLOCK, GET_NONE, GET_SEQNO_SKIP,
                             TRUNCATED, TYPE_MISMATCH, UNSUPPORTED, TableModel, index_block, item_key,
                             mvcc_queries, mvcc_table, reseal_header, with_filter)

pytestmark = pytest.mark.gpu

FIELDS = ("block_off", "block_size", "item", "seqno", "val_off", "val_len", "vtype")
U64 = 2 ** 64 - 1


def _i64(values):
    """Python ints (any u64) -> int64 cuda tensor holding the same bits."""
    import torch
    return torch.from_numpy(np.array([v & U64 for v in values], np.uint64).view(np.int64)).cuda()


def run(gpu, file, table, queries, filter=None, hashes=False, lowest_seqno=0, global_seqno=0, active=None, out=None):
    """queries: [(needle, snapshot)] -> result dict of numpy arrays.  file: bytes (uploaded
    with padding) or a padded cuda tensor."""
    import torch
    needles = b"".join(q[0] for q in queries)
    noff = np.zeros(len(queries) + 1, np.int64)
    noff[1:] = np.cumsum([len(q[0]) for q in queries])
    if isinstance(file, (bytes, bytearray)):
        table = dict(table, file_len=len(file))
        file = gpu.to_device_bytes(file)
    res = gpu.table_get(file, table, gpu.to_device_bytes(needles), torch.from_numpy(noff).cuda(),
                        _i64(q[1] for q in queries),
                        key_hash=_i64(pyoracle.xxh3_64(q[0]) for q in queries) if hashes else None,
                        active=None if active is None else torch.tensor(active, dtype=torch.uint8).cuda(),
                        filter=filter, lowest_seqno=lowest_seqno, global_seqno=global_seqno, out=out)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy()[:len(queries)] for k, v in res.items()}


def expect(model, queries):
    """[(status, (outcome, block_off, ...))] of the model, one per query."""
    return [model.lookup(k, s) for k, s in queries]


def compare(res, queries, expected, untouched=0):
    """Every output of every query against the model.  untouched: what the fields the
    kernel leaves alone on a non-hit were filled with."""
    outcomes = {}
    for q, (st, exp) in enumerate(expected):
        got_st, got_oc = int(res["status"][q]), int(res["outcome"][q])
        assert (got_st, got_oc) == (st, exp[0]), (q, queries[q], got_st, got_oc, st, exp[0])
        outcomes[exp[0]] = outcomes.get(exp[0], 0) + 1
        for f, want in zip(FIELDS, exp[1:]):
            got = int(res[f][q]) & U64 if f == "seqno" else int(res[f][q])
            if exp[0] != GET_HIT and f != "item":
                want = untouched
            assert got == want, (q, queries[q], f, got, want)
    return outcomes


@functools.lru_cache(maxsize=None)
def mvcc_case(seed, two_level, filtered):
    """Table, queries and the model's answers, computed once per table."""
    items, t = mvcc_table(seed, two_level)
    file, flt = with_filter(t, items) if filtered else (t["file"], None)
    model = TableModel(file, t["tli_off"], t["tli_size"], two_level, filter=flt)
    queries = mvcc_queries(items, seed)
    return file, dict(t, two_level=two_level), flt, model, queries, expect(model, queries)


@pytest.mark.parametrize("two_level", [False, True])
@pytest.mark.parametrize("seed", [1, 2])
def test_table_get_mvcc_tables(gpu, seed, two_level):
    file, table, _, _, queries, expected = mvcc_case(seed, two_level, False)
    outcomes = compare(run(gpu, file, table, queries), queries, expected)
    assert outcomes[GET_HIT] > 600 and outcomes[GET_MISS] > 0 and outcomes[GET_NO_BLOCK] > 0
    assert outcomes[GET_SEQNO_SKIP] >= 600  # (snapshot 0)


@pytest.mark.parametrize("hashes", [False, True])
@pytest.mark.parametrize("two_level", [False, True])
@pytest.mark.parametrize("seed", [1, 2])
def test_table_get_with_filter(gpu, seed, two_level, hashes):
    file, table, flt, _, queries, expected = mvcc_case(seed, two_level, True)
    plain = mvcc_case(seed, two_level, False)[5]
    assert any(e[1][0] == GET_FILTERED for e in expected)
    # (where the filter passes, present key or false positive, the answer is the table's)
    assert all(e == p for e, p in zip(expected, plain) if e[1][0] != GET_FILTERED)
    outcomes = compare(run(gpu, file, table, queries, filter=flt, hashes=hashes), queries, expected)
    assert outcomes[GET_FILTERED] > 0 and outcomes[GET_HIT] > 600


def test_table_get_global_and_lowest_seqno(gpu):
    """global_seqno 7, lowest_seqno = the table's minimum seqno: SEQNO_SKIP for snapshots at
    or below it (after the shift), hit seqnos shifted by 7, snapshots below 7 saturate to 0."""
    items, t = mvcc_table(1, True)
    lowest = int(items.seqno.min())
    model = TableModel(t["file"], t["tli_off"], t["tli_size"], True, lowest_seqno=lowest, global_seqno=7)
    queries = []
    for i in range(0, items.n, 3):
        k, s = item_key(items, i), int(items.seqno[i])
        queries += [(k, s + 8), (k, s + 7), (k, s + 1)]
    k = item_key(items, 0)
    queries += [(k, s) for s in (0, 1, 6, 7, 8, lowest + 6, lowest + 7, lowest + 8, U64, 1 << 63)]
    expected = expect(model, queries)
    res = run(gpu, t["file"], dict(t, two_level=True), queries, lowest_seqno=lowest, global_seqno=7)
    outcomes = compare(res, queries, expected)
    assert outcomes[GET_SEQNO_SKIP] >= 6 and outcomes[GET_HIT] > 150  # (the six snapshots <= lowest + 7 above)
    assert expected[-3][1][0] != GET_SEQNO_SKIP and expected[-4][1][0] == GET_SEQNO_SKIP
    hit = next(q for q, e in enumerate(expected) if e[1][0] == GET_HIT)
    row = next(i for i in range(items.n)
               if item_key(items, i) == queries[hit][0] and int(items.seqno[i]) + 7 < queries[hit][1])
    assert int(res["seqno"][hit]) == int(items.seqno[row]) + 7


@pytest.mark.parametrize("n,step", [(4000, 4), (2500, 2)])
def test_table_get_binary_index_step(gpu, n, step):
    """One-item blocks under a full index: 4000 entries need a 4-byte binary-index step
    in the TLI, 2500 still fit 2 bytes."""
    items = counter_items(n, key_len=16, val_len=8, seed=3)
    t = pyoracle.table_write(items, block_size=1, two_level=False)
    assert t["block_count"] == n
    tli = t["file"][t["tli_off"]:t["tli_off"] + t["tli_size"]]
    assert tli[len(tli) - 31 + 1] == step, (t["tli_size"], tli[len(tli) - 31 + 1])
    model = TableModel(t["file"], t["tli_off"], t["tli_size"], False)
    queries = [(item_key(items, i), 64) for i in range(n)]
    rng = random.Random(n)
    for j in range(100):
        queries.append((item_key(items, rng.randrange(n)) + b"\0", 64))       # between two keys
        queries.append(((n + j).to_bytes(16, "big"), rng.choice([64, 1 << 62])))  # above the last key
    expected = expect(model, queries)
    outcomes = compare(run(gpu, t["file"], dict(t, two_level=False), queries), queries, expected)
    assert outcomes[GET_HIT] == n and outcomes[GET_MISS] + outcomes[GET_NO_BLOCK] == 200
    assert outcomes[GET_NO_BLOCK] >= 100


def test_table_get_one_block(gpu):
    items = pyoracle.Items.from_list([(b"k%02d" % i, b"v" * i, 9, 0) for i in range(1, 20)])
    for two_level in (False, True):
        t = pyoracle.table_write(items, block_size=1 << 16, two_level=two_level)
        assert t["block_count"] == 1
        model = TableModel(t["file"], t["tli_off"], t["tli_size"], two_level)
        queries = [(b"a", 10), (b"k00", 10), (b"k19\0", 10), (b"z", 10), (b"", 10), (b"k05", 10), (b"k05", 9),
                   (b"k055", 10), (b"k19", 10), (b"k01", 10)]
        expected = expect(model, queries)
        assert [e[1][0] for e in expected[:5]] == [GET_MISS, GET_MISS, GET_NO_BLOCK, GET_NO_BLOCK, GET_MISS]
        compare(run(gpu, t["file"], dict(t, two_level=two_level), queries), queries, expected)


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


def test_table_get_next_handle_loop(gpu):
    """An index that disagrees with its blocks: block 0 ends below its index key, so a miss
    there (end key equal to the needle) must go on to block 1."""
    b0 = _data_block([(b"a0", b"x", 5, 0), (b"a1", b"y", 4, 0)])
    b1 = _data_block([(b"b", b"value", 3, 0)])
    file, table = _hand_table([b0, b1], lambda h: [(b"b", 5) + h[0], (b"c", 1) + h[1]])
    model = TableModel(file, table["tli_off"], table["tli_size"], False)
    queries = [(b"b", 10), (b"a0", 10), (b"a00", 10), (b"b", 3), (b"c", 10), (b"bb", 10)]
    expected = expect(model, queries)
    assert expected[0][1][:4] == (GET_HIT, len(b0), len(b1), 0)
    assert expected[1][1][:2] == (GET_HIT, 0) and expected[2][1][0] == GET_MISS
    compare(run(gpu, file, table, queries), queries, expected)


def test_table_get_active_mask(gpu):
    import torch
    file, table, _, _, queries, expected = mvcc_case(1, True, False)
    queries, expected = queries[:800], expected[:800]
    active = [q % 2 for q in range(len(queries))]
    sentinel = 0x5A
    out = {f: torch.full((len(queries),), sentinel, dtype=getattr(torch, dt), device="cuda")
           for f, dt in gpu.TABLE_GET_FIELDS}
    res = run(gpu, file, table, queries, active=active, out=out)
    on = [q for q in range(len(queries)) if active[q]]
    compare({k: v[on] for k, v in res.items()}, [queries[q] for q in on], [expected[q] for q in on],
            untouched=sentinel)
    off = [q for q in range(len(queries)) if not active[q]]
    for f, _ in gpu.TABLE_GET_FIELDS:
        assert (res[f][off] == sentinel).all(), f


def _small_table(two_level=False):
    items = counter_items(120, key_len=8, val_len=20, seed=4)
    t = pyoracle.table_write(items, block_size=512, two_level=two_level, partition_size=128)
    queries = [(item_key(items, i), 64) for i in range(items.n)] + [((1000).to_bytes(8, "big"), 64), (b"", 64)]
    return items, t, queries


def _check_status(gpu, file, table, queries, want_status, some_ok=False, filter=None):
    model = TableModel(file, table["tli_off"], table["tli_size"], table["two_level"], filter=filter)
    expected = expect(model, queries)
    bad = [e for e in expected if e[0] != 0]
    assert bad and all(e[0] == want_status and e[1][0] == GET_NONE for e in bad)
    assert (len(bad) < len(expected)) == some_ok
    compare(run(gpu, file, table, queries, filter=filter), queries, expected)


def test_table_get_status_tli_magic(gpu):
    _, t, queries = _small_table()
    file = bytearray(t["file"])
    file[t["tli_off"] + 1] ^= 0x20
    _check_status(gpu, bytes(file), dict(t, two_level=False), queries, BAD_MAGIC)


def test_table_get_status_tli_type(gpu):
    _, t, queries = _small_table()
    tli = bytearray(t["file"][t["tli_off"]:])
    tli[4] = 0  # BlockType::Data
    file = t["file"][:t["tli_off"]] + reseal_header(tli)
    _check_status(gpu, file, dict(t, two_level=False), queries, TYPE_MISMATCH)


def test_table_get_status_handle_past_file(gpu):
    """The last data block's handle runs past the file; a partition's does, on a two-level table."""
    items = counter_items(60, key_len=8, val_len=20, seed=4)
    blocks = [_data_block([(item_key(items, i), b"v" * 20, 63, 0) for i in range(b, b + 20)]) for b in (0, 20, 40)]
    ends = [item_key(items, i) for i in (19, 39, 59)]
    queries = [(item_key(items, i), 64) for i in range(items.n)]
    file, table = _hand_table(blocks, lambda h: [(ends[0], 63) + h[0], (ends[1], 63) + h[1],
                                                 (ends[2], 63, h[2][0], h[2][1] + 100000)])
    _check_status(gpu, file, table, queries, TRUNCATED, some_ok=True)
    # a handle shorter than a header
    file, table = _hand_table(blocks, lambda h: [(ends[0], 63) + h[0], (ends[1], 63, h[1][0], 32),
                                                 (ends[2], 63) + h[2]])
    _check_status(gpu, file, table, queries, TRUNCATED, some_ok=True)
    # two-level: the TLI names a partition past the file
    part = index_block([(ends[0], 63, 0, len(blocks[0]))])
    body = blocks[0] + part
    tli = index_block([(ends[0], 63, len(blocks[0]), len(part)), (ends[2], 63, len(body), 1 << 20)])
    table = {"tli_off": len(body), "tli_size": len(tli), "two_level": True}
    _check_status(gpu, body + tli, table, queries, TRUNCATED, some_ok=True)


def test_table_get_status_compressed_block(gpu):
    """A data block whose header says it is compressed (uncompressed_length != data_length),
    as every data block of an LZ4 table: UNSUPPORTED for the queries that reach it."""
    items = counter_items(40, key_len=8, val_len=20, seed=4)
    rows = [[(item_key(items, i), b"v" * 20, 63, 0) for i in range(b, b + 20)] for b in (0, 20)]
    payload = pyoracle.data_block_encode(pyoracle.Items.from_list(rows[1]))
    blocks = [_data_block(rows[0]), pyoracle.block_header(0, payload, len(payload) + 5) + payload]
    file, table = _hand_table(blocks, lambda h: [(rows[0][-1][0], 63) + h[0], (rows[1][-1][0], 63) + h[1]])
    _check_status(gpu, file, table, [(item_key(items, i), 64) for i in range(40)], UNSUPPORTED, some_ok=True)


def test_table_get_status_bloom_magic(gpu):
    items, t, queries = _small_table()
    file, (f_off, f_size) = with_filter(t, items)
    image = bytearray(file[f_off + 33:])
    image[2] ^= 1
    file = file[:f_off] + pyoracle.block_write(bytes(image), block_type=2)
    _check_status(gpu, file, dict(t, two_level=False), queries, BAD_MAGIC, filter=(f_off, f_size))
    # a filter region that is not a Filter block
    file = t["file"] + pyoracle.block_write(bytes(image), block_type=3)
    _check_status(gpu, file, dict(t, two_level=False), queries, TYPE_MISMATCH, filter=(f_off, f_size))


def test_table_get_after_write_table(gpu):
    """A two-level table built on the device by write_table, queried where it lies; the
    model runs on the downloaded bytes."""
    items, _ = mvcc_table(2, True)
    wt = gpu.write_table(gpu.items_to_device(items), block_size=256, restart_interval=4, hash_ratio=1.33,
                         two_level=True, partition_size=128)
    table = dict(wt, two_level=True)
    queries = mvcc_queries(items, 2)[::3]
    res = run(gpu, wt["file"], table, queries)
    file = wt["file"].cpu().numpy().tobytes()
    model = TableModel(file, wt["tli_off"], wt["tli_size"], True)
    outcomes = compare(res, queries, expect(model, queries))
    assert outcomes[GET_HIT] > 200
