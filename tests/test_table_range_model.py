"""CPU tests for lsm_table_range: the literal forward drain of Table::range
(tests/table_range_model.py) against brute force over the item list on the four MVCC tables,
with the coverage the GPU tests rely on asserted as conditions on the inputs (ranges whose
first or last block of the handle list yields no row, because versions of one key straddle
blocks), and the entry point's host-side argument checks (made before any HIP call; fake,
never dereferenced device addresses)."""
import ctypes as C

import pytest

from table_get_model import item_key, mvcc_table
from table_range_model import (RANGE_EMPTY, RANGE_NO_BLOCK, RANGE_ROWS, RangeModel, brute_force,
                               mvcc_range_queries)

BAD_ARG = 10


@pytest.mark.parametrize("two_level", [False, True])
@pytest.mark.parametrize("seed", [1, 2])
def test_drain_matches_brute_force(seed, two_level):
    items, t = mvcc_table(seed, two_level)
    model = RangeModel(t["file"], t["tli_off"], t["tli_size"], two_level)
    keys = [item_key(items, i) for i in range(items.n)]
    row0 = {int(t["block_off"][b]): int(t["starts"][b]) for b in range(t["block_count"])}
    count = {RANGE_ROWS: 0, RANGE_EMPTY: 0, RANGE_NO_BLOCK: 0}
    first_empty = last_empty = 0
    for q in mvcc_range_queries(seed, two_level):
        d = model.drain(*q)
        rows = [row0[h[0]] + i for h, first, end in d for i in range(first, end)]
        want = brute_force(keys, *q)
        assert rows == want, (q, rows[:3], want[:3])
        st, ans = model.answer(*q)
        assert st == 0
        count[ans[0]] += 1
        assert ans[0] == (RANGE_ROWS if want else RANGE_EMPTY if d else RANGE_NO_BLOCK), q
        if want:
            assert row0[ans[1]] + ans[3] == want[0] and row0[ans[4]] + ans[6] == want[-1], (q, ans)
        if d:
            first_empty += d[0][1] == d[0][2]
            last_empty += d[-1][1] == d[-1][2]
    print("ROWS / EMPTY / NO_BLOCK / first block empty / last block empty:", count[RANGE_ROWS], count[RANGE_EMPTY],
          count[RANGE_NO_BLOCK], first_empty, last_empty)
    assert count[RANGE_ROWS] >= 600 and count[RANGE_EMPTY] >= 50 and count[RANGE_NO_BLOCK] >= 500, count
    assert first_empty >= 100 and last_empty >= 100, (first_empty, last_empty)


def test_mvcc_tables_shape():
    """The tables the counts above are conditions on: 600 items, 26-29 blocks, 9-10 partitions."""
    for seed in (1, 2):
        items, t = mvcc_table(seed, True)
        model = RangeModel(t["file"], t["tli_off"], t["tli_size"], True)
        assert items.n == 600 and 26 <= t["block_count"] <= 29, t["block_count"]
        assert 9 <= len(model.table.index_entries(*model.table.tli)) <= 10


@pytest.fixture(scope="module")
def L():
    import lsmgpu
    if not lsmgpu.LIB_PATH.exists():
        lsmgpu.build()
    return lsmgpu


def _args(L, tbl, res, **override):
    """Every argument of lsm_table_range, valid (fake device addresses) but for the overrides."""
    a = {"d_file": C.c_void_p(0x10000), "file_len": 1 << 20, "table": C.byref(tbl), "d_lo": C.c_void_p(0x20000),
         "d_lo_off": C.c_void_p(0x30000), "d_hi": C.c_void_p(0x40000), "d_hi_off": C.c_void_p(0x50000),
         "d_flags": C.c_void_p(0x60000), "n_queries": 8, "d_data_block_off": None, "n_data_blocks": 0,
         "d_out": C.byref(res), "d_outcome": C.c_void_p(0x70000), "d_status": C.c_void_p(0x80000), "stream": None}
    a.update(override)
    return tuple(a.values())


def _result(L, **fields):
    r = L.LsmRangeResult()
    for f, v in dict({"first_item": 0x90000, "last_item": 0xA0000}, **fields).items():
        setattr(r, f, v)
    return r


def test_table_range_argument_checks(L):
    lib = L.lib()
    assert lib.lsm_abi_version() == 7  # additions only
    assert "lsm_table_range" in L.EXPORTED_SYMBOLS
    fn = lib.lsm_table_range
    table = L.LsmTableScan(4096, 100, 0, 0, 0)
    res = _result(L)
    # no queries: nothing to do, whatever the rest holds
    assert fn(*_args(L, table, res, n_queries=0, d_file=None, d_status=None)) == 0
    for null in ("d_file", "table", "d_lo", "d_lo_off", "d_hi", "d_hi_off", "d_flags", "d_out", "d_outcome",
                 "d_status"):
        assert fn(*_args(L, table, res, **{null: None})) == BAD_ARG, null
    for required in ("first_item", "last_item"):
        assert fn(*_args(L, table, _result(L, **{required: None}))) == BAD_ARG, required
    for name in ("d_file", "d_lo", "d_hi"):  # 16-byte aligned bases
        assert fn(*_args(L, table, res, **{name: C.c_void_p(0x10008)})) == BAD_ARG, name
    assert fn(*_args(L, L.LsmTableScan(4096, 100, 2, 0, 0), res)) == BAD_ARG               # two_level > 1
    assert fn(*_args(L, L.LsmTableScan(4096, 32, 0, 0, 0), res)) == BAD_ARG                # TLI shorter than a header
    assert fn(*_args(L, L.LsmTableScan((1 << 20) - 99, 100, 0, 0, 0), res)) == BAD_ARG     # TLI past the file
    assert fn(*_args(L, L.LsmTableScan(2 ** 64 - 50, 100, 0, 0, 0), res)) == BAD_ARG       # (wrapping)
    for ordinal in ("first_block", "last_block"):  # ordinals need the table's data-block offsets
        assert fn(*_args(L, table, _result(L, **{ordinal: 0xB0000}))) == BAD_ARG, ordinal
