"""CPU tests for lsm_table_get: the Table::get model (tests/table_get_model.py) against
brute force over the item list, with the coverage the GPU tests rely on asserted (the
seqno term of the index seek moves the chosen data block and, on two-level tables, the
chosen partition), and the entry point's host-side argument checks (made before any HIP
call; fake, never dereferenced device addresses)."""
import ctypes as C

import numpy as np
import pytest

from table_get_model import GET_HIT, TableModel, item_key, mvcc_queries, mvcc_table

BAD_ARG = 10


def brute_force(keys, seqnos, key, snapshot):
    """Global row of the first item in table order with key == k and seqno < s, or None."""
    for i, k in enumerate(keys):
        if k == key and seqnos[i] < snapshot:
            return i
    return None


@pytest.mark.parametrize("two_level", [False, True])
@pytest.mark.parametrize("seed", [1, 2])
def test_model_matches_brute_force(seed, two_level):
    items, t = mvcc_table(seed, two_level)
    model = TableModel(t["file"], t["tli_off"], t["tli_size"], two_level)
    starts, off = t["starts"], t["block_off"]
    keys, seqnos = [item_key(items, i) for i in range(items.n)], [int(s) for s in items.seqno]
    moved_block = moved_part = hits = 0
    for key, snap in mvcc_queries(items, seed):
        want = brute_force(keys, seqnos, key, snap)
        outcome, block_off, block_size, item, seqno, _, val_len, vtype = model.get(key, snap)
        if want is None:
            assert outcome != GET_HIT and item == -1, (key, snap, outcome)
        else:
            b = int(np.searchsorted(starts, want, side="right")) - 1
            assert outcome == GET_HIT, (key, snap, outcome)
            assert (block_off, block_size) == (int(off[b]), int(off[b + 1] - off[b])), (key, snap)
            assert item == want - int(starts[b]) and int(starts[b]) + item == want, (key, snap)
            assert seqno == int(items.seqno[want]) and vtype == int(items.vtype[want])
            assert val_len == int(items.val_off[want + 1] - items.val_off[want])
            hits += 1
        if snap > 0:  # (snapshot 0 never reaches the index)
            at, plain = model.first_handle(key, snap), model.first_handle(key, 1 << 63)
            if plain is not None and at != plain:
                moved_block += (at is None) or at[1] != plain[1]
                moved_part += (at is None) or at[0] != plain[0]
    assert hits > 600
    assert moved_block >= 100, moved_block
    if two_level:
        assert moved_part >= 100, moved_part


@pytest.fixture(scope="module")
def L():
    import lsmgpu
    if not lsmgpu.LIB_PATH.exists():
        lsmgpu.build()
    return lsmgpu


def _args(L, tbl, res, **override):
    """Every argument of lsm_table_get, valid (fake device addresses) but for the overrides."""
    a = {"d_file": C.c_void_p(0x10000), "file_len": 1 << 20, "table": C.byref(tbl), "filter_off": 0,
         "filter_size": 0, "lowest_seqno": 0, "d_needles": C.c_void_p(0x20000), "d_needle_off": C.c_void_p(0x30000),
         "d_snapshot": C.c_void_p(0x40000), "d_key_hash": None, "d_active": None, "n_queries": 8,
         "d_out": C.byref(res), "d_hit_block_off": None, "d_hit_block_size": None, "d_outcome": None,
         "d_status": C.c_void_p(0x50000), "stream": None}
    a.update(override)
    return tuple(a.values())


def test_table_get_argument_checks(L):
    lib = L.lib()
    assert lib.lsm_abi_version() == 7  # additions only
    assert "lsm_table_get" in L.EXPORTED_SYMBOLS
    fn = lib.lsm_table_get
    table = L.LsmTableScan(4096, 100, 0, 0, 0)
    res = L.LsmPointResult(C.c_void_p(0x60000), None, None, None, None)
    # no queries: nothing to do, whatever the rest holds
    assert fn(*_args(L, table, res, n_queries=0, d_file=None, d_status=None)) == 0
    for null in ("d_file", "table", "d_needles", "d_needle_off", "d_snapshot", "d_out", "d_status"):
        assert fn(*_args(L, table, res, **{null: None})) == BAD_ARG, null
    no_item = L.LsmPointResult(None, C.c_void_p(0x60000), None, None, None)
    assert fn(*_args(L, table, no_item)) == BAD_ARG
    for name in ("d_file", "d_needles"):  # 16-byte aligned bases
        assert fn(*_args(L, table, res, **{name: C.c_void_p(0x10008)})) == BAD_ARG, name
    assert fn(*_args(L, L.LsmTableScan(4096, 32, 0, 0, 0), res)) == BAD_ARG             # TLI shorter than a header
    assert fn(*_args(L, L.LsmTableScan((1 << 20) - 99, 100, 0, 0, 0), res)) == BAD_ARG  # TLI past the file
    assert fn(*_args(L, L.LsmTableScan(2 ** 64 - 50, 100, 0, 0, 0), res)) == BAD_ARG    # (wrapping)
    assert fn(*_args(L, table, res, filter_off=(1 << 20) - 10, filter_size=11)) == BAD_ARG  # filter past the file
    assert fn(*_args(L, table, res, filter_off=2 ** 64 - 5, filter_size=11)) == BAD_ARG
