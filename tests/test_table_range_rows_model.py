"""CPU tests for lsm_table_range_rows: the model (tests/table_range_rows_model.py) against the
item list sliced by brute force on the four MVCC tables, with the coverage the GPU tests rely on
asserted as conditions on the inputs, the new symbols, and the entry points' host-side argument
checks (made before any HIP call; fake, never dereferenced device addresses)."""
import ctypes as C

import pytest

import pyoracle
from table_get_model import item_key
from table_range_model import RANGE_ROWS, brute_force
from table_range_rows_model import RowsModel, item_rows, mvcc_rows_case

BAD_ARG = 10


@pytest.mark.parametrize("two_level", [False, True])
@pytest.mark.parametrize("seed", [1, 2])
def test_rows_match_brute_force(seed, two_level):
    items, t, queries, positions = mvcc_rows_case(seed, two_level)
    model = RowsModel(t["file"], t["block_off"], global_seqno=5)
    ans = model.answer(positions, base=(3, 40, 500))
    keys = [item_key(items, i) for i in range(items.n)]
    rows = item_rows(items, global_seqno=5)
    prefix = {}  # block -> prefix_len of its items

    def prefix_len(b, i):
        if b not in prefix:
            o0, o1 = int(t["block_off"][b]), int(t["block_off"][b + 1])
            n, p = pyoracle.data_block_decode(t["file"][o0 + 33:o1])
            assert n > 0
            prefix[b] = p["prefix_len"]
        return int(prefix[b][i])

    live = total = pairs = one_block = three_blocks = mid_interval = 0
    for q, (bounds, pos) in enumerate(zip(queries, positions)):
        want = brute_force(keys, *bounds)
        assert ans["row_status"][q] == 0
        assert ans["runs"][q] == [rows[i] for i in want], (q, bounds)
        assert ans["run_start"][q + 1] - ans["run_start"][q] == len(want)
        if pos[1] != RANGE_ROWS:
            assert not want
            continue
        _, _, fb, fi, lb, _ = pos
        live += 1
        total += len(want)
        pairs += lb - fb + 1
        one_block += fb == lb
        three_blocks += lb - fb >= 2
        mid_interval += fi % 4 != 0 and prefix_len(fb, fi) > 0  # (mvcc_table: restart interval 4)
    assert ans["run_start"][0] == 3 and ans["run_start"][-1] == ans["end"][0] == 3 + total
    assert ans["need"] == [pairs, total, ans["end"][1] - 40, ans["end"][2] - 500]
    print("ROWS / rows / pairs / one block / three blocks or more / first row inside an interval with a prefix:",
          live, total, pairs, one_block, three_blocks, mid_interval)
    assert live >= 700 and total >= 150_000 and pairs >= 7_000, (live, total, pairs)
    assert one_block >= 15 and three_blocks >= 600 and mid_interval >= 400, (one_block, three_blocks, mid_interval)


def test_model_statuses():
    """The validation order on a hand-damaged table: positions first, then per block the handle,
    the header, the edge items, the records; the lowest ordinal's status wins."""
    items, t, _, _ = mvcc_rows_case(1, False)
    off = [int(o) for o in t["block_off"]]
    file = bytearray(t["file"])
    file[off[2] + 1] ^= 0x20          # block 2: bad magic
    file[off[4] + 33] = 0x77          # block 4: the first record's value type
    model = RowsModel(bytes(file), off)
    n = len(off) - 1
    cases = [((0, 3, 0, 0, 1, 0), 0), ((0, 3, 1, 0, 0, 0), BAD_ARG), ((0, 3, 0, 0, n, 0), BAD_ARG),
             ((0, 3, 0, 10 ** 6, 1, 0), BAD_ARG), ((0, 3, 1, 0, 3, 0), 1), ((0, 3, 3, 0, 5, 0), 5),
             ((0, 3, 4, 10 ** 6, 5, 0), BAD_ARG), ((0, 3, 2, 0, 4, 0), 1), ((7, 0, 0, 0, 0, 0), 7),
             ((0, 2, 0, 0, 0, 0), 0)]
    ans = model.answer([c for c, _ in cases])
    assert ans["row_status"] == [st for _, st in cases]
    assert [len(r) > 0 for r in ans["runs"]] == [True] + [False] * 9
    short = RowsModel(bytes(file)[:off[1] + 10], off)  # the offsets end past the file
    assert short.query(0, 3, 0, 0, 1, 0)[0] == 8 and short.query(0, 3, 0, 0, 0, 0)[0] == 0


@pytest.fixture(scope="module")
def L():
    import lsmgpu
    if not lsmgpu.LIB_PATH.exists():
        lsmgpu.build()
    return lsmgpu


def _positions(L, **override):
    f = {"outcome": 0x90000, "status": 0xA0000, "first_block": 0xB0000, "first_item": 0xC0000,
         "last_block": 0xD0000, "last_item": 0xE0000}
    f.update(override)
    return L.LsmRangePositions(**f)


def _plan_args(L, tbl, ps, ws, **override):
    """Every argument of lsm_table_range_rows_plan, valid (fake device addresses) but for the overrides."""
    a = {"d_file": C.c_void_p(0x10000), "file_len": 1 << 20, "table": C.byref(tbl),
         "d_data_block_off": C.c_void_p(0x20000), "n_data_blocks": 64, "pos": C.byref(ps), "n_queries": 8,
         "block_cap": 100, "row_cap": 1000, "d_base": C.c_void_p(0x30000), "d_run_start": C.c_void_p(0x40000),
         "d_end": C.c_void_p(0x50000), "d_need": C.c_void_p(0x60000), "d_row_status": C.c_void_p(0x70000),
         "d_result": C.c_void_p(0x80000), "d_workspace": C.c_void_p(0x100000), "workspace_bytes": ws, "stream": None}
    a.update(override)
    return tuple(a.values())


def _rows_args(L, tbl, ps, ws, **override):
    a = {"d_file": C.c_void_p(0x10000), "file_len": 1 << 20, "table": C.byref(tbl),
         "d_data_block_off": C.c_void_p(0x20000), "n_data_blocks": 64, "pos": C.byref(ps), "n_queries": 8,
         "block_cap": 100, "row_cap": 1000, "d_base": C.c_void_p(0x30000), "d_end": C.c_void_p(0x50000),
         "d_workspace": C.c_void_p(0x100000), "workspace_bytes": ws, "d_out_key_off": C.c_void_p(0x200000),
         "d_out_val_off": C.c_void_p(0x300000), "d_out_keys": C.c_void_p(0x400000), "key_cap": 1 << 16,
         "d_out_vals": C.c_void_p(0x500000), "val_cap": 1 << 16, "d_out_seqno": C.c_void_p(0x600000),
         "d_out_vtype": C.c_void_p(0x700000), "out_item_cap": 1000, "d_result": C.c_void_p(0x80000), "stream": None}
    a.update(override)
    return tuple(a.values())


def test_table_range_rows_argument_checks(L):
    lib = L.lib()
    assert lib.lsm_abi_version() == 7  # additions only
    for name in ("lsm_table_range_rows_workspace_size", "lsm_table_range_rows_plan", "lsm_table_range_rows"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name)
    size = lib.lsm_table_range_rows_workspace_size
    ws = size(8, 100, 1000)
    assert ws > 0 and size(8, 101, 1000) >= ws and size(8, 100, 1001) >= ws and size(9, 100, 1000) >= ws
    assert size(8, 100, 1 << 20) - size(8, 100, 0) >= 31 << 20  # (the row descriptors, 32 bytes a row)
    table = L.LsmTableScan(4096, 100, 0, 5, 0)
    pos = _positions(L)
    plan, rows = lib.lsm_table_range_rows_plan, lib.lsm_table_range_rows
    for fn, args, required in (
            (plan, _plan_args, ("d_file", "table", "d_data_block_off", "pos", "d_run_start", "d_end", "d_need",
                                "d_row_status", "d_result", "d_workspace")),
            (rows, _rows_args, ("d_file", "table", "d_data_block_off", "pos", "d_end", "d_workspace",
                                "d_out_key_off", "d_out_val_off", "d_out_keys", "d_out_vals", "d_out_seqno",
                                "d_out_vtype", "d_result"))):
        for null in required:
            assert fn(*args(L, table, pos, ws, **{null: None})) == BAD_ARG, (fn.__name__, null)
        for field in ("outcome", "status", "first_block", "first_item", "last_block", "last_item"):
            assert fn(*args(L, table, _positions(L, **{field: None}), ws)) == BAD_ARG, (fn.__name__, field)
        assert fn(*args(L, table, pos, ws, d_file=C.c_void_p(0x10008))) == BAD_ARG      # 16-byte aligned base
        assert fn(*args(L, table, pos, ws, workspace_bytes=ws - 1)) == BAD_ARG           # workspace too small
        assert fn(*args(L, table, pos, ws, d_end=C.c_void_p(0x30000))) == BAD_ARG        # d_end is d_base
        assert fn(*args(L, table, pos, 1 << 62, block_cap=2 ** 32 - 1)) == BAD_ARG       # caps size grids
        assert fn(*args(L, table, pos, 1 << 62, row_cap=2 ** 32 - 1)) == BAD_ARG
    # n_queries == 0 still needs where to put the result
    assert plan(*_plan_args(L, table, pos, ws, n_queries=0, d_result=None)) == BAD_ARG
    assert plan(*_plan_args(L, table, pos, ws, n_queries=0, d_end=None)) == BAD_ARG
    assert rows(*_rows_args(L, table, pos, ws, n_queries=0, d_result=None)) == BAD_ARG
