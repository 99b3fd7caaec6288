"""CPU checks of the LZ4 table models (tests/table_lz4_model.py) and of the framed readers'
binding: the LZ4 models on a table's LZ4 twin give the plain models' answers on the original
with the block handles moved, the library exports the four framed entry points, the struct
mirror follows the header and the wrappers take frames=."""
import ctypes as C
import inspect
import re
from pathlib import Path

import pytest

import pyoracle
from table_get_model import DATA, GET_HIT, TYPE_MISMATCH, TableModel, mvcc_queries, mvcc_table, reseal_header
from table_lz4_model import (CKSUM, DECOMPRESS, LZ4RangeModel, LZ4RowsModel, LZ4TableModel, lz4_twin, remap_get,
                             remap_range)
from table_range_model import RANGE_ROWS, RangeModel, mvcc_range_queries
from table_range_rows_model import RowsModel, mvcc_rows_case, positions_of

ROOT = Path(__file__).resolve().parent.parent
FRAMED = ("lsm_table_get_framed", "lsm_table_range_framed", "lsm_table_range_rows_plan_framed",
          "lsm_table_range_rows_framed")


@pytest.fixture(scope="module")
def L():
    import lsmgpu
    if not lsmgpu.LIB_PATH.exists():
        lsmgpu.build()
    return lsmgpu


@pytest.mark.parametrize("two_level", [False, True])
@pytest.mark.parametrize("seed", [1, 2])
def test_lz4_models_on_the_twin(seed, two_level):
    items, t = mvcc_table(seed, two_level)
    twin = lz4_twin(t, two_level)
    hm = twin["handle_map"]
    assert len(hm) == t["block_count"] and twin["file"] != t["file"]
    # every twin data block is LZ4 and decompresses back to the original payload
    model = LZ4TableModel(twin["file"], twin["tli_off"], twin["tli_size"], two_level)
    for (o, z), (no, nz) in hm.items():
        st, h = pyoracle.header_decode(twin["file"][no:no + 33])
        assert st == 0 and h.block_type == DATA and h.data_length == nz - 33 and h.uncompressed_length == z - 33
        assert model._load(no, nz, DATA) == t["file"][o + 33:o + z]
    # Table::get
    queries = mvcc_queries(items, seed)
    plain = TableModel(t["file"], t["tli_off"], t["tli_size"], two_level)
    want = remap_get([plain.lookup(k, s) for k, s in queries], hm)
    got = [model.lookup(k, s) for k, s in queries]
    assert got == want and sum(e[1][0] == GET_HIT for e in got) > 600
    # Table::range
    rq = mvcc_range_queries(seed, two_level)
    pr = RangeModel(t["file"], t["tli_off"], t["tli_size"], two_level)
    lr = LZ4RangeModel(twin["file"], twin["tli_off"], twin["tli_size"], two_level)
    want = remap_range([pr.answer(*q) for q in rq], hm)
    got = [lr.answer(*q) for q in rq]
    assert got == want and sum(e[1][0] == RANGE_ROWS for e in got) >= 600
    # the rows: same positions (compression does not move the block cut), same rows
    _, _, _, positions = mvcc_rows_case(seed, two_level)
    assert positions_of(got, twin["block_off"]) == positions
    some = positions[::25]
    assert LZ4RowsModel(twin["file"], twin["block_off"], 5).answer(some) == \
        RowsModel(t["file"], t["block_off"], 5).answer(some)


def test_lz4_model_fault_order():
    """The reference's order on one block: the checksum of the stored bytes before the
    decompression, both before the type test."""
    _, t = mvcc_table(1, False)
    twin = lz4_twin(t, False)
    (o, z) = twin["handle_map"][(0, int(t["block_off"][1]))]
    blk = bytearray(twin["file"][o:o + z])

    def status(block):
        file = bytes(block) + twin["file"][z:]
        m = LZ4TableModel(file, twin["tli_off"], twin["tli_size"], False)
        with pytest.raises(Exception) as err:
            m._load(o, z, DATA)
        return err.value.status

    flipped = bytearray(blk)
    flipped[40] ^= 0x01
    assert status(flipped) == CKSUM
    bad = bytearray(blk)
    bad[33:36] = b"\xff\xff\xff"  # a literal run longer than the stream
    resealed = pyoracle.block_header(0, bytes(bad[33:]), int(t["block_off"][1]) - 33) + bytes(bad[33:])
    assert status(resealed) == DECOMPRESS
    index_typed = bytearray(blk)
    index_typed[4] = 1
    assert status(reseal_header(index_typed)) == TYPE_MISMATCH
    both = bytearray(reseal_header(index_typed))
    both[40] ^= 0x01
    assert status(both) == CKSUM


def test_library_exports_the_framed_entry_points(L):
    lib = L.lib()
    assert lib.lsm_abi_version() == 7 == L.ABI_VERSION
    for name in FRAMED:
        assert hasattr(lib, name) and name in L.EXPORTED_SYMBOLS, name
    plain, framed = ([" ".join(p.split()) for p in L.PROTOTYPES[f][1]] for f in ("lsm_table_get", FRAMED[0]))
    assert framed[:len(plain) - 1] == plain[:-1] and len(framed) == len(plain) + 2
    assert len(L.PROTOTYPES["lsm_table_range_framed"][1]) == len(L.PROTOTYPES["lsm_table_range"][1]) - 1
    for name in ("lsm_table_range_rows_plan", "lsm_table_range_rows"):
        assert len(L.PROTOTYPES[name + "_framed"][1]) == len(L.PROTOTYPES[name][1]) - 3


def test_frames_struct_follows_the_header(L):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "lsmgpu.h").read_text(), flags=re.S)
    body = re.search(r"struct\s+lsm_table_frames\s*\{([^{}]*)\}", text).group(1)
    fields = [" ".join(f.replace("*", " * ").split()) for f in body.split(";") if f.strip()]
    want = []
    for f in fields:
        words = [w for w in f.split() if w != "const"]
        ctype = C.c_void_p if "*" in words else {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32}[words[0]]
        want.append((words[-1], ctype))
    assert L.LsmTableFrames._fields_ == want
    assert [n for n, _ in want] == ["stored_off", "frames", "frame_off", "frame_status", "frames_len", "n_blocks"]


def test_wrappers_take_frames(L):
    for fn in (L.table_get, L.table_range, L.table_range_rows):
        p = inspect.signature(fn).parameters
        assert "frames" in p and p["frames"].default is None, fn.__name__
    p = inspect.signature(L.table_frames).parameters
    assert list(p) == ["file", "table", "block_off", "max_block_bytes", "stream"]
    assert p["max_block_bytes"].default == L.LZ4_MAX_BLOCK
    view = L._frames_struct({"stored_off": None, "frames": None, "frame_off": None, "n_blocks": 3, "frames_len": 99})
    assert (view.n_blocks, view.frames_len, view.frame_status) == (3, 99, None)
