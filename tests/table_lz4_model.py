"""The table models over an LZ4 table: load_block finds a data block by its handle and
Block::from_file verifies and decompresses it (src/table/util.rs:79-86, block/mod.rs:131-182),
which is what the framed readers (lsm_table_get_framed, lsm_table_range_framed,
lsm_table_range_rows_*_framed) do through an lsm_table_frames view.  Built on TableModel,
RangeModel and RowsModel and on the oracle's header_decode, xxh3_128 and lz4_decompress, never
on the library.

A data block's load, in the reference's order:
  1. the handle lies in the file, else TRUNCATED;
  2. header_decode (magic, block type byte, header checksum);
  3. data_length == size - 33, else TRUNCATED;
  4. xxh3_128 of the stored payload == the header's checksum, else CKSUM;
  5. lz4_decompress to uncompressed_length, else DECOMPRESS;
  6. the type test, else TYPE_MISMATCH.
Index blocks, the TLI and the filter block are uncompressed, as the writer leaves them
(index_block_compression_policy: None): TableModel's own load.

lz4_twin builds the LZ4 twin of a pyoracle.table_write result: same items, same block cut, same
index keys, every data block's payload compressed, every handle moved.
"""
import numpy as np

import pyoracle
from lz4_cases import lz4_compress
from table_get_model import DATA, TRUNCATED, TYPE_MISMATCH, TableError, TableModel, index_block
from table_range_model import RangeModel
from table_range_rows_model import RowsModel

CKSUM, DECOMPRESS = 4, 12


class LZ4TableModel(TableModel):
    def _load(self, off, size, want):
        if want != DATA:
            return super()._load(off, size, want)
        if size < 33 or off + size > len(self.file):
            raise TableError(TRUNCATED)
        st, h = pyoracle.header_decode(self.file[off:off + 33])
        if st:
            raise TableError(st)
        if h.data_length != size - 33:
            raise TableError(TRUNCATED)
        stored = self.file[off + 33:off + size]
        if pyoracle.xxh3_128(stored) != (h.cksum_hi << 64 | h.cksum_lo):
            raise TableError(CKSUM)
        payload = pyoracle.lz4_decompress(stored, h.uncompressed_length)
        if payload is None or len(payload) != h.uncompressed_length:
            raise TableError(DECOMPRESS)
        if h.block_type != want:
            raise TableError(TYPE_MISMATCH)
        return payload


class LZ4RangeModel(RangeModel):
    def __init__(self, file, tli_off, tli_size, two_level):
        self.table = LZ4TableModel(file, tli_off, tli_size, two_level)


class LZ4RowsModel(RowsModel):
    """block_off: the stored offsets; block b is the decompressed block of that handle."""

    def __init__(self, file, block_off, global_seqno=0):
        super().__init__(file, block_off, global_seqno)
        self.table = LZ4TableModel(file, 0, 0, False)


BAD_ARG = 10


class View:
    """An lsm_table_frames view on the host: stored_off / frame_off lists, status list or None,
    the frame arena's bytes, frames_len and n_blocks (include/lsmgpu.h)."""

    def __init__(self, stored_off, frames, frame_off, status=None, frames_len=None, n_blocks=None):
        self.stored_off = [int(o) for o in stored_off]
        self.frame_off = [int(o) for o in frame_off]
        self.status = None if status is None else [int(s) for s in status]
        self.frames = bytes(frames)
        self.frames_len = len(self.frames) if frames_len is None else frames_len
        self.n_blocks = len(self.stored_off) - 1 if n_blocks is None else n_blocks

    def frame(self, b):
        """Steps 3 and 4 of the framed load, then the plain load_block on the frame -> payload."""
        if self.status is not None and self.status[b] != 0:
            raise TableError(self.status[b])
        f0, f1 = self.frame_off[b], self.frame_off[b + 1]
        if f1 < f0 or f1 - f0 < 33 or f1 > self.frames_len:
            raise TableError(TRUNCATED)
        return TableModel(self.frames[:self.frames_len], 0, 0, False)._load(f0, f1 - f0, DATA)


class FramesModel(TableModel):
    """Table::get through a view, the five steps of the framed data-block load in their order."""

    def __init__(self, view, *args, **kw):
        super().__init__(*args, **kw)
        self.view = view

    def ordinal(self, off, size):
        v = self.view
        if v.n_blocks == 0:
            raise TableError(BAD_ARG)
        b, hi = 0, v.n_blocks - 1  # the last b with stored_off[b] <= off (0 if none), in log2 steps
        while b < hi:
            mid = b + (hi - b + 1) // 2
            b, hi = (mid, hi) if v.stored_off[mid] <= off else (b, mid - 1)
        if v.stored_off[b] != off or v.stored_off[b + 1] != off + size:
            raise TableError(BAD_ARG)
        return b

    def _load(self, off, size, want):
        if want != DATA:
            return super()._load(off, size, want)
        if size < 33 or off + size > len(self.file):
            raise TableError(TRUNCATED)
        return self.view.frame(self.ordinal(off, size))


class FramesRangeModel(RangeModel):
    def __init__(self, view, file, tli_off, tli_size, two_level):
        self.table = FramesModel(view, file, tli_off, tli_size, two_level)


class FramesRowsModel(RowsModel):
    """lsm_table_range_rows_*_framed: block b is frame b, its status first."""

    def __init__(self, view, global_seqno=0):
        super().__init__(view.frames[:view.frames_len], view.frame_off[:view.n_blocks + 1], global_seqno)
        self.view = view

    def _block(self, b):
        if self.view.status is not None and self.view.status[b] != 0:
            return self.view.status[b], 0, None
        return super()._block(b)


def lz4_block(block, block_type=None):
    """An uncompressed block (Header ‖ payload) as Block::write_into(.., Lz4) stores it."""
    stream = lz4_compress(block[33:])
    return pyoracle.block_header(block[4] if block_type is None else block_type, stream, len(block) - 33) + stream


def lz4_twin(t, two_level):
    """pyoracle.table_write's result -> the same dict for the LZ4 twin, plus handle_map
    ({original (off, size): the twin's}).  Partitions keep their entries, so both index levels
    hold the original (end_key, seqno) pairs over the new handles."""
    src = TableModel(t["file"], t["tli_off"], t["tli_size"], two_level)
    off = [int(o) for o in t["block_off"]]
    blocks = [lz4_block(t["file"][off[b]:off[b + 1]]) for b in range(len(off) - 1)]
    new_off = np.concatenate([[0], np.cumsum([len(b) for b in blocks])]).astype(np.uint64)
    handle_map = {(off[b], off[b + 1] - off[b]): (int(new_off[b]), len(blocks[b])) for b in range(len(blocks))}
    body = b"".join(blocks)
    index_off = len(body)

    def moved(entries):
        return [(k, s) + handle_map[(o, z)] for k, s, o, z in entries]

    tli = src.index_entries(*src.tli)
    if two_level:
        parts = []
        for k, s, o, z in tli:
            blk = index_block(moved(src.index_entries(o, z)))
            parts.append((k, s, len(body), len(blk)))
            body += blk
        top = index_block(parts)
    else:
        top = index_block(moved(tli))
    return dict(t, file=body + top, tli_off=len(body), tli_size=len(top), index_off=index_off, data_len=index_off,
                block_off=new_off, handle_map=handle_map)


def remap_get(expected, handle_map):
    """TableModel.lookup answers on the original -> what the LZ4 model gives on the twin."""
    return [(st, e[:1] + handle_map[e[1:3]] + e[3:] if e[1:3] in handle_map and e[0] == 5 else e)
            for st, e in expected]


def remap_range(expected, handle_map):
    """RangeModel.answer answers on the original -> on the twin (RANGE_ROWS answers move)."""
    return [(st, (e[0],) + handle_map[e[1:3]] + (e[3],) + handle_map[e[4:6]] + (e[6],) if e[0] == 3 else e)
            for st, e in expected]
