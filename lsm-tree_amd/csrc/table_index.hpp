// table_index.hpp — a table file's blocks and its block index on the device,
// shared by table_get_kernel (table_get.hip) and table_range_kernel
// (table_range.hip): load_block (src/table/util.rs:79-86) and the two seeks of
// index_block::Iter (index_block/iter.rs:25-40).  One lane per query, block
// bytes straight from HBM through the aligned-window readers.  The framed
// kernels (an LZ4 table read through an lsm_table_frames view) take their data
// blocks through load_data_block / load_frame below; table_range_rows.hip
// shares load_frame.
#pragma once

#include "lsmgpu.h"
#include "point_read.hpp"

namespace lsmgpu {

// A block of the file, addressed like every block here: a 16-aligned base,
// the payload at byte p0 of it, plen payload bytes, the parsed trailer.
struct LoadedBlock {
  const uint8_t* base;
  uint32_t p0, plen;
  TrailerInfo t;
};

// load_block (src/table/util.rs:79-86) without the payload checksum (the caller
// verifies regions once): the handle lies in the file, header fields, block
// type, extent, uncompressed, trailer.  index: an index block (restart interval 1).
// The type is tested before the extent, as the reference does (it decodes the
// header, compares the block type and only then reads data_length bytes);
// point_read_kernel and seek_kernel (point_read.hip) are given the extent by
// their caller and test it first (TRUNCATED), then the type (TYPE_MISMATCH).
// The order decides the status of a block with both faults and is pinned by
// tests/test_gpu_lookup_status.py; do not unify the two.
// P: the kernel's parameters, of which file and file_len are read (passed whole, not as two
// values: table_get_kernel then compiles to the code it had with its own load_block).
template <class Params>
__device__ __forceinline__ int32_t load_block(const Params& P, uint64_t off, uint32_t size, uint32_t type,
                                              LoadedBlock& b) {
  if (size < kHdrLen || off + size < off || off + size > P.file_len) return ST_TRUNCATED;  // (handle_in_file)
  b.base = P.file + (off & ~15ULL);
  const uint32_t hb = (uint32_t)(off & 15);
  HeaderInfo h;
  const int32_t st = check_header_fields(b.base, hb, size, h);
  if (st != ST_OK) return st;
  if (h.type != type) return ST_TYPE_MISMATCH;
  if (h.data_length != size - kHdrLen) return ST_TRUNCATED;
  if (read_u32_unaligned(b.base, hb + 25) != h.data_length) return ST_UNSUPPORTED;  // compressed (LZ4 table)
  b.p0 = hb + kHdrLen;
  b.plen = h.data_length;
  const int32_t ts = read_trailer(b.base, b.p0, b.plen, b.t);
  if (ts != ST_OK) return ts;
  if (type == LSM_BLOCK_INDEX && b.t.ri != 1) return ST_PARSE;
  return ST_OK;
}

// An lsm_table_frames view on the device: the table's data blocks as the frames
// lsm_lz4_decompress_framed leaves, a fully populated block cache of one table.
struct FramesView {
  const uint64_t* stored_off;   // [n_blocks + 1] the data-block offsets as stored in the file
  const uint8_t* frames;        // 16-aligned arena
  const uint64_t* frame_off;    // [n_blocks + 1]
  const int32_t* frame_status;  // [n_blocks] or null = every frame OK
  uint64_t frames_len;
  uint32_t n_blocks;
};

// The view of a caller's lsm_table_frames; false = an argument error (a NULL view or
// required array, an arena that is not 16-byte aligned).
inline bool frames_view(const void* frames, FramesView& V) {
  const lsm_table_frames* f = static_cast<const lsm_table_frames*>(frames);
  if (!f || !f->stored_off || !f->frames || !f->frame_off || ((uintptr_t)f->frames & 15)) return false;
  V = FramesView{f->stored_off, f->frames, f->frame_off, f->frame_status, f->frames_len, f->n_blocks};
  return true;
}

// What load_block reads of its Params, over the frame arena.
struct FrameArena {
  const uint8_t* file;
  uint64_t file_len;
};

// The ordinal of the stored handle [off, off + size) in the view: the last
// b < n_blocks with stored_off[b] <= off, which must be exactly that handle
// (block_ordinal's rule in table_range.hip).  At most ceil(log2 n_blocks) steps
// whatever the array holds; an unsorted array fails the two equalities.
__device__ __forceinline__ bool frame_ordinal(const FramesView& V, uint64_t off, uint32_t size, uint32_t& ord) {
  if (V.n_blocks == 0) return false;
  uint32_t lo = 0, hi = V.n_blocks - 1;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (V.stored_off[mid] <= off) lo = mid;
    else hi = mid - 1;
  }
  if (V.stored_off[lo] != off || V.stored_off[lo + 1] != off + size) return false;
  ord = lo;
  return true;
}

// Frame b (b < n_blocks) loaded as a data block, Block::from_file's Err first
// (block/mod.rs:131-182: header, checksum of the stored bytes, decompress, all in
// frame_status), then the frame's extent, then load_block's checks on the frame
// (util.rs:81-86).  f0: the frame's offset in the arena.
__device__ __forceinline__ int32_t load_frame(const FramesView& V, uint32_t b, LoadedBlock& blk, uint64_t& f0) {
  if (V.frame_status) {
    const int32_t fs = V.frame_status[b];
    if (fs != ST_OK) return fs;
  }
  f0 = V.frame_off[b];
  const uint64_t f1 = V.frame_off[b + 1];
  if (f1 < f0 || f1 - f0 < kHdrLen || f1 > V.frames_len) return ST_TRUNCATED;
  const uint64_t size = f1 - f0;
  if (size > 0xFFFFFFFFULL) {  // data_length (u32) cannot equal size - 33: the header's own faults first
    HeaderInfo h;
    const int32_t st = check_header_fields(V.frames + (f0 & ~15ULL), (uint32_t)(f0 & 15), size, h);
    if (st != ST_OK) return st;
    return h.type != LSM_BLOCK_DATA ? ST_TYPE_MISMATCH : ST_TRUNCATED;
  }
  return load_block(FrameArena{V.frames, V.frames_len}, f0, (uint32_t)size, LSM_BLOCK_DATA, blk);
}

// The data block of a handle the index yields.  Plain params: load_block on the
// file.  Framed params (kFramed, with a FramesView `view`): the handle lies in
// the file, its ordinal in the view (else BAD_ARG: not this table's view), then
// load_frame.  ord: the ordinal (framed only).
template <class Params>
__device__ __forceinline__ int32_t load_data_block(const Params& P, uint64_t off, uint32_t size, LoadedBlock& b,
                                                   uint32_t& ord) {
  if constexpr (Params::kFramed) {
    if (size < kHdrLen || off + size < off || off + size > P.file_len) return ST_TRUNCATED;
    if (!frame_ordinal(P.view, off, size, ord)) return ST_BAD_ARG;
    uint64_t f0;
    return load_frame(P.view, ord, b, f0);
  } else {
    return load_block(P, off, size, LSM_BLOCK_DATA, b);
  }
}

// Entry i of an index block (i < item_count = bin_len).
__device__ __forceinline__ bool index_entry(const LoadedBlock& b, uint32_t i, ItemFields& f) {
  Cursor c;
  c.init(b.base, b.p0, bin_get(b.base, b.p0, b.t, i), b.t.rec_end);
  return parse_index_record(c, f);
}

// index_block::Iter::seek: idx = the first entry failing
// end_key < needle || (end_key == needle && seqno >= snap); item_count = none.
__device__ __forceinline__ int32_t index_seek(const LoadedBlock& b, const uint8_t* nb, uint32_t np, uint32_t nn,
                                              uint64_t snap, uint32_t& idx) {
  uint32_t lo = 0, hi = b.t.item_count;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    ItemFields f;
    if (!index_entry(b, mid, f)) return ST_PARSE;
    const int cmp = cmp_span(b.base, b.p0 + f.key_off, f.key_len, nb, np, nn);
    if (cmp < 0 || (cmp == 0 && f.seqno >= snap)) lo = mid + 1;
    else hi = mid;
  }
  idx = lo;
  return ST_OK;
}

// index_block::Iter::seek_upper (index_block/iter.rs:36-40 over
// partition_point_2, block/decoder.rs:210-256): idx = the first entry with
// end_key > needle, clamped to the last entry; it never reports "none".
__device__ __forceinline__ int32_t index_seek_upper(const LoadedBlock& b, const uint8_t* nb, uint32_t np,
                                                    uint32_t nn, uint32_t& idx) {
  uint32_t lo = 0, hi = b.t.item_count;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    ItemFields f;
    if (!index_entry(b, mid, f)) return ST_PARSE;
    if (cmp_span(b.base, b.p0 + f.key_off, f.key_len, nb, np, nn) <= 0) lo = mid + 1;
    else hi = mid;
  }
  idx = min(lo, b.t.item_count - 1);  // (item_count >= 1: read_trailer rejects an empty binary index)
  return ST_OK;
}

}  // namespace lsmgpu
