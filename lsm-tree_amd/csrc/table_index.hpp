// table_index.hpp — a table file's blocks and its block index on the device,
// shared by table_get_kernel (table_get.hip) and table_range_kernel
// (table_range.hip): load_block (src/table/util.rs:79-86) and the two seeks of
// index_block::Iter (index_block/iter.rs:25-40).  One lane per query, block
// bytes straight from HBM through the aligned-window readers.
#pragma once

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
