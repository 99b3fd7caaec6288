// table_range.hip — batched Table::range (src/table/mod.rs:391-422, table
// Iter src/table/iter.rs:94-293) over a table file image in HBM: per query the
// first and the last row that a forward drain (next() only) of the range
// yields, as (block handle, item in block).
//
// The drain, as the reference runs it:
//   1. the index seeks with seqno u64::MAX (iter.rs:196,208).  An index block
//      yields its entries a..=b (Decoder::next, block/decoder.rs:443-447):
//      a = index_block::Iter::seek (index_seek with snap = ~0, 0 without a lower
//      bound; a seek that finds nothing ends the index drain), b =
//      Iter::seek_upper (index_seek_upper, the last entry without an upper
//      bound).  FullBlockIndex: the TLI's span is the handle list H.
//      TwoLevelBlockIndex (block_index/two_level.rs:78-173): the TLI's span
//      names the partitions, each spanned with the same two seeks, H their
//      spans in order; a partition whose lower seek finds nothing ends H;
//   2. every handle of H is loaded (load_block, type Data) and seeked with both
//      bounds (iter.rs:272-277: seek_block, what lsm_seek_blocks computes),
//      giving [first, end); the drain is those ranges in H order.
// Versions of one user key straddle data blocks (the writer cuts by size,
// writer/mod.rs:284-290), so the first block of H may yield nothing while the
// second does, and likewise at the end: the first row is found by walking H
// forwards to the first block with a non-empty range, the last row by walking
// H backwards from its end, down to the first row's block at the latest.
// Blocks strictly between the two are never read.
//
// The backward walk takes a partition whose lower seek finds nothing as an
// empty one and goes on below it; the forward drain would have ended there.
// The two agree on every table whose TLI and partitions agree (a partition in
// the TLI's span then holds an end key >= the lower bound).
//
// One lane per query, 256-thread workgroups, every byte straight from HBM
// through the aligned-window readers, no LDS, no workspace, no host
// synchronisation, no wait between workgroups.  Safety on arbitrary file
// bytes as table_get.hip: every handle is checked against file_len before its
// block is touched, every loop is bounded by an entry count and advances by one.
#include <hip/hip_runtime.h>

#include "host_common.hpp"
#include "lsmgpu.h"
#include "table_index.hpp"

namespace lsmgpu {

struct TableRangeParams {
  static constexpr bool kFramed = false;
  const uint8_t* file;
  uint64_t file_len;
  uint64_t tli_off;
  uint32_t tli_size;
  uint32_t two_level;
  SeekBounds bounds;
  const uint8_t* flags;
  uint32_t n;
  const uint64_t* data_block_off;
  uint32_t n_data_blocks;
  lsm_range_result out;
  uint8_t* outcome;
  int32_t* status;
};

// lsm_table_range_framed: the index from the file, every data block from the view's
// frame of its handle (load_data_block, table_index.hpp), whose ordinal is the block's.
struct TableRangeFramedParams {
  static constexpr bool kFramed = true;
  const uint8_t* file;
  uint64_t file_len;
  uint64_t tli_off;
  uint32_t tli_size;
  uint32_t two_level;
  SeekBounds bounds;
  const uint8_t* flags;
  uint32_t n;
  FramesView view;
  lsm_range_result out;
  uint8_t* outcome;
  int32_t* status;
};

// The span a..=b of one index block under query q's bounds; none = the lower
// seek finds nothing (a and b are then not meaningful).  a > b: no entry.
__device__ __forceinline__ int32_t index_span(const LoadedBlock& blk, const SeekBounds& B, uint32_t q, uint32_t fl,
                                              uint32_t& a, uint32_t& b, bool& none) {
  a = 0;
  b = blk.t.item_count - 1;
  none = false;
  if (fl & LSM_SEEK_LO) {
    const uint64_t o = B.lo_off[q];
    const uint32_t nn = (uint32_t)min(B.lo_off[q + 1] - o, (uint64_t)0xFFFFFFFFu);
    const int32_t st = index_seek(blk, B.lo + (o & ~15ULL), (uint32_t)(o & 15), nn, ~0ULL, a);
    if (st != ST_OK) return st;
    none = a >= blk.t.item_count;
  }
  if (!none && (fl & LSM_SEEK_HI)) {
    const uint64_t o = B.hi_off[q];
    const uint32_t nn = (uint32_t)min(B.hi_off[q + 1] - o, (uint64_t)0xFFFFFFFFu);
    return index_seek_upper(blk, B.hi + (o & ~15ULL), (uint32_t)(o & 15), nn, b);
  }
  return ST_OK;
}

// The data block of index entry e of part: loaded and seeked with both bounds.
// ord: its ordinal in the view (framed only).
template <class Params>
__device__ __forceinline__ int32_t range_in_block(const Params& P, const LoadedBlock& part, uint32_t e, uint32_t q,
                                                  uint32_t fl, uint64_t& off, uint32_t& size, uint32_t& ord,
                                                  uint32_t& first, uint32_t& end) {
  ItemFields ef;
  if (!index_entry(part, e, ef)) return ST_PARSE;
  off = ef.handle_off;
  size = ef.val_len;
  LoadedBlock d;
  const int32_t st = load_data_block(P, off, size, d, ord);
  if (st != ST_OK) return st;
  uint32_t found = 0;
  return seek_block(d.base, d.p0, d.t, P.bounds, q, fl, first, end, found);
}

// Partition pi of a two-level index: loaded and spanned.
template <class Params>
__device__ __forceinline__ int32_t load_partition(const Params& P, const LoadedBlock& tli, uint32_t pi,
                                                  uint32_t q, uint32_t fl, LoadedBlock& part, uint32_t& a,
                                                  uint32_t& b, bool& none) {
  ItemFields pf;
  if (!index_entry(tli, pi, pf)) return ST_PARSE;
  const int32_t st = load_block(P, pf.handle_off, pf.val_len, LSM_BLOCK_INDEX, part);
  if (st != ST_OK) return st;
  return index_span(part, P.bounds, q, fl, a, b, none);
}

// The ordinal of the data block [h_off, h_off + h_size) in the table's offsets.
__device__ __forceinline__ bool block_ordinal(const uint64_t* off, uint32_t n, uint64_t h_off, uint32_t h_size,
                                              uint32_t& ord) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (off[mid] < h_off) lo = mid + 1;
    else hi = mid;
  }
  if (lo >= n || off[lo] != h_off || off[lo + 1] != h_off + h_size) return false;
  ord = lo;
  return true;
}

// The body of both kernels (the plain one compiles to the code it had as a kernel of its own).
template <class Params>
__device__ __forceinline__ void table_range_query(const Params& P) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= P.n) return;
  const uint32_t fl = P.flags[q];

  uint32_t outcome = LSM_RANGE_NO_BLOCK;
  uint64_t f_off = 0, l_off = 0;
  uint32_t f_size = 0, f_first = 0, f_end = 0, l_size = 0, l_item = 0;
  uint32_t f_ord = 0, l_ord = 0;  // (framed: the loads give them; plain: searched at the end)

  // 1. the TLI; the partitions ta..=tb to visit (the TLI itself under a full index)
  LoadedBlock tli;
  int32_t st = load_block(P, P.tli_off, P.tli_size, LSM_BLOCK_INDEX, tli);
  uint32_t ta = 0, tb = 0;
  bool none = false;
  if (st == ST_OK && P.two_level) st = index_span(tli, P.bounds, q, fl, ta, tb, none);

  // 2. the lower walk: H forwards until a block yields a row.  part = partition
  // cur, pa..=pb its span; fe = the first row's entry in it.
  LoadedBlock part = tli;
  uint32_t cur = 0, pa = 0, pb = 0, fe = 0;
  if (st == ST_OK && !none) {
    for (uint32_t pi = ta; pi <= tb; ++pi) {
      cur = pi;
      st = P.two_level ? load_partition(P, tli, pi, q, fl, part, pa, pb, none)
                       : index_span(part, P.bounds, q, fl, pa, pb, none);
      if (st != ST_OK || none) break;  // a lower seek that finds nothing ends the drain
      for (fe = pa; fe <= pb; ++fe) {
        st = range_in_block(P, part, fe, q, fl, f_off, f_size, f_ord, f_first, f_end);
        if (st != ST_OK) break;
        outcome = LSM_RANGE_EMPTY;
        if (f_first < f_end) {
          outcome = LSM_RANGE_ROWS;
          break;
        }
      }
      if (st != ST_OK || outcome == LSM_RANGE_ROWS) break;
    }
  }

  // 3. the upper walk: H backwards from its end until a block yields a row,
  // down to the entry after the first row's; else the last row is in that block.
  if (st == ST_OK && outcome == LSM_RANGE_ROWS) {
    const uint32_t fpi = cur;
    l_off = f_off;
    l_size = f_size;
    l_ord = f_ord;
    l_item = f_end - 1;
    bool got = false;
    for (uint32_t pi = tb;; --pi) {
      if (pi != cur) {  // (two-level only; back at fpi after other partitions the same seeks give pa, pb again)
        cur = pi;
        st = load_partition(P, tli, pi, q, fl, part, pa, pb, none);
        if (st != ST_OK) break;
      }
      const uint32_t stop = pi == fpi ? fe + 1 : pa;
      for (uint32_t e = none ? stop : pb + 1; e > stop;) {
        --e;
        uint64_t off;
        uint32_t size, ord = 0, first, end;
        st = range_in_block(P, part, e, q, fl, off, size, ord, first, end);
        if (st != ST_OK) break;
        if (first < end) {
          l_off = off;
          l_size = size;
          l_ord = ord;
          l_item = end - 1;
          got = true;
          break;
        }
      }
      if (st != ST_OK || got || pi == fpi) break;
    }
  }

  // the two blocks' ordinals in the caller's data-block offsets
  bool ordinals = true;
  if constexpr (!Params::kFramed) {
    ordinals = P.data_block_off != nullptr;
    if (st == ST_OK && outcome == LSM_RANGE_ROWS && ordinals) {
      if (!block_ordinal(P.data_block_off, P.n_data_blocks, f_off, f_size, f_ord) ||
          !block_ordinal(P.data_block_off, P.n_data_blocks, l_off, l_size, l_ord))
        st = ST_BAD_ARG;  // not this table's offsets
    }
  }

  P.status[q] = st;
  P.outcome[q] = (uint8_t)(st == ST_OK ? outcome : LSM_RANGE_NONE);
  if (st == ST_OK && outcome == LSM_RANGE_ROWS) {
    if (P.out.first_block_off) P.out.first_block_off[q] = f_off;
    if (P.out.first_block_size) P.out.first_block_size[q] = f_size;
    P.out.first_item[q] = f_first;
    if (P.out.last_block_off) P.out.last_block_off[q] = l_off;
    if (P.out.last_block_size) P.out.last_block_size[q] = l_size;
    P.out.last_item[q] = l_item;
    if (ordinals) {
      if (P.out.first_block) P.out.first_block[q] = f_ord;
      if (P.out.last_block) P.out.last_block[q] = l_ord;
    }
  }
}

__global__ __launch_bounds__(256) void table_range_kernel(TableRangeParams P) { table_range_query(P); }
__global__ __launch_bounds__(256) void table_range_framed_kernel(TableRangeFramedParams P) { table_range_query(P); }

}  // namespace lsmgpu

extern "C" int lsm_table_range(const uint8_t* d_file, uint64_t file_len, const lsm_table_scan* table,
                               const uint8_t* d_lo, const uint64_t* d_lo_off, const uint8_t* d_hi,
                               const uint64_t* d_hi_off, const uint8_t* d_flags, uint32_t n_queries,
                               const uint64_t* d_data_block_off, uint32_t n_data_blocks,
                               const void* d_out, uint8_t* d_outcome, int32_t* d_status, void* stream) {
  if (n_queries == 0) return LSM_OK;
  const lsm_range_result* out = static_cast<const lsm_range_result*>(d_out);
  if (!d_file || !table || !d_lo || !d_lo_off || !d_hi || !d_hi_off || !d_flags || !out || !out->first_item ||
      !out->last_item || !d_outcome || !d_status)
    return LSM_BAD_ARG;
  // the kernel reads the file and the bounds through aligned 4-byte windows from 16-byte-aligned bases
  if (((uintptr_t)d_file & 15) || ((uintptr_t)d_lo & 15) || ((uintptr_t)d_hi & 15)) return LSM_BAD_ARG;
  if (table->two_level > 1 || !lsmgpu::tli_in_file(*table, file_len)) return LSM_BAD_ARG;
  if ((out->first_block || out->last_block) && !d_data_block_off) return LSM_BAD_ARG;
  lsmgpu::TableRangeParams P{d_file, file_len, table->tli_off, table->tli_size, table->two_level,
                             lsmgpu::SeekBounds{d_lo, d_lo_off, d_hi, d_hi_off}, d_flags, n_queries,
                             d_data_block_off, n_data_blocks, *out, d_outcome, d_status};
  hipLaunchKernelGGL(lsmgpu::table_range_kernel, dim3((n_queries + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     P);
  return lsmgpu::hip_status(hipGetLastError(), "lsm_table_range");
}

extern "C" int lsm_table_range_framed(const uint8_t* d_file, uint64_t file_len, const lsm_table_scan* table,
                                      const uint8_t* d_lo, const uint64_t* d_lo_off, const uint8_t* d_hi,
                                      const uint64_t* d_hi_off, const uint8_t* d_flags, uint32_t n_queries,
                                      const void* frames, const void* d_out, uint8_t* d_outcome, int32_t* d_status,
                                      void* stream) {
  if (n_queries == 0) return LSM_OK;
  const lsm_range_result* out = static_cast<const lsm_range_result*>(d_out);
  if (!d_file || !table || !d_lo || !d_lo_off || !d_hi || !d_hi_off || !d_flags || !out || !out->first_item ||
      !out->last_item || !d_outcome || !d_status)
    return LSM_BAD_ARG;
  if (((uintptr_t)d_file & 15) || ((uintptr_t)d_lo & 15) || ((uintptr_t)d_hi & 15)) return LSM_BAD_ARG;
  if (table->two_level > 1 || !lsmgpu::tli_in_file(*table, file_len)) return LSM_BAD_ARG;
  lsmgpu::FramesView view;
  if (!lsmgpu::frames_view(frames, view)) return LSM_BAD_ARG;
  lsmgpu::TableRangeFramedParams P{d_file, file_len, table->tli_off, table->tli_size, table->two_level,
                                   lsmgpu::SeekBounds{d_lo, d_lo_off, d_hi, d_hi_off}, d_flags, n_queries, view,
                                   *out, d_outcome, d_status};
  hipLaunchKernelGGL(lsmgpu::table_range_framed_kernel, dim3((n_queries + 255) / 256), dim3(256), 0,
                     (hipStream_t)stream, P);
  return lsmgpu::hip_status(hipGetLastError(), "lsm_table_range_framed");
}
