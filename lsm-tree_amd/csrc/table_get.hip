// table_get.hip — batched Table::get (src/table/mod.rs:229-340) over a table
// file image in HBM: the step that joins the block-level read kernels.
//
// Per query, in the reference's order:
//   1. snap' = snapshot.saturating_sub(global_seqno); metadata.seqnos.0 >= snap'
//      answers None before anything is read (mod.rs:239-243);
//   2. the table's filter block (Header ‖ standard Bloom image, regions.filter,
//      mod.rs:267-289): contains_hash(key_hash) false answers None;
//   3. BlockIndex::forward_reader(key, snap'): index_block::Iter::seek
//      (index_block/iter.rs:25-34) = Decoder::seek(pred, true) over
//      partition_point_2 (block/decoder.rs:210-304), a binary search over the
//      index block's binary index for the first entry whose (end_key, seqno)
//      fails  end_key < needle || (end_key == needle && seqno >= snap').
//      FullBlockIndex (block_index/full.rs:23-30) seeks the TLI;
//      TwoLevelBlockIndex (block_index/two_level.rs:110-173) seeks the TLI, then
//      every partition from there on, and ends at a partition whose seek
//      finds nothing;
//   4. Table::point_read's loop over the yielded handles (mod.rs:317-340):
//      load_data_block + DataBlock::point_read (point_read.hpp); a miss in a
//      block whose end key is greater than the needle ends the loop.
//
// One lane per query, 256-thread workgroups, every byte straight from HBM
// through the aligned-window readers: the TLI header, its trailer and the
// filter header are the same lines for every lane and stay in cache, the rest
// is a chain of dependent loads (binary-search probes, then one data block).
// No workspace, no host synchronisation, no wait between workgroups.
//
// Safety on arbitrary file bytes: every handle is checked against file_len
// before its block is touched, every offset taken from a trailer or a binary
// index is checked by read_trailer / the Cursor, and every loop is bounded by
// an entry count and advances by one.
#include <hip/hip_runtime.h>

#include "bloom.hpp"
#include "host_common.hpp"
#include "lsmgpu.h"
#include "table_index.hpp"

namespace lsmgpu {

struct TableGetParams {
  static constexpr bool kFramed = false;
  const uint8_t* file;
  uint64_t file_len;
  uint64_t tli_off;
  uint32_t tli_size;
  uint32_t two_level;
  uint64_t global_seqno;
  uint64_t filter_off;
  uint32_t filter_size;
  uint64_t lowest_seqno;
  const uint8_t* needles;
  const uint64_t* needle_off;
  const uint64_t* snapshot;
  const uint64_t* key_hash;
  const uint8_t* active;
  uint32_t n;
  lsm_point_result out;
  uint64_t* hit_off;
  uint32_t* hit_size;
  uint8_t* outcome;
  int32_t* status;
};

// lsm_table_get_framed: the index, the TLI and the filter from the file, every data
// block from the view's frame of its handle (load_data_block, table_index.hpp).
struct TableGetFramedParams : TableGetParams {
  static constexpr bool kFramed = true;
  FramesView view;
  uint32_t* hit_block;
};

// The body of both kernels (the plain one compiles to the code it had as a kernel of its own).
template <class Params>
__device__ __forceinline__ void table_get_query(const Params& P) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= P.n) return;
  if (P.active && !P.active[q]) return;
  const uint64_t no = P.needle_off[q];
  const uint32_t nn = (uint32_t)min(P.needle_off[q + 1] - no, (uint64_t)0xFFFFFFFFu);
  const uint8_t* nb = P.needles + (no & ~15ULL);
  const uint32_t np = (uint32_t)(no & 15);
  const uint64_t s0 = P.snapshot[q];
  const uint64_t snap = s0 > P.global_seqno ? s0 - P.global_seqno : 0;

  int32_t st = ST_OK;
  uint32_t outcome = LSM_GET_NONE;
  int64_t found = -1;
  ItemFields hit{};
  uint64_t hit_off = 0;
  uint32_t hit_size = 0, hit_ord = 0;

  if (P.lowest_seqno >= snap) outcome = LSM_GET_SEQNO_SKIP;

  if (outcome == LSM_GET_NONE && P.filter_size) {  // regions.filter: Header ‖ Bloom image, never compressed
    const uint8_t* fb = P.file + (P.filter_off & ~15ULL);
    const uint32_t hb = (uint32_t)(P.filter_off & 15);
    HeaderInfo h;
    st = check_header_fields(fb, hb, P.filter_size, h);
    if (st == ST_OK && h.type != LSM_BLOCK_FILTER) st = ST_TYPE_MISMATCH;
    if (st == ST_OK && h.data_length != P.filter_size - kHdrLen) st = ST_TRUNCATED;
    if (st == ST_OK) {
      const uint8_t* image = P.file + P.filter_off + kHdrLen;
      uint64_t m = 0, k = 0;
      if (h.data_length < kBloomHdr || !bloom_read_header(image, h.data_length, m, k)) {
        st = ST_BAD_MAGIC;  // Error::InvalidHeader("BloomFilter")
      } else if (k > kBloomMaxK) {
        st = ST_UNSUPPORTED;
      } else {
        const uint64_t hv = P.key_hash ? P.key_hash[q] : xxh3_64_any(nn, BaseReader8{nb, np}, BaseReader64{nb, np});
        if (!bloom_probe(image + kBloomHdr, m, k, hv)) outcome = LSM_GET_FILTERED;
      }
    }
  }

  if (st == ST_OK && outcome == LSM_GET_NONE) {
    LoadedBlock tli;
    st = load_block(P, P.tli_off, P.tli_size, LSM_BLOCK_INDEX, tli);
    // the partitions to visit: the TLI itself (full index), or its entries from the seek on
    uint32_t pi = 0, pend = 1;
    if (st == ST_OK && P.two_level) {
      st = index_seek(tli, nb, np, nn, snap, pi);
      pend = tli.t.item_count;
    }
    bool read_any = false;
    for (; st == ST_OK && outcome == LSM_GET_NONE && pi < pend; ++pi) {
      LoadedBlock part = tli;
      if (P.two_level) {
        ItemFields pf;
        if (!index_entry(tli, pi, pf)) {
          st = ST_PARSE;
          break;
        }
        st = load_block(P, pf.handle_off, pf.val_len, LSM_BLOCK_INDEX, part);
        if (st != ST_OK) break;
      }
      uint32_t e = 0;
      st = index_seek(part, nb, np, nn, snap, e);
      if (st != ST_OK || e >= part.t.item_count) break;  // a seek that finds nothing ends the iteration
      for (; e < part.t.item_count; ++e) {
        ItemFields ef;
        if (!index_entry(part, e, ef)) {
          st = ST_PARSE;
          break;
        }
        LoadedBlock d;
        uint32_t ord = 0;
        st = load_data_block(P, ef.handle_off, ef.val_len, d, ord);
        if (st == ST_OK) st = point_read_block(d.base, d.p0, d.plen, d.t, nb, np, nn, snap, found, hit);
        if (st != ST_OK) break;
        read_any = true;
        if (found >= 0) {
          outcome = LSM_GET_HIT;
          hit_off = ef.handle_off;
          hit_size = ef.val_len;
          hit_ord = ord;
          break;
        }
        // the block's end key is above the needle: no later block can hold it
        if (cmp_span(part.base, part.p0 + ef.key_off, ef.key_len, nb, np, nn) > 0) {
          outcome = LSM_GET_MISS;
          break;
        }
      }
    }
    if (st == ST_OK && outcome == LSM_GET_NONE) outcome = read_any ? LSM_GET_MISS : LSM_GET_NO_BLOCK;
  }

  const bool is_hit = st == ST_OK && outcome == LSM_GET_HIT;
  P.status[q] = st;
  if (P.outcome) P.outcome[q] = (uint8_t)(st == ST_OK ? outcome : LSM_GET_NONE);
  P.out.item[q] = is_hit ? (int32_t)found : -1;
  if (is_hit) {
    if (P.out.seqno) P.out.seqno[q] = hit.seqno + P.global_seqno;
    if (P.out.val_off) P.out.val_off[q] = hit.val_off;
    if (P.out.val_len) P.out.val_len[q] = hit.val_len;
    if (P.out.vtype) P.out.vtype[q] = hit.vtype;
    if (P.hit_off) P.hit_off[q] = hit_off;
    if (P.hit_size) P.hit_size[q] = hit_size;
    if constexpr (Params::kFramed) {
      if (P.hit_block) P.hit_block[q] = hit_ord;
    }
  }
}

__global__ __launch_bounds__(256) void table_get_kernel(TableGetParams P) { table_get_query(P); }
__global__ __launch_bounds__(256) void table_get_framed_kernel(TableGetFramedParams P) { table_get_query(P); }

}  // namespace lsmgpu

// The arguments both entry points share, checked and laid into P.
static int table_get_params(const uint8_t* d_file, uint64_t file_len, const lsm_table_scan* table,
                            uint64_t filter_off, uint32_t filter_size, uint64_t lowest_seqno,
                            const uint8_t* d_needles, const uint64_t* d_needle_off, const uint64_t* d_snapshot,
                            const uint64_t* d_key_hash, const uint8_t* d_active, uint32_t n_queries,
                            const lsm_point_result* d_out, uint64_t* d_hit_block_off, uint32_t* d_hit_block_size,
                            uint8_t* d_outcome, int32_t* d_status, lsmgpu::TableGetParams& P) {
  if (!d_file || !table || !d_needles || !d_needle_off || !d_snapshot || !d_out || !d_out->item || !d_status)
    return LSM_BAD_ARG;
  // the kernel reads the file and the needles through aligned 4-byte windows from 16-byte-aligned bases
  if (((uintptr_t)d_file & 15) || ((uintptr_t)d_needles & 15)) return LSM_BAD_ARG;
  if (table->two_level > 1 || !lsmgpu::tli_in_file(*table, file_len)) return LSM_BAD_ARG;
  if (filter_size && (filter_off + filter_size < filter_off || filter_off + filter_size > file_len)) return LSM_BAD_ARG;
  P = lsmgpu::TableGetParams{d_file, file_len, table->tli_off, table->tli_size, table->two_level,
                             table->global_seqno, filter_off, filter_size, lowest_seqno, d_needles, d_needle_off,
                             d_snapshot, d_key_hash, d_active, n_queries, *d_out, d_hit_block_off, d_hit_block_size,
                             d_outcome, d_status};
  return LSM_OK;
}

extern "C" int lsm_table_get(const uint8_t* d_file, uint64_t file_len, const lsm_table_scan* table,
                             uint64_t filter_off, uint32_t filter_size, uint64_t lowest_seqno,
                             const uint8_t* d_needles, const uint64_t* d_needle_off, const uint64_t* d_snapshot,
                             const uint64_t* d_key_hash, const uint8_t* d_active, uint32_t n_queries,
                             const lsm_point_result* d_out, uint64_t* d_hit_block_off, uint32_t* d_hit_block_size,
                             uint8_t* d_outcome, int32_t* d_status, void* stream) {
  if (n_queries == 0) return LSM_OK;
  lsmgpu::TableGetParams P;
  const int rc = table_get_params(d_file, file_len, table, filter_off, filter_size, lowest_seqno, d_needles,
                                  d_needle_off, d_snapshot, d_key_hash, d_active, n_queries, d_out, d_hit_block_off,
                                  d_hit_block_size, d_outcome, d_status, P);
  if (rc != LSM_OK) return rc;
  hipLaunchKernelGGL(lsmgpu::table_get_kernel, dim3((n_queries + 255) / 256), dim3(256), 0, (hipStream_t)stream, P);
  return lsmgpu::hip_status(hipGetLastError(), "lsm_table_get");
}

extern "C" int lsm_table_get_framed(const uint8_t* d_file, uint64_t file_len, const lsm_table_scan* table,
                                    uint64_t filter_off, uint32_t filter_size, uint64_t lowest_seqno,
                                    const uint8_t* d_needles, const uint64_t* d_needle_off,
                                    const uint64_t* d_snapshot, const uint64_t* d_key_hash, const uint8_t* d_active,
                                    uint32_t n_queries, const lsm_point_result* d_out, uint64_t* d_hit_block_off,
                                    uint32_t* d_hit_block_size, uint8_t* d_outcome, int32_t* d_status,
                                    const void* frames, uint32_t* d_hit_block, void* stream) {
  if (n_queries == 0) return LSM_OK;
  lsmgpu::TableGetFramedParams P;
  const int rc = table_get_params(d_file, file_len, table, filter_off, filter_size, lowest_seqno, d_needles,
                                  d_needle_off, d_snapshot, d_key_hash, d_active, n_queries, d_out, d_hit_block_off,
                                  d_hit_block_size, d_outcome, d_status, P);
  if (rc != LSM_OK) return rc;
  if (!lsmgpu::frames_view(frames, P.view)) return LSM_BAD_ARG;
  P.hit_block = d_hit_block;
  hipLaunchKernelGGL(lsmgpu::table_get_framed_kernel, dim3((n_queries + 255) / 256), dim3(256), 0,
                     (hipStream_t)stream, P);
  return lsmgpu::hip_status(hipGetLastError(), "lsm_table_get_framed");
}
