// table_range_rows.hip — the rows of batched Table::range (src/table/mod.rs:391-422,
// table Iter src/table/iter.rs:94-293, the owned InternalValue of iter.rs:272-290)
// as item runs: the positions lsm_table_range reports (first and last row of each
// query's forward drain as (block ordinal, item)) are turned into the rows between
// them, in the lsm_items shape lsm_merge_runs takes, reading only the data blocks
// first_block ..= last_block of each query.
//
// A (query, block) pair is the unit of work; a group of kRrGroup lanes takes one
// pair, its lanes the block's restart intervals, kRrGroup at a time.
// The plan call:
//   1. rr_pairs_kernel    lane per query: the position checks and the pair count;
//                         an exclusive scan (scan.hpp) gives pair_start[n + 1]
//   2. rr_measure_kernel  group per pair: load_block, read_trailer, the edge-item
//                         check; every restart interval is walked from its
//                         binary-index offset to the next one's (the whole block
//                         must parse, wherever the window lies); rows, key bytes
//                         and value bytes of the rows inside the window; a fault
//                         goes into the query's fault word by atomicMin of
//                         (block ordinal, status)
//   3. rr_fold_kernel     lane per pair: the triples of faulted queries (and past
//                         the pair count) are zeroed, d_row_status of faulted queries;
//                         three exclusive scans over the pairs;
//      rr_finish_kernel   d_run_start, d_end, d_need, *d_result
// The rows call:
//   4. rr_rows_kernel     group per pair of a non-faulted query: the intervals
//                         that intersect the window are walked again (counted,
//                         scanned over the group, then written): output offsets,
//                         seqno + global_seqno, vtype, and a row descriptor in
//                         the workspace
//   5. rr_gather_kernel   wave per 64 consecutive output rows, whatever pairs they
//                         lie in: the tile body of items_gather.hpp over the
//                         descriptors.
// Every byte comes straight from HBM through the aligned-window readers; no host
// synchronisation, no wait between workgroups.  Safety on arbitrary bytes: a
// block's handle is checked against file_len before the block is touched, every
// loop is bounded by a count read once and advances by one, every record range is
// checked against the block's record area by the parser, and every store of the
// rows call is bounded by the plan's row counts.
#include <hip/hip_runtime.h>

#include "host_common.hpp"
#include "items_gather.hpp"
#include "lsmgpu.h"
#include "scan.hpp"
#include "table_index.hpp"

// Lanes per (query, block) pair: 16 (four pairs per wave) or 64.  A 4 KiB block at
// restart interval 16 has three or four intervals; DESIGN 6.11 has the measurement.
#ifndef LSM_RR_GROUP
#define LSM_RR_GROUP 16
#endif

namespace lsmgpu {

constexpr uint32_t kRrGroup = LSM_RR_GROUP;
constexpr uint32_t kRrThreads = 256;
constexpr uint32_t kRrGroupsPerWg = kRrThreads / kRrGroup;
static_assert(kRrGroup == 16 || kRrGroup == 32 || kRrGroup == 64, "group width");
constexpr uint64_t kRrNoFault = ~0ULL;

// What the gather needs of one output row: the payload's file offset and the
// row's three ranges in it.
struct RrDesc {
  uint64_t payload;
  uint32_t head, key, val, vlen;  // payload-relative: head key, key suffix, value
  uint16_t pl, kl;
  uint32_t pad;
};
static_assert(sizeof(RrDesc) == 32, "descriptor size");

// meta: the cursor the plan started at, the totals, and whether the plan overflowed
enum { kRrBase = 0, kRrRows = 3, kRrPairs = 4, kRrOverflow = 5, kRrMeta = 8 };

struct RrParams {
  static constexpr bool kFramed = false;
  const uint8_t* file;
  uint64_t file_len;
  uint64_t global_seqno;
  const uint64_t* off;
  uint32_t n_blocks;
  lsm_range_positions pos;
  uint32_t n;
  uint64_t block_cap, row_cap;
  const uint64_t* base;  // u64[3] or null = zeros
  uint64_t* end;
  // plan outputs
  uint64_t* run_start;
  uint64_t* need;
  int32_t* row_status;
  int32_t* result;
  // workspace
  uint64_t* meta;        // [kRrMeta]
  uint32_t* qpairs;      // [n] pairs of each query
  uint64_t* pair_start;  // [n + 1]
  uint64_t* fault;       // [n] (block ordinal << 8 | status) of the lowest faulted block, kRrNoFault
  uint64_t* prow;        // [block_cap] each: rows, key bytes, value bytes of a pair
  uint64_t* pkey;
  uint64_t* pval;
  uint64_t* srow;  // [block_cap + 1] each: their exclusive scans
  uint64_t* skey;
  uint64_t* sval;
  uint64_t* tiles;  // scan tile sums
  RrDesc* desc;     // [row_cap]
  // rows call outputs
  uint64_t* out_key_off;
  uint64_t* out_val_off;
  uint8_t* out_keys;
  uint8_t* out_vals;
  uint64_t* out_seqno;
  uint8_t* out_vtype;
  uint64_t item_cap, key_cap, val_cap;
};

// The framed calls: file / file_len / off are the view's frame arena, its length and
// frame_off, so block b is frame b and the kernels that load no block (pairs, fold,
// finish, gather) are the plain ones; the two that do take the frames' statuses too.
struct RrFramedParams : RrParams {
  static constexpr bool kFramed = true;
  const int32_t* frame_status;  // [n_blocks] or null
};

// ---------------------------------------------------------------- group helpers
__device__ __forceinline__ uint64_t rr_shfl_xor(uint64_t v, int m) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, (int)kRrGroup);
  const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, (int)kRrGroup);
  return (uint64_t)lo | ((uint64_t)hi << 32);
}
__device__ __forceinline__ uint64_t rr_shfl_up(uint64_t v, int d) {
  const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d, (int)kRrGroup);
  const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d, (int)kRrGroup);
  return (uint64_t)lo | ((uint64_t)hi << 32);
}
__device__ __forceinline__ uint64_t rr_shfl(uint64_t v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, (int)kRrGroup);
  const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, (int)kRrGroup);
  return (uint64_t)lo | ((uint64_t)hi << 32);
}
// Sum over the group, in every lane of it.
__device__ __forceinline__ uint64_t rr_group_sum(uint64_t v) {
#pragma unroll
  for (int m = kRrGroup / 2; m >= 1; m >>= 1) v += rr_shfl_xor(v, m);
  return v;
}
// Inclusive scan over the group (gl = the lane's index in it).
__device__ __forceinline__ uint64_t rr_group_incl_scan(uint64_t v, uint32_t gl) {
#pragma unroll
  for (int d = 1; d < (int)kRrGroup; d <<= 1) {
    const uint64_t t = rr_shfl_up(v, d);
    if (gl >= (uint32_t)d) v += t;
  }
  return v;
}

// The query of pair p: the last q with pair_start[q] <= p (p < pair_start[n], so
// that query has a pair).
__device__ __forceinline__ uint32_t rr_pair_query(const uint64_t* pair_start, uint32_t n, uint64_t p) {
  uint32_t lo = 0, hi = n - 1;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (pair_start[mid] <= p) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// One pair: its query, its block and the window's edges in that block.
struct RrPair {
  uint32_t q, b;
  bool first, last;   // the block is the query's first / last
  uint32_t fi, li;    // first_item / last_item (meaningful with first / last)
};
__device__ __forceinline__ RrPair rr_pair(const RrParams& P, uint64_t p) {
  RrPair x;
  x.q = rr_pair_query(P.pair_start, P.n, p);
  const uint32_t fb = P.pos.first_block[x.q], lb = P.pos.last_block[x.q];
  x.b = fb + (uint32_t)(p - P.pair_start[x.q]);
  x.first = x.b == fb;
  x.last = x.b == lb;
  x.fi = P.pos.first_item[x.q];
  x.li = P.pos.last_item[x.q];
  return x;
}
__device__ __forceinline__ bool rr_in_window(const RrPair& x, uint32_t k) {
  return !(x.first && k < x.fi) && !(x.last && k > x.li);
}

// Block b of the offsets, loaded as a data block: the handle test (a handle
// shorter than a header, one that decreases, one ending past the file), then
// load_block's checks in its order.  Framed: the frame's status before them
// (load_frame, table_index.hpp); one that the fault word's byte cannot carry
// (not a status of this library) counts as LSM_BAD_ARG.
template <class Params>
__device__ __forceinline__ int32_t rr_load(const Params& P, uint32_t b, LoadedBlock& blk, uint64_t& o0) {
  if constexpr (Params::kFramed) {
    const int32_t st =
        load_frame(FramesView{nullptr, P.file, P.off, P.frame_status, P.file_len, P.n_blocks}, b, blk, o0);
    return st < 0 || st > 0xFF ? (int32_t)ST_BAD_ARG : st;
  }
  o0 = P.off[b];
  const uint64_t o1 = P.off[b + 1];
  if (o1 < o0 || o1 - o0 < kHdrLen || o1 > P.file_len) return ST_TRUNCATED;
  const uint64_t size = o1 - o0;
  if (size > 0xFFFFFFFFULL) {  // data_length (u32) cannot equal size - 33: the header's own faults first
    HeaderInfo h;
    const int32_t st = check_header_fields(P.file + (o0 & ~15ULL), (uint32_t)(o0 & 15), size, h);
    if (st != ST_OK) return st;
    return h.type != LSM_BLOCK_DATA ? ST_TYPE_MISMATCH : ST_TRUNCATED;
  }
  return load_block(P, o0, (uint32_t)size, LSM_BLOCK_DATA, blk);
}

// The edge-item check of a loaded block.
__device__ __forceinline__ int32_t rr_edges(const RrPair& x, const TrailerInfo& t) {
  if (x.first && x.fi >= t.item_count) return ST_BAD_ARG;
  if (x.last && x.li >= t.item_count) return ST_BAD_ARG;
  if (x.first && x.last && x.fi > x.li) return ST_BAD_ARG;
  return ST_OK;
}

// Walks restart interval iv of a loaded block as oracle/block.c:359-396 requires
// it: it starts where the binary index says (interval 0 at byte 0), holds ri
// records (the remainder in the last interval), each parsed against the record
// area, and ends exactly where the next interval starts (at the marker for the
// last).  each(k, f, head): item k of the block, its fields, its restart head's
// key offset.  false = the block does not parse.
template <class Each>
__device__ __forceinline__ bool rr_walk(const LoadedBlock& blk, uint32_t iv, Each&& each) {
  const TrailerInfo& t = blk.t;
  uint32_t pos = bin_get(blk.base, blk.p0, t, iv);
  const uint32_t stop = iv + 1 < t.bin_len ? bin_get(blk.base, blk.p0, t, iv + 1) : t.rec_end;
  if ((iv == 0 && pos != 0) || pos > stop || stop > t.rec_end) return false;
  const uint32_t k0 = iv * t.ri;
  const uint32_t cnt = min(t.ri, t.item_count - k0);
  uint32_t head = 0;
  for (uint32_t j = 0; j < cnt; ++j) {
    ItemFields f;
    uint32_t next;
    const int rc = parse_data_fast(blk.base, blk.p0, pos, t.rec_end, j == 0, head, f, next);
    if (rc < 0) return false;
    if (rc == 0) {
      Cursor c;
      c.init(blk.base, blk.p0, pos, t.rec_end);
      if (!parse_data_record(c, j == 0, head, f)) return false;
      next = c.pos;
    }
    if (j == 0) head = f.key_off;
    each(k0 + j, f, head);
    pos = next;
  }
  return pos == stop;
}

// ---------------------------------------------------------------- plan
__global__ __launch_bounds__(256) void rr_pairs_kernel(RrParams P) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= P.n) return;
  const int32_t st_in = P.pos.status[q];
  int32_t st = st_in;
  uint32_t pairs = 0;
  if (st_in == LSM_OK && P.pos.outcome[q] == LSM_RANGE_ROWS) {
    const uint32_t fb = P.pos.first_block[q], lb = P.pos.last_block[q];
    if (fb > lb || lb >= P.n_blocks) st = ST_BAD_ARG;
    else pairs = lb - fb + 1;
  }
  P.qpairs[q] = pairs;
  P.fault[q] = kRrNoFault;
  P.row_status[q] = st;
}

struct RrPrefixOut {
  uint64_t* dst;
  __device__ void operator()(uint64_t i, uint64_t prefix) const { dst[i] = prefix; }
};

// The bodies of rr_measure_kernel / rr_rows_kernel and of their framed twins (the
// plain ones compile to the code they had as kernels of their own).
template <class Params>
__device__ __forceinline__ void rr_measure(const Params& P) {
  const uint32_t gl = threadIdx.x & (kRrGroup - 1);
  const uint64_t p = (uint64_t)blockIdx.x * kRrGroupsPerWg + threadIdx.x / kRrGroup;
  const uint64_t np = P.pair_start[P.n];
  if (np > P.block_cap || p >= np) return;  // (group-uniform)
  const RrPair x = rr_pair(P, p);
  LoadedBlock blk;
  uint64_t o0;
  int32_t st = rr_load(P, x.b, blk, o0);
  if (st == ST_OK) st = rr_edges(x, blk.t);
  uint64_t rows = 0, kb = 0, vb = 0;
  if (st == ST_OK) {
    bool ok = true;
    for (uint32_t iv0 = 0; iv0 < blk.t.bin_len; iv0 += kRrGroup) {
      const uint32_t iv = iv0 + gl;
      if (iv < blk.t.bin_len)
        ok &= rr_walk(blk, iv, [&](uint32_t k, const ItemFields& f, uint32_t) {
          if (rr_in_window(x, k)) {
            rows += 1;
            kb += (uint32_t)f.prefix_len + f.key_len;
            vb += f.val_len;
          }
        });
    }
    if (rr_group_sum(ok ? 0 : 1)) st = ST_PARSE;
  }
  rows = rr_group_sum(rows);
  kb = rr_group_sum(kb);
  vb = rr_group_sum(vb);
  if (gl == 0) {
    P.prow[p] = st == ST_OK ? rows : 0;
    P.pkey[p] = st == ST_OK ? kb : 0;
    P.pval[p] = st == ST_OK ? vb : 0;
    if (st != ST_OK) atomicMin((unsigned long long*)&P.fault[x.q], ((unsigned long long)x.b << 8) | (uint32_t)st);
  }
}

__global__ __launch_bounds__(kRrThreads) void rr_measure_kernel(RrParams P) { rr_measure(P); }
__global__ __launch_bounds__(kRrThreads) void rr_measure_framed_kernel(RrFramedParams P) { rr_measure(P); }

__global__ __launch_bounds__(256) void rr_fold_kernel(RrParams P) {
  const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P.block_cap) return;
  const uint64_t np = P.pair_start[P.n];
  bool zero = np > P.block_cap || p >= np;
  if (!zero) {
    const uint32_t q = rr_pair_query(P.pair_start, P.n, p);
    const uint64_t f = P.fault[q];
    if (f != kRrNoFault) {
      zero = true;
      if (p == P.pair_start[q]) P.row_status[q] = (int32_t)(f & 0xFF);
    }
  }
  if (zero) P.prow[p] = P.pkey[p] = P.pval[p] = 0;
}

// empty: no query (nothing else of the plan ran).
__global__ __launch_bounds__(256) void rr_finish_kernel(RrParams P, bool empty) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > P.n) return;
  const uint64_t b0 = P.base ? P.base[0] : 0, b1 = P.base ? P.base[1] : 0, b2 = P.base ? P.base[2] : 0;
  const uint64_t np = empty ? 0 : P.pair_start[P.n];
  const bool pairs_over = np > P.block_cap;
  const bool none = empty || pairs_over || P.block_cap == 0;  // (no pair was measured: no scan entry to read)
  if (P.run_start) P.run_start[i] = b0 + (none ? 0 : P.srow[P.pair_start[i]]);
  if (i != P.n) return;
  const uint64_t rows = none ? 0 : P.srow[P.block_cap], kb = none ? 0 : P.skey[P.block_cap],
                 vb = none ? 0 : P.sval[P.block_cap];
  const bool over = pairs_over || rows > P.row_cap;
  P.end[0] = b0 + rows;
  P.end[1] = b1 + kb;
  P.end[2] = b2 + vb;
  if (P.need) {
    P.need[0] = np;
    P.need[1] = rows;
    P.need[2] = kb;
    P.need[3] = vb;
  }
  *P.result = over ? LSM_OVERFLOW : LSM_OK;
  if (!empty) {
    P.meta[kRrBase + 0] = b0;
    P.meta[kRrBase + 1] = b1;
    P.meta[kRrBase + 2] = b2;
    P.meta[kRrRows] = rows;
    P.meta[kRrPairs] = np;
    P.meta[kRrOverflow] = over;
  }
}

// ---------------------------------------------------------------- rows
// All rows or none: the plan did not overflow (nor does it under this call's
// row_cap) and its cursor fits the outputs.
__device__ __forceinline__ bool rr_fits(const RrParams& P) {
  return !P.meta[kRrOverflow] && P.meta[kRrRows] <= P.row_cap && P.end[0] <= P.item_cap &&
         P.end[1] <= P.key_cap && P.end[2] <= P.val_cap && P.meta[kRrBase + 0] + P.meta[kRrRows] == P.end[0];
}

template <class Params>
__device__ __forceinline__ void rr_rows(const Params& P) {
  const uint32_t gl = threadIdx.x & (kRrGroup - 1);
  const uint64_t p = (uint64_t)blockIdx.x * kRrGroupsPerWg + threadIdx.x / kRrGroup;
  const bool fits = rr_fits(P);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *P.result = fits ? LSM_OK : LSM_OVERFLOW;
    if (fits) {  // the entry after the last row
      P.out_key_off[P.end[0]] = P.end[1];
      P.out_val_off[P.end[0]] = P.end[2];
    }
  }
  if (!fits || p >= P.meta[kRrPairs]) return;  // (group-uniform)
  const RrPair x = rr_pair(P, p);
  if (P.fault[x.q] != kRrNoFault) return;
  LoadedBlock blk;
  uint64_t o0;
  if (rr_load(P, x.b, blk, o0) != ST_OK || rr_edges(x, blk.t) != ST_OK) return;  // (not the plan's file)
  const uint64_t b0 = P.meta[kRrBase + 0], b1 = P.meta[kRrBase + 1], b2 = P.meta[kRrBase + 2];
  const uint64_t row_limit = b0 + P.srow[p + 1];  // this pair's rows end here, whatever the walk finds
  uint64_t r0 = b0 + P.srow[p], k0 = b1 + P.skey[p], v0 = b2 + P.sval[p];
  const uint32_t iv_lo = x.first ? x.fi / blk.t.ri : 0;
  const uint32_t iv_hi = x.last ? x.li / blk.t.ri : blk.t.bin_len - 1;
  const uint64_t payload = o0 + kHdrLen;
  for (uint32_t iv0 = iv_lo; iv0 <= iv_hi && iv0 >= iv_lo; iv0 += kRrGroup) {
    const uint32_t iv = iv0 + gl;
    const bool mine = iv >= iv0 && iv <= iv_hi;
    uint64_t rows = 0, kb = 0, vb = 0;
    if (mine)
      rr_walk(blk, iv, [&](uint32_t k, const ItemFields& f, uint32_t) {
        if (rr_in_window(x, k)) {
          rows += 1;
          kb += (uint32_t)f.prefix_len + f.key_len;
          vb += f.val_len;
        }
      });
    const uint64_t ri = rr_group_incl_scan(rows, gl), ki = rr_group_incl_scan(kb, gl),
                   vi = rr_group_incl_scan(vb, gl);
    uint64_t r = r0 + ri - rows, ko = k0 + ki - kb, vo = v0 + vi - vb;
    if (mine)
      rr_walk(blk, iv, [&](uint32_t k, const ItemFields& f, uint32_t head) {
        if (!rr_in_window(x, k) || r >= row_limit || r - b0 >= P.row_cap) return;
        gstore(P.out_key_off, r, ko);
        gstore(P.out_val_off, r, vo);
        gstore(P.out_seqno, r, f.seqno + P.global_seqno);
        gstore(P.out_vtype, r, f.vtype);
        RrDesc d;
        d.payload = payload;
        d.head = head;
        d.key = f.key_off;
        d.val = f.val_off;
        d.vlen = f.val_len;
        d.pl = f.prefix_len;
        d.kl = f.key_len;
        d.pad = 0;
        P.desc[r - b0] = d;
        r += 1;
        ko += (uint32_t)f.prefix_len + f.key_len;
        vo += f.val_len;
      });
    r0 += rr_shfl(ri, kRrGroup - 1);
    k0 += rr_shfl(ki, kRrGroup - 1);
    v0 += rr_shfl(vi, kRrGroup - 1);
  }
}

__global__ __launch_bounds__(kRrThreads) void rr_rows_kernel(RrParams P) { rr_rows(P); }
__global__ __launch_bounds__(kRrThreads) void rr_rows_framed_kernel(RrFramedParams P) { rr_rows(P); }

// The gather's row source: the descriptors of the rows pass (items_gather.hpp).
// A descriptor that does not lie in the file names no bytes (the rows pass
// writes none: the workspace was not left alone).
struct RrDescRows {
  static constexpr bool kMeta = false;  // (seqno and vtype are the rows pass's)
  const RrParams& P;
  __device__ __forceinline__ void locate(uint64_t, uint64_t, uint64_t) {}
  __device__ __forceinline__ MiRow row(uint64_t i) const {
    const RrDesc d = gload_pod(P.desc, i);
    const uint64_t top = max(max((uint64_t)d.head + d.pl, (uint64_t)d.key + d.kl), (uint64_t)d.val + d.vlen);
    if (d.payload > P.file_len || top > P.file_len - d.payload) return MiRow{P.file, P.file, P.file, 0, 0, 0, false};
    const uint8_t* pay = P.file + d.payload;
    return MiRow{pay + d.head, pay + d.key, pay + d.val, d.pl, d.kl, d.vlen, true};
  }
  __device__ __forceinline__ uint64_t seqno(uint64_t) const { return 0; }
  __device__ __forceinline__ uint8_t vtype(uint64_t) const { return 0; }
};

__global__ __launch_bounds__(kMiWaves * 64) void rr_gather_kernel(RrParams P) {
  __shared__ __attribute__((aligned(16))) uint8_t buf[kMiWaves][kMiBuf + 32];
  if (!rr_fits(P)) return;  // (rr_rows_kernel has reported it)
  RrDescRows S{P};
  const ItemsOut O{P.meta + kRrBase, P.end,      P.out_key_off, P.out_val_off, P.item_cap,  P.key_cap,
                   P.val_cap,        P.out_keys, P.out_vals,    P.out_seqno,   P.out_vtype, P.result};
  items_gather_tile(S, O, min(P.meta[kRrRows], P.row_cap), P.file, buf);
}

// The workspace: byte offsets of its regions, in layout order, and their sum.
struct RrWorkspace {
  size_t meta, qpairs, pair_start, fault, prow, pkey, pval, srow, skey, sval, tiles, desc, total;
  RrWorkspace(uint32_t n_queries, uint64_t block_cap, uint64_t row_cap) {
    const uint64_t n = n_queries ? n_queries : 1, bc = block_cap ? block_cap : 1, rc = row_cap ? row_cap : 1;
    Carver c;
    meta = c.take(kRrMeta * 8);
    qpairs = c.take(n * 4);
    pair_start = c.take((n + 1) * 8);
    fault = c.take(n * 8);
    prow = c.take(bc * 8);
    pkey = c.take(bc * 8);
    pval = c.take(bc * 8);
    srow = c.take((bc + 1) * 8);
    skey = c.take((bc + 1) * 8);
    sval = c.take((bc + 1) * 8);
    tiles = c.take(scan_tiles(n > bc ? n : bc) * 8);
    desc = c.take(rc * sizeof(RrDesc));
    total = c.total();
  }
};

// The caps size grids: 32 bits of pairs and of rows are more than a table image holds.
constexpr uint64_t kRrMaxCap = 0xFFFFFFFEULL;

}  // namespace lsmgpu

using namespace lsmgpu;

extern "C" size_t lsm_table_range_rows_workspace_size(uint32_t n_queries, uint64_t block_cap, uint64_t row_cap) {
  return RrWorkspace(n_queries, block_cap, row_cap).total;
}

// The arguments both calls share, checked and carved into P.
static int rr_params(const uint8_t* d_file, uint64_t file_len, const lsm_table_scan* table,
                     const uint64_t* d_data_block_off, uint32_t n_data_blocks, const void* pos, uint32_t n_queries,
                     uint64_t block_cap, uint64_t row_cap, const uint64_t* d_base, const uint64_t* d_end,
                     void* d_workspace, size_t workspace_bytes, RrParams& P) {
  const lsm_range_positions* ps = static_cast<const lsm_range_positions*>(pos);
  if (!d_file || !table || !d_data_block_off || !ps || !ps->outcome || !ps->status || !ps->first_block ||
      !ps->first_item || !ps->last_block || !ps->last_item || !d_end || d_end == d_base)
    return LSM_BAD_ARG;
  if ((uintptr_t)d_file & 15) return LSM_BAD_ARG;  // (the readers take 16-byte-aligned bases)
  if (block_cap > kRrMaxCap || row_cap > kRrMaxCap) return LSM_BAD_ARG;
  const RrWorkspace W(n_queries, block_cap, row_cap);
  if (!d_workspace || workspace_bytes < W.total) return LSM_BAD_ARG;
  uint8_t* ws = (uint8_t*)d_workspace;
  P = RrParams{};
  P.file = d_file;
  P.file_len = file_len;
  P.global_seqno = table->global_seqno;
  P.off = d_data_block_off;
  P.n_blocks = n_data_blocks;
  P.pos = *ps;
  P.n = n_queries;
  P.block_cap = block_cap;
  P.row_cap = row_cap;
  P.base = d_base;
  P.end = const_cast<uint64_t*>(d_end);
  P.meta = (uint64_t*)(ws + W.meta);
  P.qpairs = (uint32_t*)(ws + W.qpairs);
  P.pair_start = (uint64_t*)(ws + W.pair_start);
  P.fault = (uint64_t*)(ws + W.fault);
  P.prow = (uint64_t*)(ws + W.prow);
  P.pkey = (uint64_t*)(ws + W.pkey);
  P.pval = (uint64_t*)(ws + W.pval);
  P.srow = (uint64_t*)(ws + W.srow);
  P.skey = (uint64_t*)(ws + W.skey);
  P.sval = (uint64_t*)(ws + W.sval);
  P.tiles = (uint64_t*)(ws + W.tiles);
  P.desc = (RrDesc*)(ws + W.desc);
  return LSM_OK;
}

static uint32_t rr_grid(uint64_t n, uint32_t per_wg) { return (uint32_t)((n + per_wg - 1) / per_wg); }

// The view's arrays in the places of the file and the offsets (RrFramedParams).
static int rr_framed_params(const lsm_table_scan* table, const void* frames, const void* pos, uint32_t n_queries,
                            uint64_t block_cap, uint64_t row_cap, const uint64_t* d_base, const uint64_t* d_end,
                            void* d_workspace, size_t workspace_bytes, RrFramedParams& P) {
  FramesView V;
  if (!frames_view(frames, V)) return LSM_BAD_ARG;
  const int rc = rr_params(V.frames, V.frames_len, table, V.frame_off, V.n_blocks, pos, n_queries, block_cap,
                           row_cap, d_base, d_end, d_workspace, workspace_bytes, P);
  P.frame_status = V.frame_status;
  return rc;
}

// n_queries == 0: the cursor does not move.
static int rr_plan_empty(const uint64_t* d_base, uint64_t* d_run_start, uint64_t* d_end, uint64_t* d_need,
                         int32_t* d_result, hipStream_t st, const char* what) {
  if (!d_end || !d_result || d_end == d_base) return LSM_BAD_ARG;
  RrParams P{};
  P.base = d_base;
  P.end = d_end;
  P.run_start = d_run_start;
  P.need = d_need;
  P.result = d_result;
  hipLaunchKernelGGL(rr_finish_kernel, dim3(1), dim3(256), 0, st, P, true);
  return hip_status(hipGetLastError(), what);
}

// The plan's launches over checked params (RrParams or RrFramedParams).
template <class Params>
static int rr_plan(Params& P, uint32_t n_queries, uint64_t block_cap, uint64_t* d_run_start, uint64_t* d_need,
                   int32_t* d_row_status, int32_t* d_result, hipStream_t st, const char* what) {
  if (!d_run_start || !d_need || !d_row_status || !d_result) return LSM_BAD_ARG;
  P.run_start = d_run_start;
  P.need = d_need;
  P.row_status = d_row_status;
  P.result = d_result;
  const RrParams& base = P;
  hipLaunchKernelGGL(rr_pairs_kernel, dim3(rr_grid(n_queries, 256)), dim3(256), 0, st, base);
  hipError_t e = launch_excl_scan(P.qpairs, (uint64_t)n_queries, P.tiles, RrPrefixOut{P.pair_start}, st);
  if (e != hipSuccess) return hip_status(e, what);
  if (block_cap) {
    const dim3 grid(rr_grid(block_cap, kRrGroupsPerWg));
    if constexpr (Params::kFramed) hipLaunchKernelGGL(rr_measure_framed_kernel, grid, dim3(kRrThreads), 0, st, P);
    else hipLaunchKernelGGL(rr_measure_kernel, grid, dim3(kRrThreads), 0, st, P);
    hipLaunchKernelGGL(rr_fold_kernel, dim3(rr_grid(block_cap, 256)), dim3(256), 0, st, base);
    const struct {
      const uint64_t* in;
      uint64_t* out;
    } cols[3] = {{P.prow, P.srow}, {P.pkey, P.skey}, {P.pval, P.sval}};
    for (const auto& c : cols) {
      e = launch_excl_scan(c.in, block_cap, P.tiles, RrPrefixOut{c.out}, st);
      if (e != hipSuccess) return hip_status(e, what);
    }
  }
  hipLaunchKernelGGL(rr_finish_kernel, dim3(rr_grid((uint64_t)n_queries + 1, 256)), dim3(256), 0, st, base, false);
  return hip_status(hipGetLastError(), what);
}

extern "C" int lsm_table_range_rows_plan(const uint8_t* d_file, uint64_t file_len, const lsm_table_scan* table,
                                         const uint64_t* d_data_block_off, uint32_t n_data_blocks, const void* pos,
                                         uint32_t n_queries, uint64_t block_cap, uint64_t row_cap,
                                         const uint64_t* d_base, uint64_t* d_run_start, uint64_t* d_end,
                                         uint64_t* d_need, int32_t* d_row_status, int32_t* d_result,
                                         void* d_workspace, size_t workspace_bytes, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const char* what = "lsm_table_range_rows_plan";
  if (n_queries == 0) return rr_plan_empty(d_base, d_run_start, d_end, d_need, d_result, st, what);
  RrParams P;
  const int rc = rr_params(d_file, file_len, table, d_data_block_off, n_data_blocks, pos, n_queries, block_cap,
                           row_cap, d_base, d_end, d_workspace, workspace_bytes, P);
  if (rc != LSM_OK) return rc;
  return rr_plan(P, n_queries, block_cap, d_run_start, d_need, d_row_status, d_result, st, what);
}

extern "C" int lsm_table_range_rows_plan_framed(const lsm_table_scan* table, const void* frames, const void* pos,
                                                uint32_t n_queries, uint64_t block_cap, uint64_t row_cap,
                                                const uint64_t* d_base, uint64_t* d_run_start, uint64_t* d_end,
                                                uint64_t* d_need, int32_t* d_row_status, int32_t* d_result,
                                                void* d_workspace, size_t workspace_bytes, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const char* what = "lsm_table_range_rows_plan_framed";
  if (n_queries == 0) return rr_plan_empty(d_base, d_run_start, d_end, d_need, d_result, st, what);
  RrFramedParams P;
  const int rc = rr_framed_params(table, frames, pos, n_queries, block_cap, row_cap, d_base, d_end, d_workspace,
                                  workspace_bytes, P);
  if (rc != LSM_OK) return rc;
  return rr_plan(P, n_queries, block_cap, d_run_start, d_need, d_row_status, d_result, st, what);
}

__global__ void rr_result_kernel(int32_t* result) { *result = LSM_OK; }

// n_queries == 0: nothing to write but the result.
static int rr_rows_empty(int32_t* d_result, hipStream_t st, const char* what) {
  if (!d_result) return LSM_BAD_ARG;
  hipLaunchKernelGGL(rr_result_kernel, dim3(1), dim3(1), 0, st, d_result);
  return hip_status(hipGetLastError(), what);
}

// The rows call's launches over checked params (RrParams or RrFramedParams).
template <class Params>
static int rr_rows_call(Params& P, uint64_t block_cap, uint64_t row_cap, uint64_t* d_out_key_off,
                        uint64_t* d_out_val_off, uint8_t* d_out_keys, uint64_t key_cap, uint8_t* d_out_vals,
                        uint64_t val_cap, uint64_t* d_out_seqno, uint8_t* d_out_vtype, uint64_t out_item_cap,
                        int32_t* d_result, hipStream_t st, const char* what) {
  if (!d_out_key_off || !d_out_val_off || !d_out_keys || !d_out_vals || !d_out_seqno || !d_out_vtype || !d_result)
    return LSM_BAD_ARG;
  P.out_key_off = d_out_key_off;
  P.out_val_off = d_out_val_off;
  P.out_keys = d_out_keys;
  P.out_vals = d_out_vals;
  P.out_seqno = d_out_seqno;
  P.out_vtype = d_out_vtype;
  P.item_cap = out_item_cap;
  P.key_cap = key_cap;
  P.val_cap = val_cap;
  P.result = d_result;
  // (block_cap == 0: one workgroup still reports the result and writes the closing offsets)
  const dim3 grid(rr_grid(block_cap ? block_cap : 1, kRrGroupsPerWg));
  if constexpr (Params::kFramed) hipLaunchKernelGGL(rr_rows_framed_kernel, grid, dim3(kRrThreads), 0, st, P);
  else hipLaunchKernelGGL(rr_rows_kernel, grid, dim3(kRrThreads), 0, st, P);
  if (row_cap) {
    const RrParams& base = P;
    hipLaunchKernelGGL(rr_gather_kernel, dim3(rr_grid(row_cap, kMiWaves * 64)), dim3(kMiWaves * 64), 0, st, base);
  }
  return hip_status(hipGetLastError(), what);
}

extern "C" int lsm_table_range_rows(const uint8_t* d_file, uint64_t file_len, const lsm_table_scan* table,
                                    const uint64_t* d_data_block_off, uint32_t n_data_blocks, const void* pos,
                                    uint32_t n_queries, uint64_t block_cap, uint64_t row_cap, const uint64_t* d_base,
                                    const uint64_t* d_end, void* d_workspace, size_t workspace_bytes,
                                    uint64_t* d_out_key_off, uint64_t* d_out_val_off, uint8_t* d_out_keys,
                                    uint64_t key_cap, uint8_t* d_out_vals, uint64_t val_cap, uint64_t* d_out_seqno,
                                    uint8_t* d_out_vtype, uint64_t out_item_cap, int32_t* d_result, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const char* what = "lsm_table_range_rows";
  if (n_queries == 0) return rr_rows_empty(d_result, st, what);
  RrParams P;
  const int rc = rr_params(d_file, file_len, table, d_data_block_off, n_data_blocks, pos, n_queries, block_cap,
                           row_cap, d_base, d_end, d_workspace, workspace_bytes, P);
  if (rc != LSM_OK) return rc;
  return rr_rows_call(P, block_cap, row_cap, d_out_key_off, d_out_val_off, d_out_keys, key_cap, d_out_vals, val_cap,
                      d_out_seqno, d_out_vtype, out_item_cap, d_result, st, what);
}

extern "C" int lsm_table_range_rows_framed(const lsm_table_scan* table, const void* frames, const void* pos,
                                           uint32_t n_queries, uint64_t block_cap, uint64_t row_cap,
                                           const uint64_t* d_base, const uint64_t* d_end, void* d_workspace,
                                           size_t workspace_bytes, uint64_t* d_out_key_off, uint64_t* d_out_val_off,
                                           uint8_t* d_out_keys, uint64_t key_cap, uint8_t* d_out_vals,
                                           uint64_t val_cap, uint64_t* d_out_seqno, uint8_t* d_out_vtype,
                                           uint64_t out_item_cap, int32_t* d_result, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const char* what = "lsm_table_range_rows_framed";
  if (n_queries == 0) return rr_rows_empty(d_result, st, what);
  RrFramedParams P;
  const int rc = rr_framed_params(table, frames, pos, n_queries, block_cap, row_cap, d_base, d_end, d_workspace,
                                  workspace_bytes, P);
  if (rc != LSM_OK) return rc;
  return rr_rows_call(P, block_cap, row_cap, d_out_key_off, d_out_val_off, d_out_keys, key_cap, d_out_vals, val_cap,
                      d_out_seqno, d_out_vtype, out_item_cap, d_result, st, what);
}
