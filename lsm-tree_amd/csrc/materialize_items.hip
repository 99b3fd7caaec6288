// materialize_items.hip — decoded blocks -> merge-ready item runs on the device:
// DataBlockParsedItem::materialize producing an owned InternalValue, key AND
// value (src/table/data_block/mod.rs:296-315), as Scanner::next yields it
// (src/table/scanner.rs:74-92) into Merger::new (compaction/worker.rs:149-182).
// The parsed rows of one table (lsm_decode_blocks / lsm_scan_table outputs) are
// appended to an lsm_items-shaped SoA at a device-held cursor, so several tables
// chain into the "runs back to back" input of lsm_merge_runs with nothing
// downloaded.
//   1. mi_lengths_kernel   lane per row: key and value length (0 for rejected
//                          blocks and rows no block covers), both sums of each
//                          scan tile; the cursor's row part
//   2. scan_tile_sums x 2, mi_offsets_kernel: one exclusive scan of both lengths
//                          (scan.hpp's pieces) -> d_out_key_off / d_out_val_off
//                          at the cursor, d_end
//   3. mi_gather_kernel    wave per tile of 64 consecutive rows, whatever blocks
//                          they lie in: keys (prefix || suffix), values, seqno
//                          and vtype of the tile in one pass.
#include <hip/hip_runtime.h>

#include "block_format.hpp"
#include "host_common.hpp"
#include "items_gather.hpp"
#include "lsmgpu.h"
#include "scan.hpp"

namespace lsmgpu {

struct MiParams {
  const uint8_t* blocks;
  const uint64_t* block_off;
  uint32_t n_blocks;
  const uint32_t* d_n_blocks;  // device block count (<= n_blocks), or null
  const uint32_t* item_start;
  const int32_t* status;
  const uint32_t* key_off;
  const uint32_t* val_off;
  const uint32_t* val_len;
  const uint16_t* key_len;
  const uint16_t* prefix_len;
  const uint64_t* seqno;
  const uint8_t* vtype;
  uint64_t n_items;
  const uint64_t* base;  // u64[3] {items, key bytes, value bytes}, or null = zeros
  uint64_t* end;         // u64[3]: written by the plan, read by the gather
  uint64_t* out_key_off;
  uint64_t* out_val_off;
  uint64_t item_cap, key_cap, val_cap;
  uint8_t* out_keys;
  uint8_t* out_vals;
  uint64_t* out_seqno;
  uint8_t* out_vtype;
  int32_t* result;
  // plan workspace
  uint64_t* meta;  // [kMiMeta]
  uint32_t* klens;
  uint32_t* vlens;
  uint64_t* ktiles;  // [scan_tiles(n_items)] each: the tiles' sums, then their exclusive scan
  uint64_t* vtiles;
};
// meta: the row count, the cursor this plan starts at, and whether it fits out_item_cap
enum { kMiRows = 0, kMiBase = 1, kMiOverflow = 4, kMiMeta = 8 };

__device__ __forceinline__ uint32_t mi_block_count(const MiParams& P) {
  return P.d_n_blocks ? min(*P.d_n_blocks, P.n_blocks) : P.n_blocks;
}
__device__ __forceinline__ uint64_t mi_row_count(const MiParams& P, uint32_t count) {
  return P.n_items && count ? min((uint64_t)P.item_start[count], P.n_items) : 0;
}
// The last block of [lo, hi] whose first row is <= i (the block holding row i
// when item_start[lo] <= i; empty blocks before it are skipped).
__device__ __forceinline__ uint32_t mi_find_block(const uint32_t* item_start, uint32_t lo, uint32_t hi, uint64_t i) {
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (item_start[mid] <= i) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}
// The same over [0, count - 1], galloping away from a guess g: a few dependent
// loads when the guess is near, against log2(count) of them for the plain
// search (a wave waits for every one of them).  Any item_start gives an index
// below count.
__device__ __forceinline__ uint32_t mi_find_block_near(const uint32_t* item_start, uint32_t count, uint64_t i,
                                                       uint32_t g) {
  g = min(g, count - 1);
  uint32_t lo, hi;
  if (item_start[g] <= i) {
    lo = g;
    hi = count - 1;
    for (uint64_t step = 1; lo + step < count; step *= 2) {
      if (item_start[lo + step] > i) {
        hi = (uint32_t)(lo + step - 1);
        break;
      }
      lo = (uint32_t)(lo + step);
    }
  } else {  // the answer is below hi (exclusive here)
    hi = g;
    lo = 0;
    for (uint32_t step = 1; hi > 0; step *= 2) {
      const uint32_t p = hi > step ? hi - step : 0;
      if (item_start[p] <= i) {
        lo = p;
        break;
      }
      hi = p;
    }
    if (hi == 0) return 0;  // item_start[0] > i: not a prefix sum
    hi -= 1;
  }
  return mi_find_block(item_start, lo, hi, i);
}
// The block of every row of the tile [i0, i0 + 64) (clipped to the R rows):
// two wave-uniform searches (the first seeded by the tile's share of the blocks,
// the second by the first) bracket a per-lane search over the few blocks between.
__device__ __forceinline__ uint32_t mi_tile_block(const MiParams& P, uint32_t count, uint64_t R, uint64_t i0,
                                                  uint64_t i) {
  const uint32_t b0 = mi_find_block_near(P.item_start, count, i0, (uint32_t)(i0 * count / R));
  const uint32_t b1 = mi_find_block_near(P.item_start, count, min(i0 + 63, R - 1), b0);
  return mi_find_block(P.item_start, b0, max(b0, b1), min(i, R - 1));
}

// Parsed row i of block b as the gather copies it (MiRow, items_gather.hpp).  A
// row is rejected (ok = false, all lengths 0) when its block's status is not
// LSM_OK, the block is not a data or meta block, or a byte range of the row does
// not lie in the block's payload.
__device__ __forceinline__ MiRow mi_row(const MiParams& P, uint64_t i, uint32_t b) {
  MiRow r{P.blocks, P.blocks, P.blocks, 0, 0, 0, false};
  const uint64_t s = P.item_start[b], e = P.item_start[b + 1];
  if (P.status[b] != LSM_OK || i < s || i >= e) return r;
  const uint64_t bo = P.block_off[b], be = P.block_off[b + 1];
  if (be < bo + kHdrLen + kTrailerLen) return r;
  const uint32_t type = P.blocks[bo + 4];
  if (type != LSM_BLOCK_DATA && type != LSM_BLOCK_META) return r;
  const uint64_t plen = be - bo - kHdrLen;
  const uint32_t ri = P.blocks[be - kTrailerLen];  // trailer byte 0, trailer.rs:78-173
  const uint32_t k = (uint32_t)(i - s);
  const uint64_t head = s + (ri ? k - k % ri : k);
  const uint32_t pl = P.prefix_len[i], kl = P.key_len[i], vl = P.val_len[i];
  const uint64_t ko = P.key_off[i], vo = P.val_off[i], ho = pl ? P.key_off[head] : 0;
  if (ko + kl > plen || vo + vl > plen || ho + pl > plen) return r;
  const uint8_t* payload = P.blocks + bo + kHdrLen;
  r.pre = payload + ho;
  r.suf = payload + ko;
  r.val = payload + vo;
  r.pl = pl;
  r.kl = kl;
  r.vl = vl;
  r.ok = true;
  return r;
}

// Plan pass 1, workgroup per scan tile (kScanTile rows, 64 consecutive rows per
// wave and step): the rows' key and value lengths, and the tile's two sums.
__global__ __launch_bounds__(kScanThreads) void mi_lengths_kernel(MiParams P) {
  __shared__ uint64_t sh[kScanThreads / 64];
  const uint32_t count = mi_block_count(P);
  const uint64_t R = mi_row_count(P, count);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const uint64_t b0 = P.base ? P.base[0] : 0, b1 = P.base ? P.base[1] : 0, b2 = P.base ? P.base[2] : 0;
    const bool over = b0 + R > P.item_cap;
    P.meta[kMiRows] = R;
    P.meta[kMiBase + 0] = b0;
    P.meta[kMiBase + 1] = b1;
    P.meta[kMiBase + 2] = b2;
    P.meta[kMiOverflow] = over;
    P.end[0] = b0 + R;
    *P.result = over ? LSM_OVERFLOW : LSM_OK;
    if (P.n_items == 0) {  // no offsets pass runs: the cursor does not move
      P.end[1] = b1;
      P.end[2] = b2;
      if (!over) {
        P.out_key_off[b0] = b1;
        P.out_val_off[b0] = b2;
      }
    }
  }
  uint64_t ks = 0, vs = 0;
  for (int j = 0; j < kScanPerThread; ++j) {
    const uint64_t i = (uint64_t)blockIdx.x * kScanTile + (uint64_t)j * kScanThreads + threadIdx.x;
    const uint64_t i0 = i & ~63ULL;  // (the wave's 64 rows of this step)
    uint32_t kl = 0, vl = 0;
    if (i0 < R) {
      const uint32_t b = mi_tile_block(P, count, R, i0, i);
      if (i < R) {
        const MiRow r = mi_row(P, i, b);
        kl = r.pl + r.kl;
        vl = r.vl;
      }
    }
    if (i < P.n_items) {
      P.klens[i] = kl;
      P.vlens[i] = vl;
    }
    ks += kl;
    vs += vl;
  }
  uint64_t kt, vt;
  block_excl_scan_u64(ks, sh, kt);
  block_excl_scan_u64(vs, sh, vt);
  if (threadIdx.x == 0) {
    P.ktiles[blockIdx.x] = kt;
    P.vtiles[blockIdx.x] = vt;
  }
}

// Offsets land at the cursor, entries 0 .. R; the total is d_end[field].
struct MiOffOut {
  uint64_t* off;
  uint64_t* end;
  const uint64_t* meta;
  uint32_t field;  // 1 = keys, 2 = values
  __device__ void operator()(uint64_t i, uint64_t prefix) const {
    const uint64_t R = meta[kMiRows];
    if (i > R) return;
    const uint64_t v = meta[kMiBase + field] + prefix;
    if (!meta[kMiOverflow]) off[meta[kMiBase] + i] = v;
    if (i == R) end[field] = v;
  }
};

// Plan pass 2 (after scan_tile_sums over both tile-sum arrays; tiled = false for
// a single tile): scan.hpp's scan_tile_apply over both length arrays at once.
__global__ __launch_bounds__(kScanThreads) void mi_offsets_kernel(MiParams P, bool tiled) {
  __shared__ uint64_t sh[kScanThreads / 64];
  const uint64_t n = P.n_items;
  const uint64_t base = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanPerThread;
  uint64_t k[kScanPerThread], v[kScanPerThread];
  scan_load(P.klens, base, n, k);
  scan_load(P.vlens, base, n, v);
  uint64_t ks = 0, vs = 0;
#pragma unroll
  for (int i = 0; i < kScanPerThread; ++i) {
    ks += k[i];
    vs += v[i];
  }
  uint64_t total;
  uint64_t kex = block_excl_scan_u64(ks, sh, total) + (tiled ? P.ktiles[blockIdx.x] : 0);
  uint64_t vex = block_excl_scan_u64(vs, sh, total) + (tiled ? P.vtiles[blockIdx.x] : 0);
  const MiOffOut ko{P.out_key_off, P.end, P.meta, 1}, vo{P.out_val_off, P.end, P.meta, 2};
#pragma unroll
  for (int i = 0; i < kScanPerThread; ++i) {
    if (base + i < n) {
      ko(base + i, kex);
      vo(base + i, vex);
    }
    kex += k[i];
    vex += v[i];
    if (base + i == n - 1) {
      ko(n, kex);
      vo(n, vex);
    }
  }
}

// The gather's row source: the parsed SoA of a decode (items_gather.hpp).
struct MiParsedRows {
  static constexpr bool kMeta = true;
  const MiParams& P;
  uint32_t count, b;
  __device__ __forceinline__ void locate(uint64_t R, uint64_t i0, uint64_t i) { b = mi_tile_block(P, count, R, i0, i); }
  __device__ __forceinline__ MiRow row(uint64_t i) const { return mi_row(P, i, b); }
  __device__ __forceinline__ uint64_t seqno(uint64_t i) const { return P.seqno[i]; }
  __device__ __forceinline__ uint8_t vtype(uint64_t i) const { return P.vtype[i]; }
};

__global__ __launch_bounds__(kMiWaves * 64) void mi_gather_kernel(MiParams P) {
  __shared__ __attribute__((aligned(16))) uint8_t buf[kMiWaves][kMiBuf + 32];
  const uint32_t count = mi_block_count(P);
  MiParsedRows S{P, count, 0};
  const ItemsOut O{P.base,    P.end,      P.out_key_off, P.out_val_off, P.item_cap,  P.key_cap,
                   P.val_cap, P.out_keys, P.out_vals,    P.out_seqno,   P.out_vtype, P.result};
  items_gather_tile(S, O, mi_row_count(P, count), P.blocks, buf);
}

// The plan's workspace: byte offsets of its regions, in layout order, and their sum.
struct MiWorkspace {
  size_t meta;            // u64 [kMiMeta]
  size_t klens, vlens;    // u32 [n] each
  size_t ktiles, vtiles;  // u64 scan tile sums
  size_t total;
  explicit MiWorkspace(uint64_t n_items) {
    const uint64_t n = n_items ? n_items : 1;
    Carver c;
    meta = c.take(kMiMeta * 8);
    klens = c.take(n * 4);
    vlens = c.take(n * 4);
    ktiles = c.take(scan_tiles(n) * 8);
    vtiles = c.take(scan_tiles(n) * 8);
    total = c.total();
  }
};

}  // namespace lsmgpu

using namespace lsmgpu;

extern "C" size_t lsm_materialize_items_workspace_size(uint64_t n_items) {
  return MiWorkspace(n_items).total;
}

static int mi_params(const uint8_t* d_blocks, const uint64_t* d_block_off, uint32_t n_blocks,
                     const uint32_t* d_n_blocks, const uint32_t* d_item_start, const int32_t* d_status,
                     const lsm_parsed_items* d_parsed, uint64_t n_items, const uint64_t* d_base, MiParams& P) {
  if (!d_blocks || !d_block_off || !d_item_start || !d_status || !d_parsed || !d_parsed->key_off ||
      !d_parsed->key_len || !d_parsed->prefix_len || !d_parsed->val_off || !d_parsed->val_len || !d_parsed->seqno ||
      !d_parsed->vtype)
    return LSM_BAD_ARG;
  P = MiParams{};
  P.blocks = d_blocks;
  P.block_off = d_block_off;
  P.n_blocks = n_blocks;
  P.d_n_blocks = d_n_blocks;
  P.item_start = d_item_start;
  P.status = d_status;
  P.key_off = d_parsed->key_off;
  P.val_off = d_parsed->val_off;
  P.val_len = d_parsed->val_len;
  P.key_len = d_parsed->key_len;
  P.prefix_len = d_parsed->prefix_len;
  P.seqno = d_parsed->seqno;
  P.vtype = d_parsed->vtype;
  P.n_items = n_items;
  P.base = d_base;
  return LSM_OK;
}

extern "C" int lsm_materialize_items_plan(const uint8_t* d_blocks, const uint64_t* d_block_off, uint32_t n_blocks,
                                          const uint32_t* d_n_blocks, const uint32_t* d_item_start,
                                          const int32_t* d_status, const lsm_parsed_items* d_parsed, uint64_t n_items,
                                          const uint64_t* d_base, uint64_t* d_out_key_off, uint64_t* d_out_val_off,
                                          uint64_t out_item_cap, uint64_t* d_end, int32_t* d_result, void* d_workspace,
                                          size_t workspace_bytes, void* stream) {
  MiParams P;
  int rc = mi_params(d_blocks, d_block_off, n_blocks, d_n_blocks, d_item_start, d_status, d_parsed, n_items, d_base, P);
  if (rc != LSM_OK) return rc;
  if (!d_out_key_off || !d_out_val_off || !d_end || !d_result || d_end == d_base) return LSM_BAD_ARG;
  const MiWorkspace W(n_items);
  if (!d_workspace || workspace_bytes < W.total) return LSM_BAD_ARG;
  const hipStream_t st = (hipStream_t)stream;
  const uint64_t n = n_items ? n_items : 1;
  uint8_t* ws = (uint8_t*)d_workspace;
  P.meta = (uint64_t*)(ws + W.meta);
  P.klens = (uint32_t*)(ws + W.klens);
  P.vlens = (uint32_t*)(ws + W.vlens);
  P.ktiles = (uint64_t*)(ws + W.ktiles);
  P.vtiles = (uint64_t*)(ws + W.vtiles);
  P.end = d_end;
  P.out_key_off = d_out_key_off;
  P.out_val_off = d_out_val_off;
  P.item_cap = out_item_cap;
  P.result = d_result;
  const uint64_t tiles = scan_tiles(n);
  hipLaunchKernelGGL(mi_lengths_kernel, dim3((uint32_t)tiles), dim3(kScanThreads), 0, st, P);
  if (n_items) {
    if (tiles > 1) {
      hipLaunchKernelGGL(scan_tile_sums, dim3(1), dim3(kScanThreads), 0, st, P.ktiles, tiles);
      hipLaunchKernelGGL(scan_tile_sums, dim3(1), dim3(kScanThreads), 0, st, P.vtiles, tiles);
    }
    hipLaunchKernelGGL(mi_offsets_kernel, dim3((uint32_t)tiles), dim3(kScanThreads), 0, st, P, tiles > 1);
  }
  return hip_status(hipGetLastError(), "lsm_materialize_items_plan");
}

extern "C" int lsm_materialize_items(const uint8_t* d_blocks, const uint64_t* d_block_off, uint32_t n_blocks,
                                     const uint32_t* d_n_blocks, const uint32_t* d_item_start, const int32_t* d_status,
                                     const lsm_parsed_items* d_parsed, uint64_t n_items, const uint64_t* d_base,
                                     const uint64_t* d_end, const uint64_t* d_out_key_off,
                                     const uint64_t* d_out_val_off, uint8_t* d_out_keys, uint64_t key_cap,
                                     uint8_t* d_out_vals, uint64_t val_cap, uint64_t* d_out_seqno,
                                     uint8_t* d_out_vtype, uint64_t out_item_cap, int32_t* d_result, void* stream) {
  MiParams P;
  int rc = mi_params(d_blocks, d_block_off, n_blocks, d_n_blocks, d_item_start, d_status, d_parsed, n_items, d_base, P);
  if (rc != LSM_OK) return rc;
  if (!d_end || !d_out_key_off || !d_out_val_off || !d_out_keys || !d_out_vals || !d_out_seqno || !d_out_vtype ||
      !d_result)
    return LSM_BAD_ARG;
  P.end = const_cast<uint64_t*>(d_end);
  P.out_key_off = const_cast<uint64_t*>(d_out_key_off);
  P.out_val_off = const_cast<uint64_t*>(d_out_val_off);
  P.item_cap = out_item_cap;
  P.key_cap = key_cap;
  P.val_cap = val_cap;
  P.out_keys = d_out_keys;
  P.out_vals = d_out_vals;
  P.out_seqno = d_out_seqno;
  P.out_vtype = d_out_vtype;
  P.result = d_result;
  const uint64_t tiles = n_items ? (n_items + 63) / 64 : 1;
  hipLaunchKernelGGL(mi_gather_kernel, dim3((uint32_t)((tiles + kMiWaves - 1) / kMiWaves)), dim3(kMiWaves * 64), 0,
                     (hipStream_t)stream, P);
  return hip_status(hipGetLastError(), "lsm_materialize_items");
}
