// decode.hip — batched SST block decode on gfx950 (the north-star hot path): the host side.
//
// Replaces, per block, Block::from_file (header decode + xxh3_128 verify,
// src/table/block/mod.rs:131-182), the load_block type check
// (src/table/util.rs:79-86) and the full forward DataBlock::iter() /
// IndexBlock::iter() (src/table/block/decoder.rs:442-483) over a whole batch.
//
// Launch shape: 4-wave workgroups, four per CU.  Workgroup w
// owns blocks [w*BPW, (w+1)*BPW) and walks them in GROUPS — the longest run of
// consecutive blocks that fits the 33.75 KiB LDS stage (consecutive blocks are
// contiguous on disk, so a group is one contiguous span):
//   1. lane j of every wave holds block j's handle and item range;
//   2. all waves copy the span HBM -> LDS with global_load_lds_dwordx4;
//   3. one wave (it rotates with the group): lane j checks block j's header
//      fields and trailer, a row scan numbers the restart intervals of the group,
//   4. and the same wave goes on into phase A (lane = restart interval), which
//      walks record boundaries only, while the other waves verify the payload
//      xxh3_128 (16-lane DPP rows) and the header checksums from step 2 on;
//   5. phase B on all waves (thread = record) parses and validates every
//      field and stores the parsed-item SoA with coalesced global stores.
// Blocks larger than the stage, index blocks and rare record shapes go to
// decode_deferred_staged_kernel (one block per 4-wave workgroup, LEB cursor).
//
// The kernels by stage: decode_group.hip (the group kernel), decode_big.hpp (the big-block
// kernel and the general path) and decode_huge.hip (the huge-block pool path); what they share
// is in decode_common.hpp.  Here: the trailer-count and item-start pass, the workspace layout
// and launch_decode, which calls the stages in order.
#include <hip/hip_runtime.h>

#include "decode_common.hpp"
#include "fill.hpp"
#include "scan.hpp"

namespace lsmgpu {

// item counts from the trailers (trailer.rs:57-75), same rule as
// oracle/batch.c: 0 unless the handle holds header + a 32-byte minimum payload,
// and at most (payload - 32) / 3 (every record is >= 3 bytes), so a corrupt,
// not-yet-verified trailer cannot reserve more than its bytes could hold.
__device__ __forceinline__ uint64_t trailer_count(const uint8_t* __restrict__ blocks, const uint64_t* __restrict__ off,
                                                  uint32_t b) {
  const uint64_t o = off[b], e = off[b + 1];
  uint64_t c = 0;
  if (e >= o && e - o >= kHdrLen + kTrailerLen + 1) {
    const uint8_t* p = blocks + e - 4;
    c = (uint64_t)p[0] | ((uint64_t)p[1] << 8) | ((uint64_t)p[2] << 16) | ((uint64_t)p[3] << 24);
    const uint64_t most = (e - o - kHdrLen - 32) / 3;  // records are >= 3 bytes each
    c = c < most ? c : most;
  }
  return c;
}

// (workgroup 0 also clears the call's four list counters: no clear launch of their own)
__global__ __launch_bounds__(256) void trailer_counts_kernel(const uint8_t* __restrict__ blocks,
                                                             const uint64_t* __restrict__ off, uint32_t n,
                                                             uint64_t* __restrict__ counts, uint32_t* __restrict__ clear4) {
  if (blockIdx.x == 0 && threadIdx.x < 4) clear4[threadIdx.x] = 0;
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  counts[b] = trailer_count(blocks, off, b);
}

// Batches of at most one scan tile (kScanTile blocks): the counts and their
// exclusive scan into item_start in one workgroup (one launch, not two), and
// the four list counters cleared.
__global__ __launch_bounds__(kScanThreads) void trailer_counts_scan_kernel(const uint8_t* __restrict__ blocks,
                                                                           const uint64_t* __restrict__ off, uint32_t n,
                                                                           uint32_t* __restrict__ item_start, uint64_t cap,
                                                                           uint32_t* __restrict__ clear4) {
  __shared__ uint64_t sh[kScanThreads / 64];
  if (threadIdx.x < 4) clear4[threadIdx.x] = 0;
  const uint32_t base = threadIdx.x * kScanPerThread;
  uint64_t v[kScanPerThread], s = 0;
#pragma unroll
  for (int i = 0; i < kScanPerThread; ++i) {
    v[i] = base + i < n ? trailer_count(blocks, off, base + i) : 0;
    s += v[i];
  }
  uint64_t total;
  uint64_t ex = block_excl_scan_u64(s, sh, total);
#pragma unroll
  for (int i = 0; i < kScanPerThread; ++i) {
    if (base + i < n) item_start[base + i] = (uint32_t)(ex < cap ? ex : cap);
    ex += v[i];
    if (base + i + 1 == n) item_start[n] = (uint32_t)(ex < cap ? ex : cap);
  }
}

struct ItemStartOut {
  uint32_t* item_start;
  uint64_t cap;
  __device__ void operator()(uint64_t i, uint64_t prefix) const {
    item_start[i] = (uint32_t)(prefix < cap ? prefix : cap);
  }
};

// ------------------------------------------------------------ the workspace
// The regions of the caller's workspace for a batch of n_blocks blocks, each 256-byte aligned:
// byte offsets from the workspace's start, in layout order, and their sum.  The size functions
// return it and launch_decode takes every pointer from here.
struct DecodeWorkspace {
  size_t counts;    // u64 [n_blocks]: item counts from the trailers
  size_t tiles;     // u64 scan tile sums
  size_t counters;  // one cell: the u32 counts of the three lists (and a fourth word, cleared with them)
  size_t defer, defer2, defer3;  // u32 [n_blocks] each: the hand-off lists
  size_t total;
  explicit DecodeWorkspace(uint32_t n_blocks) {
    Carver c;
    counts = c.take((size_t)n_blocks * 8);
    tiles = c.take(scan_tiles(n_blocks) * 8);
    counters = c.take(256);
    defer = c.take((size_t)n_blocks * 4);
    defer2 = c.take((size_t)n_blocks * 4);
    defer3 = c.take((size_t)n_blocks * 4);
    total = c.total();
  }
  // where the huge-block pool starts in a workspace that carries one (lsm_decode_workspace_size_ex)
  size_t pool_base() const { return round256(total); }
};

size_t decode_workspace_size(uint32_t n_blocks) { return DecodeWorkspace(n_blocks).total; }

size_t decode_pool_min_bytes(uint32_t n_blocks) {
  return DecodeWorkspace(n_blocks).pool_base() + decode_huge_pool_min_bytes();
}

// + the huge-block pool for a batch of blocks_bytes bytes
size_t decode_workspace_size_ex(uint32_t n_blocks, uint64_t blocks_bytes) {
  const size_t ex = DecodeWorkspace(n_blocks).total + decode_huge_pool_bytes(n_blocks, blocks_bytes);
  return ex > decode_pool_min_bytes(n_blocks) ? ex : decode_pool_min_bytes(n_blocks);
}

// The group kernel's dynamic LDS (decode_blocks_kernel lays it out in this order).
uint32_t decode_lds_bytes(uint32_t stage_bytes, uint32_t tile_items, uint32_t blocks_per_wave) {
  const uint32_t g = blocks_per_wave < kMaxGroup ? blocks_per_wave : kMaxGroup;
  return g * (uint32_t)sizeof(BlockMeta) + ((8 * (tile_items + 1) + 15) & ~15u) + ((tile_items + 15) & ~15u) +
         ((stage_bytes + 15) & ~15u) + kStagePad + (uint32_t)sizeof(LongSecret);
}

// The item starts (unless the caller gave them) and the three list counters cleared.
static hipError_t launch_item_starts(const DecodeParams& P, uint64_t* counts, uint64_t* tiles, uint32_t* counters,
                                     hipStream_t st) {
  if (P.flags & LSM_DECODE_ITEM_START_VALID) return fill_words_async(counters, 4, 0, st);
  if (scan_tiles(P.n_blocks) == 1) {  // (the counts kernel clears the list counters)
    hipLaunchKernelGGL(trailer_counts_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, P.blocks, P.block_off,
                       P.n_blocks, P.item_start_w, P.item_cap, counters);
    return hipSuccess;
  }
  hipLaunchKernelGGL(trailer_counts_kernel, dim3((P.n_blocks + 255) / 256), dim3(256), 0, st, P.blocks,
                     P.block_off, P.n_blocks, counts, counters);
  return launch_excl_scan(counts, P.n_blocks, tiles, ItemStartOut{P.item_start_w, P.item_cap}, st);
}

hipError_t launch_decode(const DecodeParams& P0, void* ws, size_t ws_bytes, hipStream_t st) {
  DecodeParams P = P0;
  const DecodeWorkspace W(P.n_blocks);
  uint8_t* w = (uint8_t*)ws;
  uint32_t* counters = (uint32_t*)(w + W.counters);
  P.defer_count = counters;
  P.defer2_count = counters + 1;
  P.defer3_count = counters + 2;
  P.defer_list = (uint32_t*)(w + W.defer);
  P.defer2_list = (uint32_t*)(w + W.defer2);
  P.defer3_list = (uint32_t*)(w + W.defer3);
  // the pool only when the caller asks for it (LSM_DECODE_HUGE_POOL; the ABI checked the size)
  P.huge_pool = (P.flags & LSM_DECODE_HUGE_POOL) && ws_bytes >= decode_pool_min_bytes(P.n_blocks)
                    ? w + W.pool_base() : nullptr;
  P.huge_pool_bytes = P.huge_pool ? ws_bytes - W.pool_base() : 0;
  // kernel variants: every field present or not, 32- or 16-bit offsets
  const bool all = all_fields(P.out);
  const int variant = (all ? 1 : 0) | (P.compact ? 2 : 0);
  hipError_t e;
  if ((e = launch_item_starts(P, (uint64_t*)(w + W.counts), (uint64_t*)(w + W.tiles), counters, st)) != hipSuccess)
    return e;
  if ((e = launch_decode_group(P, variant, st)) != hipSuccess) return e;
  uint32_t bgrid = 0;
  if ((e = launch_decode_big(P, variant, &bgrid, st)) != hipSuccess) return e;
  const bool pool = P.huge_pool && bgrid;
  if (pool && (e = launch_decode_huge_plan(P, st)) != hipSuccess) return e;
  if ((e = launch_decode_general(P, st)) != hipSuccess) return e;
  if (pool && (e = launch_decode_huge(P, all, st)) != hipSuccess) return e;
  return hipGetLastError();
}

}  // namespace lsmgpu

#if defined(LSM_DIAG) && !defined(LSM_DIAG_NOTIME)
// Diagnostic builds only: copy out and clear the kernels' phase totals.  Entries 0..7 are the
// big-block kernel's, 8..14 the huge kernel's, 15 both their counts, 16..31 the group kernel's
// (wave 0 per group, role timers summed over waves).
extern "C" int lsm_diag_decode_phases(uint64_t* out32) {
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  for (int i = 0; i < 32; ++i) out32[i] = 0;
  if (lsmgpu::decode_large_phases(out32) != hipSuccess) return -1;
  return lsmgpu::decode_group_phases(out32) == hipSuccess ? 0 : -1;
}
#endif
