// encode.hip — batched SST block encode on gfx950: the host side.
//
// Replaces, per block, DataBlock::encode_into / IndexBlock::encode_into
// (src/table/data_block/mod.rs:523-549, src/table/index_block/mod.rs:110-127,
// Encoder src/table/block/encoder.rs:84-164, Trailer trailer.rs:78-173) and
// Block::write_into (src/table/block/mod.rs:45-84, CompressionType::None):
// the payload xxh3_128 and the 33-byte header are fused into the same pass.
//
// Pipeline (all on one stream, DESIGN.md "Encode kernels"); this file sizes the
// workspace, decides the path of a batch once and calls the stages in order:
//   E1  encode_plan.hip: a 256-thread workgroup plans up to 128 consecutive
//       blocks (plan_blocks_per_wg), data blocks wave by wave (encode_plan.hpp):
//       shared prefix with the restart head (encoder.rs:140-143), record
//       length and offset (erec), per block its size, binary-index step,
//       hash-index size, size class, key / value span starts.  Batches of huge
//       blocks are planned item-parallel instead (E1p).
//   S   device exclusive scan of block sizes -> d_block_off (packed output)
//       and the list of the blocks E2 does not take.
//       (Fused plan: E1 runs inside E2 on each run of 32 blocks and a decoupled
//       look-back over the runs replaces S.)
//   E2  encode_group.hip, encode_group_kernel: 4-wave workgroups write runs of
//       32 consecutive blocks.  Runs of small data blocks go wave per block,
//       without barriers.  The others go in groups staged by LDS-DMA (key and
//       value spans), thread per record into an LDS image of the group's output
//       span, binary index, hash index (LDS min/max atomics reproduce the
//       order-independent FREE/idx/CONFLICT rule, hash_index/builder.rs:64-110),
//       trailer, the payload xxh3_128 split over the workgroup's 16 DPP rows in
//       1 KiB units, headers, and a 16 B/lane copy-out in two parts: the pieces
//       without header bytes under the checksum chains, the header pieces after.
//   L   encode_large.hip, blocks that do not fit a group: listed 1-wave / 8-wave
//       kernels (LDS image of 20 / 96 KiB), or E3 straight in HBM, one workgroup
//       per block or, with the workspace pool, across the GPU.
#include <hip/hip_runtime.h>

#include <math.h>

#include "encode_common.hpp"

namespace lsmgpu {

#ifdef LSM_DIAG
static unsigned long long* diag_phase_buffer() {
  static unsigned long long* d = nullptr;
  if (!d && hipMalloc(&d, 16 * sizeof(unsigned long long)) == hipSuccess) (void)hipMemset(d, 0, 16 * sizeof(unsigned long long));
  return d;
}
#endif

// A plan workgroup walks its blocks' items serially (chunks of 512), so it
// owns about 16 Ki items: kPlanBlocks blocks of the 4 KiB shapes, down to one
// block each for 1-4 MiB data blocks (which gave a single workgroup 3 M items
// and a 27 ms plan for 60 blocks of 4 MiB).
static uint32_t plan_blocks_per_wg(uint64_t n_items, uint32_t n_blocks) {
  const uint64_t avg = n_blocks ? (n_items + n_blocks - 1) / n_blocks : 1;
  const uint64_t bpw = (16384 + avg - 1) / (avg ? avg : 1);
  return (uint32_t)std::min<uint64_t>(kPlanBlocks, std::max<uint64_t>(1, bpw));
}

size_t encode_workspace_size(uint64_t n_items, uint32_t n_blocks) { return EncodeWorkspace(n_items, n_blocks).total; }

// Huge-list entries for an output of out_cap bytes: a huge block's image
// exceeds kImgBig, so its encoded bytes exceed 32 KiB (entries past the
// capacity stay with the one-workgroup E3).
static uint64_t enc_huge_cap(uint32_t n_blocks, uint64_t out_cap) {
  return std::min<uint64_t>(n_blocks, out_cap / 32768 + 1);
}

size_t encode_workspace_size_ex(uint64_t n_items, uint32_t n_blocks, uint64_t out_cap) {
  const size_t ex = EncodeWorkspace(n_items, n_blocks).pool_base() +
                    enc_huge_fixed_bytes(enc_huge_cap(n_blocks, out_cap)) + 65 * (out_cap / 1024 + 1) + 256;
  return std::max(ex, encode_pool_min_bytes(n_items, n_blocks, out_cap));
}

size_t encode_pool_min_bytes(uint64_t n_items, uint32_t n_blocks, uint64_t out_cap) {
  return EncodeWorkspace(n_items, n_blocks).pool_base() + enc_huge_fixed_bytes(enc_huge_cap(n_blocks, out_cap)) +
         65 * 128;
}

uint64_t encode_bound(uint64_t n_items, uint32_t n_blocks, uint64_t key_bytes, uint64_t val_bytes,
                      const lsm_block_params* params) {
  const float ratio = params ? params->hash_ratio : 0.0f;
  uint64_t hash = 0;
  if (ratio > 0.0f) hash = (uint64_t)ceil((double)n_items * (double)ratio) + n_blocks;
  return 29ULL * n_items + key_bytes + val_bytes + 4ULL * n_items + hash +
         (uint64_t)n_blocks * (kHdrLen + 1 + kTrailerLen + 16) + 64;
}

hipError_t launch_encode(const lsm_items& items, const uint32_t* starts, uint32_t n_blocks,
                         const lsm_block_params& params, uint8_t* out, uint64_t out_cap, uint64_t* block_off,
                         int32_t* status, void* ws, size_t ws_bytes, hipStream_t st, bool off32) {
  EncodeParams P;
  P.it = items;
  P.off32 = off32 ? 1u : 0u;
  P.starts = starts;
  P.n_blocks = n_blocks;
  P.ri = params.block_type == 1 ? 1 : params.restart_interval;
  P.ratio = params.block_type == 1 ? 0.0f : params.hash_ratio;
  P.type = params.block_type;
  P.diag = params.reserved;
#ifdef LSM_DIAG
  P.phase = diag_phase_buffer();
#else
  P.phase = nullptr;
#endif
  P.out = out;
  P.out_cap = out_cap;
  P.block_off = block_off;
  P.status = status;
  const EncodeWorkspace W(items.n_items, n_blocks);
  uint8_t* const w = (uint8_t*)ws;
  P.kspan = (uint64_t*)(w + W.kspan);
  P.vspan = (uint64_t*)(w + W.vspan);
  P.sizes = (uint64_t*)(w + W.sizes);
  P.plans = (BlockPlan*)(w + W.plans);
  P.lists = (uint32_t*)(w + W.lists);
  P.list_count = (uint32_t*)(w + W.counts);
  P.e1p_flag = P.list_count + 1;
  uint64_t* const tiles = (uint64_t*)(w + W.tiles);
  P.erec = (uint32_t*)(w + W.erec);
  P.hbucket = (uint16_t*)(w + W.hbucket);
  P.hb_fix = (uint32_t*)(w + W.hb_fix);
  P.pfirst = (uint32_t*)(w + W.pfirst);
  P.wpart = (uint64_t*)(w + W.wpart);
  hipError_t e;
  P.plan_bpw = plan_blocks_per_wg(items.n_items, n_blocks);
  const bool e1p = P.type != 1 && P.plan_bpw <= kE1pMaxBpw && items.n_items > 0 && items.n_items < 0xFFFFFFFFull;
  {  // the whole-GPU E3 pool, when the caller asks for it (the ABI checked the size)
    const size_t base = W.pool_base();
    const uint64_t cap = enc_huge_cap(n_blocks, out_cap);
    const bool pool = cap && (params.flags & LSM_ENCODE_HUGE_POOL) &&
                      ws_bytes >= encode_pool_min_bytes(items.n_items, n_blocks, out_cap);
    P.huge_pool = pool ? w + base : nullptr;
    P.huge_pool_bytes = pool ? ws_bytes - base : 0;
    P.huge_cap = pool ? (uint32_t)cap : 0;
    // (E1p's lengths kernel writes the E1p flag whole and clears the huge-block count:
    // no clear launch; otherwise the pool header is cleared here)
    if (pool && !e1p && (e = fill_words_async(P.huge_pool, 64, 0, st)) != hipSuccess) return e;
  }
  // The run-level plan fused into the group kernel (decoupled look-back for the offsets):
  // data blocks without a hash index, up to 512 items per block on average, no pool, and
  // fewer than 2^21 blocks (the listed count's bits in a look-back word); asked for
  // (LSM_ENCODE_RUN_PLAN) or at >= kFusedAutoItems items per block on average, where it
  // measured faster (profiles/r06_experiments.txt, ab6h / ab6i).
#ifdef LSM_NO_FUSED_PLAN
  constexpr bool kFusedOk = false;
#else
  constexpr bool kFusedOk = true;
#endif
  const uint64_t avg_items = n_blocks ? items.n_items / n_blocks : 0;
  const bool fused = kFusedOk && !e1p && P.type != 1 && !(P.ratio > 0.0f) && !P.huge_pool && P.plan_bpw >= 32 &&
                     n_blocks > 0 && n_blocks < (1u << 21) &&
                     ((params.flags & LSM_ENCODE_RUN_PLAN) || avg_items >= kFusedAutoItems);
  if ((e = launch_encode_plan(P, e1p, fused, tiles, st)) != hipSuccess) return e;
  launch_encode_group(P, fused, st);
  if ((e = launch_encode_large(P, st)) != hipSuccess) return e;
  return hipGetLastError();
}

}  // namespace lsmgpu

#ifdef LSM_DIAG
// Diagnostic builds only: copy out and clear the per-phase cycle totals.
extern "C" int lsm_diag_encode_phases(uint64_t* out16) {
  unsigned long long* d = lsmgpu::diag_phase_buffer();
  if (!d || hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpy(out16, d, 16 * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return hipMemset(d, 0, 16 * sizeof(uint64_t)) == hipSuccess ? 0 : -1;
}
#endif
