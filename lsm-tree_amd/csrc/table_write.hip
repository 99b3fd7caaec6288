// table_write.hip — the step between lsm_merge_runs and the table image: the
// writer's block cut on device offsets, and the block index's entries.
//
// lsm_cut_blocks_device: Writer::write's chunking (src/table/writer/mod.rs:284-290,
// the last partial block :374; with extra_per_item and no values
// PartitionedIndexWriter::register_data_block, writer/index/partitioned.rs:166-179).
// The offsets are prefix sums already: with P[i] = key_off[i] + val_off[i] + extra * i,
// a block that starts at s ends at next(s) = the least j in (s, n] with
// P[j] - P[s] >= block_size (n if there is none), so only the chain
// 0 -> next(0) -> ... is serial.  Plain launches, no atomics, no wait between
// workgroups:
//   0. fill kernel       the header (bad flag) and the tiles' entries and counts cleared
//   1. cut_tile_kernel   workgroup per tile of kCutTile items: next(i) of every item
//                        (gallop, then binary search over P), then pointer doubling in
//                        LDS: jump[i] = the first chain element from i at or past the
//                        tile's end (it may skip whole tiles), cnt[i] = the blocks that
//                        start inside the tile on the chain from i; offsets checked
//   2. cut_walk_kernel   one lane: s = jump[s] from 0, one dependent load per tile
//                        the chain enters; records each tile's entry item and count
//   3. exclusive scan    of the tiles' counts: each tile's first block index,
//                        *d_n_blocks, *d_status, the last start
//   4. cut_emit_kernel   workgroup per tile: the tile's links staged in LDS, one lane
//                        walks from the entry and writes the starts
//
// lsm_index_entries: Writer::spill_block's KeyedBlockHandle(last key, last seqno,
// (file_pos, size)) of every block of an encoded batch (writer/mod.rs:332-337), the
// input of FullIndexWriter (writer/index/full.rs:55-69) and, run again over the
// partitions, of the TLI (cut_index_block, partitioned.rs:80-84,113-115).
//   1. index_lens_kernel    lane per block: the last item's key length
//   2. exclusive scan       -> d_out_key_off
//   3. index_gather_kernel  wave per 64 blocks: the keys assembled in LDS and stored
//                           16 B per lane (gather.hpp), seqnos and handles
#include <hip/hip_runtime.h>

#include "device_common.hpp"
#include "fill.hpp"
#include "gather.hpp"
#include "host_common.hpp"
#include "lsmgpu.h"
#include "scan.hpp"

namespace lsmgpu {

// Items per tile.  One u32 of LDS per item (a 16-bit tile-relative link and a 16-bit
// count): 64 KiB, two workgroups per CU.  lsmgpu.py mirrors it as CUT_TILE_ITEMS.
constexpr uint32_t kCutTile = 16384;
constexpr uint32_t kCutTileLog2 = 14;
constexpr uint32_t kCutThreads = 1024;
constexpr uint32_t kCutEmitThreads = 256;
constexpr uint32_t kCutExit = 0xFFFF;  // link of an item whose block ends at or past the tile's end
static_assert((1u << kCutTileLog2) == kCutTile && kCutTile < kCutExit, "16-bit links and counts");

struct CutHdr {
  uint32_t bad;  // some offset decreases
  uint32_t pad[63];
};

struct CutParams {
  const uint64_t* key_off;
  const uint64_t* val_off;  // may be null
  uint64_t cap_items;       // n_items of the call: the arrays' capacity
  const uint64_t* d_n;      // may be null: cap_items items
  uint64_t extra;
  uint64_t block_size;
  uint32_t* starts;
  uint64_t cap_blocks;
  uint64_t* n_blocks;
  int32_t* status;
  uint32_t n_tiles;
  // workspace
  CutHdr* hdr;
  uint32_t* entry1;  // [n_tiles] 1 + the item at which the chain enters the tile, 0 = it skips the tile
  uint32_t* tcnt;    // [n_tiles] blocks that start in the tile
  uint64_t* tbase;   // [n_tiles + 1] first block index of each tile
  uint32_t* jump;    // [n]
  uint32_t* link;    // [n] tile-relative next (kCutExit: leaves the tile) | cnt << 16
};

__device__ __forceinline__ uint64_t cut_n(const CutParams& P) {
  return P.d_n ? min(*P.d_n, P.cap_items) : P.cap_items;
}
__device__ __forceinline__ uint64_t cut_prefix(const CutParams& P, uint64_t i) {
  return gload(P.key_off, i) + (P.val_off ? gload(P.val_off, i) : 0) + P.extra * i;
}

// next(i): the least j in (i, n] with P[j] - P[i] >= block_size, n if there is none.
// Any offsets give i < next(i) <= n, and only entries 0 .. n are read.
__device__ __forceinline__ uint64_t cut_next(const CutParams& P, uint64_t i, uint64_t n) {
  const uint64_t base = cut_prefix(P, i);
  uint64_t lo = i, hi, d = 1;  // lo: not reached (or i itself); hi: reached (or n)
  for (;;) {
    hi = i + d;
    if (hi >= n) {
      hi = n;
      break;
    }
    if (cut_prefix(P, hi) - base >= P.block_size) break;
    lo = hi;
    d <<= 1;
  }
  while (hi - lo > 1) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (cut_prefix(P, mid) - base >= P.block_size) hi = mid;
    else lo = mid;
  }
  return hi;
}

__global__ __launch_bounds__(kCutThreads) void cut_tile_kernel(CutParams P) {
  __shared__ uint32_t tab[kCutTile];  // root-ward link | hops to it << 16
  const uint64_t n = cut_n(P);
  const uint64_t base = (uint64_t)blockIdx.x * kCutTile;
  if (base >= n) return;
  const uint32_t cnt = (uint32_t)min((uint64_t)kCutTile, n - base);
  const uint64_t end = base + cnt;
  bool bad = false;
  for (uint32_t r = threadIdx.x; r < cnt; r += kCutThreads) {
    const uint64_t i = base + r;
    bad |= gload(P.key_off, i + 1) < gload(P.key_off, i);
    if (P.val_off) bad |= gload(P.val_off, i + 1) < gload(P.val_off, i);
    const uint64_t nx = cut_next(P, i, n);
    gstore(P.jump, i, (uint32_t)nx);
    // an item whose block leaves the tile is a root: it links to itself
    tab[r] = nx < end ? (uint32_t)(nx - base) | (1u << 16) : r;
  }
  if (bad) P.hdr->bad = 1;
  __syncthreads();
  // Pointer doubling in place: an entry always names an ancestor and the hops to
  // it (one u32, read and written whole), so reading an entry that another thread
  // has already advanced only gets further; a barrier per round bounds the rounds.
  for (uint32_t round = 0; round < kCutTileLog2; ++round) {
    for (uint32_t r = threadIdx.x; r < cnt; r += kCutThreads) {
      const uint32_t a = tab[r], p = a & 0xFFFF;
      if (p != r) {
        const uint32_t b = tab[p];
        tab[r] = (b & 0xFFFF) | (((a >> 16) + (b >> 16)) << 16);
      }
    }
    __syncthreads();
  }
  // jump of a root is its own next (written above, never rewritten); the others copy their root's
  for (uint32_t r = threadIdx.x; r < cnt; r += kCutThreads) {
    const uint64_t i = base + r;
    const uint32_t a = tab[r], root = a & 0xFFFF;
    const uint32_t own = gload(P.jump, i);
    const uint32_t rel = own < end ? (uint32_t)(own - base) : kCutExit;
    gstore(P.link, i, rel | (((a >> 16) + 1) << 16));
    if (root != r) gstore(P.jump, i, gload(P.jump, base + root));
  }
}

__global__ __launch_bounds__(64) void cut_walk_kernel(CutParams P) {
  if (threadIdx.x != 0) return;
  P.starts[0] = 0;
  if (P.hdr->bad) return;
  const uint64_t n = cut_n(P);
  uint64_t s = 0;
  while (s < n) {
    const uint32_t t = (uint32_t)(s / kCutTile);
    const uint32_t j = gload(P.jump, s);
    const uint32_t l = gload(P.link, s);
    P.entry1[t] = (uint32_t)s + 1;
    P.tcnt[t] = l >> 16;
    if (j <= s) break;  // (cut_tile_kernel wrote jump[s] >= the tile's end)
    s = j;
  }
}

struct CutOut {  // scan of the tiles' block counts
  CutParams P;
  __device__ void operator()(uint64_t t, uint64_t prefix) const {
    P.tbase[t] = prefix;
    if (t != P.n_tiles) return;
    const bool bad = P.hdr->bad != 0;
    *P.n_blocks = bad ? 0 : prefix;
    *P.status = bad ? LSM_BAD_ARG : prefix > P.cap_blocks ? LSM_OVERFLOW : LSM_OK;
    if (!bad && prefix <= P.cap_blocks) P.starts[prefix] = (uint32_t)cut_n(P);
  }
};

__global__ __launch_bounds__(kCutEmitThreads) void cut_emit_kernel(CutParams P) {
  __shared__ uint32_t tab[kCutTile];
  const uint32_t e1 = P.entry1[blockIdx.x];
  if (e1 == 0) return;
  const uint64_t n = cut_n(P);
  const uint64_t base = (uint64_t)blockIdx.x * kCutTile;
  const uint32_t cnt = (uint32_t)min((uint64_t)kCutTile, n - base);
  uint32_t r = (uint32_t)(e1 - 1 - base);
  for (uint32_t x = r + threadIdx.x; x < cnt; x += kCutEmitThreads) tab[x] = gload(P.link, base + x);
  __syncthreads();
  if (threadIdx.x != 0) return;
  uint64_t k = P.tbase[blockIdx.x];
  const uint32_t blocks = tab[r] >> 16;
  for (uint32_t c = 0; c < blocks && k <= P.cap_blocks; ++c, ++k) {
    gstore(P.starts, k, (uint32_t)(base + r));
    const uint32_t nr = tab[r] & 0xFFFF;
    if (nr <= r || nr >= cnt) break;  // the tile's last block (kCutExit)
    r = nr;
  }
}

struct CutWorkspace {
  size_t hdr, entry1, tcnt, clear_end, tbase, tiles, jump, link, total;
  uint32_t n_tiles;
  explicit CutWorkspace(uint64_t n_items) {
    const uint64_t n = n_items ? n_items : 1;
    n_tiles = (uint32_t)((n + kCutTile - 1) / kCutTile);
    Carver c;
    hdr = c.take(sizeof(CutHdr));
    entry1 = c.take((uint64_t)n_tiles * 4);
    tcnt = c.take((uint64_t)n_tiles * 4);
    clear_end = c.total();  // hdr, entry1 and tcnt are cleared by every call
    tbase = c.take(((uint64_t)n_tiles + 1) * 8);
    tiles = c.take(scan_tiles(n_tiles) * 8);
    jump = c.take(n * 4);
    link = c.take(n * 4);
    total = c.total();
  }
};

// ------------------------------------------------------------ index entries
constexpr uint32_t kIdxWaves = 4;

struct IdxParams {
  const uint8_t* keys;
  const uint64_t* key_off;
  const uint64_t* seqno;
  uint64_t n_items;
  const uint32_t* starts;
  const uint64_t* block_off;
  uint32_t n_blocks;
  uint64_t base_offset;
  uint8_t* out_keys;
  uint64_t key_cap;
  uint64_t* out_key_off;
  uint64_t* out_seqno;
  uint64_t* out_handle_off;
  uint32_t* out_handle_size;
  int32_t* result;
  uint32_t* lens;  // workspace [n_blocks]
};

// The last item of block b, or n_items when the start array does not name one.
__device__ __forceinline__ uint64_t idx_last_item(const IdxParams& P, uint32_t b) {
  const uint64_t e = gload(P.starts, (uint64_t)b + 1);
  return e >= 1 && e <= P.n_items ? e - 1 : P.n_items;
}

__global__ __launch_bounds__(256) void index_lens_kernel(IdxParams P) {
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b >= P.n_blocks) return;
  const uint64_t j = idx_last_item(P, b);
  gstore(P.lens, b, j < P.n_items ? (uint32_t)(gload(P.key_off, j + 1) - gload(P.key_off, j)) : 0u);
}

struct IdxOffOut {
  uint64_t* off;
  __device__ void operator()(uint64_t b, uint64_t prefix) const { off[b] = prefix; }
};

__global__ __launch_bounds__(kIdxWaves * 64) void index_gather_kernel(IdxParams P) {
  __shared__ __attribute__((aligned(16))) uint8_t buf[kIdxWaves][kGatherBuf + 32];
  // a capped arena: all entries or none (the caller sized it without a host sync)
  const bool fits = P.out_key_off[P.n_blocks] <= P.key_cap;
  if (blockIdx.x == 0 && threadIdx.x == 0) *P.result = fits ? LSM_OK : LSM_OVERFLOW;
  if (!fits) return;
  const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t c = ((uint64_t)blockIdx.x * kIdxWaves + w) * 64;
  if (c >= P.n_blocks) return;
  const uint64_t b = c + lane;
  const uint64_t ce = min(c + 64, (uint64_t)P.n_blocks);
  uint32_t kl = 0;
  uint64_t ko = 0;
  const uint8_t* ks = P.keys;
  if (b < P.n_blocks) {
    const uint64_t j = idx_last_item(P, (uint32_t)b);
    kl = gload(P.lens, b);
    ko = gload(P.out_key_off, b);
    const uint64_t o0 = gload(P.block_off, b), o1 = gload(P.block_off, b + 1);
    if (j < P.n_items) ks = P.keys + gload(P.key_off, j);
    gstore(P.out_seqno, b, j < P.n_items ? gload(P.seqno, j) : (uint64_t)0);
    gstore(P.out_handle_off, b, P.base_offset + o0);
    gstore(P.out_handle_size, b, (uint32_t)(o1 - o0));
  }
  gather_field(ks, kl, P.out_keys, ko, P.out_key_off[c], P.out_key_off[ce], buf[w], lane);
}

struct IdxWorkspace {
  size_t lens, tiles, total;
  explicit IdxWorkspace(uint32_t n_blocks) {
    const uint64_t n = n_blocks ? n_blocks : 1;
    Carver c;
    lens = c.take(n * 4);
    tiles = c.take(scan_tiles(n) * 8);
    total = c.total();
  }
};

}  // namespace lsmgpu

using namespace lsmgpu;

extern "C" size_t lsm_cut_workspace_size(uint64_t n_items) { return CutWorkspace(n_items).total; }

extern "C" int lsm_cut_blocks_device(const uint64_t* d_key_off, const uint64_t* d_val_off, uint64_t n_items,
                                     const uint64_t* d_n_items, uint32_t extra_per_item, uint32_t block_size,
                                     uint32_t* d_block_item_start, uint64_t cap_blocks, uint64_t* d_n_blocks,
                                     int32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream) {
  if (!d_key_off || !d_block_item_start || !d_n_blocks || !d_status || !d_workspace) return LSM_BAD_ARG;
  if (n_items > 0xFFFFFFFEULL) return LSM_BAD_ARG;
  if (cap_blocks == 0 && n_items) return LSM_BAD_ARG;
  const CutWorkspace W(n_items);
  if (workspace_bytes < W.total) return LSM_BAD_ARG;
  const hipStream_t st = (hipStream_t)stream;
  uint8_t* ws = (uint8_t*)d_workspace;
  CutParams P;
  P.key_off = d_key_off;
  P.val_off = d_val_off;
  P.cap_items = n_items;
  P.d_n = d_n_items;
  P.extra = extra_per_item;
  P.block_size = block_size;
  P.starts = d_block_item_start;
  P.cap_blocks = cap_blocks;
  P.n_blocks = d_n_blocks;
  P.status = d_status;
  P.n_tiles = W.n_tiles;
  P.hdr = (CutHdr*)(ws + W.hdr);
  P.entry1 = (uint32_t*)(ws + W.entry1);
  P.tcnt = (uint32_t*)(ws + W.tcnt);
  P.tbase = (uint64_t*)(ws + W.tbase);
  P.jump = (uint32_t*)(ws + W.jump);
  P.link = (uint32_t*)(ws + W.link);
  const char* where = "lsm_cut_blocks_device";
  // (a kernel, not a memset node: fill.hpp on memset nodes in replayed graphs)
  hipError_t e = fill_words_grid_async(ws, (uint32_t)(W.clear_end / 4), 0, st);
  if (e != hipSuccess) return hip_status(e, where);
  if (n_items) hipLaunchKernelGGL(cut_tile_kernel, dim3(W.n_tiles), dim3(kCutThreads), 0, st, P);
  hipLaunchKernelGGL(cut_walk_kernel, dim3(1), dim3(64), 0, st, P);
  e = launch_excl_scan(P.tcnt, W.n_tiles, (uint64_t*)(ws + W.tiles), CutOut{P}, st);
  if (e != hipSuccess) return hip_status(e, where);
  if (n_items) hipLaunchKernelGGL(cut_emit_kernel, dim3(W.n_tiles), dim3(kCutEmitThreads), 0, st, P);
  return hip_status(hipGetLastError(), where);
}

extern "C" size_t lsm_index_entries_workspace_size(uint32_t n_blocks) {
  return IdxWorkspace(n_blocks).total;
}

extern "C" int lsm_index_entries(const lsm_items* d_items, const uint32_t* d_block_item_start,
                                 const uint64_t* d_block_off, uint32_t n_blocks, uint64_t base_offset,
                                 uint8_t* d_out_keys, uint64_t key_cap, uint64_t* d_out_key_off,
                                 uint64_t* d_out_seqno, uint64_t* d_out_handle_off, uint32_t* d_out_handle_size,
                                 int32_t* d_result, void* d_workspace, size_t workspace_bytes, void* stream) {
  if (!d_items || !d_out_key_off || !d_result) return LSM_BAD_ARG;
  const hipStream_t st = (hipStream_t)stream;
  const char* where = "lsm_index_entries";
  if (n_blocks == 0) {  // no entry: the first offset and LSM_OK (= 0)
    hipError_t e = fill_words_async(d_out_key_off, 2, 0, st);
    if (e == hipSuccess) e = fill_words_async(d_result, 1, 0, st);
    return hip_status(e, where);
  }
  if (!d_items->keys || !d_items->key_off || !d_items->seqno || !d_block_item_start || !d_block_off || !d_out_keys ||
      !d_out_seqno || !d_out_handle_off || !d_out_handle_size || !d_workspace)
    return LSM_BAD_ARG;
  if (workspace_bytes < lsm_index_entries_workspace_size(n_blocks)) return LSM_BAD_ARG;
  IdxParams P;
  P.keys = d_items->keys;
  P.key_off = d_items->key_off;
  P.seqno = d_items->seqno;
  P.n_items = d_items->n_items;
  P.starts = d_block_item_start;
  P.block_off = d_block_off;
  P.n_blocks = n_blocks;
  P.base_offset = base_offset;
  P.out_keys = d_out_keys;
  P.key_cap = key_cap;
  P.out_key_off = d_out_key_off;
  P.out_seqno = d_out_seqno;
  P.out_handle_off = d_out_handle_off;
  P.out_handle_size = d_out_handle_size;
  P.result = d_result;
  const IdxWorkspace W(n_blocks);
  P.lens = (uint32_t*)((uint8_t*)d_workspace + W.lens);
  uint64_t* tiles = (uint64_t*)((uint8_t*)d_workspace + W.tiles);
  hipLaunchKernelGGL(index_lens_kernel, dim3((n_blocks + 255) / 256), dim3(256), 0, st, P);
  const hipError_t e = launch_excl_scan(P.lens, n_blocks, tiles, IdxOffOut{d_out_key_off}, st);
  if (e != hipSuccess) return hip_status(e, where);
  hipLaunchKernelGGL(index_gather_kernel, dim3((n_blocks + kIdxWaves * 64 - 1) / (kIdxWaves * 64)),
                     dim3(kIdxWaves * 64), 0, st, P);
  return hip_status(hipGetLastError(), where);
}
