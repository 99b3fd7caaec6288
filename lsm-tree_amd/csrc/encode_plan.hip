// encode_plan.hip — the plan stage of the encode path (E1, E1p, the size scan); see encode.hip.
#include "encode_plan.hpp"

namespace lsmgpu {

// ---------------------------------------------------------------- E1: plan
// A 256-thread workgroup owns kPlanBlocks consecutive blocks and walks their
// items (contiguous) in chunks of 1024, four consecutive items per thread, so
// each wave has four items' loads in flight at once.  Per chunk:
//   1. item fields (key / value offsets, seqno, type); key offsets to LDS;
//   2. the shared prefix with the restart head (encoder.rs:140-143,
//      util.rs:125-130): the head's key offset from LDS (global only for a
//      head before the chunk), both keys' first 16 bytes as two aligned 16-B
//      loads each, all four items' loads issued together (longer equal
//      prefixes continue in lcp_global);
//   3. record lengths, a workgroup scan in item order -> each record's offset
//      in its block, kept for E2 in erec.
// Per block: size, binary-index step, hash-index size, size class, and the
// key / value span starts E2 stages.
constexpr uint32_t kPlanPer = 2;          // consecutive items per thread
constexpr uint32_t kPlanChunk = 256 * kPlanPer;      // items per chunk

template <bool kIndex>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1))) void encode_plan_kernel(EncodeParams P) {
  __shared__ uint32_t bst[kPlanBlocks + 1];
  __shared__ unsigned long long bfirst[kPlanBlocks], bend[kPlanBlocks], lhead[kPlanBlocks];
  __shared__ unsigned long long psum[4];
  __shared__ uint32_t badf[kPlanBlocks];
  __shared__ uint32_t mono;
  __shared__ unsigned long long kos[kPlanChunk + 1];  // key offsets of the chunk's items (+ the next)
  const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const uint32_t b0 = blockIdx.x * P.plan_bpw;
  const uint32_t nb = min(P.plan_bpw, P.n_blocks - b0);
  if (tid <= nb) bst[tid] = clamped_start(P, b0 + tid);
  if (tid < nb) {
    bfirst[tid] = bend[tid] = lhead[tid] = 0;
    badf[tid] = 0;
  }
  if (tid == 0) mono = 1;
  __syncthreads();
  if (tid < nb && bst[tid + 1] < bst[tid]) mono = 0;  // (benign race: every writer stores 0)
  __syncthreads();
  const uint32_t ri = kIndex ? 1 : P.ri;
  constexpr bool index = kIndex;
  // a non-monotone item_start run is a caller error: its blocks are rejected below
  // (wave-uniform: chunk bases stay in SGPRs, so item loads take the saddr form)
  const uint64_t i_begin = (uint32_t)__builtin_amdgcn_readfirstlane(bst[0]);
  const uint64_t i_end = (uint32_t)__builtin_amdgcn_readfirstlane(mono ? bst[nb] : bst[0]);
  uint64_t carry = 0;
  for (uint64_t base = i_begin; base < i_end; base += kPlanChunk) {
    const uint64_t i0 = base + kPlanPer * tid;
    // ---- 1. item fields, block of each item
    RawItem raw[kPlanPer];
#pragma unroll
    for (uint32_t q = 0; q < kPlanPer; ++q)
      raw[q] = load_raw_rel<kIndex>(P, base, (uint32_t)min(i0 + q, i_end - 1) - (uint32_t)base);
    ItemMeta m[kPlanPer];
    uint32_t jq[kPlanPer], jjq[kPlanPer];
    uint32_t j = 0;
    if (i0 < i_end) {
      uint32_t lo = 0, hi = nb;  // block j: bst[j] <= i0 < bst[j + 1]
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (bst[mid] <= i0) lo = mid;
        else hi = mid;
      }
      j = lo;
    }
#pragma unroll
    for (uint32_t q = 0; q < kPlanPer; ++q) {
      const uint64_t i = i0 + q;
      jq[q] = jjq[q] = 0;
      if (i < i_end) {
        while (j + 1 < nb && bst[j + 1] <= i) ++j;
        jq[q] = j;
        jjq[q] = (uint32_t)(i - bst[j]);
      }
    }
#pragma unroll
    for (uint32_t q = 0; q < kPlanPer; ++q) {
      bool bad = false;
      m[q] = cook_item<kIndex>(raw[q], bad);
      if (i0 + q < i_end) {
        if (bad) atomicOr(&badf[jq[q]], 1u);
        kos[kPlanPer * tid + q] = m[q].ko;
      }
    }
    __syncthreads();
    // ---- 2. shared prefix with the restart head
    if (!index) {
      Win16 wa[kPlanPer], wb[kPlanPer];
      uint32_t nq[kPlanPer];
      uint64_t hq[kPlanPer];
#pragma unroll
      for (uint32_t q = 0; q < kPlanPer; ++q) {
        const uint64_t i = i0 + q;
        nq[q] = 0;
        hq[q] = 0;
        if (i < i_end && jjq[q] % ri != 0) {
          const uint64_t h = i - jjq[q] % ri;  // restart head of item i
          const uint64_t hko = h >= base ? kos[h - base] : koff(P, h);
          const uint64_t hke = h + 1 >= base ? kos[h + 1 - base] : koff(P, h + 1);
          const uint32_t hkl = (uint32_t)min(hke - hko, (uint64_t)0xFFFF);
          nq[q] = min(hkl, m[q].klen);
          hq[q] = hko;
          wa[q] = gwin16(P.it.keys + hko);
          wb[q] = gwin16(P.it.keys + m[q].ko);
        }
      }
#pragma unroll
      for (uint32_t q = 0; q < kPlanPer; ++q) {
        if (!nq[q]) continue;
        const uint64_t x0 = wa[q].lo ^ wb[q].lo, x1 = wa[q].hi ^ wb[q].hi;
        const uint32_t n = nq[q];
        uint32_t sh;
        if (x0) sh = min(n, (uint32_t)(__builtin_ctzll(x0) >> 3));
        else if (x1) sh = min(n, 8 + (uint32_t)(__builtin_ctzll(x1) >> 3));
        else sh = n <= 16 ? n : lcp_tail(P.it.keys, hq[q], m[q].ko, n);
        m[q].sh = sh;
      }
    }
    // ---- 3. record lengths, workgroup scan in item order
    uint64_t rec[kPlanPer], tsum = 0;
#pragma unroll
    for (uint32_t q = 0; q < kPlanPer; ++q) {
      rec[q] = 0;
      if (i0 + q < i_end) rec[q] = item_record_len(P, m[q], jjq[q] % ri == 0);
      tsum += rec[q];
    }
    const uint64_t incl = wave_incl_scan_u64(tsum);
    if (lane == kWave - 1) psum[wave] = incl;
    __syncthreads();
    uint64_t wbase = 0, ptot = 0;
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) {
      const uint64_t v = psum[w];
      wbase += w < wave ? v : 0;
      ptot += v;
    }
    uint64_t ex = carry + wbase + incl - tsum;
    uint64_t exq[kPlanPer];
#pragma unroll
    for (uint32_t q = 0; q < kPlanPer; ++q) {
      exq[q] = ex;
      if (i0 + q < i_end) {
        const uint32_t jb = jq[q], jj = jjq[q], ridx = jj / ri;
        const uint32_t n = bst[jb + 1] - bst[jb];
        if (jj == 0) bfirst[jb] = ex;
        if (jj + 1 == n) bend[jb] = ex + rec[q];
        if (jj == ridx * ri && ridx == (n - 1) / ri) lhead[jb] = ex;
      }
      ex += rec[q];
    }
    __syncthreads();  // (also orders this chunk's psum / kos reads before the next chunk's writes)
#pragma unroll
    for (uint32_t q = 0; q < kPlanPer; ++q) {
      if (i0 + q < i_end) {
        const uint32_t jj = jjq[q], ridx = jj / ri;
        const bool head = jj == ridx * ri;
        const uint64_t roff = exq[q] - bfirst[jq[q]];
        const uint32_t x = head ? ridx : m[q].sh;
        // blocks of more than kGItems items are never group-class: their items
        // keep the whole 32-bit record offset, for E3
        P.erec[i0 + q] = bst[jq[q] + 1] - bst[jq[q]] > kGItems ? (uint32_t)min(roff, (uint64_t)0xFFFFFFFFu)
                                     : (uint32_t)min(roff, (uint64_t)0x7FFF) | (head ? kErecHead : 0u) |
                                           (min(x, 0xFFFFu) << 16);
      }
    }
    carry += ptot;
  }
  __syncthreads();
  if (tid >= nb) return;
  const uint32_t b = b0 + tid, s = bst[tid], e = bst[tid + 1];
  const bool bad = !mono || e <= s || badf[tid] || start_past_items(P, b + 1);
  const uint64_t ks = koff(P, s), ke = koff(P, e);
  const uint64_t vs = kIndex ? 0 : voff(P, s), ve = kIndex ? 0 : voff(P, e);
  BlockPlan pl;
  P.sizes[b] =
      plan_block<kIndex>(P, b, s, e, bad, bend[tid] - bfirst[tid], lhead[tid] - bfirst[tid], ks, ke, vs, ve, pl);
  P.kspan[b] = ks;
  P.vspan[b] = vs;
  if (b + 1 == P.n_blocks) {
    P.kspan[b + 1] = ke;
    P.vspan[b + 1] = ve;
  }
}

template <bool kBkt, int kOW>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void encode_plan_wave_kernel(EncodeParams P) {
  __shared__ PlanWaveLds S;
  const uint32_t b0 = blockIdx.x * P.plan_bpw;
  plan_wave_run<kBkt, kOW, false>(P, b0, min(P.plan_bpw, P.n_blocks - b0), S, nullptr, nullptr);
}

// ---------------------------------------- E1p: the plan of huge-block batches
// Blocks of ~4 Ki items and more on average (the writer's 1-4 MiB data blocks,
// writer/mod.rs:193-198) leave encode_plan_kernel one workgroup per one to four
// blocks, walking 512-item chunks one after another (60 workgroups for 60 blocks
// of 4 MiB: 0.21 ms for 240 x 1 MiB).  E1p computes the same outputs item-parallel:
//   lengths  thread per item: fields, shared prefix with its restart head
//            (encoder.rs:140-143), record length -> erec (for now), shared
//            length -> hbucket (unused by these batches' E2), per-block exact
//            record totals and bad flags (wave-segmented sums: a block's total,
//            or the parts at a wave's two ends)
//   scan     the device scan over every item's record length, in place (low
//            32 bits: a block's offsets are differences of two prefixes)
//   blocks   wave per block: its total from the wave parts, then plan_block
//   offsets  thread per item: erec = prefix - its block's first prefix (the
//            packed word for blocks of <= kGItems items); huge blocks keep the
//            prefix (their writers subtract pfirst)
// A non-monotone item_start array rejects every block (the one-workgroup
// plan rejects the run of blocks its workgroup holds).
__device__ __forceinline__ uint32_t block_of_item(const EncodeParams& P, uint32_t i) {
  uint32_t lo = 0, hi = P.n_blocks;  // last b < n_blocks with start[b] <= i
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (clamped_start(P, mid) <= i) lo = mid;
    else hi = mid;
  }
  return lo;
}

constexpr uint64_t kE1pBad = 1ULL << 63;
// Sum of two (record bytes | bad flag) words.
__device__ __forceinline__ uint64_t e1p_add(uint64_t a, uint64_t b) {
  return ((a | b) & kE1pBad) | ((a + b) & ~kE1pBad);
}

__device__ __forceinline__ uint64_t shfl_down64(uint64_t v, int o) {
  return (uint64_t)(uint32_t)__shfl_down((int)(uint32_t)v, o) |
         ((uint64_t)(uint32_t)__shfl_down((int)(uint32_t)(v >> 32), o) << 32);
}

// Items per thread in the item-parallel E1p kernels (strided by 256: each pass
// of a workgroup is 256 consecutive items); the four items' loads are issued
// together, and a workgroup's block search serves 1024 items.
constexpr uint32_t kE1pPer = 4;
constexpr uint32_t kE1pLenPer = 1;  // (the lengths kernel: 4 items took 136 VGPRs, 2 ran as 1)

// The block holding item `first` (the workgroup's first item), by a 256-way
// search of the starts (every thread one sample per round: one round for
// batches of <= 256 blocks; a thread-0 binary search was eight dependent loads
// before any item load of the workgroup).  Every thread calls it (a barrier).
__device__ __forceinline__ uint32_t wg_first_block(const EncodeParams& P, uint32_t first) {
  const uint32_t i_end = clamped_start(P, P.n_blocks);
  uint32_t lo = 0, hi = P.n_blocks;  // last b in [lo, hi) with start[b] <= first
  if (first >= i_end) hi = 1;       // (no item of the batch here: block 0, unused)
  while (hi - lo > 1) {             // (uniform)
    const uint32_t st = (hi - lo + 255) / 256;
    const uint32_t x = lo + threadIdx.x * st;
    const uint32_t c = (uint32_t)__syncthreads_count(x < hi && clamped_start(P, x) <= first);
    const uint32_t nlo = lo + (c ? c - 1 : 0) * st;  // (c = 0 only for a non-monotone array: rejected anyway)
    hi = min(hi, nlo + st);
    lo = nlo;
  }
  return lo;
}

// This thread's kE1pPer items (base + 256 j + tid): each one's block and range,
// walking forward from the workgroup's first block (blocks of >= 4 Ki items on
// average: a step or two at most).
template <uint32_t K>
struct E1pItems {
  uint32_t i[K], b[K], s[K], e[K];
  bool in[K];
};
template <uint32_t K>
__device__ __forceinline__ E1pItems<K> e1p_items(const EncodeParams& P) {
  E1pItems<K> t;
  const uint32_t i_begin = clamped_start(P, 0), i_end = clamped_start(P, P.n_blocks);
  const uint32_t base = blockIdx.x * (256 * K);
  uint32_t b = wg_first_block(P, max(base, i_begin));
  uint32_t bs = clamped_start(P, b), be = clamped_start(P, b + 1);
#pragma unroll
  for (uint32_t j = 0; j < K; ++j) {
    const uint32_t i = base + 256 * j + threadIdx.x;
    const bool in = i >= i_begin && i < i_end && (uint64_t)i < P.it.n_items;
    while (in && b + 1 < P.n_blocks && be <= i) {
      ++b;
      bs = be;
      be = clamped_start(P, b + 1);
    }
    t.i[j] = i;
    t.b[j] = b;
    t.s[j] = bs;
    t.e[j] = be;
    t.in[j] = in;
  }
  return t;
}

template <int kOW>
__global__ __launch_bounds__(256) void encode_e1p_lengths_kernel(EncodeParams P) {
  if (blockIdx.x == 0) {  // the starts' monotonicity over every block, the flag written whole (no prior clear)
    int bad = 0;
    for (uint32_t x = threadIdx.x; x < P.n_blocks; x += 256)
      bad |= clamped_start(P, x + 1) < clamped_start(P, x) ? 1 : 0;
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) {
      P.e1p_flag[0] = bad ? 1u : 0u;
      if (P.huge_pool) reinterpret_cast<uint32_t*>(P.huge_pool)[kEncHugeCountWord] = 0;  // (the size scan counts into it)
    }
  }
  const E1pItems<kE1pLenPer> T = e1p_items<kE1pLenPer>(P);
  const uint32_t ri = P.ri, lane = threadIdx.x & 63;
  bool live[kE1pLenPer], head[kE1pLenPer];
  RawItemT<kOW> r[kE1pLenPer];
  uint64_t hko[kE1pLenPer], hko1[kE1pLenPer];
#pragma unroll
  for (uint32_t j = 0; j < kE1pLenPer; ++j) {  // every item's loads first
    const uint32_t i = T.i[j];
    live[j] = T.in[j] && T.s[j] <= i && i < T.e[j];  // (not, for a non-monotone array: every block is rejected)
    head[j] = (i - T.s[j]) % ri == 0;
    hko[j] = hko1[j] = 0;
    if (live[j]) {
      r[j] = load_raw<false, kOW>(P, i);
      if (!head[j]) {
        const uint64_t h = (uint64_t)i - (i - T.s[j]) % ri;
        hko[j] = koff<kOW>(P, h);
        hko1[j] = koff<kOW>(P, h + 1);
      }
    }
  }
  ItemMeta m[kE1pLenPer];
  bool bad[kE1pLenPer];
  Win16 wa[kE1pLenPer], wb[kE1pLenPer];
#pragma unroll
  for (uint32_t j = 0; j < kE1pLenPer; ++j) {  // then the key windows of the shared prefixes
    bad[j] = false;
    if (live[j]) {
      m[j] = cook_item<false>(r[j], bad[j]);
      if (!head[j]) {
        wa[j] = gwin16(P.it.keys + hko[j]);
        wb[j] = gwin16(P.it.keys + m[j].ko);
      }
    }
  }
#pragma unroll
  for (uint32_t j = 0; j < kE1pLenPer; ++j) {
    const uint32_t i = T.i[j];
    uint64_t rec = 0;
    if (live[j]) {
      if (!head[j]) {
        const uint32_t n = min((uint32_t)min(hko1[j] - hko[j], (uint64_t)0xFFFF), m[j].klen);
        const uint64_t x0 = wa[j].lo ^ wb[j].lo, x1 = wa[j].hi ^ wb[j].hi;
        uint32_t sh;
        if (x0) sh = min(n, (uint32_t)(__builtin_ctzll(x0) >> 3));
        else if (x1) sh = min(n, 8 + (uint32_t)(__builtin_ctzll(x1) >> 3));
        else sh = n <= 16 ? n : lcp_tail(P.it.keys, hko[j], m[j].ko, n);
        m[j].sh = sh;
        P.hbucket[i] = (uint16_t)min(sh, 0xFFFFu);
      }
      rec = item_record_len(P, m[j], head[j]);
    }
    if ((uint64_t)i < P.it.n_items) P.erec[i] = (uint32_t)min(rec, (uint64_t)0xFFFFFFFFu);
    // per-block exact totals without same-address atomics (a 4-MiB block's ~800
    // waves would serialise on one word): lanes of one block summed first (blocks
    // are runs of lanes); a block inside this wave stores its total, one that began
    // in an earlier wave its part as this wave's head, one that goes on past this
    // wave its part as this wave's tail (encode_e1p_blocks_kernel adds them up)
    const uint32_t b = T.b[j], s = T.s[j], e = T.e[j];
    const uint32_t bb = live[j] ? b : 0xFFFFFFFFu;
    uint64_t sum = rec | (bad[j] ? kE1pBad : 0);
    for (int o = 1; o < 64; o <<= 1) {  // segmented wave reduction: run heads end with their run's total
      const uint64_t v = shfl_down64(sum, o);
      const uint32_t bo = (uint32_t)__shfl_down((int)bb, o);
      if ((int)lane + o < 64 && bo == bb) sum = e1p_add(sum, v);
    }
    const uint32_t bprev = (uint32_t)__shfl_up((int)bb, 1);
    if (live[j] && (lane == 0 || bprev != bb)) {
      const uint32_t w0 = i - lane;
      if (s >= w0 && e - w0 <= 64) P.sizes[b] = sum;
      else if (s < w0) P.wpart[2 * (uint64_t)(w0 / 64)] = sum;
      else P.wpart[2 * (uint64_t)(w0 / 64) + 1] = sum;
    }
  }
}

// Scan output: each item's record prefix (low 32 bits) in place; the total in pfirst[n_blocks].
struct E1pOut {
  uint32_t* erec;
  uint32_t* total;
  uint64_t n;
  __device__ void operator()(uint64_t i, uint64_t prefix) const {
    if (i < n) erec[i] = (uint32_t)prefix;
    else *total = (uint32_t)prefix;
  }
};

__device__ __forceinline__ uint32_t e1p_prefix(const EncodeParams& P, uint32_t i) {
  return (uint64_t)i < P.it.n_items ? P.erec[i] : P.pfirst[P.n_blocks];
}

// Wave per block: its record total from the lengths kernel's per-wave parts,
// then the plan (plan_block) on lane 0.
__global__ __launch_bounds__(256) void encode_e1p_blocks_kernel(EncodeParams P) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t bq = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / 64;
  if (bq >= P.n_blocks) return;  // (wave-uniform)
  const uint32_t b = (uint32_t)bq;
  const uint32_t ri = P.ri;
  const uint32_t s = clamped_start(P, b), e = clamped_start(P, b + 1);
  uint64_t acc = 0;
  if (e > s && !P.e1p_flag[0]) {
    const uint32_t ws = s / 64, we = (e - 1) / 64;
    if (ws == we) {
      acc = P.sizes[b];
    } else {
      uint64_t x = lane == 0 ? P.wpart[2 * (uint64_t)ws + 1] : 0;
      for (uint64_t w = (uint64_t)ws + 1 + lane; w <= we; w += 64) x = e1p_add(x, P.wpart[2 * w]);
      for (int o = 32; o; o >>= 1) x = e1p_add(x, shfl_xor64(x, o));
      acc = x;
    }
  }
  if (lane) return;
  const bool bad = P.e1p_flag[0] || e <= s || (acc & kE1pBad) || start_past_items(P, b + 1);
  const uint32_t p_s = bad ? 0 : e1p_prefix(P, s);
  P.pfirst[b] = p_s;
  // (the last restart head: item ((n - 1) / ri) * ri of the block)
  const uint64_t last_head = bad ? 0 : (uint32_t)(e1p_prefix(P, s + (e - s - 1) / ri * ri) - p_s);
  const uint64_t ks = koff(P, s), ke = koff(P, e);
  const uint64_t vs = voff(P, s), ve = voff(P, e);
  BlockPlan pl;
  P.sizes[b] = plan_block<false>(P, b, s, e, bad, acc & ~kE1pBad, last_head, ks, ke, vs, ve, pl);
  P.kspan[b] = ks;
  P.vspan[b] = vs;
  if (b + 1 == P.n_blocks) {
    P.kspan[b + 1] = ke;
    P.vspan[b + 1] = ve;
  }
}

__global__ __launch_bounds__(256) void encode_e1p_offsets_kernel(EncodeParams P) {
  const E1pItems<kE1pPer> T = e1p_items<kE1pPer>(P);
  if (P.e1p_flag[0]) return;
  const uint32_t ri = P.ri;
  // (huge blocks keep the record prefix in erec: their writers subtract the block's first
  // prefix themselves, so their items, nearly all of such a batch, cost only the flag load here)
  uint32_t fl[kE1pPer], er[kE1pPer], pf[kE1pPer], hb[kE1pPer];
  bool cv[kE1pPer];
#pragma unroll
  for (uint32_t j = 0; j < kE1pPer; ++j) fl[j] = T.in[j] ? gload_pod(P.plans, T.b[j]).step_flags : 0;
#pragma unroll
  for (uint32_t j = 0; j < kE1pPer; ++j) {  // every converted item's loads first
    er[j] = pf[j] = hb[j] = 0;
    cv[j] = T.in[j] && !((fl[j] >> 8) & kPlanBad) && (fl[j] >> 8) != kPlanHuge;
    if (cv[j]) {
      er[j] = gload(P.erec, T.i[j]);
      pf[j] = gload(P.pfirst, T.b[j]);
      hb[j] = gload(P.hbucket, T.i[j]);
    }
  }
#pragma unroll
  for (uint32_t j = 0; j < kE1pPer; ++j) {
    if (!cv[j]) continue;
    const uint32_t n = T.e[j] - T.s[j], roff = er[j] - pf[j], jj = T.i[j] - T.s[j];
    const bool head = jj % ri == 0;
    const uint32_t x = head ? jj / ri : hb[j];
    P.erec[T.i[j]] = n > kGItems ? roff : min(roff, 0x7FFFu) | (head ? kErecHead : 0u) | (min(x, 0xFFFFu) << 16);
  }
}

// The size scan's outputs: block offsets (low 40 bits of the prefix) and the
// list of the listed blocks (high bits = their running count); with the pool,
// the huge blocks are also collected (hdr->count) for the whole-GPU E3.
struct EncodeOffOut {
  uint64_t* off;
  const uint64_t* sizes;
  uint32_t* list;
  uint32_t* count;
  uint64_t n;
  const BlockPlan* plans;
  uint32_t* huge_count;  // null: no pool
  uint32_t* huge_list;
  uint32_t huge_cap;
};

// The size scan's apply pass (scan_tile_apply's shape, the outputs above): a
// thread's kScanPerThread sizes, and for its listed blocks their plan flags,
// are all read before the scan; the huge blocks take their list slots from one
// atomic per wave (a per-block atomic on one counter serialised a batch of 240
// huge blocks at 7.8 us).
__global__ __launch_bounds__(kScanThreads) void encode_offsets_apply_kernel(const uint64_t* __restrict__ tile_offsets,
                                                                            EncodeOffOut o) {
  __shared__ uint64_t sh[kScanThreads / 64];
  const uint64_t n = o.n;
  const uint64_t base = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanPerThread;
  const uint32_t lane = threadIdx.x & (kWave - 1);
  uint64_t v[kScanPerThread];
  scan_load(o.sizes, base, n, v);
  bool huge[kScanPerThread];
  uint32_t hc = 0;
  uint64_t s = 0;
#pragma unroll
  for (int i = 0; i < kScanPerThread; ++i) {
    huge[i] = o.huge_count && base + i < n && (v[i] & ~kOffMask) &&
              (o.plans[base + i].step_flags >> 8) == kPlanHuge;
    hc += huge[i] ? 1u : 0u;
    s += v[i];
  }
  uint64_t total;
  uint64_t ex = block_excl_scan_u64(s, sh, total) + (tile_offsets ? tile_offsets[blockIdx.x] : 0);
  uint32_t slot = 0;
  if (o.huge_count) {  // (uniform)
    const uint32_t incl = wave_incl_scan_u32(hc);
    const uint32_t wtot = (uint32_t)__shfl((int)incl, kWave - 1);
    uint32_t wb = 0;
    if (lane == 0 && wtot) wb = atomicAdd(o.huge_count, wtot);
    slot = (uint32_t)__shfl((int)wb, 0) + incl - hc;
  }
#pragma unroll
  for (int i = 0; i < kScanPerThread; ++i) {
    const uint64_t k = base + i;
    if (k < n) {
      o.off[k] = ex & kOffMask;
      if (v[i] & ~kOffMask) o.list[ex >> 40] = (uint32_t)k;
      if (huge[i]) {
        if (slot < o.huge_cap) o.huge_list[slot] = (uint32_t)k;
        ++slot;
      }
    }
    if (k == n - 1) {
      o.off[n] = (ex + v[i]) & kOffMask;
      *o.count = (uint32_t)((ex + v[i]) >> 40);
    }
    ex += v[i];
  }
}

hipError_t launch_encode_plan(EncodeParams& P, bool e1p, bool fused, uint64_t* tiles, hipStream_t st) {
  hipError_t e;
  const uint64_t n_items = P.it.n_items;
  const uint32_t n_blocks = P.n_blocks;
  const dim3 pgrid((n_blocks + P.plan_bpw - 1) / P.plan_bpw);
  P.hb_valid = 0;
  P.hb_sh = 0;
  if (fused) {  // the look-back words (P.sizes, unused by this path) start cleared
    if ((e = fill_words_grid_async(P.sizes, 2 * ((n_blocks + kGRunFused - 1) / kGRunFused), 0, st)) != hipSuccess)
      return e;
  } else if (e1p) {  // batches of huge blocks: the plan item-parallel
    P.hb_sh = 1;
    const dim3 igrid((uint32_t)((n_items + 256 * kE1pPer - 1) / (256 * kE1pPer)));
    const dim3 lgrid((uint32_t)((n_items + 256 * kE1pLenPer - 1) / (256 * kE1pLenPer)));
    by_offset_width(P, [&](auto w) {
      hipLaunchKernelGGL(encode_e1p_lengths_kernel<decltype(w)::value>, lgrid, dim3(256), 0, st, P);
    });
    if ((e = launch_excl_scan(P.erec, n_items, tiles, E1pOut{P.erec, P.pfirst + n_blocks, n_items}, st)) != hipSuccess)
      return e;
    hipLaunchKernelGGL(encode_e1p_blocks_kernel, dim3((uint32_t)(((uint64_t)n_blocks + 3) / 4)), dim3(256), 0, st, P);
    hipLaunchKernelGGL(encode_e1p_offsets_kernel, igrid, dim3(256), 0, st, P);
  } else if (P.type == 1) {
    hipLaunchKernelGGL(encode_plan_kernel<true>, pgrid, dim3(256), 0, st, P);
  } else if (P.plan_bpw >= 16) {
    // (the wave kernel gives each wave whole blocks: with a few blocks of many items
    // per workgroup most waves would idle, so those batches keep the workgroup walk)
    if (P.ratio > 0.0f) {  // (only this plan kernel fills hbucket)
      P.hb_valid = 1;
      if ((e = fill_words_async(P.hb_fix, 1, 0, st)) != hipSuccess) return e;
      by_offset_width(P, [&](auto w) {
        hipLaunchKernelGGL((encode_plan_wave_kernel<true, decltype(w)::value>), pgrid, dim3(256), 0, st, P);
      });
      hipLaunchKernelGGL(encode_bucket_fixup_kernel, dim3(1024), dim3(256), 0, st, P);
    } else {
      by_offset_width(P, [&](auto w) {
        hipLaunchKernelGGL((encode_plan_wave_kernel<false, decltype(w)::value>), pgrid, dim3(256), 0, st, P);
      });
    }
  } else {
    hipLaunchKernelGGL(encode_plan_kernel<false>, pgrid, dim3(256), 0, st, P);
  }
  if (fused) return hipSuccess;  // (the group kernel's look-back gives the offsets and the list)
  EncodeOffOut oo{P.block_off, P.sizes, P.lists, P.list_count, n_blocks, P.plans, nullptr, nullptr, 0};
  if (P.huge_pool) {  // the huge blocks are collected for the whole-GPU E3
    const EncHugeLayout H = enc_huge_layout(P);
    oo.huge_count = &H.hdr->count;
    oo.huge_list = H.list;
    oo.huge_cap = P.huge_cap;
  }
  const uint64_t* offs;
  if ((e = launch_scan_tile_offsets(P.sizes, n_blocks, tiles, st, &offs)) != hipSuccess) return e;
  hipLaunchKernelGGL(encode_offsets_apply_kernel, dim3((uint32_t)scan_tiles(n_blocks)), dim3(kScanThreads), 0, st, offs,
                     oo);
  return hipSuccess;
}

}  // namespace lsmgpu
