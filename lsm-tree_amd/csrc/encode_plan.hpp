// encode_plan.hpp — the wave-level plan of a run of blocks (E1), shared by encode_plan_wave_kernel
// (encode_plan.hip) and the fused group kernel (encode_group.hip).
#pragma once

#include "encode_common.hpp"

namespace lsmgpu {

// LDS a block's image needs in E2: worst-case 16-B pad + the block + 32 B of
// read slack for the window reads, then the hash-index vote arrays.
__device__ __forceinline__ uint64_t e2_need(uint64_t total, uint32_t hash_w) {
  return ((15 + total + 15) & ~15ULL) + 32 + 8ULL * ((hash_w + 3) & ~3u);
}

// The plan of block b = items [s, e), from what its plan kernel found: `bad` (a caller error in the
// block's range or items), the bytes of its records, its last restart head's offset, and the key /
// value offsets at s and e.  Sizes the binary and the hash index, checks the limits, picks the class
// (group_fits, else by e2_need), stores P.plans[b] (and ST_BAD_ARG) and returns the block's word for
// the size scan: its bytes, 0 for a bad block, plus kListedOne (bits 40..: the scan numbers the
// listed blocks) if no group takes it.
template <bool kIndex>
__device__ __forceinline__ uint64_t plan_block(const EncodeParams& P, uint32_t b, uint32_t s, uint32_t e, bool bad,
                                               uint64_t recs, uint64_t last_head, uint64_t ks, uint64_t ke,
                                               uint64_t vs, uint64_t ve, BlockPlan& pl) {
  const uint32_t ri = kIndex ? 1 : P.ri;
  const uint32_t n = bad ? 0 : e - s;
  if (bad) recs = last_head = 0;
  const uint32_t bin_len = n ? (n + ri - 1) / ri : 0;
  const uint32_t step = last_head <= 0xFFFF ? 2 : 4;
  const uint32_t buckets = kIndex ? 0 : bucket_count(n, P.ratio);
  const uint32_t hash_w = (buckets > 0 && bin_len <= kHashMaxPointers) ? buckets : 0;
  const uint64_t total = kHdrLen + recs + 1 + (uint64_t)bin_len * step + hash_w + kTrailerLen;
  if (recs > 0xFFFFFFF0ULL || total > 0xFFFFFF00ULL) bad = true;
  uint32_t flags = 0;
  if (bad) {
    flags = kPlanBad;
    P.status[b] = ST_BAD_ARG;
  } else if (!group_fits(n, ke - ks, ve - vs, total, hash_w)) {
    const uint64_t need = e2_need(total, hash_w);
    flags = need <= kImgMedium ? kPlanMedium : need <= kImgBig ? kPlanBig : kPlanHuge;
  }
  pl = BlockPlan{(uint32_t)recs, bin_len, hash_w, step | (flags << 8)};
  P.plans[b] = pl;
  return (bad ? 0 : total) | ((flags & (kPlanMedium | kPlanBig | kPlanHuge)) ? kListedOne : 0);
}

// 16 bytes at p (global, any alignment): one unaligned 16-B load (the arenas are
// padded).  Two aligned loads and a funnel shift issued twice the loads and ~10 VALU
// more per window, and held 20 more VGPRs in the plan kernel (113 -> 93, u32 offsets):
// 1-1.5 % faster encodes (profiles/r06_experiments.txt, ab6k).
__device__ __forceinline__ Win16 gwin16(const uint8_t* p) {
  Win16 r;
  __builtin_memcpy(&r, p, 16);
  return r;
}
__device__ __forceinline__ Win16 gwin16a(const uint8_t* p) { return gwin16(p); }

// Shared prefix past an equal first 16 bytes: 16 bytes per step (rare: long
// common key prefixes; kept narrow so the common path's registers stay low).
__device__ __noinline__
uint32_t lcp_tail(const uint8_t* keys, uint64_t a, uint64_t b, uint32_t n) {
  for (uint32_t k = 16; k < n; k += 16) {
    const Win16 wa = gwin16(keys + a + k), wb = gwin16(keys + b + k);
    const uint64_t x0 = wa.lo ^ wb.lo, x1 = wa.hi ^ wb.hi;
    if (x0) return min(n, k + (uint32_t)(__builtin_ctzll(x0) >> 3));
    if (x1) return min(n, k + 8 + (uint32_t)(__builtin_ctzll(x1) >> 3));
  }
  return n;
}

// ------------------------------------- E1 for data blocks: wave-level runs
// The outputs of encode_plan_kernel<false> without workgroup barriers in the
// item loop: the workgroup's blocks are split among its four waves by item
// count (whole blocks each), and every wave walks its own items in steps of
// 128 (two consecutive items per lane).  Record offsets come from a wave scan
// plus a carry (a block never spans two waves); the shared prefix with the
// restart head (encoder.rs:140-143, util.rs:125-130) takes the head's key
// offset from the step's LDS copy, or for a head before the step from the
// carried last head; and the next step's item fields are loaded while this
// step's key windows are in flight.
constexpr uint32_t kPW = 2;  // consecutive items per lane
constexpr uint32_t kPWStep = kPW * kWave;
struct PlanWaveLds {
  uint32_t bst[kPlanBlocks + 1];
  uint32_t badf[kPlanBlocks];
  uint32_t wcut[5];
  uint32_t mono;
  unsigned long long bfirst[kPlanBlocks], bend[kPlanBlocks], lhead[kPlanBlocks];
  unsigned long long kos[4][kPWStep];
  uint32_t kls[4][kPWStep];
  Win16 kwin[4][kPWStep];  // each item's first 16 key bytes
};

// The plan of blocks [b0, b0 + nb) on one 256-thread workgroup (all threads call it).
// kFused (encode_group_kernel's run-level plan): each block's plan and size also go to
// fplan / fsize in LDS (thread j = block b0 + j), and P.sizes is not written (the fused
// kernel keeps its look-back words there).
template <bool kBkt, int kOW, bool kFused>
__device__ __forceinline__ void plan_wave_run(const EncodeParams& P, uint32_t b0, uint32_t nb, PlanWaveLds& S,
                                              BlockPlan* fplan, uint64_t* fsize) {
  uint32_t* const bst = S.bst;
  unsigned long long* const bfirst = S.bfirst;
  unsigned long long* const bend = S.bend;
  unsigned long long* const lhead = S.lhead;
  auto& kos = S.kos;
  auto& kls = S.kls;
  auto& kwin = S.kwin;
  uint32_t* const badf = S.badf;
  uint32_t* const wcut = S.wcut;
  uint32_t& mono = S.mono;
  const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1);
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  if (tid <= nb) bst[tid] = clamped_start(P, b0 + tid);
  if (tid < nb) {
    bfirst[tid] = bend[tid] = lhead[tid] = 0;
    badf[tid] = 0;
  }
  if (tid == 0) mono = 1;
  __syncthreads();
  if (tid < nb && bst[tid + 1] < bst[tid]) mono = 0;  // (benign race: every writer stores 0)
  if (tid <= 4) {  // wave t's first block: the first at or after a quarter of the items
    const uint32_t target = bst[0] + (uint32_t)(((uint64_t)(bst[nb] - bst[0]) * tid) / 4);
    uint32_t lo = 0, hi = nb;  // first j with bst[j] >= target (bst[nb] >= target)
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (bst[mid] >= target) hi = mid;
      else lo = mid + 1;
    }
    wcut[tid] = tid == 4 ? nb : lo;
  }
  __syncthreads();
  const uint32_t ri = P.ri;
  const uint32_t jlo = __builtin_amdgcn_readfirstlane(wcut[wave]);
  const uint32_t jhi = __builtin_amdgcn_readfirstlane(mono ? wcut[wave + 1] : wcut[wave]);
  const uint32_t ia = __builtin_amdgcn_readfirstlane(bst[jlo]);
  const uint32_t ie = __builtin_amdgcn_readfirstlane(bst[jhi]);
  unsigned long long* wkos = kos[wave];
  uint32_t* wkls = kls[wave];
  Win16* wkwin = kwin[wave];
  // a lane's two consecutive items: key / value offsets [t, t + 3), seqnos and types [t, t + 2)
  struct StepRaw {  // (offsets at their loaded width: see RawItemT)
    typename RawItemT<kOW>::off_t ko[kPW + 1], vo[kPW + 1];
    uint64_t seq[kPW];
    uint32_t vt[kPW];
  };
  auto load_step = [&](uint32_t base, StepRaw& r) {
    // (items past the run are clamped to its last one and ignored; offsets index up to ie)
    const uint32_t n = ie - base, t = min(kPW * lane, n - 1);
    auto at64 = [&](const uint64_t* a, uint32_t k) {
      return *reinterpret_cast<const uint64_t*>(reinterpret_cast<const uint8_t*>(a + base) + 8u * k);
    };
#pragma unroll
    for (uint32_t q = 0; q <= kPW; ++q) {
      r.ko[q] = (typename RawItemT<kOW>::off_t)off_rel<kOW>(P, P.it.key_off, base, min(t + q, n));
      r.vo[q] = (typename RawItemT<kOW>::off_t)off_rel<kOW>(P, P.it.val_off, base, min(t + q, n));
    }
#pragma unroll
    for (uint32_t q = 0; q < kPW; ++q) {
      r.seq[q] = at64(P.it.seqno, min(t + q, n - 1));
      r.vt[q] = (P.it.vtype + base)[min(t + q, n - 1)];
    }
  };
  StepRaw raw;
  if (ia < ie) load_step(ia, raw);
  uint64_t carry = 0;     // record bytes of this wave's items before the step
  uint64_t hk_ko = 0;     // the last restart head of the previous step: key offset, key length
  uint32_t hk_kl = 0;
  Win16 hk_win{0, 0};
  for (uint32_t base = ia; base < ie; base += kPWStep) {
    const uint32_t t0 = kPW * lane;
    ItemMeta m[kPW];
    uint32_t jq[kPW], jjq[kPW];
    bool ok[kPW];
    uint32_t j = jlo;
    {
      uint32_t lo = jlo, hi = jhi;  // block j: bst[j] <= base + t0 < bst[j + 1]
      const uint32_t i0 = min(base + t0, ie - 1);
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (bst[mid] <= i0) lo = mid;
        else hi = mid;
      }
      j = lo;
    }
#pragma unroll
    for (uint32_t q = 0; q < kPW; ++q) {
      const uint32_t i = base + t0 + q;
      ok[q] = i < ie;
      while (j + 1 < jhi && bst[j + 1] <= i) ++j;
      jq[q] = j;
      jjq[q] = ok[q] ? i - bst[j] : 0;
      bool bad = false;
      RawItem r;
      r.ko = raw.ko[q];
      r.ko1 = raw.ko[q + 1];
      r.vo = raw.vo[q];
      r.vo1 = raw.vo[q + 1];
      r.seq = raw.seq[q];
      r.vt = raw.vt[q];
      r.e = 0;
      r.hb = kNoBucket;
      m[q] = cook_item<false>(r, bad);
      if (ok[q] && bad) atomicOr(&badf[j], 1u);
      wkos[t0 + q] = m[q].ko;
      wkls[t0 + q] = m[q].klen;
    }
    // the next step's item fields, into the registers just consumed (no copy at the
    // step's end, which made the compiler wait for them there), in flight under this
    // step; issued before the key windows, which the step waits for
    if (base + kPWStep < ie) load_step(base + kPWStep, raw);
    // ---- shared prefix with the restart head: every item loads its own first 16
    // key bytes once; the others of its interval read the head's from LDS
    Win16 wa[kPW], wb[kPW];
#pragma unroll
    for (uint32_t q = 0; q < kPW; ++q) wb[q] = gwin16a(P.it.keys + m[q].ko);
#pragma unroll
    for (uint32_t q = 0; q < kPW; ++q) wkwin[t0 + q] = wb[q];
    if (kBkt) {  // hash-index batches: each key's bucket in its block, for E2 (keys of <= 16
                 // bytes from their window here, longer ones by encode_bucket_fixup_kernel)
#pragma unroll
      for (uint32_t q = 0; q < kPW; ++q) {
        if (!ok[q]) continue;
        const uint32_t n = bst[jq[q] + 1] - bst[jq[q]];
        const uint32_t buckets = bucket_count(n, P.ratio);
        const uint32_t hw = (buckets > 0 && (n + ri - 1) / ri <= kHashMaxPointers) ? buckets : 0;
        uint32_t hb = kNoBucket;
        if (hw && hw < kNeedHash) {  // (group-class blocks have at most kGHash buckets)
          if (m[q].klen <= 16)
            hb = (uint32_t)(xxh3_64_le16(m[q].klen, WinReader8{wb[q].lo, wb[q].hi},
                                         WinReader64{wb[q].lo, wb[q].hi}) % hw);
          else
            hb = kNeedHash, P.hb_fix[0] = 1;
        }
        P.hbucket[(uint64_t)base + t0 + q] = (uint16_t)hb;
      }
    }
    wave_lds_sync();
    uint32_t nq[kPW];
    uint64_t hq[kPW];
#pragma unroll
    for (uint32_t q = 0; q < kPW; ++q) {
      nq[q] = 0;
      hq[q] = 0;
      wa[q] = wb[q];
      if (ok[q] && jjq[q] % ri != 0) {
        const uint32_t h = base + t0 + q - jjq[q] % ri;
        const bool in = h >= base;
        const uint64_t hko = in ? (uint64_t)wkos[h - base] : hk_ko;
        const uint32_t hkl = in ? wkls[h - base] : hk_kl;
        nq[q] = min(hkl, m[q].klen);
        hq[q] = hko;
        wa[q] = in ? wkwin[h - base] : hk_win;
      }
    }
#pragma unroll
    for (uint32_t q = 0; q < kPW; ++q) {
      if (!nq[q]) continue;
      const uint64_t x0 = wa[q].lo ^ wb[q].lo, x1 = wa[q].hi ^ wb[q].hi;
      const uint32_t n = nq[q];
      uint32_t sh;
      if (x0) sh = min(n, (uint32_t)(__builtin_ctzll(x0) >> 3));
      else if (x1) sh = min(n, 8 + (uint32_t)(__builtin_ctzll(x1) >> 3));
      else sh = n <= 16 ? n : lcp_tail(P.it.keys, hq[q], m[q].ko, n);
      m[q].sh = sh;
    }
    // ---- record lengths, wave scan (a block never spans two waves)
    uint64_t rec[kPW], tsum = 0;
#pragma unroll
    for (uint32_t q = 0; q < kPW; ++q) {
      rec[q] = ok[q] ? item_record_len(P, m[q], jjq[q] % ri == 0) : 0;
      tsum += rec[q];
    }
    const uint64_t incl = wave_incl_scan_u64(tsum);
    uint64_t ex = carry + incl - tsum;
    uint64_t exq[kPW];
#pragma unroll
    for (uint32_t q = 0; q < kPW; ++q) {
      exq[q] = ex;
      if (ok[q]) {
        const uint32_t jb = jq[q], jj = jjq[q], ridx = jj / ri;
        const uint32_t n = bst[jb + 1] - bst[jb];
        if (jj == 0) bfirst[jb] = ex;
        if (jj + 1 == n) bend[jb] = ex + rec[q];
        if (jj == ridx * ri && ridx == (n - 1) / ri) lhead[jb] = ex;
      }
      ex += rec[q];
    }
    wave_lds_sync();
#pragma unroll
    for (uint32_t q = 0; q < kPW; ++q) {
      if (ok[q]) {
        const uint32_t jj = jjq[q], ridx = jj / ri;
        const bool head = jj == ridx * ri;
        const uint64_t roff = exq[q] - bfirst[jq[q]];
        const uint32_t x = head ? ridx : m[q].sh;
        // blocks of more than kGItems items are never group-class: their items
        // keep the whole 32-bit record offset, for E3
        P.erec[(uint64_t)base + t0 + q] =
            bst[jq[q] + 1] - bst[jq[q]] > kGItems
                ? (uint32_t)min(roff, (uint64_t)0xFFFFFFFFu)
                : (uint32_t)min(roff, (uint64_t)0x7FFF) | (head ? kErecHead : 0u) | (min(x, 0xFFFFu) << 16);
      }
    }
    carry += wave_bcast_u64(incl, kWave - 1);
    {  // the restart head of the step's last item, for the next step's first items
      const uint32_t last = min(ie, base + kPWStep) - 1, ll = (last - base) / kPW, lq = (last - base) % kPW;
      uint32_t jsel = jjq[0];
#pragma unroll
      for (uint32_t q = 1; q < kPW; ++q) jsel = lq == q ? jjq[q] : jsel;
      const uint32_t jjl = __builtin_amdgcn_readlane((int)jsel, (int)ll);
      const uint32_t h = last - jjl % ri;
      if (h >= base) {
        hk_ko = wkos[h - base];
        hk_kl = wkls[h - base];
        hk_win = wkwin[h - base];
      }
    }
    wave_lds_sync();  // (the next step rewrites kos / kls)
  }
  __syncthreads();
  if (tid >= nb) return;
  const uint32_t b = b0 + tid, s = bst[tid], e = bst[tid + 1];
  const bool bad = !mono || e <= s || badf[tid] || start_past_items(P, b + 1);
  const uint64_t ks = koff<kOW>(P, s), ke = koff<kOW>(P, e);
  const uint64_t vs = voff<kOW>(P, s), ve = voff<kOW>(P, e);
  BlockPlan pl;
  const uint64_t size =
      plan_block<false>(P, b, s, e, bad, bend[tid] - bfirst[tid], lhead[tid] - bfirst[tid], ks, ke, vs, ve, pl);
  if (kFused) {
    fplan[tid] = pl;
    fsize[tid] = size;
    // (a listed block's status until its list kernel writes it: stays if the run's
    // output offset never arrives, see run_lookback)
    if (size & ~kOffMask) P.status[b] = ST_INCOMPLETE;
  } else {
    P.sizes[b] = size;
  }
  P.kspan[b] = ks;
  P.vspan[b] = vs;
  if (b + 1 == P.n_blocks) {
    P.kspan[b + 1] = ke;
    P.vspan[b + 1] = ve;
  }
}

}  // namespace lsmgpu
