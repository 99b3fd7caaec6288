// decode_big.hpp — the kernels for the blocks the group kernel hands on: the big-block kernel
// (one block per stage, decode_big_kernel) and the general path with the LEB cursor
// (decode_deferred_staged_kernel).  Kernel bodies in a header: they are compiled in
// decode_huge.hip, in one unit with the huge-block kernels (see there for why).
#pragma once

#include "decode_common.hpp"

namespace lsmgpu {

// Deferred blocks up to kBigStage bytes (the 16..64 KiB data blocks larger
// than a group stage, and blocks with rare record shapes): one 4-wave
// workgroup per block, the block staged in LDS by LDS-DMA, then wave 0
// verifies the payload checksum while waves 1..3 walk the restart intervals
// (lane = interval) from LDS and store every record; statuses merge in
// oracle order (header, checksum, trailer / parse).  Larger blocks (full
// index blocks) take the HBM path on wave 0.
constexpr uint32_t kBigWaves = 4;
constexpr uint32_t kBigStage = 72 * 1024;

constexpr uint32_t kBigContrib = 256;                        // LDS: contributions, 64 B per KiB
constexpr uint32_t kBigStageOff = kBigContrib + (kBigStage / 1024 + 1) * 64;

// A data or index block larger than the stage (a full block index: ~25 B
// per data block, hundreds of KiB for a 64 MiB table; a data block of the
// writer's up-to-4-MiB targets, writer/mod.rs:193-198), on all four waves of
// the general-path workgroup, through the stage in 64 KiB chunks (staged with
// 7.5 KiB of overlap past the chunk).  Per chunk: all waves compute the
// per-KiB XXH3 contributions of the chunk's KiB blocks, wave 0 carries the
// serial chain across chunks; each thread parses the restart intervals
// (r = tid, tid + 256, ...) that start in the chunk from LDS when the whole
// interval (+ the parsers' read-ahead) is staged, else walks it from HBM.  The
// interval starts come from the binary index in HBM (the block's tail is not
// in the chunk).  Same results as the interval walk of decode_block_direct.
constexpr uint32_t kChunkBytes = 64 * 1024;
constexpr uint32_t kChunkOverlap = 7 * 1024 + 512;
constexpr uint32_t kChunkReadAhead = 192;  // parsers read at most this far past a record start window
static_assert(kChunkBytes + kChunkOverlap + 256 <= kBigStage, "chunk + overlap + pad");

__device__ __forceinline__ void decode_chunked(const DecodeParams& P, uint32_t b, const uint8_t* gbase,
                                               uint32_t span, BlockMeta* meta, uint32_t* cks_bad,
                                               uint64_t* contrib, uint8_t* stage) {
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int lane = tid & (kWave - 1);
  constexpr uint32_t kThreads = kBigWaves * kWave;
  const BlockMeta m = meta[1];
  const TrailerInfo t = trailer_of(m);
  const uint32_t p0 = m.p0;  // span-relative payload start
  const uint32_t plen = m.len - kHdrLen;
  const uint64_t item_base = gload(P.item_start, b);
  const bool hash = !(P.flags & LSM_DECODE_PAYLOAD_VERIFIED);
  const uint32_t nbk = plen > 240 ? (plen - 1) / 1024 : 0;
  uint64_t a0, a1;
  xxh3_acc_init(lane & 3, a0, a1);
  const uint64_t scr0 = kLongSecret.acc[16 + 2 * (lane & 3)], scr1 = kLongSecret.acc[16 + 2 * (lane & 3) + 1];
  const uint32_t nint = t.bin_len;
  auto emit = [&](uint32_t j, const ItemFields& f) { emit_global(P.out, item_base + j, f, P.seqno_add, P.compact); };
  uint32_t r = tid;
  uint32_t s_cur = r < nint ? bin_get(gbase, p0, t, r) : 0xFFFFFFFFu;
  bool ok = true;
  for (uint32_t cs = 0; cs < span; cs += kChunkBytes) {
    const uint32_t ce = min(cs + kChunkBytes, span);
    const uint32_t ss = min(ce + kChunkOverlap, span);  // staged: [cs, ss)
    stage_to_lds(gbase + cs, stage, (ss - cs + 15) >> 4, wave, kBigWaves, lane);
    vm_wait<0>();
    lds_barrier();
    const uint8_t* sbase = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(stage) - cs);  // span-relative
    // the KiB blocks that start in this chunk
    const uint32_t n0 = min(nbk, cs > p0 ? (cs - p0 + 1023) / 1024 : 0u);
    const uint32_t n1 = min(nbk, ce > p0 ? (ce - p0 + 1023) / 1024 : 0u);
    if (hash && n1 > n0)
      xxh3_kib_contribs(sbase, p0 + 1024 * n0, (n1 - n0) * 1024 + 1, &kLongSecret, contrib, wave, kBigWaves);
    // the intervals that start in this chunk
    while (r < nint && p0 + s_cur < ce) {
      const bool last = r + 1 == nint;
      const uint32_t stop = last ? t.rec_end : bin_get(gbase, p0, t, r + 1);
      const bool staged = p0 + s_cur >= cs && stop <= t.rec_end && (p0 + stop + kChunkReadAhead <= ss || ss == span);
      ok &= walk_interval_at(staged ? sbase : gbase, p0, m, t, r, s_cur, stop, emit);
      r += kThreads;
      s_cur = r < nint ? bin_get(gbase, p0, t, r) : 0xFFFFFFFFu;
    }
    lds_barrier();
    // the chain over this chunk's KiB blocks, in order
    if (wave == 0 && hash) xxh3_quad_chain<1>(contrib + 2 * (lane & 3), n1 - n0, scr0, scr1, a0, a1);
    lds_barrier();  // (the next chunk overwrites the stage and the contributions)
  }
  if (r < nint) ok = false;  // a record start beyond the block
  if (!ok) atomicCAS(&meta[1].st, ST_OK, ST_PARSE);
  if (wave == 0 && hash) {
    uint64_t lo, hi;
    if (plen > 240) xxh3_wave_tail_merge(gbase, p0, plen, &kLongSecret, a0, a1, lo, hi);
    else xxh3_128_wave(gbase, p0, plen, &kLongSecret, lo, hi);
    if (lane == 0) *cks_bad = lo != m.ck_lo || hi != m.ck_hi;
  }
  lds_barrier();
  if (tid == 0) {
    const int32_t st = meta[0].st != ST_OK ? meta[0].st : *cks_bad ? (int32_t)ST_CKSUM : meta[1].st;
    gstore(P.status, b, st);
  }
}

__global__ __launch_bounds__(kBigWaves * kWave) void decode_deferred_staged_kernel(DecodeParams P) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  BlockMeta* meta = reinterpret_cast<BlockMeta*>(smem);  // [0] header view, [1] trailer view
  uint32_t* cks_bad = reinterpret_cast<uint32_t*>(smem + 2 * sizeof(BlockMeta));
  uint64_t* contrib = reinterpret_cast<uint64_t*>(smem + kBigContrib);
  uint8_t* stage = smem + kBigStageOff;
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int lane = tid & (kWave - 1);
  const uint32_t n = gload(P.defer_count, 0);
  for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
    const uint32_t b = gload(P.defer_list, i);
    const uint64_t off = gload(P.block_off, b), end = gload(P.block_off, b + 1);
    const uint64_t span0 = off & ~15ULL, span1 = (max(end, off) + 15) & ~15ULL;
    if (span1 - span0 > kBigStage) {  // larger than the stage
      const uint8_t* gbase = P.blocks + span0;
      const uint32_t cap = gload(P.item_start, b + 1) - gload(P.item_start, b);
      if (tid == 0) {
        meta_header(gbase, (uint32_t)(off - span0), end >= off ? end - off : 0, meta[0]);
        meta[1] = meta[0];
        meta_trailer(gbase, P.expect_type, cap, meta[1], P.compact);
        *cks_bad = 0;
      }
      lds_barrier();
      if (meta[0].st == ST_OK && meta[1].st == ST_OK) {  // data / index / meta blocks: chunked through the stage
        decode_chunked(P, b, gbase, (uint32_t)(span1 - span0), meta, cks_bad, contrib, stage);
      } else if (wave == 0) {  // a failing header or trailer: one wave (statuses in oracle order)
        decode_block_direct(P, b, meta);
      }
      lds_barrier();
      continue;
    }
    stage_to_lds(P.blocks + span0, stage, (uint32_t)((span1 - span0) >> 4), wave, kBigWaves, lane);
    const uint64_t item_base = gload(P.item_start, b);
    const uint32_t cap = gload(P.item_start, b + 1) - (uint32_t)item_base;
    vm_lgkm_wait0();  // this wave's DMA has landed
    lds_barrier();
    const uint32_t hb = (uint32_t)(off & 15);
    if (tid == 0) {
      meta_header(stage, hb, end >= off ? end - off : 0, meta[0]);
      meta[1] = meta[0];
      meta_trailer(stage, P.expect_type, cap, meta[1], P.compact);
      *cks_bad = 0;
    }
    lds_barrier();
    // payload checksum: per-KiB contributions on all waves, then the chain on wave 0
    const bool hdr_ok = meta[0].st == ST_OK && !(P.flags & LSM_DECODE_PAYLOAD_VERIFIED);
    const uint32_t plen = meta[0].len - kHdrLen;
    if (hdr_ok && plen > 240) xxh3_kib_contribs(stage, hb + kHdrLen, plen, &kLongSecret, contrib, wave, kBigWaves);
    lds_barrier();
    if (wave == 0) {
      if (hdr_ok) {
        uint64_t lo, hi;
        if (plen > 240) xxh3_128_wave_finish(stage, hb + kHdrLen, plen, &kLongSecret, contrib, lo, hi);
        else xxh3_128_wave(stage, hb + kHdrLen, plen, &kLongSecret, lo, hi);
        if (lane == 0) *cks_bad = lo != meta[0].ck_lo || hi != meta[0].ck_hi;
      }
    } else {
      const BlockMeta m = meta[1];
      if (m.st == ST_OK) {
        bool ok = true;
        for (uint32_t r = tid - kWave; r < m.bin_len; r += (kBigWaves - 1) * kWave) {
          ok &= walk_interval(stage, hb + kHdrLen, m, r,
                              [&](uint32_t j, const ItemFields& f) { emit_global(P.out, item_base + j, f, P.seqno_add, P.compact); });
        }
        if (!ok) atomicCAS(&meta[1].st, ST_OK, ST_PARSE);
      }
    }
    lds_barrier();
    if (tid == 0) {
      const int32_t st = meta[0].st != ST_OK ? meta[0].st : *cks_bad ? (int32_t)ST_CKSUM : meta[1].st;
      gstore(P.status, b, st);
    }
    lds_barrier();
  }
}

// Large blocks (SURVEY configs[4]: 16 / 64 KiB data blocks) listed by the
// group kernel: persistent 8-wave workgroups, two per CU (one stage each:
// the other workgroup's decode overlaps this one's DMA).  Per block, after
// the LDS-DMA, three concurrent streams hand off through LDS flags:
//   wave 0      header fields and trailer (lane 0), then phase A over every
//               restart interval (lane = interval), then phase B
//   waves 1..6  the per-KiB XXH3 contributions, each published as it is
//               done, then phase B once phase A has finished
//   wave 7      the serial XXH3 scramble chain over the contributions as they
//               arrive, the tail and the header checksum (raised priority:
//               it is the block's critical path)
// Blocks larger than the stage, with more items than kBigGTile, index blocks
// and rare record shapes go on to the general path (defer2 list).
constexpr uint32_t kBigGWaves = 8;
constexpr uint32_t kBigGStage = 69376;  // 67.75 KiB: a 64 KiB-target block of 69.2 KB plus alignment
constexpr uint32_t kBigGSlot = kBigGStage + kStagePad;
constexpr uint32_t kBigGTile = 832;
constexpr uint32_t kBigGRec = ((kBigGTile + 1) * 8 + 15) & ~15u;
constexpr uint32_t kBigGContrib = (kBigGStage / 1024 + 1) * 64;
constexpr uint32_t kBigGOwner = (kBigGTile + 15) & ~15u;
// Cross-wave hand-offs of one block (tags: the block's list index + 1, so
// nothing is reset between blocks).
struct BigSync {
  uint32_t a_done;  // phase A finished
  uint32_t hck;     // header checksum ok (chain wave)
  uint64_t lo, hi;  // payload xxh3_128 (chain wave)
  uint32_t ready[kBigGStage / 1024 + 1];  // KiB block n's contribution published
};
constexpr uint32_t kBigGSync = (sizeof(BigSync) + 15) & ~15u;
constexpr uint32_t kBigGLds = 80 + kBigGSync + kBigGRec + kBigGOwner + kBigGContrib + kBigGSlot;
constexpr uint32_t kBigGPerCU = 2;
static_assert(kBigGLds * kBigGPerCU <= 160 * 1024, "big-block workgroups per CU");

// A listed block's handle and item range; fits = it takes the stage path.
struct BigBlk {
  uint32_t li, b, it0, it1;
  uint64_t off, end, span0, span1;
  bool fits;
};
__device__ __forceinline__ BigBlk big_blk(const DecodeParams& P, uint32_t li) {
  BigBlk x;
  x.li = li;
  x.b = gload(P.defer_list, li);
  x.off = gload(P.block_off, x.b);
  x.end = gload(P.block_off, x.b + 1);
  x.it0 = gload(P.item_start, x.b);
  x.it1 = gload(P.item_start, x.b + 1);
  x.span0 = x.off & ~15ULL;
  x.span1 = (max(x.end, x.off) + 15) & ~15ULL;
  x.fits = x.end >= x.off && x.span1 - x.span0 <= kBigGStage && x.it1 - x.it0 <= kBigGTile;
  return x;
}

#if defined(LSM_DIAG) && !defined(LSM_DIAG_NOTIME)
// wave 0 of every big-block workgroup: entries 0..7; of every huge-unit workgroup: 8..14;
// blocks and units counted in 15
__device__ unsigned long long g_large_phase[32];
#endif

template <bool kAllFields, bool kCompact>
__global__ __launch_bounds__(kBigGWaves * kWave) void decode_big_kernel(DecodeParams P) {
#if defined(LSM_DIAG) && !defined(LSM_DIAG_NOTIME)
  uint64_t t_last = __builtin_amdgcn_s_memtime(), ph[8] = {};
  uint32_t nblk = 0;
#endif
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  BlockMeta* meta = reinterpret_cast<BlockMeta*>(smem);
  BigSync* sync = reinterpret_cast<BigSync*>(smem + 80);
  uint64_t* rec = reinterpret_cast<uint64_t*>(smem + 80 + kBigGSync);
  uint8_t* owner = smem + 80 + kBigGSync + kBigGRec;
  uint64_t* contrib = reinterpret_cast<uint64_t*>(smem + 80 + kBigGSync + kBigGRec + kBigGOwner);
  uint8_t* stages = smem + 80 + kBigGSync + kBigGRec + kBigGOwner + kBigGContrib;
  constexpr uint32_t kThreads = kBigGWaves * kWave;
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int lane = tid & (kWave - 1);
  const uint32_t n = gload(P.defer_count, 0);
  // the listed blocks of this workgroup that fit a stage, in list order
  auto next_fit = [&](uint32_t li) -> BigBlk {
    for (;; li += gridDim.x) {
      if (li >= n) {
        BigBlk z{};
        z.li = li;
        z.fits = false;
        return z;
      }
      const BigBlk x = big_blk(P, li);
      if (x.fits) return x;
      if (tid == 0) {  // (workgroup-uniform)
        if (P.huge_pool && x.end >= x.off && x.span1 - x.span0 > kBigStage) defer3_block(P, x.b);
        else defer2_block(P, x.b);
      }
    }
  };
  auto issue_dma = [&](const BigBlk& x, uint8_t* dst) {  // wave w moves 1-KiB pieces w, w + 8, ...
    stage_to_lds(P.blocks + x.span0, dst, (uint32_t)((x.span1 - x.span0) >> 4), wave, kBigGWaves, lane);
  };
  for (uint32_t x = tid; x < kBigGStage / 1024 + 1; x += kThreads) sync->ready[x] = 0;
  if (tid == 0) sync->a_done = 0;
  BigBlk X = next_fit(blockIdx.x);
  if (X.fits) issue_dma(X, stages);
  while (X.fits) {
    uint8_t* stage = stages;
    const uint32_t b = X.b, n_items = X.it1 - X.it0;
    const uint32_t tag = X.li + 1;  // this block's publication tag (list indices only grow)
    for (uint32_t x = tid; x <= n_items; x += kThreads) rec[x] = 0;
    DEC_PHASE(7);
    vm_wait<0>();  // this block's stage (and every earlier store)
    lds_barrier();
    DEC_PHASE(0);
    const uint32_t hb = (uint32_t)(X.off - X.span0);
    const uint64_t hlen = X.end - X.off;
    // the payload checksum as the handle gives it: it counts only if the
    // header's fields check out (then data_length == handle - 33)
    const bool hash = !(P.flags & LSM_DECODE_PAYLOAD_VERIFIED) && !(kDiagBuild && (P.flags & kDiagSkipHash)) &&
                      hlen >= kHdrLen;
    const uint32_t plen = hash ? (uint32_t)hlen - kHdrLen : 0;
    if (wave == kBigGWaves - 1) {
      // the serial XXH3 chain, consuming the contributions as waves 1.. publish
      // them, then the tail and the header checksum (raised priority: the
      // chain is the block's critical path)
      if (hash) {
        __builtin_amdgcn_s_setprio(3);
        uint64_t lo, hi;
        if (plen > 240) xxh3_128_wave_finish(stage, hb + kHdrLen, plen, &kLongSecret, contrib, lo, hi, sync->ready, tag);
        else xxh3_128_wave(stage, hb + kHdrLen, plen, &kLongSecret, lo, hi);
        const bool hck = header_cksum_ok(stage, hb);
        if (lane == 0) {
          sync->lo = lo;
          sync->hi = hi;
          sync->hck = hck;
        }
        __builtin_amdgcn_s_setprio(0);
      }
    } else {
      if (wave == 0) {  // header, trailer, then phase A over every restart interval
        if (lane == 0) {
          BlockMeta m;
          meta_header_fields(stage, hb, hlen, m);
          m.item0 = 0;
          m.hdr_st = m.st;
          m.ck_bad = 0;
          m.hck_bad = 0;
          meta_trailer(stage, P.expect_type, n_items, m, P.compact);
          if (m.st == ST_OK && m.type == 1) m.st = ST_DEFER;  // index blocks: general path
          m.chain0 = 0;
          meta[0] = m;
        }
        wave_sync();
        const uint32_t total = meta[0].st == ST_OK ? meta[0].bin_len : 0;
        for (uint32_t r = lane; r < total; r += kWave) owner[r] = 0;
        wave_sync();
        __builtin_amdgcn_s_setprio(2);  // (the record walk is the block's longest role)
        phase_a<true>(stage, meta, owner, rec, 0, kWave, total, kBigGTile);
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
        if (lane == 0) __hip_atomic_store(&sync->a_done, tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      } else {  // the per-KiB contributions, then wait for phase A
        if (hash && plen > 240)
          xxh3_kib_contribs(stage, hb + kHdrLen, plen, &kLongSecret, contrib, wave - 1, kBigGWaves - 2, sync->ready,
                            tag);
        while (__hip_atomic_load(&sync->a_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != tag)
          __builtin_amdgcn_s_sleep(1);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
      }
      // phase B on waves 0 .. kBigGWaves - 2, under the chain
      if (!(kDiagBuild && (P.flags & kDiagSkipPhaseB)))
        phase_b<kAllFields, kCompact, true>(P, stage, meta, rec, n_items, X.it0, tid, (kBigGWaves - 1) * kWave);
    }
    lds_barrier();
    DEC_PHASE(4);
    const BigBlk Xn = next_fit(X.li + gridDim.x);
    if (tid == 0) {  // statuses in oracle order: header, header checksum, payload checksum, trailer / parse
      const BlockMeta& m = meta[0];
      const bool chk = hash && m.hdr_st == ST_OK;
      const int32_t st = m.hdr_st != ST_OK                              ? m.hdr_st
                         : (chk && !sync->hck)                          ? (int32_t)ST_HDR_CKSUM
                         : (chk && (sync->lo != m.ck_lo || sync->hi != m.ck_hi)) ? (int32_t)ST_CKSUM
                                                                         : m.st;
      if (st == ST_DEFER) defer2_block(P, b);
      else gstore(P.status, b, st);
    }
    lds_barrier();  // (meta / rec / owner / the stage are rewritten for the next block)
    DEC_PHASE(5);
    if (Xn.fits) issue_dma(Xn, stages);
    DEC_PHASE(6);
#if defined(LSM_DIAG) && !defined(LSM_DIAG_NOTIME)
    ++nblk;
#endif
    X = Xn;
  }
#if defined(LSM_DIAG) && !defined(LSM_DIAG_NOTIME)
  if (tid == 0) {
    for (int i = 0; i < 8; ++i) atomicAdd(&g_large_phase[i], (unsigned long long)ph[i]);
    atomicAdd(&g_large_phase[15], (unsigned long long)nblk);
  }
#endif
}

}  // namespace lsmgpu
