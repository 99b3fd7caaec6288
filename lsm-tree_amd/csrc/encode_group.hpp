// encode_group.hpp — the group write kernel of the encode path (E2); see encode.hip.
// A header because two units instantiate the kernel: encode_group.hip all instantiations but
// <false, true, false, *>, which hashes keys itself and so lives in encode_large.hip (see there).
#pragma once

#include "encode_plan.hpp"

namespace lsmgpu {

// ------------------------------------------------ E2: group write kernel
// One 4-wave workgroup owns kGRun consecutive blocks and writes them in
// GROUPS: the longest run of consecutive group-class blocks whose items,
// key bytes, value bytes, encoded bytes and hash-index buckets fit the LDS
// budget (one 4 KiB data block is ~1/4 of a group; a 16 KiB one fills it).
// Consecutive blocks' items are contiguous in the arenas and their encoded
// bytes are contiguous in the output, so per group:
//   DMA    key and value spans HBM -> LDS stage (global_load_lds, 1 KiB per
//          wave instruction); thread t loads item t's offsets, seqno, type
//   shape  thread = item: shared prefix with its restart head (from the
//          stage), record length, workgroup scan -> record offset in block
//   write  thread = item: its record (header bytes, key suffix, value LEB +
//          bytes) into the LDS image of the group's output span, binary
//          index entry, hash-index vote; the next group's DMA is issued.
//          The values' interior dwords go wave by wave, in a loop whose trip
//          count is the wave's shortest interior (lds_copy_uniform); the
//          edges and what longer values have left, lane by lane (lds_copy)
//   tails  wave per block: marker, hash-index bytes, trailer
//   hash   the 16 DPP rows of the workgroup split every block's payload
//          into 1 KiB units (XXH3 per-KiB contributions, then one short
//          serial scramble chain per block)
//   header wave 0, lane per block: header fields + 29-byte checksum
//   out    16 B/lane copy of the group's span: the header-free pieces by three waves
//          while the fourth runs the chains, then the header pieces
// Blocks that do not fit are written by the list / HBM kernels.
// Runs of small data blocks (no hash index, no fused plan) are written wave per block
// instead, without the groups and their barriers: WaveSlot below and the loop in the kernel.
struct GBlk {
  uint32_t it0, n;         // first item (group-relative), items
  uint32_t img, plen;      // header position in the image, payload length
  uint32_t recs, bin_len;  // record bytes, restart heads
  uint32_t step, hash_w;   // binary-index step, hash-index buckets
  uint32_t hash_base, u0;  // first vote pair, first hash unit
  uint32_t nbk, spare;     // full KiB units of the payload
};
static_assert(sizeof(GBlk) == 48, "GBlk");

// The wave-per-block loop of the group kernel (data blocks without a hash index or the
// fused plan): each wave of the workgroup has a stage and an image of its own, over the
// group loop's LDS (the secret lies past them).  A 4 KiB block of 52 items, 16 B keys
// and 64 B values (832 B of keys, 3328 B of values, 3.8 KB encoded) fits, and so does the
// random-key 4 KiB class (4466 B blocks); four slots and the secret stay within the
// 40,960 B that keep four workgroups on a CU.
#ifdef LSM_NO_WAVE_BLOCKS
constexpr bool kWaveBlocks = false;  // (A/B build: the group loop alone)
#else
constexpr bool kWaveBlocks = true;
#endif
constexpr uint32_t kWKeys = 1024, kWVals = 4096, kWImg = 4496;  // per-wave stage and image, as kGKeys / kGVals / kGImg
constexpr uint32_t kWItems = kWave;                              // one lane per item
constexpr uint32_t kWUnits = 5;                                  // hash units of an image, at most
static_assert((kWImg - 1) / 1024 <= 4 && (kWImg - 1) / 1024 + 1 <= kWUnits,
              "full KiB units and the tail unit of a payload");
// Blocks of a wave whose scramble chains, checksum tails and headers are finished together, a
// lane quad per block (flush_headers).  Every kept block costs two VGPRs (its contributions)
// and two selects per block; 4 measured faster than 6 and 8, the wave's whole share of a
// run.
constexpr uint32_t kWDefer = 4;
static_assert(kWDefer >= 1 && kWDefer <= kWave / 4, "one lane quad per deferred block");
static_assert(kWDefer * kWUnits * 8 * 8 <= kWImg, "the kept contributions fit the free image at the flush");
struct WaveSlot {
  uint8_t keys[kWKeys + kGSlack];
  uint8_t vals[kWVals + kGSlack];
  uint8_t img[kWImg + kGSlack];
  uint64_t contrib[kWUnits * 8];
};
static_assert(offsetof(WaveSlot, vals) % 16 == 0 && offsetof(WaveSlot, img) % 16 == 0 && sizeof(WaveSlot) % 16 == 0,
              "stage DMA and 16-B copy-out alignment");
constexpr uint32_t kGroupBody = kGKeys + kGVals + kGImg + 3 * kGSlack + kGUnion + 2 * kGBlocks * (uint32_t)sizeof(GBlk);
constexpr uint32_t kWaveSlots = kGWaves * (uint32_t)sizeof(WaveSlot);
constexpr uint32_t kWavePad = kWaveSlots > kGroupBody ? kWaveSlots - kGroupBody : 16;

struct GroupLds {
  uint8_t keys[kGKeys + kGSlack];
  uint8_t vals[kGVals + kGSlack];
  uint8_t img[kGImg + kGSlack];
  uint32_t uni[kGUnion / 4];
  GBlk blk[2][kGBlocks];  // this group's block table and the next one's (built under the chain)
  uint8_t wave_pad[kWavePad];  // (the wave-per-block loop's slots, which lie over all of the above, end here)
  LongSecret secret;
};
// (the fused kernel's run-level plan keeps its LDS over vals + img, and its per-block
// outputs in uni, before the first group's DMA)
static_assert(offsetof(GroupLds, uni) - offsetof(GroupLds, vals) >= sizeof(PlanWaveLds), "plan LDS over the stage");
static_assert(offsetof(GroupLds, vals) % 16 == 0, "plan LDS alignment");
static_assert(kGRunFused * (sizeof(BlockPlan) + 8) + 16 <= kGUnion, "fused plan outputs in uni");
static_assert(offsetof(GroupLds, wave_pad) == kGroupBody, "GroupLds layout");
static_assert(kGWaves * sizeof(WaveSlot) <= offsetof(GroupLds, secret), "the wave slots lie over the group loop's LDS");
static_assert(sizeof(GroupLds) <= 40960, "four workgroups per CU");

__device__ __host__ __forceinline__ bool wave_fits(uint64_t n, uint64_t kspan, uint64_t vspan, uint64_t total) {
  return n >= 1 && n <= kWItems && kspan + 15 <= kWKeys && vspan + 15 <= kWVals && total + 15 <= kWImg;
}


// n bytes src[s ..) (LDS) -> dst[d ..) (LDS): byte stores for the dst bytes
// that share a dword with a neighbour record, aligned dword stores inside
// (each from two source dwords and v_alignbyte); reads up to 8 bytes past.
// Lane `rot` starts its dword loop at a lane-dependent point of the span and
// wraps: records with a power-of-two source stride (64 B values: every lane
// of a 32-lane group on 2 banks) then read and write conflict-free.
// `done`: the span's first `done` interior dwords are already in place
// (lds_copy_uniform); the head bytes, the dwords past them and the tail bytes
// are copied here.
__device__ __forceinline__ void lds_copy(uint8_t* dst, uint32_t d, const uint8_t* src, uint32_t s, uint32_t n,
                                         uint32_t rot, uint32_t done = 0) {
  if (!n) return;
  // (every read of a step is issued before its writes: one LDS round trip per step)
  const uint32_t h = min(n, (4u - (d & 3u)) & 3u);
  uint32_t hb[3];
#pragma unroll
  for (uint32_t k = 0; k < 3; ++k)
    if (k < h) hb[k] = src[s + k];
#pragma unroll
  for (uint32_t k = 0; k < 3; ++k)
    if (k < h) dst[d + k] = (uint8_t)hb[k];
  if (n == h) return;
  const uint32_t d1 = d + h + 4 * done, e = d + n, body = ((e & ~3u) - d1) >> 2;
  const uint32_t sp = s + h + 4 * done, sh = sp & 3u;
  const uint32_t* s32 = reinterpret_cast<const uint32_t*>(src + (sp & ~3u));
  uint32_t* d32 = reinterpret_cast<uint32_t*>(dst + d1);
  // 32 start points: a ds_read_b32 wave access is two groups of 32 lanes, so
  // lanes with a 64-B source stride (16 dwords: two per bank) all differ.
  uint32_t q = ((rot & 31u) * body) >> 5;  // 0 <= q < body
  constexpr uint32_t U = 4;  // dwords per step (all reads before the writes)
  // Each source dword is read once: destination dword p is
  // alignbyte(src[p + 1], src[p]) and src[p] is the previous step's src[p + 1],
  // except after the wrap to p = 0, which takes w0 = src[0].
  const uint32_t w0 = body ? s32[0] : 0;
  uint32_t carry = body ? s32[q] : 0;
  for (uint32_t j0 = 0; j0 < body; j0 += U) {
    uint32_t hi[U], at[U];
#pragma unroll
    for (uint32_t t = 0; t < U; ++t) {
      uint32_t p = q + t;
      p = p >= body ? p - body : p;
      at[t] = p;
      if (j0 + t < body) hi[t] = s32[p + 1];
    }
#pragma unroll
    for (uint32_t t = 0; t < U; ++t) {
      if (j0 + t < body) {
        const uint32_t lo = t == 0 ? carry : (at[t] == 0 ? w0 : hi[t - 1]);
        d32[at[t]] = alignbyte(hi[t], lo, sh);
      }
    }
    q += U;
    q = q >= body ? q - body : q;
    carry = q == 0 ? w0 : hi[U - 1];
  }
  const uint32_t t0 = d1 + 4 * body;  // 0..3 tail bytes
  uint32_t tb[3];
#pragma unroll
  for (uint32_t k = 0; k < 3; ++k)
    if (t0 + k < e) tb[k] = src[s + (t0 + k - d)];
#pragma unroll
  for (uint32_t k = 0; k < 3; ++k)
    if (t0 + k < e) dst[t0 + k] = (uint8_t)tb[k];
}

// The group kernel's value copy, first part: the interior dwords that every
// value-carrying lane of the wave has, in a loop with a wave-uniform trip count.
// Lane by lane lds_copy's dword loop tests the wrap, the end of the span and the
// carry per dword (the spans' dword counts differ between lanes, by one already
// for equal lengths at different destination alignments), which compiles to an
// exec-mask write and branches per dword (per 4 dwords 43 VALU, 40 scalar and
// branch instructions).  Here B, the wave-wide minimum of the lanes' interior
// dword counts, is in an SGPR: the loop runs ceil(B / 4) steps of 4 dwords, the
// wrap is min(x, x - B), the exec mask is set once around the loop, and the body
// has no per-lane condition but a select of the carried source dword at the wrap
// (32 VALU, under one scalar instruction per 4 dwords).  The rotation is
// lds_copy's, modulo B.  After the loop a lane with more than B dwords copies one
// more, so that equal-length values leave lds_copy only their head and tail bytes.
// Called with every lane active; `has`: this lane copies n > 0 bytes
// src[s ..) -> dst[d ..).  Returns the lane's number of interior dwords now in
// place (0: B under kUniformMin, or no lane with `has`), to be handed to lds_copy
// as `done`.  The bytes written are the same whichever way they are copied.
// Measured in scripts/exp/lds_copy_bench.cpp (variant 10) and in the kernel:
// DESIGN §6.7, profiles/uniform_copy_ab.txt.
#ifdef LSM_NO_UNIFORM_COPY
constexpr bool kUniformCopy = false;  // (A/B build: the general loop alone)
#else
constexpr bool kUniformCopy = true;
#endif
constexpr uint32_t kUniformMin = 4;  // dwords per step; fewer than one step: the general loop alone
__device__ __forceinline__ uint32_t lds_copy_uniform(uint8_t* dst, uint32_t d, const uint8_t* src, uint32_t s,
                                                     uint32_t n, bool has, uint32_t rot) {
  if (!kUniformCopy) return 0;
  const uint32_t h = min(n, (4u - (d & 3u)) & 3u);
  const uint32_t body = n > h ? (((d + n) & ~3u) - (d + h)) >> 2 : 0u;
  const uint32_t B = wave_min_u32(has ? body : 0xFFFFFFFFu);
  if (B < kUniformMin || B == 0xFFFFFFFFu) return 0;
  if (has) {
    const uint8_t* sb = src + ((s + h) & ~3u);
    uint8_t* db = dst + d + h;
    const uint32_t sh = (s + h) & 3u, B4 = 4 * B;
    auto ld = [&](uint32_t x) { return *reinterpret_cast<const uint32_t*>(sb + x); };
    auto st = [&](uint32_t x, uint32_t v) { *reinterpret_cast<uint32_t*>(db + x) = v; };
    constexpr uint32_t U = kUniformMin;
    uint32_t x = (((rot & 31u) * B) >> 5) * 4;  // byte offset of the lane's next dword, < B4
    // destination dword x is alignbyte(src[x + 4], src[x]); src[x] is the dword
    // carried from the step before, except after the wrap to x = 0 (w0)
    const uint32_t w0 = ld(0);
    uint32_t carry = ld(x);
    // (B is no multiple of U: the last step wraps on over dwords already copied and
    // stores the same bytes again, which is cheaper than a remainder loop's LDS round
    // trip per dword)
    for (uint32_t j = 0; j < B; j += U) {
      uint32_t at[U], hi[U];
#pragma unroll
      for (uint32_t t = 0; t < U; ++t) {
        const uint32_t y = x + 4 * t;
        at[t] = t == 0 ? x : min(y, y - B4);  // (y < B4: y - B4 wraps high)
        hi[t] = ld(at[t] + 4);
      }
#pragma unroll
      for (uint32_t t = 0; t < U; ++t) {
        const uint32_t lo = at[t] == 0 ? w0 : (t == 0 ? carry : hi[t - 1]);
        st(at[t], alignbyte(hi[t], lo, sh));
      }
      carry = hi[U - 1];
      x += 4 * U;
      x = min(x, x - B4);
    }
    // one dword more where the lane has it (equal lengths differ by at most this one,
    // by the destination alignment): lds_copy then finds no dword left and skips its loop
    if (body > B) {
      st(B4, alignbyte(ld(B4 + 4), ld(B4), sh));
      return B + 1;
    }
  }
  return B;
}

__device__ __forceinline__ uint32_t lds_put_leb(uint8_t* dst, uint32_t pos, uint64_t v) {
  while (v >= 0x80) {
    dst[pos++] = (uint8_t)(v | 0x80);
    v >>= 7;
  }
  dst[pos++] = (uint8_t)v;
  return pos;
}

// A record up to its value, into the LDS image at `pos` (both loops of the group kernel):
// type byte, varints, key (suffix from byte `from`; the key starts at keys[kst]), value
// length.  Returns the value's place.
template <bool kIndex>
__device__ __forceinline__ uint32_t put_record_header(uint8_t* img, uint32_t pos, const uint8_t* keys, uint32_t kst,
                                                      const ItemMeta& m, bool head, uint32_t from, uint32_t rot) {
  if (kIndex) {
    img[pos++] = 0;
    pos = lds_put_leb(img, pos, m.vo);
    pos = lds_put_leb(img, pos, m.vl);
    pos = lds_put_leb(img, pos, m.seq);
    pos = lds_put_leb(img, pos, m.klen);
    lds_copy(img, pos, keys, kst, m.klen, rot);
  } else {
    img[pos++] = (uint8_t)m.vt;
    pos = lds_put_leb(img, pos, m.seq);
    if (!head) pos = lds_put_leb(img, pos, m.sh);
    pos = lds_put_leb(img, pos, m.klen - from);
    lds_copy(img, pos, keys, kst + from, m.klen - from, rot);
    pos += m.klen - from;
    if (!is_tombstone(m.vt)) pos = lds_put_leb(img, pos, m.vl);
  }
  return pos;
}

// A restart head's binary-index entry: its record offset, `step` bytes little-endian.
// (`step` by reference: the group loop hands in its block table's word in LDS, read as
// before between the byte stores; by value that loop took 6 VGPRs more in every instantiation)
__device__ __forceinline__ void put_bin_entry(uint8_t* img, uint32_t bp, const uint32_t& step, uint32_t roff) {
  for (uint32_t q = 0; q < step; ++q) img[bp + q] = (uint8_t)(roff >> (8 * q));
}

__device__ __forceinline__ void group_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// The group kernel's barrier: a release fence on LDS counts in-flight LDS-DMA
// as LDS stores and waits for it and for every other outstanding load
// (vmcnt(0)), which would expose the next group's stage DMA and item loads at
// the first barrier after they are issued.  Only this wave's own LDS
// operations are completed here (lgkmcnt(0)); the asm's memory clobber keeps
// the compiler from moving memory operations across it.  The stage and the
// prefetched item fields are waited for explicitly (vmcnt(0)) before the
// copy-out, and the next iteration's first barrier orders every wave's wait
// before any read of the stage.
__device__ __forceinline__ void group_barrier_lds() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

#ifdef LSM_DIAG
// Diagnostic per-phase cycle totals of wave 0 of every group workgroup
// (kDiagGroupPhases; read by lsm_diag_encode_phases).
#define ENC_PHASE(i)                                 \
  if (P.diag & kDiagGroupPhases) {                              \
    const uint64_t t_ = __builtin_amdgcn_s_memtime(); \
    ph_acc[i] += (uint32_t)(t_ - t_last);            \
    t_last = t_;                                     \
  }
#else
#define ENC_PHASE(i)
#endif

// ---- the fused plan's run offsets: a decoupled look-back over the runs (one word per
// run in P.sizes, cleared before the launch): bits 62-63 the state (1: this run's own
// bytes, 2: the inclusive prefix through this run), bit 61 poison, bits 0-60 the value
// (output bytes in bits 0-39, listed blocks above, as P.sizes' words).  A run publishes
// its own total as soon as its plan is done, before it looks back, and looks back only
// at lower runs, which were dispatched before it: every wait ends.  The wait is also
// bounded in time (100 ms without progress): a run that gives up publishes poison, and
// its blocks and every later run's report LSM_INCOMPLETE instead of bytes at a wrong
// offset.
constexpr uint64_t kLbAgg = 1ULL << 62, kLbIncl = 2ULL << 62, kLbPoison = 1ULL << 61, kLbVal = kLbPoison - 1;
constexpr uint64_t kLookbackTicks = 10000000;  // s_memrealtime runs at 100 MHz

__device__ __forceinline__ uint64_t lb_load(const uint64_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void lb_store(uint64_t* p, uint64_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One wave: publishes `agg` for `run`, returns the sum of the runs before it.
__device__ __noinline__ uint64_t run_lookback(uint64_t* lb, uint32_t run, uint64_t agg, uint32_t diag, bool& poisoned) {
  const int lane = threadIdx.x & (kWave - 1);
  if (lane == 0) lb_store(lb + run, (run == 0 ? kLbIncl : kLbAgg) | agg);
  uint64_t excl = 0;
  bool poison = false;
  if (run != 0) {
    int64_t top = (int64_t)run - 1;  // lane l looks at run top - l
    uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    for (;;) {
      const int64_t idx = top - lane;
      const uint64_t v = idx >= 0 ? lb_load(lb + idx) : kLbIncl;  // (before run 0: an inclusive 0)
      const uint64_t incl_m = __ballot((v >> 62) == 2), ready_m = __ballot((v >> 62) != 0);
      const uint32_t stop = incl_m ? (uint32_t)__builtin_ctzll(incl_m) : 64u;  // the nearest inclusive prefix
      const uint64_t need = stop >= 63 ? ~0ULL : (2ULL << stop) - 1;
      if ((ready_m & need) == need && !(kDiagBuild && (diag & kDiagLookbackGiveUp))) {
        const bool mine = (uint32_t)lane <= stop;
        poison = poison || __ballot(mine && (v & kLbPoison)) != 0;
        excl += wave_bcast_u64(wave_incl_scan_u64(mine ? (v & kLbVal) : 0), kWave - 1);
        if (stop < 64) break;
        top -= 64;
        t0 = __builtin_amdgcn_s_memrealtime();
        continue;
      }
      if (__builtin_amdgcn_s_memrealtime() - t0 > kLookbackTicks || (kDiagBuild && (diag & kDiagLookbackGiveUp))) {
        poison = true;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
    if (lane == 0) lb_store(lb + run, kLbIncl | (poison ? kLbPoison : 0) | ((excl + agg) & kLbVal));
  }
  poisoned = poison;
  return excl;
}

// v of lane l (clamped to the wave)
__device__ __forceinline__ uint32_t lane_u32(uint32_t v, uint32_t l) {
  return (uint32_t)__shfl((int)v, (int)min(l, 63u));
}
__device__ __forceinline__ uint64_t lane_u64(uint64_t v, uint32_t l) { return wave_shfl_u64(v, (int)min(l, 63u)); }
// the same for a wave-uniform lane index: v_readlane into a scalar register
__device__ __forceinline__ uint32_t rl32(uint32_t v, uint32_t l) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)min(l, 63u));
}
__device__ __forceinline__ uint64_t rl64(uint64_t v, uint32_t l) {
  const int q = (int)min(l, 63u);
  return (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, q) |
         ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), q) << 32);
}
// Groups of few items (16 KiB blocks of long values: 56 items) give each item 2 or 4 threads
// (tpi = 1 << tsh), which split its value copy; thread t serves item t >> tsh, part t & (tpi - 1).
__device__ __forceinline__ uint32_t tpi_shift(uint32_t n) {
  return n <= kGThreads / 4 ? 2u : n <= kGThreads / 2 ? 1u : 0u;
}
// a group-class item's derived fields (the plan pass has vetted every one: no `bad` checks here)
template <bool kIndex, class Raw>
__device__ __forceinline__ ItemMeta cook_vetted(const Raw& r) {
  bool bad = false;
  return cook_item<kIndex>(r, bad);
}

// kIndex: index blocks (restart interval 1, handle fields); kHash: the batch
// has hash indexes (hash ratio > 0).  Both are batch-wide, so the paths a
// batch never takes are compiled out (their registers would spill the
// common path: every scratch reload waits for all outstanding loads).
// The kernel is one function on purpose: its three parts (the run registers' prologue, the
// wave-per-block loop, the group loop) share the run registers r_* through capturing lambdas.  As
// functions of their own over a struct of those registers they compiled to other code: the group
// loop's instruction stream changed in every instantiation, and the wave loop's extraction changed
// the VGPR count of the diagnostic build (profiles/encode_split_isa.txt, section 3).
template <bool kIndex, bool kHash, bool kPlanBkt, int kOW, bool kFused = false>
__global__ __launch_bounds__(kGThreads) __attribute__((amdgpu_waves_per_eu(4))) void encode_group_kernel(EncodeParams P) {
  static_assert(!kFused || (!kIndex && !kHash), "the fused plan is for data blocks without a hash index");
  __shared__ GroupLds L;
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int lane = tid & (kWave - 1);
  constexpr uint32_t kRun = kFused ? kGRunFused : kGRun;
  const uint32_t b_begin = blockIdx.x * kRun;
  const uint32_t b_end = min(b_begin + kRun, P.n_blocks);
  const uint32_t ri = kIndex ? 1 : P.ri;
  constexpr bool index = kIndex;
  if (tid < sizeof(LongSecret) / 8)
    reinterpret_cast<uint64_t*>(&L.secret)[tid] = reinterpret_cast<const uint64_t*>(&kLongSecret)[tid];
  // the run's blocks, lane l = block b_begin + l (every wave holds the same registers)
  const uint32_t rb = b_begin + lane;
  const bool in_run = rb <= b_end;
  const uint32_t r_start = in_run ? P.starts[rb] : 0;
  uint64_t r_off, r_ks, r_vs;
  BlockPlan r_plan;
  bool run_ok = true;
  if (kFused) {
    // the plan pass's code on this run's blocks (its LDS over the stage, before the first
    // DMA), then the run's output offset by the look-back: no plan launch, no size scan,
    // and the item fields and keys this loop reads again are the ones the plan just read
    BlockPlan* const fplan = reinterpret_cast<BlockPlan*>(L.uni);               // [kRun]
    uint64_t* const fsize = reinterpret_cast<uint64_t*>(L.uni) + 2 * kRun;      // [kRun]
    uint64_t* const fbase = fsize + kRun;                                       // prefix, poison
    plan_wave_run<false, kOW, true>(P, b_begin, b_end - b_begin, *reinterpret_cast<PlanWaveLds*>(L.vals), fplan,
                                    fsize);
    __syncthreads();
    r_plan = rb < b_end ? fplan[lane] : BlockPlan{0, 0, 0, 0};
    const uint64_t sz = rb < b_end ? fsize[lane] : 0;
    const uint64_t incl = wave_incl_scan_u64(sz);
    if (wave == 0) {
      bool poisoned;
      const uint64_t base = run_lookback(P.sizes, blockIdx.x, wave_bcast_u64(incl, kWave - 1), P.diag, poisoned);
      if (lane == 0) {
        fbase[0] = base;
        fbase[1] = poisoned ? 1 : 0;
      }
    }
    __syncthreads();
    const uint64_t ex = fbase[0] + incl - sz;
    run_ok = fbase[1] == 0;
    r_off = in_run ? (ex & kOffMask) : 0;
    if (wave == 0 && rb < b_end) {
      P.block_off[rb] = r_off;
      if (!run_ok) P.status[rb] = ST_INCOMPLETE;
      else if (sz & ~kOffMask) P.lists[ex >> 40] = rb;
    }
    if (wave == 0 && rb == b_end && b_end == P.n_blocks) {  // the last run: the total and the list length
      P.block_off[rb] = r_off;
      P.list_count[0] = run_ok ? (uint32_t)(ex >> 40) : 0u;
    }
    const uint32_t cs = in_run ? clamped_start(P, rb) : 0;
    r_ks = in_run ? koff<kOW>(P, cs) : 0;
    r_vs = in_run ? voff<kOW>(P, cs) : 0;
    __syncthreads();  // (L.uni is the group loop's from here)
  } else {
    r_off = in_run ? P.block_off[rb] : 0;
    r_ks = in_run ? P.kspan[rb] : 0;
    r_vs = in_run ? P.vspan[rb] : 0;
    r_plan = (in_run && rb < b_end) ? P.plans[rb] : BlockPlan{0, 0, 0, 0};
  }
  const uint32_t r_hash = r_plan.hash_w;
  const uint32_t r_hpre = wave_incl_scan_u32(r_hash) - r_hash;  // exclusive prefix over the run
  // payload hash units (1 KiB, long path only) per block, exclusive prefix over the run
  uint32_t r_upre;
  {
    const uint64_t nx = wave_shfl_u64(r_off, min(lane + 1, 63));
    const uint32_t plen = (rb < b_end) ? (uint32_t)(nx - r_off) - kHdrLen : 0;
    const uint32_t units = plen > 240 ? (plen - 1) / 1024 + 1 : 0;
    r_upre = wave_incl_scan_u32(units) - units;
  }
  struct Grp {
    uint32_t b, k;
  };
  // the longest group from block b (k = 0: block b is listed / rejected / over capacity)
  auto form = [&](uint32_t b) -> Grp {
    const uint32_t r0 = b - b_begin, rj = r0 + lane;
    const uint32_t s0 = rl32(r_start, r0), s1 = lane_u32(r_start, rj + 1);
    const uint64_t o0 = rl64(r_off, r0), o1 = lane_u64(r_off, rj + 1);
    const uint64_t k0 = rl64(r_ks, r0), k1 = lane_u64(r_ks, rj + 1);
    const uint64_t v0 = rl64(r_vs, r0), v1 = lane_u64(r_vs, rj + 1);
    const uint32_t flags = lane_u32(r_plan.step_flags, rj) >> 8;
    const uint32_t hsum = lane_u32(r_hpre, rj + 1) - rl32(r_hpre, r0);
    const bool ok = b + lane < b_end && lane < (int)kGBlocks && flags == 0 && o1 <= P.out_cap &&
                    group_fits(s1 - s0, k1 - (k0 & ~15ULL), v1 - (v0 & ~15ULL), o1 - (o0 & ~15ULL), hsum);
    return Grp{b, (uint32_t)__builtin_ctzll(~__ballot(ok))};
  };
  // the run's group-class blocks (listed / rejected ones are passed over at once)
  const uint64_t gmask = __ballot(rb < b_end && (r_plan.step_flags >> 8) == 0);
  auto next_group = [&](uint32_t b) -> Grp {
    for (;;) {
      if (b >= b_end) return Grp{b, 0};
      const Grp g = form(b);
      if (g.k) return g;
      const uint64_t rest = gmask >> (b - b_begin);
      if (rest & 1) {
        if (lane == 0) P.status[b] = ST_OVERFLOW;  // group class, but past out_cap
        ++b;
      } else {
        b = rest ? b + (uint32_t)__builtin_ctzll(rest) : b_end;
      }
    }
  };
  auto issue_dma = [&](const Grp& g) {
    const uint32_t r0 = g.b - b_begin;
    const uint64_t ka = rl64(r_ks, r0) & ~15ULL, kb = rl64(r_ks, r0 + g.k);
    const uint64_t va = rl64(r_vs, r0) & ~15ULL, vb = rl64(r_vs, r0 + g.k);
    const uint32_t kc = (uint32_t)((kb - ka + 15) >> 4), vc = index ? 0 : (uint32_t)((vb - va + 15) >> 4);
    stage_to_lds(P.it.keys + ka, L.keys, kc, wave, kGWaves, lane);
    stage_to_lds(P.it.vals + va, L.vals, vc, wave, kGWaves, lane);
  };
  uint32_t* hlo = L.uni;                           // [kGHash] vote min
  uint32_t* hhi = hlo + kGHash;                    // [kGHash] vote max
  uint64_t* contrib = reinterpret_cast<uint64_t*>(L.uni);  // [kGUnits][4][2] (after the records)

  // item t's raw fields of group g: plain loads, no arithmetic and no branch
  // (threads past the group's items load its last item), so nothing waits
  // for them until the next iteration cooks them (cook_vetted); thread t
  // loads the item it serves (tpi_shift)
  auto load_items = [&](const Grp& g, RawItemT<kOW, kIndex>& r) {
    const uint32_t r0 = g.b - b_begin;
    const uint32_t i0 = rl32(r_start, r0), n = rl32(r_start, r0 + g.k) - i0;
    const uint64_t i = (uint64_t)i0 + min(tid >> tpi_shift(n), n - 1);
    r = load_raw<kIndex, kOW>(P, i);
    r.e = P.erec[i];
    if (kPlanBkt) r.hb = P.hbucket[i];
  };

  // group g's block table (lane j = block j; one wave, every lane active for the shuffles)
  auto build_table = [&](const Grp& g, GBlk* tb) {
    const uint32_t gr0 = g.b - b_begin, gk = g.k;
    const uint32_t gi0 = rl32(r_start, gr0);
    const uint64_t gob = rl64(r_off, gr0);
    const uint32_t gpad = (uint32_t)(((uint64_t)(uintptr_t)P.out + gob) & 15);
    const uint32_t rj = gr0 + lane;
    const uint32_t st = lane_u32(r_start, rj), st1 = lane_u32(r_start, rj + 1);
    const uint64_t of = lane_u64(r_off, rj), of1 = lane_u64(r_off, rj + 1);
    const uint32_t recs = lane_u32(r_plan.recs, rj), bin_len = lane_u32(r_plan.bin_len, rj);
    const uint32_t sf = lane_u32(r_plan.step_flags, rj), hw = lane_u32(r_plan.hash_w, rj);
    const uint32_t hb = lane_u32(r_hpre, rj) - rl32(r_hpre, gr0);
    const bool in = (uint32_t)lane < gk;
    const uint32_t plen = in ? (uint32_t)(of1 - of) - kHdrLen : 0;
    const uint32_t nbk = plen > 240 ? (plen - 1) / 1024 : 0;
    const uint32_t units = plen > 240 ? nbk + 1 : 0;
    const uint32_t u0 = wave_incl_scan_u32(units) - units;
    if (in) {
      GBlk B;
      B.it0 = st - gi0;
      B.n = st1 - st;
      B.img = (uint32_t)(of - gob) + gpad;
      B.plen = plen;
      B.recs = recs;
      B.bin_len = bin_len;
      B.step = sf & 0xFF;
      B.hash_w = hw;
      B.hash_base = hb;
      B.u0 = u0;
      B.nbk = nbk;
      B.spare = 0;
      tb[lane] = B;
    }
  };

  // ---- The wave-per-block loop.  A run whose every block is group-class, has at most
  // kWItems items, fits a wave slot (wave_fits) and ends at or before out_cap is written
  // wave per block: wave w takes blocks w, w + 4, ... of the run, lane = item, the four DPP
  // rows of the wave hash the payload's 1 KiB units, and the wave copies the payload out;
  // once per kWDefer of its blocks a lane quad per block runs the scramble chain and the
  // rest of the checksum and writes the header to the output.  Any other run (listed, bad,
  // oversize or overflowing blocks, mixed batches) takes the group loop below, untouched.
  // The choice is a ballot over the run registers, which every wave holds alike, so it is
  // uniform over the workgroup.
  // SYNCHRONISATION: the loop has no s_barrier, no __syncthreads() and no wait on another
  // wave or workgroup; the waves' trip counts differ, so a barrier in it would hang.  The
  // only barrier is the one below, before the loop, after the secret is copied to LDS.
  // Within a wave, LDS writes and reads of different lanes are ordered by wave_lds_wait()
  // (s_waitcnt lgkmcnt(0)), and the stage DMA by an explicit vmcnt(0).
  constexpr bool kWaveLoop = kWaveBlocks && !kIndex && !kHash && !kPlanBkt && !kFused;
  if constexpr (kWaveLoop) {
    bool wave_run;
    {
      const uint32_t s1 = lane_u32(r_start, lane + 1);
      const uint64_t o1 = lane_u64(r_off, lane + 1), k1 = lane_u64(r_ks, lane + 1), v1 = lane_u64(r_vs, lane + 1);
      const bool fit = (r_plan.step_flags >> 8) == 0 && o1 <= P.out_cap &&
                       wave_fits(s1 - r_start, k1 - (r_ks & ~15ULL), v1 - (r_vs & ~15ULL), o1 - (r_off & ~15ULL));
      wave_run = __ballot(rb < b_end && !fit) == 0 &&
                 !(kDiagBuild && (P.diag & (kDiagNoWaveBlocks | kDiagGroupLoopBits)));
    }
    if (wave_run) {
      WaveSlot& W = reinterpret_cast<WaveSlot*>(&L)[wave];
      auto wave_lds_wait = [&]() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); };
      auto wave_dma = [&](uint32_t r) {
        const uint64_t ka = rl64(r_ks, r) & ~15ULL, kb = rl64(r_ks, r + 1);
        const uint64_t va = rl64(r_vs, r) & ~15ULL, vb = rl64(r_vs, r + 1);
        const uint32_t kc = (uint32_t)((kb - ka + 15) >> 4), vc = (uint32_t)((vb - va + 15) >> 4);
        stage_to_lds(P.it.keys + ka, W.keys, kc, 0, 1, lane);
        stage_to_lds(P.it.vals + va, W.vals, vc, 0, 1, lane);
      };
      auto wave_items = [&](uint32_t r, RawItemT<kOW, kIndex>& x) {
        const uint32_t i0 = rl32(r_start, r), n = rl32(r_start, r + 1) - i0;
        const uint64_t i = (uint64_t)i0 + min((uint32_t)lane, n - 1);
        x = load_raw<kIndex, kOW>(P, i);
        x.e = P.erec[i];
      };
      group_barrier_lds();  // the secret is in LDS; the last barrier of this run
      uint32_t r = wave;
      const uint32_t nr = b_end - b_begin;
      RawItemT<kOW, kIndex> raw{};
      if (r < nr) {
        wave_dma(r);
        wave_items(r, raw);
      }
      vm_wait<0>();
      // Deferred checksums and headers: what follows a block's row hashing (the scramble
      // chain, the merge, the avalanche, the header checksum and the header bytes) is one
      // instruction stream for a lane quad, so it runs once per kWDefer blocks of the wave, a
      // quad per block, instead of once per block in all sixteen quads.  Until then the wave
      // keeps, per block, the 40 contribution words of a long payload (lane x: word x, two
      // VGPRs per kept block), or in quad j the finished digest of the j-th kept block's
      // payload of <= 240 B (the short path reads the image, so it runs at block time).
      uint64_t d0 = 0, d1 = 0;
      uint64_t kc[kWDefer] = {};
      uint32_t dn = 0, dr = wave;  // blocks kept since the last flush; the first one's place in the run
      auto flush_headers = [&]() {  // (every lane active: quad_sum64 and the shuffles read other lanes)
        const uint32_t rj = dr + kGWaves * ((uint32_t)lane >> 2);
        const int q = lane & 3;
        const bool in = ((uint32_t)lane >> 2) < dn;
        const uint64_t ob = lane_u64(r_off, rj);
        const uint32_t plen = (uint32_t)(lane_u64(r_off, rj + 1) - ob) - kHdrLen;
        const bool lng = in && plen > 240;
        uint64_t lo = 0, hi = 0;
        // the kept contributions go to the image, which is free after the copy-out, and quad j
        // runs block j's chain over them as the group loop's chain wave does (its batch's
        // read-ahead past a block's units stays inside the kept words, unused)
        constexpr uint32_t kCW = kWUnits * 8;
        uint64_t* const side = reinterpret_cast<uint64_t*>(W.img);
        if ((uint32_t)lane < kCW) {
#pragma unroll
          for (uint32_t s = 0; s < kWDefer; ++s) side[kCW * s + (uint32_t)lane] = kc[s];
        }
        wave_lds_wait();
        if (lng) {
          const uint32_t nbk = (plen - 1) / 1024;
          uint64_t a0, a1;
          xxh3_acc_init(q, a0, a1);
          const uint64_t scr0 = L.secret.acc[16 + 2 * q], scr1 = L.secret.acc[16 + 2 * q + 1];
          static_assert((kWImg - 1) / 1024 <= 4 && 4 <= kWUnits, "nbk <= 4: one batch is the whole chain");
          const uint64_t* cb = side + kCW * ((uint32_t)lane >> 2) + 2 * q;
          const uint64_t t0 = cb[8 * nbk], t1 = cb[8 * nbk + 1];
          xxh3_quad_chain_batch<4>(cb, 0, nbk, scr0, scr1, a0, a1);
          d0 = a0 + t0;
          d1 = a1 + t1;
        }
        if (lng) xxh3_merge_part(&L.secret, q, d0, d1, lo, hi);
        lo = quad_sum64(lo);
        hi = quad_sum64(hi);
        if (in) {
          if (lng) {
            xxh3_finish128(plen, lo, hi, lo, hi);
          } else {
            lo = d0;
            hi = d1;
          }
          write_header_quad((__attribute__((address_space(1))) uint8_t*)(P.out + ob), 0, P.type, lo, hi, plen, q);
          if (q == 0) P.status[b_begin + rj] = ST_OK;
        }
      };
      while (r < nr) {
        const uint32_t i0 = rl32(r_start, r), n = rl32(r_start, r + 1) - i0;
        const uint64_t kbase = rl64(r_ks, r) & ~15ULL, vbase = rl64(r_vs, r) & ~15ULL;
        const uint64_t obase = rl64(r_off, r);
        const uint32_t total = (uint32_t)(rl64(r_off, r + 1) - obase), plen = total - kHdrLen;
        const uint32_t recs = rl32(r_plan.recs, r), bin_len = rl32(r_plan.bin_len, r);
        const uint32_t step = rl32(r_plan.step_flags, r) & 0xFF;
        const uint64_t dabs = (uint64_t)(uintptr_t)P.out + obase;
        const uint32_t pad = (uint32_t)(dabs & 15), p0 = pad + kHdrLen;
        const uint32_t rn = r + kGWaves;
        const bool more = rn < nr;
        // the next block's item fields: in flight under this whole block
        ItemMeta m = cook_vetted<kIndex>(raw);
        if (more) wave_items(rn, raw);
        // ---- lane = item: its record into the image (the group loop's one-thread writer)
        {
          const bool live = (uint32_t)lane < n;
          const bool head = (m.e & kErecHead) != 0;
          m.sh = head ? 0u : m.e >> 16;
          const uint32_t roff = m.e & 0x7FFFu, from = head ? 0 : m.sh;
          const uint32_t kst = (uint32_t)(m.ko - kbase), vsrc = (uint32_t)(m.vo - vbase);
          const bool has_val = live && !is_tombstone(m.vt);
          uint32_t vpos = 0;
          if (live) vpos = put_record_header<false>(W.img, p0 + roff, W.keys, kst, m, head, from, lane);
          const uint32_t done = lds_copy_uniform(W.img, vpos, W.vals, vsrc, m.vl, has_val && m.vl != 0, lane);
          if (live) {
            if (has_val) lds_copy(W.img, vpos, W.vals, vsrc, m.vl, lane, done);
            if (head) put_bin_entry(W.img, p0 + recs + 1 + (m.e >> 16) * step, step, roff);
          }
        }
        // ---- marker and trailer
        if (lane == 0) W.img[p0 + recs] = kTrailerMarker;
        write_trailer_bytes(W.img, p0 + plen - kTrailerLen, ri, step, bin_len, recs + 1, 0, 0, n);
        wave_lds_wait();
        // the stage is free: the next block's DMA runs under the hash, the chain and the copy-out
        if (more) wave_dma(rn);
        // ---- payload xxh3_128: the wave's four DPP rows take the 1 KiB units
        if (plen > 240) {
          const uint32_t nbk = (plen - 1) / 1024;
          {
            const uint32_t row = (uint32_t)lane >> 4, rr = lane & 15;
            for (uint32_t u = row; u <= nbk; u += 4) {
              uint64_t c0, c1;
              xxh3_row_unit(W.img, p0, plen, nbk, u, rr, &L.secret, c0, c1);
              if (rr < 4) {
                W.contrib[8 * u + 2 * rr] = c0;
                W.contrib[8 * u + 2 * rr + 1] = c1;
              }
            }
          }
          wave_lds_wait();
          // the block's contributions, lane x word x, into the registers of kept block dn
          {
            const uint64_t cv = W.contrib[min((uint32_t)lane, kWUnits * 8 - 1)];
#pragma unroll
            for (uint32_t s = 0; s < kWDefer; ++s) kc[s] = dn == s ? cv : kc[s];
          }
        } else if (((uint32_t)lane >> 2) == dn) {  // (the short path reads the image, so it runs now)
          xxh3_128_short(plen, BaseReader8{W.img, p0}, BaseReader64{W.img, p0}, d0, d1);
        }
        ++dn;
        // the next block's DMA pieces and item fields, before this block's stores are
        // issued: the stores never count in this wait
        vm_wait<0>();
        // ---- copy-out of the payload [p0, end); the header's 33 bytes are stored by
        // flush_headers alone, so no output byte is stored twice.  The whole 16-B pieces
        // [ch, c1) past the header, then the partial pieces at the payload's two ends with
        // one masked byte store each (lane x stores byte x of the piece; the rest of those
        // pieces is header, or belongs to the next block)
        {
          const uint32_t end = pad + total, ch = (p0 + 15) >> 4, c1 = end >> 4;
          const u32x4* const csrc = reinterpret_cast<const u32x4*>(W.img);
          u32x4* const cdst = reinterpret_cast<u32x4*>(dabs & ~15ULL);
          for (uint32_t c = ch + (uint32_t)lane; c < c1; c += kWave)
            *(__attribute__((address_space(1))) u32x4*)(cdst + c) = csrc[c];
          auto* gb = (__attribute__((address_space(1))) uint8_t*)cdst;
          const uint32_t x = (uint32_t)lane;
          if (p0 + x < min(16 * ch, end)) gb[p0 + x] = W.img[p0 + x];
          if (c1 >= ch && 16 * c1 + x < end) gb[16 * c1 + x] = W.img[16 * c1 + x];
        }
        wave_lds_wait();  // (the image is read out before the next block's records are written)
        if (dn == kWDefer || !more) {
          flush_headers();
          dn = 0;
          dr = rn;
        }
        r = rn;
      }
      return;
    }
  }

  // Software pipeline: group G's stage DMA and item fields are issued one
  // group ahead and waited for (vmcnt(0)) just before the previous group's
  // copy-out, so no group waits on HBM latency after its stores.
#ifdef LSM_DIAG
  uint64_t t_last = __builtin_amdgcn_s_memtime();
  uint32_t ph_acc[12] = {};
  uint32_t ph_n = 0;
#endif
  Grp G = run_ok ? next_group(b_begin) : Grp{b_end, 0};
  RawItemT<kOW, kIndex> raw{};
  if (G.k) {
    issue_dma(G);
    load_items(G, raw);
    if (wave == 0) build_table(G, L.blk[0]);  // (later tables are built under the previous chain)
  }
  vm_lgkm_wait0();  // the first group's DMA pieces and item fields
  ENC_PHASE(11);
  uint32_t iter = 0;  // rotates the chain wave over the SIMDs
  while (G.k) {
    ENC_PHASE(0);
    const uint32_t r0 = G.b - b_begin, k = G.k;
    const uint32_t i0 = rl32(r_start, r0), n_items = rl32(r_start, r0 + k) - i0;
    const uint64_t kbase = rl64(r_ks, r0) & ~15ULL, vbase = rl64(r_vs, r0) & ~15ULL;
    const uint64_t obase = rl64(r_off, r0);
    const uint64_t dabs = (uint64_t)(uintptr_t)P.out + obase;
    const uint32_t pad = (uint32_t)(dabs & 15);
    const uint32_t tsh = tpi_shift(n_items), part = tid & ((1u << tsh) - 1), item = tid >> tsh;
    const bool live = item < n_items;
    // the next group's item fields: in flight under this whole group
    const Grp Gn = next_group(G.b + k);
    ItemMeta m = cook_vetted<kIndex>(raw);
    if (Gn.k) load_items(Gn, raw);
    ENC_PHASE(9);
    GBlk* const TB = L.blk[iter & 1];  // this group's block table (built one group ahead)
    // (shuffles only with every lane active: a bpermute from an inactive lane is undefined)
    const uint32_t hsum = rl32(r_hpre, r0 + k) - rl32(r_hpre, r0);
    for (uint32_t h = tid; h < hsum; h += kGThreads) {
      hlo[h] = 0xFFFFFFFFu;
      hhi[h] = 0;
    }
    group_barrier_lds();
    ENC_PHASE(1);
    // ---- item t: its block (record offset and shared prefix from E1)
    // (block starts from the run registers, v_readlane: no LDS round trip)
    uint32_t j = 0;
    for (uint32_t jb = 1; jb < k; ++jb) j += (rl32(r_start, r0 + jb) - i0 <= item) ? 1u : 0u;
    const bool head = (m.e & kErecHead) != 0;
    m.sh = head ? 0u : m.e >> 16;
    // ---- item t: its record into the image (one thread per item, or for
    // groups of few items tpi threads per item splitting the value copy)
    // Two writers on purpose: the split one (tsh > 0) also covers tsh = 0, but as
    // the only writer it measured 0.6 % slower on configs[1] and 0.5 % on
    // configs[3] (3.237 vs 3.218 ms, 3.131 vs 3.115 ms; profiles/r03_encode_experiments.txt).
    // They share the header (put_header), the binary-index entry and hash vote,
    // and the value copy: once the header is written (for the parts past the first,
    // once its length is computed) every lane knows where its value goes, so
    // between the writers' `if (writes)` regions, with every lane active,
    // lds_copy_uniform copies the interior dwords common to the wave's values
    // (DESIGN §6.7), and lds_copy finishes each lane's head bytes, surplus dwords
    // and tail bytes.
    const bool writes = live && !(kDiagBuild && (P.diag & (kDiagNoRecordStores | kDiagNoRecordsTails)));
    const uint32_t roff = m.e & 0x7FFFu;
    const uint32_t from = head ? 0 : m.sh;
    const uint32_t kst = (uint32_t)(m.ko - kbase);
    const bool has_val = writes && !index && !is_tombstone(m.vt);
    const uint32_t vsrc = (uint32_t)(m.vo - vbase);
    // type byte, varints, key (suffix), value length: up to the value, whose place it returns
    auto put_header = [&]() -> uint32_t {
      return put_record_header<index>(L.img, TB[j].img + kHdrLen + roff, L.keys, kst, m, head, from, lane);
    };
    auto put_index_and_vote = [&]() {
      const GBlk& B = TB[j];
      if (head) put_bin_entry(L.img, B.img + kHdrLen + B.recs + 1 + (m.e >> 16) * B.step, B.step, roff);
      if (kHash && B.hash_w) {
        const uint32_t ridx = (item - B.it0) / ri;
        const uint32_t hb =
            kPlanBkt ? m.hb
                     : (uint32_t)(xxh3_64_any(m.klen, BaseReader8{L.keys, kst}, BaseReader64{L.keys, kst}) % B.hash_w);
        const uint32_t bk = B.hash_base + hb;
        atomicMin(&hlo[bk], ridx);
        atomicMax(&hhi[bk], ridx);
      }
    };
    constexpr bool uniform = !index;
    if (tsh == 0) {
      uint32_t vpos = 0;
      if (writes) vpos = put_header();
      const uint32_t done =
          uniform ? lds_copy_uniform(L.img, vpos, L.vals, vsrc, m.vl, has_val && m.vl != 0, lane) : 0u;
      if (writes) {
        if (has_val) lds_copy(L.img, vpos, L.vals, vsrc, m.vl, lane, done);
        put_index_and_vote();
      }
    } else {
      // the value: part q copies bytes [q vl / tpi, (q + 1) vl / tpi)
      const uint32_t va = (part * m.vl) >> tsh, vb = ((part + 1) * m.vl) >> tsh;
      uint32_t vpos = 0;
      if (writes) {
        if (part == 0)
          vpos = put_header();
        else if (has_val)
          vpos = TB[j].img + kHdrLen + roff + 1 + leb_len(m.seq) + (head ? 0u : leb_len(m.sh)) + leb_len(m.klen - from) +
                 (m.klen - from) + leb_len(m.vl);
      }
      const uint32_t done =
          uniform ? lds_copy_uniform(L.img, vpos + va, L.vals, vsrc + va, vb - va, has_val && vb != va, lane) : 0u;
      if (writes) {
        if (has_val) lds_copy(L.img, vpos + va, L.vals, vsrc + va, vb - va, lane, done);
        if (part == 0) put_index_and_vote();
      }
    }
    // ---- tails, wave per block: marker, hash-index bytes, trailer (trailer.rs:78-173);
    // without hash indexes they need nothing from the other waves' records
    // (disjoint bytes), so they go before the barrier
    auto tails = [&]() {
      for (uint32_t jb = wave; jb < (kDiagBuild && (P.diag & kDiagNoRecordsTails) ? 0 : k); jb += kGWaves) {
        const GBlk& B = TB[jb];
        const uint32_t p0 = B.img + kHdrLen, bin_off = B.recs + 1;
        if (lane == 0) L.img[p0 + B.recs] = kTrailerMarker;
        const uint32_t hash_off = B.hash_w ? bin_off + B.bin_len * B.step : 0;
        if (kHash)
          for (uint32_t q = lane; q < B.hash_w; q += kWave)
            L.img[p0 + hash_off + q] = (uint8_t)bucket_byte(hlo[B.hash_base + q], hhi[B.hash_base + q]);
        write_trailer_bytes(L.img, p0 + B.plen - kTrailerLen, ri, B.step, B.bin_len, bin_off, B.hash_w, hash_off,
                            B.n);
      }
    };
    if (!kHash) tails();
    group_barrier_lds();
    ENC_PHASE(3);
    // the stage is free: the next group's DMA runs under the tails and the hash
    if (Gn.k && !(kDiagBuild && (P.diag & kDiagNoNextDma))) issue_dma(Gn);
    ENC_PHASE(10);
    if (kHash) {  // the hash-index bytes need every vote
      tails();
      group_barrier_lds();
    }
    ENC_PHASE(4);
    // ---- payload xxh3_128: 1 KiB units over the 16 DPP rows
    {
      const uint32_t row = wave * 4 + (lane >> 4), r = lane & 15, q = r & 3;  // (4 kGWaves rows)
      const uint32_t ubase = rl32(r_upre, r0);
      const uint32_t units =
          (kDiagBuild && (P.diag & (kDiagNoHash | kDiagNoRecordsTails))) ? 0 : rl32(r_upre, r0 + k) - ubase;
      for (uint32_t u = row; u < units; u += 4 * kGWaves) {
        uint32_t jb = 0;  // (unit starts from the run registers: no dependent LDS reads)
        for (uint32_t x = 1; x < k; ++x) jb += (rl32(r_upre, r0 + x) - ubase <= u) ? 1u : 0u;
        const GBlk& B = TB[jb];
        uint64_t c0, c1;
        xxh3_row_unit(L.img, B.img + kHdrLen, B.plen, B.nbk, u - B.u0, r, &L.secret, c0, c1);
        if (r < 4) {
          contrib[8 * u + 2 * q] = c0;
          contrib[8 * u + 2 * q + 1] = c1;
        }
      }
    }
    group_barrier_lds();
    ENC_PHASE(5);
    // ---- one wave, a lane quad per block (k <= 16): the scramble chain and
    // the merge (or the short path), then the header.  Lane q of the quad
    // holds accumulator pair q; the chain is one instruction stream for all
    // the group's blocks.
    // The copy-out runs in two parts: the waves other than the chain wave store every whole
    // 16-B piece of the span that holds no header byte while the chain wave computes the
    // checksums and headers; after the barrier the header pieces (three per block) and the
    // partial pieces at both ends follow.  (Before, the whole copy-out waited for the chain.)
    const uint32_t cw = iter & (kGWaves - 1);  // the chain wave of this group
    const uint32_t total = (uint32_t)(rl64(r_off, r0 + k) - obase);
    const uint32_t end = (kDiagBuild && (P.diag & kDiagNoCopyOut)) ? pad : pad + total;
    const uint32_t c0 = (pad + 15) >> 4, c1 = end >> 4;  // the whole 16-B pieces [c0, c1)
    const u32x4* const csrc = reinterpret_cast<const u32x4*>(L.img);
    u32x4* const cdst = reinterpret_cast<u32x4*>(dabs & ~15ULL);
    // the chain wave's header pieces
    const uint32_t hpc = (wave == cw && (uint32_t)lane < 3 * k) ? (TB[lane / 3].img >> 4) + lane % 3 : ~0u;
    if (wave == cw) {
      if (!(kDiagBuild && (P.diag & (kDiagNoHash | kDiagNoRecordsTails)))) {
        const uint32_t jb = (uint32_t)lane >> 2;
        const int q = lane & 3;
        const bool in = jb < k;
        const GBlk& B = TB[in ? jb : 0];
        const uint32_t p0 = B.img + kHdrLen, plen = B.plen;
        uint64_t lo = 0, hi = 0;
        if (in && plen > 240) {
          uint64_t a0, a1;
          xxh3_acc_init(q, a0, a1);
          const uint64_t scr0 = L.secret.acc[16 + 2 * q], scr1 = L.secret.acc[16 + 2 * q + 1];
          const uint64_t* cb = contrib + 8 * B.u0 + 2 * q;
          // (the batches' read-ahead past the block: other contributions in L.uni, unused)
          xxh3_quad_chain<4>(cb, B.nbk, scr0, scr1, a0, a1);
          a0 += cb[8 * B.nbk];
          a1 += cb[8 * B.nbk + 1];
          xxh3_merge_part(&L.secret, q, a0, a1, lo, hi);
        }
        lo = quad_sum64(lo);  // (every lane: DPP reads of inactive lanes are undefined)
        hi = quad_sum64(hi);
        if (in) {
          if (plen > 240) {
            xxh3_finish128(plen, lo, hi, lo, hi);
          } else {
            xxh3_128_short(plen, BaseReader8{L.img, p0}, BaseReader64{L.img, p0}, lo, hi);
          }
          write_header_quad(L.img, B.img, P.type, lo, hi, plen, q);
          if (q == 0) P.status[G.b + jb] = ST_OK;
        }
      }
    } else {  // (no vmcnt wait here: the next group's DMA may still be landing)
      // the next group's block table, into the other buffer, by the wave after the chain wave
      if (Gn.k && wave == ((cw + 1) & (kGWaves - 1))) build_table(Gn, L.blk[(iter + 1) & 1]);
      const uint32_t t3 = ((wave + kGWaves - cw - 1) & (kGWaves - 1)) * kWave + (uint32_t)lane;  // 0 .. 191
      constexpr uint32_t kT3 = (kGWaves - 1) * kWave;
      // block j's header pieces are [hc_j, hc_j + 3) (33 bytes from any offset); its
      // header-free pieces run from hc_j + 3 to the next block's hc
      uint32_t hc = __builtin_amdgcn_readfirstlane(TB[0].img) >> 4;
      for (uint32_t jb = 0; jb < k; ++jb) {
        const uint32_t hn = jb + 1 < k ? __builtin_amdgcn_readfirstlane(TB[jb + 1].img) >> 4 : c1;
        for (uint32_t c = max(hc + 3, c0) + t3; c < min(hn, c1); c += kT3)
          *(__attribute__((address_space(1))) u32x4*)(cdst + c) = csrc[c];  // (plain stores, r06)
        hc = hn;
      }
    }
    group_barrier_lds();
    ENC_PHASE(6);
    vm_lgkm_wait0();  // the next group's DMA pieces and item fields (vmcnt(0); the call waits on lgkmcnt as well)
    ENC_PHASE(7);
    // ---- copy-out, part 2: the header pieces and the partial pieces at both ends
    {
      if (hpc >= c0 && hpc < c1) *(__attribute__((address_space(1))) u32x4*)(cdst + hpc) = csrc[hpc];
      // (shared with the neighbouring groups' bytes)
      auto* gb = (__attribute__((address_space(1))) uint8_t*)cdst;
      if (tid == 0)
        for (uint32_t x = pad; x < min(16 * c0, end); ++x) gb[x] = L.img[x];
      if (tid == kWave && c1 >= c0)
        for (uint32_t x = 16 * c1; x < end; ++x) gb[x] = L.img[x];
    }
    ENC_PHASE(8);
#ifdef LSM_DIAG
    ++ph_n;
#endif
    ++iter;
    G = Gn;
  }
#ifdef LSM_DIAG
  if ((P.diag & kDiagGroupPhases) && tid == 0) {
    for (int i = 0; i < 12; ++i) atomicAdd(&P.phase[i], (unsigned long long)ph_acc[i]);
    atomicAdd(&P.phase[15], (unsigned long long)ph_n);
  }
#endif
}

// (instantiated in encode_large.hip, with the other callers of xxh3_64_long_lane)
extern template __global__ void encode_group_kernel<false, true, false, 4, false>(EncodeParams);
extern template __global__ void encode_group_kernel<false, true, false, 8, false>(EncodeParams);

}  // namespace lsmgpu
