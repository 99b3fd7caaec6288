// decode_huge.hip — the listed blocks of the decode path: the huge-block pool path (plan, unit
// table, work units with streamed chains, chain pass) and, from decode_big.hpp, the big-block
// kernel and the general path, with every launcher of these stages.
//
// One unit for all three: before it inlines them, the device compiler propagates constants and
// value ranges into the helpers of decode_common.hpp (phase_a<true> / phase_b<.., true>,
// walk_interval_at, xxh3_kib_contribs, stage_to_lds, ...) from ALL their call sites in a unit.
// The big-block, general-path and huge kernels share those helpers, and with any of the three
// compiled apart the others come out with other register allocation and schedules
// (profiles/decode_split_isa.txt); together they are bit for bit what the one-unit decode.hip
// gave.  The group kernel shares none of them with other arguments (decode_group.hip).
#include "decode_big.hpp"

namespace lsmgpu {

// ---- Blocks larger than the general path's stage across the whole GPU (the
// writer's up-to-4-MiB data blocks, writer/mod.rs:193-198; full block
// indexes): decode_chunked walks such a block on ONE workgroup, chunk by
// chunk.  Here its work is cut into units that any workgroup takes:
//   plan   (decode_huge_plan_kernel, one workgroup, after decode_big_kernel lists them):
//          per huge block the header (incl. its checksum) and trailer views
//          from HBM, its KiB-block and parse-unit counts, prefix sums of both
//          over the list (contributions in the workspace pool: 64 B per KiB)
//   units  (decode_huge_units_kernel, thread per restart interval): per unit
//          the first interval that starts in it and that interval's offset
//   work   (decode_huge_kernel, every CU): units = kHugeWin-byte windows of a
//          block's span.  A unit stages its window (+ kHugeOverlap) in LDS by
//          LDS-DMA, takes the restart intervals that start in it from the unit
//          table (a block whose binary index is not monotone: a 256-way search
//          of the index in HBM, two or three round trips),
//          walks them from LDS (thread per interval, walk_interval_at: every
//          oracle check, the LEB cursor for rare shapes; from HBM when one
//          runs past the staged bytes) and computes the XXH3 contributions
//          of the KiB blocks that start in the window, from LDS too
//   chain  (inside decode_huge_kernel: its first workgroups): one wave per
//          block, the eight accumulator chains on lanes 0..7 (xxh3_chain8)
//          over the KiB contributions as the units publish them (unit-done
//          flags), then the tail merge, the checksum compare and the status
// A block whose header fails, or that no longer fits the pool, goes to the
// general path (defer2) as before: statuses and outputs are the same on both.
constexpr uint32_t kHugeWin = 32 * 1024;  // span bytes per unit
constexpr uint32_t kHugeOverlap = ((8 * 1024 - 256));  // staged past the window (intervals that straddle it)
constexpr uint32_t kHugeStage = kHugeWin + kHugeOverlap;
constexpr uint32_t kHugeMaxIv = 512;                   // intervals per window for phase A / B (else thread walks)
constexpr uint32_t kHugeTile = 32 * 32;  // items per window for phase A / B
constexpr uint32_t kHugeBix = kHugeStage + kStagePad;  // LDS: the window's binary-index entries
constexpr uint32_t kHugeMeta = kHugeBix + 4 * (kHugeMaxIv + 4);
constexpr uint32_t kHugeOwner = kHugeMeta + 80;
constexpr uint32_t kHugeRec = kHugeOwner + kHugeMaxIv;
constexpr uint32_t kHugeLds = 64 + kHugeRec + 8 * (kHugeTile + 1);
constexpr uint32_t kHugeWgsPerCU = 3;  // decode_huge_kernel's residency (3 waves per SIMD, ~51 KB of LDS)
constexpr uint32_t kStreamRing = 12;    // the same for the chain waves inside decode_huge_kernel (4 per workgroup)
// A chain wave gives its block up after this long without progress (s_memrealtime ticks, 100 MHz:
// 5 ms, ~25x a whole 4 MiB decode); the block is then re-verified by the fallback chain pass.
constexpr uint64_t kStreamStallTicks = 500000;
constexpr uint32_t kStreamChainWgs = 16;     // chain workgroups: 64 chain waves (a 1 KiB step of 20 ns each)
constexpr uint32_t kStreamMinUnits = 64;     // stream the chains for batches holding a block of >= 2 MiB
constexpr uint32_t kChainRing = 16;          // the chain kernel's ring (KiB of contribution rows in flight per wave)
constexpr uint32_t kHugeChainGrid = 1024;    // chain kernel workgroups (one block each, grid-stride)
constexpr uint32_t kHugeUnitsGrid = 1024;  // unit-table workgroups (thread per restart interval, grid-stride)

struct HugeRec {
  BlockMeta m;         // header view, trailer fields merged in: m.st = trailer status (header checks passed)
  uint64_t span0, item_base;
  uint64_t acc[8];     // chain results (accumulator k from chain wave k)
  uint32_t b, nbk, accepted, parse_bad;
  uint32_t done, span;  // span: the block's 16-B-aligned byte span
  uint32_t nonmono;     // its binary index is not monotone (units kernel): the units search it
  uint32_t pad;
};
static_assert(sizeof(HugeRec) % 16 == 0, "HugeRec layout");

struct HugeHdr {
  uint64_t total_kib;  // contribution rows over every listed block (each block's padded to 16)
  uint32_t n3;         // listed huge blocks (HugeRec entries)
  uint32_t total_pu;   // work units (kHugeWin windows)
  uint64_t total_iv;   // restart intervals + 1 per parsed block (units kernel threads)
  uint32_t max_npu;    // most units of one accepted block
  uint32_t stream;     // chains inside decode_huge_kernel, streaming behind the units (blocks of >= 2 MiB)
};

// Pool: [HugeHdr | 256][kpre, ppre, ipre: u64 x (n + 1) each][HugeRec x n][contributions, 64 B per KiB
// from the front, each block's rows padded to a multiple of 16 (one 1-KiB chain chunk holds no
// other block's rows)] .. [unit table, 16 B per unit, from the back: entry u at uend[-1 - u]:
// first interval, its payload offset, the unit-done flag].
struct HugeLayout {
  HugeHdr* hdr;
  uint64_t* kpre;
  uint64_t* ppre;
  uint64_t* ipre;
  HugeRec* rec;
  uint64_t* contrib;
  uint4* uend;    // unit u: {first restart interval starting in it, that interval's payload offset, done flag}
  uint64_t rest;  // pool bytes after the fixed part
  bool ok;
};
__host__ __device__ constexpr uint64_t huge_fixed_bytes(uint64_t n) {
  return (256 + 24 * (n + 1) + sizeof(HugeRec) * n + 255) & ~255ULL;
}
__device__ __forceinline__ HugeLayout huge_layout(const DecodeParams& P, uint32_t n) {
  HugeLayout L;
  uint8_t* b = P.huge_pool;
  L.hdr = reinterpret_cast<HugeHdr*>(b);
  L.kpre = reinterpret_cast<uint64_t*>(b + 256);
  L.ppre = L.kpre + (n + 1);
  L.ipre = L.ppre + (n + 1);
  L.rec = reinterpret_cast<HugeRec*>(L.ipre + (n + 1));
  const uint64_t fixed = huge_fixed_bytes(n);
  L.contrib = reinterpret_cast<uint64_t*>(b + fixed);
  L.ok = b != nullptr && fixed <= P.huge_pool_bytes;
  L.rest = L.ok ? (P.huge_pool_bytes - fixed) & ~15ULL : 0;
  L.uend = reinterpret_cast<uint4*>(b + fixed + L.rest);
  return L;
}

// Plan over the huge list, by one workgroup of nthr threads (nthr / 64 <= 16
// waves); sh: 56 u64 of LDS; hstage: kHugePlanStage bytes of LDS per thread.
// Blocks it does not accept go to defer2.
constexpr uint32_t kHugePlanStage = 128;
__device__ void huge_plan(const DecodeParams& P, uint64_t* sh, uint32_t nthr, uint8_t* hstage) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = nthr >> 6;
  const uint32_t n = gload(P.defer3_count, 0);
  const HugeLayout L = huge_layout(P, n);
  if (!L.ok) {  // (uniform) no pool, or too small for the records: the general path takes them all
    for (uint32_t i = tid; i < n; i += nthr) defer2_block(P, gload(P.defer3_list, i));
    if (P.huge_pool && P.huge_pool_bytes >= 256 && tid == 0) {
      L.hdr->n3 = 0;
      L.hdr->total_pu = 0;
      L.hdr->total_kib = 0;
      L.hdr->total_iv = 0;
      L.hdr->max_npu = 0;
      L.hdr->stream = 0;
    }
    return;
  }
  const bool hash = !(P.flags & LSM_DECODE_PAYLOAD_VERIFIED);
  if (tid == 0) sh[48] = 0, sh[49] = 0, sh[50] = 0, sh[51] = 0;
  __syncthreads();
  for (uint32_t c = 0; c < n; c += nthr) {
    const uint32_t i = c + tid;
    uint64_t nbk = 0, npu = 0, niv = 0;
    bool acc = false;
    uint32_t b = 0;
    BlockMeta m{};
    uint64_t span0 = 0, item_base = 0, span = 0;
    if (i < n) {
      b = gload(P.defer3_list, i);
      const uint64_t off = gload(P.block_off, b), end = gload(P.block_off, b + 1);
      span0 = off & ~15ULL;
      item_base = gload(P.item_start, b);
      const uint32_t cap = gload(P.item_start, b + 1) - (uint32_t)item_base;
      const uint8_t* gbase = P.blocks + span0;
      // the header's and the trailer's 64-B windows staged in LDS, all eight loads at once (the
      // checks' serial reads then cost LDS round trips, not HBM ones); the trailer copy is
      // addressed span-relative like gbase, and the marker byte before the binary index is read
      // from HBM (blocks here span more than the 72 KiB stage; the input padding covers the reads)
      uint8_t* hs = hstage + kHugePlanStage * tid;
      const uint64_t tend = (max(end, off) + 15) & ~15ULL;
      {
        const u32x4* gh = reinterpret_cast<const u32x4*>(gbase);
        const u32x4* gt = reinterpret_cast<const u32x4*>(P.blocks + tend - 64);
        u32x4 x[8];
#pragma unroll
        for (int q = 0; q < 4; ++q) x[q] = gh[q], x[4 + q] = gt[q];
#pragma unroll
        for (int q = 0; q < 8; ++q) reinterpret_cast<u32x4*>(hs)[q] = x[q];
      }
      const uint8_t* tbase = hs + 128 - (tend - span0);  // (span offset o -> hs[128 - (tend - span0) + o])
      meta_header(hs, (uint32_t)(off - span0), end >= off ? end - off : 0, m);
      acc = m.st == ST_OK;  // every header check, its checksum included
      if (acc) {
        const uint32_t plen = m.len - kHdrLen;
        nbk = hash ? (plen - 1) / 1024 : 0;  // (plen > 72 KiB here: the long path)
        meta_trailer(tbase, P.expect_type, cap, m, P.compact, gbase);  // (after the payload checksum in oracle order)
        span = ((max(end, off) + 15) & ~15ULL) - span0;
        npu = (nbk || m.st == ST_OK) ? (span + kHugeWin - 1) / kHugeWin : 0;
        niv = m.st == ST_OK ? trailer_of(m).bin_len + 1 : 0;  // (+1: the units kernel's end-of-block thread)
      }
    }
    const uint64_t nbk16 = (nbk + 15) & ~15ULL;  // (rows padded to whole 1-KiB chain chunks)
    const uint64_t ik = wave_incl_scan_u64(nbk16), ip = wave_incl_scan_u64(npu), ii = wave_incl_scan_u64(niv);
    if (lane == 63) sh[wave] = ik, sh[16 + wave] = ip, sh[32 + wave] = ii;
    __syncthreads();
    uint64_t bk = sh[48], bp = sh[49], bi = sh[50], tk = 0, tp = 0, ti = 0;
    for (uint32_t w = 0; w < nw; ++w) {
      bk += w < wave ? sh[w] : 0;
      bp += w < wave ? sh[16 + w] : 0;
      bi += w < wave ? sh[32 + w] : 0;
      tk += sh[w];
      tp += sh[16 + w];
      ti += sh[32 + w];
    }
    const uint64_t kp = bk + ik - nbk16, pp = bp + ip - npu, ivp = bi + ii - niv;
    if (i < n) {
      // (the pool holds the contributions, front, and unit entries, back, of a prefix of the list)
      acc = acc && 64 * (kp + nbk16) + 16 * (pp + npu) <= L.rest;
      HugeRec* r = L.rec + i;
      r->m = m;
      r->span0 = span0;
      r->item_base = item_base;
      r->b = b;
      r->nbk = (uint32_t)nbk;
      r->accepted = acc;
      r->parse_bad = 0;
      r->done = 0;
      r->span = (uint32_t)span;
      r->nonmono = 0;
      gstore(L.kpre, i, kp);
      gstore(L.ppre, i, pp);
      gstore(L.ipre, i, ivp);
      if (!acc) defer2_block(P, b);
    }
    {  // the most units of an accepted block: one LDS atomic per wave
      const uint32_t mx = wave_max_u32(i < n && acc ? (uint32_t)npu : 0u);
      if (lane == 0 && mx) atomicMax(reinterpret_cast<unsigned int*>(&sh[51]), mx);
    }
    __syncthreads();
    if (tid == 0) sh[48] += tk, sh[49] += tp, sh[50] += ti;
    __syncthreads();
  }
  if (tid == 0) {
    gstore(L.kpre, n, sh[48]);
    gstore(L.ppre, n, sh[49]);
    gstore(L.ipre, n, sh[50]);
    L.hdr->total_kib = sh[48];
    L.hdr->total_pu = (uint32_t)sh[49];
    L.hdr->total_iv = sh[50];
    L.hdr->max_npu = (uint32_t)sh[51];
    L.hdr->stream = (uint32_t)sh[51] >= kStreamMinUnits;
    L.hdr->n3 = n;
  }
}

__global__ __launch_bounds__(1024) void decode_huge_plan_kernel(DecodeParams P) {
  __shared__ uint64_t sh[56];
  extern __shared__ __attribute__((aligned(16))) uint8_t hstage[];  // kHugePlanStage B per thread
  huge_plan(P, sh, 1024, hstage);
}

// The last i in [0, n) with a[i] <= v (a[0] = 0, nondecreasing): the huge
// block that owns unit / KiB block v (blocks without any are passed over).
__device__ __forceinline__ uint32_t last_le(const uint64_t* a, uint32_t n, uint64_t v) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (gload(a, mid) <= v) lo = mid;
    else hi = mid;
  }
  return lo;
}

// The unit table of the parsed huge blocks: thread per restart interval x of
// block i (plus one past its last), start s_x (span offset).  Unit u (window
// [uW, uW + W)) gets the first interval that starts at or after uW, and that
// interval's payload offset (the bound the window's last walk stops at): x
// writes the units in (floor(s_{x-1} / W), floor(s_x / W)].  For a monotone
// binary index every unit of the block is written once; a block whose index
// is not monotone is flagged, and the work kernel searches its index instead.
__global__ __launch_bounds__(256) void decode_huge_units_kernel(DecodeParams P) {
  __shared__ uint32_t sb;
  const HugeHdr* hp = reinterpret_cast<const HugeHdr*>(P.huge_pool);
  const uint32_t n = hp->n3;
  if (!n) return;
  const HugeLayout L = huge_layout(P, n);
  if (hp->stream)  // this call's unit-done flags start clear (entries inside the pool only)
    for (uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x; u < hp->total_pu && 16 * (u + 1) <= L.rest;
         u += (uint64_t)gridDim.x * 256)
      L.uend[-1 - (int64_t)u].z = 0;
  const uint64_t tiv = hp->total_iv;
  for (uint64_t t0 = (uint64_t)blockIdx.x * 256; t0 < tiv; t0 += (uint64_t)gridDim.x * 256) {
    if (threadIdx.x == 0) sb = last_le(L.ipre, n, t0);
    __syncthreads();
    const uint64_t tt = t0 + threadIdx.x;
    uint32_t i = sb;
    __syncthreads();  // (sb is rewritten in the next round)
    if (tt >= tiv) continue;
    while (i + 1 < n && gload(L.ipre, i + 1) <= tt) ++i;
    HugeRec* r = L.rec + i;
    if (!r->accepted) continue;
    const BlockMeta m = r->m;
    const TrailerInfo t = trailer_of(m);
    const uint32_t x = (uint32_t)(tt - gload(L.ipre, i)), nint = t.bin_len;
    const uint8_t* gbase = P.blocks + r->span0;
    const uint64_t ub = gload(L.ppre, i);
    const int64_t npu = (int64_t)(gload(L.ppre, i + 1) - ub);
    const uint32_t sv = x < nint ? bin_get(gbase, m.p0, t, x) : t.rec_end;  // payload offset
    const uint32_t sp = x > 0 ? bin_get(gbase, m.p0, t, x - 1) : 0;
    if (x > 0 && x < nint && sv < sp) __hip_atomic_store(&r->nonmono, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int64_t ulo = x > 0 ? (int64_t)((m.p0 + (uint64_t)sp) / kHugeWin) + 1 : 0;
    const int64_t uhi = x < nint ? min((int64_t)((m.p0 + (uint64_t)sv) / kHugeWin), npu - 1) : npu - 1;
    for (int64_t u = ulo; u <= uhi; ++u) *reinterpret_cast<uint2*>(&L.uend[-1 - (int64_t)(ub + u)]) = make_uint2(x, sv);
  }
}

// Huge-block work units (see huge_plan): unit u = window c of block i.  Data
// windows whose intervals are all staged take phase A / B (decode_big_kernel's
// record walk: lane = interval for the boundaries, thread = record for the
// fields) on a window view of the block (meta offsets relative to the stage,
// interval numbers absolute, the binary-index entries copied next to the
// stage); others walk their intervals thread by thread.
// Unit-done flags: unit u's entry .z = the call's tag once its records and
// contributions are written.  The contributions are agent-scope stores
// (through the writer XCD's L2), waited for (vmcnt) before the flag store;
// a chain wave reads a 1-KiB chunk of rows (LDS-DMA) only after the flags of
// every unit that writes into it: no L2 of this launch holds a line of the
// chunk before that, and every block's rows are padded to whole chunks.
// ready_upto: units [0, ready_upto) of the block are known done; polls 64
// flags per load.  Returns false (the caller gives the block up) after
// kStreamStallTicks of wall time without progress: a bound in time, not in
// polls, whose length does not depend on the load latency.
__device__ __forceinline__ bool huge_wait_units(const HugeLayout& L, uint64_t ub, uint32_t need, uint32_t tag,
                                                uint32_t npu, uint32_t& ready_upto, bool give_up) {
  const uint32_t lane = threadIdx.x & 63;
  need = min(need, npu);
  if (ready_upto >= need) return true;
  if (give_up) return false;  // (diagnostic builds: kDiagStreamGiveUp)
  uint64_t t_prog = __builtin_amdgcn_s_memrealtime();
  while (ready_upto < need) {
    const uint32_t c = ready_upto + lane;
    const uint32_t f = c < npu ? __hip_atomic_load(&L.uend[-1 - (int64_t)(ub + c)].z, __ATOMIC_RELAXED,
                                                    __HIP_MEMORY_SCOPE_AGENT)
                               : tag;
    const uint64_t done = __ballot(f == tag);
    const uint32_t adv = (uint32_t)__builtin_ctzll(~done);  // (done == ~0: 64)
    ready_upto = min(npu, ready_upto + (done == ~0ULL ? 64u : adv));
    if (ready_upto < need && adv == 0) {
      const uint64_t now = __builtin_amdgcn_s_memrealtime();
      if (now - t_prog > kStreamStallTicks) return false;
      __builtin_amdgcn_s_sleep(2);
    } else {
      t_prog = __builtin_amdgcn_s_memrealtime();
    }
  }
  return true;
}

// One block's chain on this wave, its rows consumed as the units publish
// them, then the tail merge, the checksum compare and the status (oracle
// order: payload checksum, then trailer, then parse) once every unit is done.
__device__ void huge_chain_streamed(const DecodeParams& P, const HugeLayout& L, uint32_t i, uint8_t* ring) {
  const HugeRec* r = L.rec + i;
  const uint32_t lane = threadIdx.x & 63, k = lane & 7, q = lane & 3;
  const bool hash = !(P.flags & LSM_DECODE_PAYLOAD_VERIFIED);
  const BlockMeta m = r->m;
  const uint64_t ub = gload(L.ppre, i);
  const uint32_t npu = (uint32_t)(gload(L.ppre, i + 1) - ub);
  const uint32_t tag = P.huge_tag;
  const bool give_up = kDiagBuild && (P.flags & kDiagStreamGiveUp);
  uint32_t ready_upto = 0;
  bool ok = true;
  int32_t st = ST_OK;
  if (hash) {
    uint64_t a0, a1;
    xxh3_acc_init((int)(k >> 1), a0, a1);
    uint64_t x = (k & 1) ? a1 : a0;
    const uint32_t nbk = r->nbk;
    if (nbk) {
      // chunk c of 16 rows needs the units holding the starts of KiB blocks 16c .. 16c + 15
      auto wait = [&](uint64_t c) {
        const uint64_t last = min((uint64_t)nbk - 1, 16 * c + 15);
        const uint32_t need = (uint32_t)((m.p0 + 1024 * last) / kHugeWin) + 1;
        ok = ok && huge_wait_units(L, ub, need, tag, npu, ready_upto, give_up);
      };
      x = xxh3_chain8<kStreamRing>(L.contrib + 8 * gload(L.kpre, i), nbk, x, kLongSecret.acc[16 + k], ring, wait);
    }
    const uint64_t c0 = wave_shfl_u64(x, (int)(2 * q)), c1 = wave_shfl_u64(x, (int)(2 * q + 1));
    uint64_t lo, hi;
    xxh3_wave_tail_merge(P.blocks + r->span0, m.p0, m.len - kHdrLen, &kLongSecret, c0, c1, lo, hi);
    if (lo != m.ck_lo || hi != m.ck_hi) st = ST_CKSUM;
  }
  ok = ok && huge_wait_units(L, ub, npu, tag, npu, ready_upto, give_up);  // every unit's parse result
  if (st == ST_OK) {
    const uint32_t bad = __hip_atomic_load(&r->parse_bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    st = m.st != ST_OK ? m.st : bad ? (int32_t)ST_PARSE : (int32_t)ST_OK;
  }
  // A chain that gave up decides nothing: its rows or parse results may be missing, so it
  // marks the block for decode_huge_chain_kernel, which runs after this kernel has ended
  // (every unit done) and writes the block's real status.
  if (!ok) st = ST_INCOMPLETE;
  if (lane == 0) gstore(P.status, r->b, st);
}

template <bool kAllFields>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void decode_huge_kernel(DecodeParams P, uint32_t chain_wgs) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint8_t* stage = smem + 64;
  uint32_t* cnt = reinterpret_cast<uint32_t*>(smem);  // [0, 1]: search counts; [2..]: per-wave partials
  const HugeHdr* hp = reinterpret_cast<const HugeHdr*>(P.huge_pool);
  const uint32_t n = hp->n3;
  if (!n) return;
  const HugeLayout L = huge_layout(P, n);
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  const bool hash = !(P.flags & LSM_DECODE_PAYLOAD_VERIFIED);
  const bool stream = hp->stream != 0;
  if (blockIdx.x < chain_wgs) {
    if (!stream) return;  // (decode_huge_chain_kernel runs the chains after this kernel)
    // chain workgroups (dispatched first): wave q = 4 g + w takes blocks q, q + 4 chain_wgs, ...
    uint8_t* ring = smem + 64 + wave * kStreamRing * 1024;
    for (uint32_t i = 4 * blockIdx.x + wave; i < n; i += 4 * chain_wgs)
      if (L.rec[i].accepted) huge_chain_streamed(P, L, i, ring);
    return;
  }
  // Unit order: batches of B = 4 chain_wgs blocks (one per chain wave), window-major
  // inside a batch: virtual unit v = (batch, window c, block in batch), so the blocks
  // of a batch progress together, each chain streams behind its own, and a chain
  // wave's next block (the next batch) is produced while it finishes this one.
  // Without streaming: a run of consecutive units per workgroup (one block search
  // per run, and a window's first interval is the previous window's end).
  const uint32_t pgrid = gridDim.x - chain_wgs, pb = blockIdx.x - chain_wgs;
  const uint32_t B = 4 * chain_wgs, mx = hp->max_npu;
  const uint64_t vtot = stream ? (uint64_t)((n + B - 1) / B) * B * mx : hp->total_pu;
  // (streaming: unit v goes to workgroup v mod pgrid, so the whole grid works along the windows in
  // order and the chains stream behind it; a grid-sized run per workgroup made every window
  // progress at once and the chains wait for their last windows: 4 MiB 0.202 -> 0.256 ms)
  const uint64_t per = stream ? 1 : (vtot + pgrid - 1) / pgrid;
  const uint64_t v_begin = stream ? pb : (uint64_t)pb * per, v_end = stream ? vtot : min(vtot, v_begin + per);
  const uint64_t v_step = stream ? pgrid : 1;
  uint32_t iseq = !stream && v_begin < v_end ? last_le(L.ppre, n, v_begin) : 0;
  uint32_t carry_u = 0xFFFFFFFFu, carry_r = 0;  // unit whose r1 search answer is carry_r (block iseq)
#if defined(LSM_DIAG) && !defined(LSM_DIAG_NOTIME)
  // diagnostic builds: per-phase s_memtime totals of wave 0 (g_large_phase[8..13], units in [14])
  uint64_t t_last = __builtin_amdgcn_s_memtime(), ph[8] = {};
  uint32_t nunits = 0;
#define HUGE_PHASE(k) DEC_PHASE(k)
#else
#define HUGE_PHASE(k)
#endif
  uint32_t pending = ~0u;  // a processed unit whose done flag is not yet published
  for (uint64_t v = v_begin; v < v_end; v += v_step) {
    HUGE_PHASE(6);
    uint32_t i, wc;
    uint64_t ub;
    if (stream) {
      const uint64_t bw = (uint64_t)B * mx, rem = v % bw;
      i = (uint32_t)(v / bw) * B + (uint32_t)(rem % B);
      wc = (uint32_t)(rem / B);
      if (i >= n) continue;
      if (!L.rec[i].accepted) continue;  // (uniform)
      ub = gload(L.ppre, i);
      if (wc >= gload(L.ppre, i + 1) - ub) continue;  // the block has fewer windows
    } else {
      while (iseq + 1 < n && gload(L.ppre, iseq + 1) <= v) ++iseq, carry_u = 0xFFFFFFFFu;
      i = iseq;
      if (!L.rec[i].accepted) continue;
      ub = gload(L.ppre, i);
      wc = (uint32_t)(v - ub);
    }
    const HugeRec* r = L.rec + i;
    const uint32_t u = (uint32_t)(ub + wc);
    const BlockMeta m = r->m;
    const TrailerInfo t = trailer_of(m);
    const uint32_t span = r->span;
    const uint8_t* gbase = P.blocks + r->span0;
    const uint32_t cs = wc * kHugeWin;
    const uint32_t ce = min(cs + kHugeWin, span), ss = min(ce + kHugeOverlap, span);
    // stage [cs, ss): wave w moves 1-KiB pieces w, w + 4, ...
    stage_to_lds(gbase + cs, stage, (ss - cs + 15) >> 4, wave, 4, lane);
    // the intervals that start in [cs, ce): [r0, r1), from the unit table, or (a binary index
    // that is not monotone) by a 256-way search of the binary index (HBM)
    const bool parse = m.st == ST_OK;
    const bool table = !r->nonmono;
    uint32_t r0 = 0, r1 = 0, stop1 = 0;  // stop1: payload offset where the window's last interval ends
    if (parse && table) {
      const uint4 e0 = L.uend[-1 - (int64_t)u];
      const bool last = ce == span;
      const uint2 e1 = last ? make_uint2(t.bin_len, t.rec_end) : make_uint2(L.uend[-2 - (int64_t)u].x, L.uend[-2 - (int64_t)u].y);
      r0 = cs == 0 ? 0 : e0.x;
      r1 = last ? t.bin_len : e1.x;
      stop1 = e1.y;
    } else if (parse) {
      const uint32_t nint = t.bin_len, p0 = m.p0;
      uint32_t lo0 = 0, hi0 = nint, lo1 = 0, hi1 = nint;  // r0 in [lo0, hi0], r1 in [lo1, hi1]
      if (carry_u + 1 == u) lo0 = hi0 = carry_r;
      while (hi0 > lo0 || hi1 > lo1) {  // (uniform) each round narrows both ranges 256-fold
        const uint32_t len0 = hi0 - lo0, len1 = hi1 - lo1;
        const uint32_t st0 = (len0 + 255) / 256, st1 = (len1 + 255) / 256;
        const uint32_t x0 = lo0 + tid * st0, x1 = lo1 + tid * st1;
        const bool b0 = x0 < hi0 && p0 + bin_get(gbase, p0, t, x0) < cs;
        const bool b1 = x1 < hi1 && p0 + bin_get(gbase, p0, t, x1) < ce;
        const uint32_t c0 = (uint32_t)__builtin_popcountll(__ballot(b0)), c1 = (uint32_t)__builtin_popcountll(__ballot(b1));
        if (lane == 0) cnt[2 + wave] = c0, cnt[6 + wave] = c1;
        lds_barrier();
        const uint32_t k0 = cnt[2] + cnt[3] + cnt[4] + cnt[5], k1 = cnt[6] + cnt[7] + cnt[8] + cnt[9];
        lds_barrier();
        // k samples lie below the bound (a prefix of them, for monotone starts): the
        // answer is in (lo + (k - 1) st, lo + k st]; with st = 1 the range closes
        if (len0) {
          const uint32_t nlo = k0 ? lo0 + (k0 - 1) * st0 + 1 : lo0;
          hi0 = min(hi0, lo0 + k0 * st0);
          lo0 = min(nlo, hi0);
        }
        if (len1) {
          const uint32_t nlo = k1 ? lo1 + (k1 - 1) * st1 + 1 : lo1;
          hi1 = min(hi1, lo1 + k1 * st1);
          lo1 = min(nlo, hi1);
        }
      }
      // the same bound gives the same answer in the neighbouring unit, and the first
      // / last windows take every interval before / after: each interval is walked
      // at least once even when the binary index is not monotone (its walk then fails)
      r0 = cs == 0 ? 0 : lo0;
      r1 = ce == span ? nint : lo1;
      carry_u = stream ? 0xFFFFFFFFu : u;  // (streaming: the next unit is another block's)
      carry_r = lo1;
    }
    const uint8_t* sbase = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(stage) - cs);  // span-relative
    HUGE_PHASE(0);
    if (parse) {
      const uint64_t item_base = r->item_base;
      const uint32_t p0 = m.p0, ri = t.ri, niv = r1 - r0;
      const uint32_t items_w = niv ? min(r1 * ri, t.item_count) - r0 * ri : 0;
      // phase A / B when every interval of the window is staged (a wave-uniform vote)
      bool fast = m.type != 1 && niv <= kHugeMaxIv && items_w <= kHugeTile;
      if (fast && table) {  // (monotone: every interval of the window ends by stop1)
        fast = r1 == r0 || (stop1 <= t.rec_end && (p0 + stop1 + kChunkReadAhead <= ss || ss == span));
      } else if (fast) {
        bool mine = true;
        for (uint32_t x = r0 + tid; x < r1; x += 256) {
          const uint32_t s_cur = bin_get(gbase, p0, t, x);
          const uint32_t stop = x + 1 == t.bin_len ? t.rec_end : bin_get(gbase, p0, t, x + 1);
          mine = mine && p0 + s_cur >= cs && stop <= t.rec_end && (p0 + stop + kChunkReadAhead <= ss || ss == span);
        }
        if (lane == 0) cnt[10 + wave] = __ballot(!mine) != 0;
        lds_barrier();
        fast = !(cnt[10] | cnt[11] | cnt[12] | cnt[13]);
      }
      uint8_t* bix = smem + 64 + kHugeBix;
      BlockMeta* wmeta = reinterpret_cast<BlockMeta*>(smem + 64 + kHugeMeta);
      uint8_t* owner = smem + 64 + kHugeOwner;
      uint64_t* rec = reinterpret_cast<uint64_t*>(smem + 64 + kHugeRec);
      if (fast) {
        // the entries r0 .. min(r1, nint - 1) as dwords next to the stage
        const uint32_t e1 = min(r1, t.bin_len - 1);
        const uint32_t eb = p0 + t.bin_off + r0 * t.step, elen = (e1 - r0 + 1) * t.step;
        for (uint32_t d = tid; 4 * d < elen; d += 256)
          reinterpret_cast<uint32_t*>(bix)[d] = read_u32_unaligned(gbase, eb + 4 * d);
        for (uint32_t x = tid; x < niv; x += 256) owner[x] = 0;
        for (uint32_t x = tid; x <= items_w; x += 256) rec[x] = 0;
        if (tid == 0) {
          BlockMeta w = m;
          w.p0 = m.p0 - cs;  // stage offsets (the window starts at span offset cs)
          w.rec_end = m.rec_end - cs;
          w.bin_off = kHugeBix - w.p0 - r0 * t.step;  // bin_get(stage, w.p0, r) reads bix[r - r0]
          w.item0 = 0u - r0 * ri;                     // descriptors numbered from the window's first item
          w.chain0 = 0u - r0;                         // phase A's interval c is interval r0 + c
          w.st = ST_OK;
          *wmeta = w;
        }
      }
      HUGE_PHASE(1);
      vm_wait<0>();
      lds_barrier();
      if (tid == 0 && pending != ~0u)  // (streaming) the previous unit: its stores have completed (vmcnt(0) above)
        __hip_atomic_store(&L.uend[-1 - (int64_t)pending].z, P.huge_tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      HUGE_PHASE(2);
      // phase A (serial LDS walks: latency) on wave 0, the contributions (VALU) on the
      // other waves meanwhile; without phase A on all four
      const bool split = fast;
      if (fast && (split ? wave == 0 : true)) {
        if (split) __builtin_amdgcn_s_setprio(2);  // (the walk is the unit's longest role)
        phase_a<true>(stage, wmeta, owner, rec, split ? 0 : wave * kWave, split ? kWave : 4 * kWave, niv, kHugeTile);
        __builtin_amdgcn_s_setprio(0);
      }
      HUGE_PHASE(3);
      if (hash && r->nbk && (!split || wave != 0)) {  // the KiB blocks that start in [cs, ce)
        const uint32_t nbk = r->nbk;
        const uint32_t n0 = min(nbk, cs > p0 ? (cs - p0 + 1023) / 1024 : 0u);
        const uint32_t n1 = min(nbk, ce > p0 ? (ce - p0 + 1023) / 1024 : 0u);
        if (n1 > n0) {  // (streaming: agent-scope stores, read by a chain wave of this launch)
          if (stream)
            xxh3_kib_contribs<true, true>(stage, p0 + 1024 * n0 - cs, (n1 - n0) * 1024 + 1, &kLongSecret,
                                          L.contrib + 8 * (gload(L.kpre, i) + n0), split ? wave - 1 : wave, split ? 3 : 4);
          else
            xxh3_kib_contribs(stage, p0 + 1024 * n0 - cs, (n1 - n0) * 1024 + 1, &kLongSecret,
                              L.contrib + 8 * (gload(L.kpre, i) + n0), split ? wave - 1 : wave, split ? 3 : 4);
        }
      }
      HUGE_PHASE(4);
      bool walk = !fast;
      if (fast) {
        lds_barrier();
        phase_b<kAllFields, false, true>(P, stage, wmeta, rec, items_w, (uint32_t)(item_base + r0 * ri), tid, 256);
        lds_barrier();
        const int32_t wst = wmeta->st;
        if (wst == ST_PARSE && tid == 0) atomicOr(const_cast<uint32_t*>(&r->parse_bad), 1u);
        walk = wst == ST_DEFER;  // a record shape the straight-line parsers do not take: the LEB cursor
      }
      if (walk) {
        bool ok = true;
        for (uint32_t x = r0 + tid; x < r1; x += 256) {
          const uint32_t s_cur = bin_get(gbase, p0, t, x);
          const bool last = x + 1 == t.bin_len;
          const uint32_t stop = last ? t.rec_end : bin_get(gbase, p0, t, x + 1);
          const bool staged = p0 + s_cur >= cs && stop <= t.rec_end && (p0 + stop + kChunkReadAhead <= ss || ss == span);
          ok &= walk_interval_at(staged ? sbase : gbase, p0, m, t, x, s_cur, stop, [&](uint32_t j, const ItemFields& f) {
            emit_global(P.out, item_base + j, f, P.seqno_add, P.compact);
          });
        }
        const uint64_t bad = __ballot(!ok);
        if (bad && lane == (uint32_t)__builtin_ctzll(bad)) atomicOr(const_cast<uint32_t*>(&r->parse_bad), 1u);
      }
    } else if (hash && r->nbk) {
      vm_wait<0>();
      lds_barrier();
      if (tid == 0 && pending != ~0u)  // (streaming) the previous unit: its stores have completed (vmcnt(0) above)
        __hip_atomic_store(&L.uend[-1 - (int64_t)pending].z, P.huge_tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const uint32_t p0 = m.p0, nbk = r->nbk;
      const uint32_t n0 = min(nbk, cs > p0 ? (cs - p0 + 1023) / 1024 : 0u);
      const uint32_t n1 = min(nbk, ce > p0 ? (ce - p0 + 1023) / 1024 : 0u);
      if (n1 > n0) {
        if (stream)
          xxh3_kib_contribs<true, true>(stage, p0 + 1024 * n0 - cs, (n1 - n0) * 1024 + 1, &kLongSecret,
                                        L.contrib + 8 * (gload(L.kpre, i) + n0), wave, 4);
        else
          xxh3_kib_contribs(stage, p0 + 1024 * n0 - cs, (n1 - n0) * 1024 + 1, &kLongSecret,
                            L.contrib + 8 * (gload(L.kpre, i) + n0), wave, 4);
      }
    }
    HUGE_PHASE(5);
    lds_barrier();  // (the next unit rewrites the stage)
    // published after the next unit's DMA wait (vmcnt(0): this unit's contribution
    // stores and parse_bad update have completed by then), or after the loop
    if (stream) pending = u;
#if defined(LSM_DIAG) && !defined(LSM_DIAG_NOTIME)
    ++nunits;
#endif
  }
  if (pending != ~0u) {
    vm_wait<0>();
    lds_barrier();
    if (tid == 0) __hip_atomic_store(&L.uend[-1 - (int64_t)pending].z, P.huge_tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
#if defined(LSM_DIAG) && !defined(LSM_DIAG_NOTIME)
  if (threadIdx.x == 0) {
    for (int k = 0; k < 7; ++k) atomicAdd(&g_large_phase[8 + k], (unsigned long long)ph[k]);
    atomicAdd(&g_large_phase[15], (unsigned long long)nunits);
  }
#endif
#undef HUGE_PHASE
}

// Chains of the huge blocks when they do not stream, and, when they stream,
// of the blocks whose streamed chain gave up (status ST_INCOMPLETE; every
// other block returns at once): a single-wave workgroup per block,
// its eight accumulators on lanes 0..7 (xxh3_chain8), then on the same wave
// the tail merge, the checksum compare and the status (oracle order: payload
// checksum, then trailer, then parse).  The contributions cross a kernel
// boundary here; the chain results stay in the wave.
__global__ __launch_bounds__(64) void decode_huge_chain_kernel(DecodeParams P) {
  __shared__ __attribute__((aligned(16))) uint8_t ring[kChainRing * 1024];
  const HugeHdr* hp = reinterpret_cast<const HugeHdr*>(P.huge_pool);
  const uint32_t n = hp->n3;
  if (!n) return;
  const bool streamed = hp->stream != 0;
  if (streamed && kDiagBuild && (P.flags & kDiagNoChainFallback)) return;
  const HugeLayout L = huge_layout(P, n);
  const bool hash = !(P.flags & LSM_DECODE_PAYLOAD_VERIFIED);
  const uint32_t lane = threadIdx.x & 63, k = lane & 7, q = lane & 3;
  for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
    const HugeRec* r = L.rec + i;
    if (!r->accepted) continue;
    if (streamed && gload(P.status, r->b) != ST_INCOMPLETE) continue;  // (the streamed chain decided it)
    const BlockMeta m = r->m;
    int32_t st = m.st != ST_OK ? m.st : r->parse_bad ? (int32_t)ST_PARSE : (int32_t)ST_OK;
    if (hash) {
      uint64_t a0, a1;
      xxh3_acc_init((int)(k >> 1), a0, a1);
      uint64_t x = (k & 1) ? a1 : a0;
      if (r->nbk)
        x = xxh3_chain8<kChainRing>(L.contrib + 8 * gload(L.kpre, i), r->nbk, x, kLongSecret.acc[16 + k], ring);
      // lane quad position q takes accumulators 2q, 2q + 1 (lanes 2q, 2q + 1 hold them)
      const uint64_t c0 = wave_shfl_u64(x, (int)(2 * q)), c1 = wave_shfl_u64(x, (int)(2 * q + 1));
      uint64_t lo, hi;
      xxh3_wave_tail_merge(P.blocks + r->span0, m.p0, m.len - kHdrLen, &kLongSecret, c0, c1, lo, hi);
      if (lo != m.ck_lo || hi != m.ck_hi) st = ST_CKSUM;
    }
    if (lane == 0) gstore(P.status, r->b, st);
  }
}

// ------------------------------------------------------------ host: the pool's size
// Every huge block spans more than kBigStage bytes; contributions 64 B per KiB, unit entries
// 8 B per kHugeWin window (and one more per block).
size_t decode_huge_pool_bytes(uint32_t n_blocks, uint64_t blocks_bytes) {
  const uint64_t most = blocks_bytes / kBigStage + 1;
  const uint64_t n3 = most < n_blocks ? most : n_blocks;
  return huge_fixed_bytes(n3) + 64 * (blocks_bytes / 1024 + 1 + 16 * n3) + 16 * (blocks_bytes / kHugeWin + n3 + 1) + 256;
}

size_t decode_huge_pool_min_bytes() {
  static_assert(huge_fixed_bytes(1) + 64 * 128 == 8704, "the threshold lsmgpu.h documents");
  return huge_fixed_bytes(1) + 64 * 128;
}

// ------------------------------------------------------------ host: the stage launchers
// listed blocks: the big-block kernel (two workgroups per CU), then the
// general path for what it hands on (its list read as defer_count / defer_list)
hipError_t launch_decode_big(const DecodeParams& P, int variant, uint32_t* bgrid, hipStream_t st) {
  const void* const big_k[4] = {(const void*)decode_big_kernel<false, false>, (const void*)decode_big_kernel<true, false>,
                                (const void*)decode_big_kernel<false, true>, (const void*)decode_big_kernel<true, true>};
  hipError_t e;
  int n_cu = 0;
  if ((e = device_cu_count(&n_cu)) != hipSuccess) return e;
  *bgrid = min(P.n_blocks, (uint32_t)n_cu * kBigGPerCU);
  if (!*bgrid) return hipSuccess;
  static uint64_t done_bg[4] = {};
  if ((e = set_lds_attr(big_k[variant], kBigGLds, &done_bg[variant])) != hipSuccess) return e;
  void* args[] = {const_cast<DecodeParams*>(&P)};
  return hipLaunchKernel(big_k[variant], dim3(*bgrid), dim3(kBigGWaves * kWave), args, kBigGLds, st);
}

// the huge blocks the big-block kernel listed: plan (rejects go to defer2)
hipError_t launch_decode_huge_plan(const DecodeParams& P, hipStream_t st) {
  static uint64_t done_hp = 0;
  const hipError_t e = set_lds_attr((const void*)decode_huge_plan_kernel, 1024 * kHugePlanStage, &done_hp);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(decode_huge_plan_kernel, dim3(1), dim3(1024), 1024 * kHugePlanStage, st, P);
  return hipSuccess;
}

hipError_t launch_decode_general(const DecodeParams& P, hipStream_t st) {
  const uint32_t dgrid = P.n_blocks < 1024 ? P.n_blocks : 1024;
  if (!dgrid) return hipSuccess;
  DecodeParams P2 = P;
  P2.defer_count = P.defer2_count;
  P2.defer_list = P.defer2_list;
  static uint64_t done_big = 0;
  const uint32_t big = kBigStageOff + kBigStage + kStagePad;
  const hipError_t e = set_lds_attr((const void*)decode_deferred_staged_kernel, big, &done_big);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(decode_deferred_staged_kernel, dim3(dgrid), dim3(kBigWaves * kWave), big, st, P2);
  return hipSuccess;
}

hipError_t launch_decode_huge(const DecodeParams& P0, bool all, hipStream_t st) {
  DecodeParams P = P0;
  P.huge_tag = 1;  // (the units kernel clears the flags first)
  const void* hk = all ? (const void*)decode_huge_kernel<true> : (const void*)decode_huge_kernel<false>;
  hipError_t e;
  static uint64_t done_hk[2] = {};
  if ((e = set_lds_attr(hk, kHugeLds, &done_hk[all ? 1 : 0])) != hipSuccess) return e;
  int n_cu = 0;
  if ((e = device_cu_count(&n_cu)) != hipSuccess) return e;
  hipLaunchKernelGGL(decode_huge_units_kernel, dim3(kHugeUnitsGrid), dim3(256), 0, st, P);
  // chain workgroups first (four blocks each, at most one per CU), then the units
  uint32_t chain_wgs = min((P.n_blocks + 3) / 4, kStreamChainWgs);
  void* hargs[] = {&P, &chain_wgs};
  // unit workgroups: as many as are resident beside the chain workgroups (one wave of
  // workgroups: no partly filled last wave; 256 KiB / 1 MiB decode 0.229 / 0.202 -> 0.220 / 0.196 ms
  // against a 2048-workgroup grid)
  const uint32_t ugrid = max(64u, kHugeWgsPerCU * (uint32_t)n_cu - chain_wgs);
  if ((e = hipLaunchKernel(hk, dim3(chain_wgs + ugrid), dim3(256), hargs, kHugeLds, st)) != hipSuccess) return e;
  // (when streamed: only the blocks whose chain gave up, LSM_INCOMPLETE; the others return at once)
  hipLaunchKernelGGL(decode_huge_chain_kernel, dim3(kHugeChainGrid), dim3(64), 0, st, P);
  return hipSuccess;
}

#if defined(LSM_DIAG) && !defined(LSM_DIAG_NOTIME)
hipError_t decode_large_phases(uint64_t* sum32) { return take_dec_phases(g_large_phase, sum32); }
#endif

}  // namespace lsmgpu
