// decode_group.hip — the group kernel of the decode path: blocks that fit the LDS stage,
// several per group (decode.hip has the launch shape).
#include "decode_common.hpp"

namespace lsmgpu {

// Blocks whose span exceeds this go to the big-block kernel: those larger
// than the stage.  (Half the stage measured slower: the 17 KB blocks of the
// 16 KiB random-key class run at 0.82 TB/s through the big-block kernel, one
// block per iteration, and at 1.42 TB/s here, one block per group.)
__device__ __forceinline__ uint32_t lone_bytes(const DecodeParams& P) { return P.stage_bytes; }

// A group: the longest run of consecutive blocks from b that fits the stage
// (k == 0: block b alone is too large and takes the direct path).  Lane j of
// every wave holds block b+j's handle and item range.
struct Group {
  uint32_t b, k, g_item0, n_items;
  uint64_t span0, span1;
  uint64_t off_j, end_j;
  uint32_t it0_j, it1_j;
};

// offr / itr: lane l holds block_off / item_start of block b_begin + l.
__device__ __forceinline__ Group form_group(const DecodeParams& P, uint32_t b, uint32_t b_begin, uint32_t b_end,
                                            uint32_t gmax, uint64_t offr, uint32_t itr, uint32_t& skip) {
  const int lane = threadIdx.x & (kWave - 1);
  Group G;
  G.b = b;
  const uint32_t li = b - b_begin + lane;
  const bool in_run = b + lane < b_end && (uint32_t)lane < gmax;
  const int s0 = (int)(in_run ? li : 0), s1 = (int)(in_run ? li + 1 : 0);
  G.off_j = wave_shfl_u64(offr, s0);
  G.end_j = wave_shfl_u64(offr, s1);
  G.it0_j = (uint32_t)__shfl((int)itr, s0);
  G.it1_j = (uint32_t)__shfl((int)itr, s1);
  if (!in_run) G.off_j = G.end_j = 0, G.it0_j = G.it1_j = 0;
  const uint64_t off_b = wave_readlane_u64(G.off_j, 0);
  G.g_item0 = wave_readlane_u32(G.it0_j, 0);
  G.span0 = off_b & ~15ULL;
  // lone blocks (lone_block) never join a group: they are listed for the general path up front
  const bool lone = ((G.end_j + 15) & ~15ULL) - (G.off_j & ~15ULL) > lone_bytes(P) ||
                    G.it1_j - G.it0_j > P.tile_items;
  const bool fits = in_run && !lone && G.end_j >= G.off_j && G.off_j >= off_b &&
                    ((G.end_j + 15) & ~15ULL) - G.span0 <= P.stage_bytes && G.it1_j - G.g_item0 <= P.tile_items;
  G.k = (uint32_t)__builtin_ctzll(~__ballot(fits));  // lanes >= gmax never fit
  // (k = 0: the run of lone blocks from b, at least one, passed over at once:
  // 64 huge blocks one form_group at a time took 17 us)
  skip = max(1u, (uint32_t)__builtin_ctzll(~__ballot(in_run && lone)));
  G.span1 = G.k ? (wave_readlane_u64(G.end_j, G.k - 1) + 15) & ~15ULL : G.span0;
  G.n_items = G.k ? wave_readlane_u32(G.it1_j, G.k - 1) - G.g_item0 : 0;
  return G;
}

// Inclusive scan over lanes 0..15 (one DPP row: a group has at most kMaxGroup = 16 blocks):
// four row_shr steps, no LDS round trip.  Every lane of the wave must be active.
static_assert(kMaxGroup <= 16, "the block scan is one 16-lane DPP row");
__device__ __forceinline__ uint32_t row_incl_scan_u32(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, false);  // row_shr:1
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, false);  // row_shr:2
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false);  // row_shr:4
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false);  // row_shr:8
  return v;
}

// Lane-level: one block's header fields and trailer, the checks of meta_header_fields +
// meta_trailer with the same statuses in the same order, but every load that does not depend
// on a loaded value issued at once: the trailer lies at a place the handle gives (its last
// kTrailerLen bytes), so the header words and the trailer words are one LDS round trip and
// the marker byte before the binary index a second one; the statuses are then selected from
// the loaded values.  (The helpers return at the first failed check, which makes magic,
// type, checksum words, trailer words and marker five dependent round trips.)
// hb / len: the block in the stage (len <= stage bytes); cap: its item capacity.
__device__ __forceinline__ void group_block_meta(const uint8_t* stage, uint32_t hb, uint32_t len, int32_t expect_type,
                                                 uint32_t cap, bool compact, BlockMeta& m) {
  const uint32_t p0 = hb + kHdrLen, plen = len - kHdrLen;
  const bool has_tr = len >= kHdrLen + kTrailerLen + 1;
  const uint32_t tp = has_tr ? hb + len - kTrailerLen : hb;  // (no trailer: any address inside the stage)
  // header and trailer words (reads past a short block stay inside the stage and its pad)
  const uint32_t magic = read_u32_unaligned(stage, hb);
  const uint32_t type = read_u32_unaligned(stage, hb + 4) & 0xFF;
  const BaseReader64 r{stage, hb};
  m.ck_lo = r(5);
  m.ck_hi = r(13);
  const uint32_t data_length = read_u32_unaligned(stage, hb + 21);
  const uint32_t w0 = read_u32_unaligned(stage, tp);
  const uint32_t ri = w0 & 0xFF, step = (w0 >> 8) & 0xFF;
  const uint32_t bin_len = read_u32_unaligned(stage, tp + 2);
  const uint32_t bin_off = read_u32_unaligned(stage, tp + 6);
  const uint32_t item_count = read_u32_unaligned(stage, tp + 27);
  // Header::decode_from order (check_header_fields)
  const int32_t hst = len < 4                ? (int32_t)ST_TRUNCATED
                      : magic != 0x034D534CU ? (int32_t)ST_BAD_MAGIC
                      : len < 5              ? (int32_t)ST_TRUNCATED
                      : type > 3             ? (int32_t)ST_BAD_TYPE
                      : len < kHdrLen        ? (int32_t)ST_TRUNCATED
                                             : (int32_t)ST_OK;
  // read_trailer's structural checks up to the marker
  const bool shape_ok = has_tr && ri != 0 && (step == 2 || step == 4) && bin_len != 0 && bin_off != 0 &&
                        (uint64_t)bin_off + (uint64_t)bin_len * step <= (uint64_t)(plen - kTrailerLen);
  const uint32_t marker = read_u32_unaligned(stage, shape_ok ? p0 + bin_off - 1 : hb) & 0xFF;
  // bin_len == ceil(item_count / ri) in 32 bits (bin_len != 0 here, so no items never matches)
  const bool count_ok = item_count != 0 && (item_count - 1) / (ri ? ri : 1u) + 1 == bin_len;
  const int32_t tst = !shape_ok || marker != kTrailerMarker || !count_ok || (type == 1 && ri != 1) ? (int32_t)ST_PARSE
                      : item_count > cap                                                           ? (int32_t)ST_OVERFLOW
                                                                                                   : (int32_t)ST_OK;
  // meta_trailer order: data length, expected type, block kinds without items, trailer
  const int32_t st = hst != ST_OK                                        ? hst
                     : data_length != plen                               ? (int32_t)ST_TRUNCATED
                     : (expect_type >= 0 && (int32_t)type != expect_type) ? (int32_t)ST_TYPE_MISMATCH
                     : type == 2                                         ? (int32_t)ST_UNSUPPORTED
                     : (compact && (type == 1 || plen > 0xFFFFu))        ? (int32_t)ST_UNSUPPORTED
                                                                         : tst;
  const bool ok = st == ST_OK;
  m.p0 = p0;
  m.rec_end = ok ? p0 + bin_off - 1 : 0;
  m.st = st;
  m.type = type;
  m.hb = hb;
  m.len = len;
  m.ri = ri;
  m.step = step;
  m.bin_len = ok ? bin_len : 0;
  m.bin_off = bin_off;
  m.item_count = item_count;
  m.chain0 = 0;
  m.hdr_st = hst;
}

#if defined(LSM_DIAG) && !defined(LSM_DIAG_NOTIME)
// wave 0 per group, role timers summed over waves: entries 16..31
__device__ unsigned long long g_group_phase[32];
hipError_t decode_group_phases(uint64_t* sum32) { return take_dec_phases(g_group_phase, sum32); }
#endif

// Workgroup = kGroupWaves waves sharing one LDS stage (default 32 KiB: eight
// 4-KiB blocks, ~32 restart intervals).  Per group, three barriers (DMA landed, phase A and
// hash done, phase B done):
//   all waves   LDS-DMA of the span (wave w moves 1-KiB pieces w, w+4, ...)
//   wave pa     headers + trailers (lane j = block j), interval numbering, then phase A
//               (every lane walks one interval) with no barrier in between: the wave reads
//               what its own lanes wrote, which a wave-level ordering covers
//   other waves payload and header checksums (16-lane DPP rows, four blocks per wave), from
//               the DMA barrier on: a block's place in the stage follows from its handle,
//               and the verdict is consulted only in the status merge, where a block whose
//               header failed has its digest ignored
//   all waves   phase B (thread = record), coalesced SoA stores
// pa rotates with the group index so the serial walk lands on each SIMD in
// turn.  Phase A needs only the trailer, not the checksum, so it runs
// concurrently with the hash; statuses merge in oracle order at the end.
// A group of more than 64 restart intervals has phase A on up to three waves.  The hash
// waves cannot know that before the numbering is done, so that path keeps a fourth barrier:
// wave pa walks its share at once, the others theirs after the hash (the interval total is
// handed over in the stage pad's last word), and the workgroup meets once more before phase B.
constexpr uint32_t kGroupWaves = 4;
// 17-bit record descriptors for stages of 64 KiB and more (two 8-wave workgroups per CU)
constexpr bool kDecWide = kDefaultStageBytes >= 65536;

template <bool kAllFields, bool kCompact>
__global__ __launch_bounds__(kGroupWaves * kWave) __attribute__((amdgpu_waves_per_eu(3))) void decode_blocks_kernel(DecodeParams P) {
  // LDS: [meta: G x 80 B][rec: u64 per item + 1 scratch][owner: u8 per item][staged bytes + pad][secret]
#if defined(LSM_DIAG) && !defined(LSM_DIAG_NOTIME)
  uint64_t t_last = __builtin_amdgcn_s_memtime(), ph[16] = {};
#endif
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const uint32_t gmax = min(kMaxGroup, P.blocks_per_wave);
  BlockMeta* meta = reinterpret_cast<BlockMeta*>(smem);
  uint64_t* rec = reinterpret_cast<uint64_t*>(smem + gmax * (uint32_t)sizeof(BlockMeta));
  uint8_t* owner = reinterpret_cast<uint8_t*>(rec) + ((8 * (P.tile_items + 1) + 15) & ~15u);
  uint8_t* img = owner + ((P.tile_items + 15) & ~15u);
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int lane = tid & (kWave - 1);
  const uint32_t b_begin = blockIdx.x * P.blocks_per_wave;
  const uint32_t b_end = min(b_begin + P.blocks_per_wave, P.n_blocks);
  // the workgroup's handles and item starts, once per wave (blocks_per_wave <= 63)
  uint64_t offr = 0;
  uint32_t itr = 0;
  if (b_begin + lane <= b_end) {
    offr = gload(P.block_off, b_begin + lane);
    itr = gload(P.item_start, b_begin + lane);
  }
  // XXH3 long-path secret words in LDS (read per use by the lean row hash).
  const uint32_t slot_stride = ((P.stage_bytes + 15) & ~15u) + kStagePad;
  LongSecret* ls = reinterpret_cast<LongSecret*>(img + slot_stride);
  // A group's restart-interval total, from the wave that numbers the intervals to the others:
  // the last 16 bytes of the stage pad (the parsers read at most 138 bytes past a span).
  uint32_t* const grp_total = reinterpret_cast<uint32_t*>(img + slot_stride - 16);
  if (tid < sizeof(LongSecret) / 8)
    reinterpret_cast<uint64_t*>(ls)[tid] = reinterpret_cast<const uint64_t*>(&kLongSecret)[tid];
  uint32_t iter = 0;
  // Next stageable group at or after bb (larger blocks go to the general path).
  auto next_group = [&](uint32_t bb) -> Group {
    for (;;) {
      if (bb >= b_end) {
        Group z;
        z.b = bb;
        z.k = 0;
        return z;
      }
      uint32_t skip;
      const Group g = form_group(P, bb, b_begin, b_end, gmax, offr, itr, skip);
      if (g.k) return g;
      bb += skip;  // a run of lone blocks: listed for the general path before the loop
    }
  };
  // LDS-DMA of a group's span (wave w moves 1-KiB pieces w, w + 4, ...).
  auto issue_dma = [&](const Group& g, uint8_t* dst) {
    const uint32_t chunks = (kDiagBuild && (P.flags & kDiagSkipDma)) ? 0u : (uint32_t)((g.span1 - g.span0) >> 4);
    stage_to_lds(P.blocks + g.span0, dst, chunks, wave, kGroupWaves, lane);
  };
  // Lone blocks (larger than the stage, or more items than a tile) go to the
  // general path, decode_deferred_staged_kernel (a 72 KiB stage, the block
  // hashed by four waves): listed here, one atomic per workgroup.
  if (wave == 0) {
    const uint64_t nx = wave_shfl_u64(offr, min(lane + 1, kWave - 1));
    const uint32_t ix = (uint32_t)__shfl((int)itr, min(lane + 1, kWave - 1));
    const bool in = b_begin + lane < b_end;
    const bool lone = in && (((nx + 15) & ~15ULL) - (offr & ~15ULL) > lone_bytes(P) || ix - itr > P.tile_items);
    defer_blocks_wave(P, lone, b_begin + lane);
  }
  Group G = next_group(b_begin);
  if (G.k) issue_dma(G, img);
  for (; G.k; ++iter) {
    const uint32_t b = G.b;
    const uint32_t k = G.k;
    uint8_t* const stage = img;
    // ---- 1. this group's span has landed; clear the record descriptors
    for (uint32_t i = tid; i < G.n_items; i += kGroupWaves * kWave) rec[i] = 0;
    vm_wait<0>();
    lds_barrier();
    DEC_PHASE(0);
    const Group Gn = next_group(b + k);
    const uint32_t role = (wave + kGroupWaves - iter % kGroupWaves) % kGroupWaves;  // rotates per group
    // payload checksums (not when verified upstream: the LZ4 path checks the stored bytes)
    const bool hash = !(kDiagBuild && (P.flags & kDiagSkipHash)) && !(P.flags & LSM_DECODE_PAYLOAD_VERIFIED);
    // ---- 2. role 0: headers, trailers, numbering, phase A  ||  checksums on the other three waves
    if (role == 0) {
      // lane j = block j; owner[c] = block of restart interval c
      uint32_t total = 0;
      if (!(kDiagBuild && (P.flags & kDiagSkipHeader))) {
        uint32_t chains = 0;
        BlockMeta m;
        if ((uint32_t)lane < k) {
          group_block_meta(stage, (uint32_t)(G.off_j - G.span0), (uint32_t)(G.end_j - G.off_j), P.expect_type,
                           G.it1_j - G.it0_j, P.compact, m);
          m.item0 = G.it0_j - G.g_item0;
          if (m.st == ST_OK && m.type == 1) m.st = ST_DEFER;  // index blocks: general path
          chains = m.st == ST_OK ? m.bin_len : 0;
        }
        const uint32_t incl = row_incl_scan_u32(chains);
        if ((uint32_t)lane < k) {
          m.chain0 = incl - chains;
          // all but ck_bad / hck_bad: those two belong to the hash waves, which may have written them already
          __builtin_memcpy(&meta[lane], &m, offsetof(BlockMeta, ck_bad));
          for (uint32_t r = 0; r < chains; ++r) owner[m.chain0 + r] = (uint8_t)lane;
        }
        total = wave_readlane_u32(incl, k - 1);
      }
      if (kDiagBuild && (P.flags & kDiagSkipParse)) total = 0;
      if (lane == 0) *grp_total = total;
      wave_sync();  // meta and owner: written and read by this wave alone until the barrier
      DEC_ROLE(14);
      // its share of phase A (all of it up to 64 intervals)
      if (total) {
        const uint32_t nA = min((total + kWave - 1) / kWave, kGroupWaves - 1);
        phase_a<kDecWide>(stage, meta, owner, rec, 0, nA * kWave, total, P.tile_items);
        DEC_ROLE(8);
      }
    } else if (hash) {
      // Block jb of the group lies at hb_j of lane jb, len_j bytes (a handle shorter than a
      // header has no checksums to compare: its header status is final).  The expected
      // digest is read from the header bytes here; ck_bad / hck_bad are read after the
      // next barriers, in the status merge, and only for blocks whose header fields passed.
      const uint32_t hb_j = (uint32_t)(G.off_j - G.span0), len_j = (uint32_t)(G.end_j - G.off_j);
      const uint32_t hw = kGroupWaves - 1, hr = role - 1;  // three hash waves, this one's index
      if (k <= hw || (k <= hw * 4 && hr * 4 + 1 == k)) {
        // few (large) blocks: one wave per block, the 64-lane XXH3 (1 KiB per
        // step); also a wave whose share of the rows below is one block
        // (k = 4 h + 1, e.g. nine 4 KiB blocks on three hash waves): the whole
        // wave hashes it instead of one row with three rows idle
        const uint32_t jb = k <= hw ? hr : k - 1;
        if (jb < k) {
          const uint32_t hb = wave_readlane_u32(hb_j, jb), len = wave_readlane_u32(len_j, jb);
          if (len >= kHdrLen) {
            uint64_t lo, hi;
            xxh3_128_wave(stage, hb + kHdrLen, len - kHdrLen, ls, lo, hi);
            const bool hck = header_cksum_ok(stage, hb);
            if (lane == 0) {
              const BaseReader64 r{stage, hb};
              meta[jb].ck_bad = lo != r(5) || hi != r(13);
              meta[jb].hck_bad = !hck;
            }
          }
        }
        DEC_ROLE(10);
      } else {
        const uint32_t rows = hw * 4;
        for (uint32_t j0 = 0; j0 < k; j0 += rows) {  // wave-uniform: the shuffles run with every lane active
          const uint32_t jb = j0 + hr * 4 + (lane >> 4);
          const uint32_t hb = (uint32_t)__shfl((int)hb_j, (int)min(jb, kWave - 1u));
          const uint32_t len = (uint32_t)__shfl((int)len_j, (int)min(jb, kWave - 1u));
          if (jb < k && len >= kHdrLen) {
            uint64_t lo, hi;
            const uint32_t plen = len - kHdrLen;
            if (plen > 240) xxh3_128_row_long_lean(stage, hb + kHdrLen, plen, ls, lo, hi);
            else xxh3_128_short(plen, BaseReader8{stage, hb + kHdrLen}, BaseReader64{stage, hb + kHdrLen}, lo, hi);
            const bool hck = header_cksum_ok(stage, hb);
            if ((lane & 15) == 0) {
              const BaseReader64 r{stage, hb};
              meta[jb].ck_bad = lo != r(5) || hi != r(13);
              meta[jb].hck_bad = !hck;
            }
          }
        }
        DEC_ROLE(12);
      }
    }
    lds_barrier();
    DEC_PHASE(2);
    // ---- 3. more than 64 intervals: the other phase-A waves' shares, and the barrier this path keeps
    {
      const uint32_t total = *grp_total;  // the same for every wave: written before the barrier above
      const uint32_t nA = min((total + kWave - 1) / kWave, kGroupWaves - 1);
      if (nA > 1) {
        if (role != 0 && role < nA) {
          phase_a<kDecWide>(stage, meta, owner, rec, role * kWave, nA * kWave, total, P.tile_items);
          DEC_ROLE(8);
        }
        lds_barrier();
        DEC_PHASE(1);
      }
    }
    // ---- 4. phase B: thread = record; full parse + validation; coalesced stores
    if (!(kDiagBuild && (P.flags & (kDiagSkipParse | kDiagSkipPhaseB))))
      phase_b<kAllFields, kCompact, kDecWide>(P, stage, meta, rec, G.n_items, G.g_item0, threadIdx.x, blockDim.x);
    lds_barrier();
    DEC_PHASE(3);
    // refill the stage after phase B, before wave 0's status merge (which reads
    // only meta, after the barriers behind every writer of it): 0.2-0.8 % faster
    // than after it over five batch shapes
    if (Gn.k) issue_dma(Gn, img);
    if (wave == 0) {
      int32_t st = ST_OK;
      if ((uint32_t)lane < k) {
        const BlockMeta& m = meta[lane];
        st = m.hdr_st != ST_OK ? m.hdr_st
             : (hash && m.hck_bad) ? (int32_t)ST_HDR_CKSUM  // (no hash: nobody wrote the two verdicts)
             : (hash && m.ck_bad)  ? (int32_t)ST_CKSUM
                                   : m.st;
        if (st != ST_DEFER) gstore(P.status, b + lane, st);
      }
      defer_blocks_wave(P, (uint32_t)lane < k && st == ST_DEFER, b + lane);
    }
    DEC_PHASE(4);
#if defined(LSM_DIAG) && !defined(LSM_DIAG_NOTIME)
    ph[5] += 1;
    ph[6] += k;
#endif
    G = Gn;
  }
#if defined(LSM_DIAG) && !defined(LSM_DIAG_NOTIME)
  if (lane == 0) {
    for (int i = 0; i < 16; ++i)
      if ((i >= 8 || wave == 0) && ph[i]) atomicAdd(&g_group_phase[16 + i], (unsigned long long)ph[i]);
  }
#endif
}

hipError_t launch_decode_group(const DecodeParams& P, int variant, hipStream_t st) {
  // kernel variants: every field present or not, 32- or 16-bit offsets
  const void* const group_k[4] = {(const void*)decode_blocks_kernel<false, false>,
                                  (const void*)decode_blocks_kernel<true, false>,
                                  (const void*)decode_blocks_kernel<false, true>,
                                  (const void*)decode_blocks_kernel<true, true>};
  const uint32_t lds = decode_lds_bytes(P.stage_bytes, P.tile_items, P.blocks_per_wave);
  hipError_t e;
  if (lds > 64 * 1024) {
    static uint64_t done[4] = {};
    if ((e = set_lds_attr(group_k[variant], 160 * 1024, &done[variant])) != hipSuccess) return e;
  }
  const uint32_t grid = (P.n_blocks + P.blocks_per_wave - 1) / P.blocks_per_wave;
  void* args[] = {const_cast<DecodeParams*>(&P)};
  return hipLaunchKernel(group_k[variant], dim3(grid), dim3(kGroupWaves * kWave), args, lds, st);
}

}  // namespace lsmgpu
