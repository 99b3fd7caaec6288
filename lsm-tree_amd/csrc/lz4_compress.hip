// lz4_compress.hip — Block::write_into with CompressionType::Lz4
// (src/table/block/mod.rs:60-74): lz4_flex::compress of the payload, hash128 of
// the stored bytes, then the header.  The input is what lsm_encode_blocks wrote
// (Header || payload, CompressionType::None); the output is the same block as
// the reference would have written it under the default data-block policy.
//
// LZ4 compression is a serial chain of sequences, so the unit of parallelism
// is the block: one wave per block.  The match search inside a block is wide:
// one step looks at the 64 positions p .. p + 63 at once (lane i hashes the four
// bytes at p + i into a table of earlier positions), the lowest lane
// with a verified candidate wins the step, the match is extended backwards and
// forwards 64 bytes per round, and the 64 lanes copy the literals.  The walk
// state (anchor, p, output cursor) is wave-uniform.
//
// Three launches on one stream:
//   1. lz4c_small_kernel / lz4c_big_kernel: block b's stream into its workspace
//      slot (slot start = a function of d_block_off[b] and b alone), 33 + its
//      length (0 for a rejected block) into a u32 array, the status.
//        small  payload <= 5 KiB: 4 waves / workgroup, per wave an LDS copy of
//               the payload and the tables (10-bit match table, 32-bit entries).
//        big    one wave / workgroup: payload <= 64 KiB staged in LDS, 16-bit
//               positions; larger ones read from HBM, 32-bit positions
//               (correct, not tuned).  12-bit match table.
//      Every class writes the stream straight to the slot (byte stores the wave
//      never waits for): an LDS image of it would halve the small class's
//      occupancy.
//   2. the scan of the sizes (scan.hpp) -> d_out_off.
//   3. lz4c_pack_kernel, one wave per block: xxh3_128 of the stream (read back
//      from the slot), the header, the stream copied to its final place.
//
// The stream is a pure function of the payload: both tables are cleared per
// block, and where several lanes of one step store to one table entry the
// entry ends as the largest (match table) or smallest (step table) position,
// whichever lane's store lands last: by LDS atomic max where the entries are
// 32-bit, by a store / read-back loop where they are 16-bit.
#include <hip/hip_runtime.h>

#include "block_format.hpp"
#include "device_common.hpp"
#include "host_common.hpp"
#include "lsmgpu.h"
#include "scan.hpp"

namespace lsmgpu {

// Match table: 2^bits earlier positions by the hash of their 4 bytes.  Step table:
// this step's positions by the low hash bits.  The four-wave class takes the
// smaller pair with 32-bit entries: the same LDS as 11 bits of 16-bit entries
// (16 waves per CU), and atomics in place of the read-back loops (measured
// rates and ratios: DESIGN.md 4.7).
constexpr uint32_t kLzBits = 12, kLzStepTab = 512;
constexpr uint32_t kLzSmallBits = 10, kLzSmallStepTab = 128;
constexpr uint32_t kLzTab = 1u << kLzBits, kLzSmallTab = 1u << kLzSmallBits;
constexpr uint32_t kLzMaxOffset = 65535;
constexpr uint32_t kLzMaxInput = 0x7E000000u;         // LZ4_MAX_INPUT_SIZE
constexpr uint32_t kLzSmallMax = 5120;                // payload bytes of the four-wave class
constexpr uint32_t kLzStagedMax = 65536;              // payload bytes staged in LDS (16-bit positions)

// The stream of an n-byte payload is at most n + n / 255 + 16 bytes.
__host__ __device__ constexpr uint64_t lz4c_stream_bound(uint64_t n) { return n + n / 255 + 16; }

// Slot of block b in the workspace's slot region: 16-byte aligned, at least
// lz4c_stream_bound(size - 33) + 32 bytes before the next slot for any
// non-decreasing offsets (floor(x / 255) is superadditive; 32 b pays for the
// alignment and the pack kernel's reads past the stream's end).
__host__ __device__ constexpr uint64_t lz4c_slot_start(uint64_t rel_off, uint64_t b) {
  return (rel_off + rel_off / 255 + 32 * b + 15) & ~15ULL;
}
__host__ __device__ constexpr uint64_t lz4c_slots_bytes(uint64_t blocks_bytes, uint64_t n) {
  return lz4c_slot_start(blocks_bytes, n) + 64;
}

struct LzBlock {
  const uint8_t* base;  // 16-aligned
  uint32_t p0;          // payload position in base
  uint32_t len;         // payload bytes
  uint8_t* slot;
};

// Input checks of block b (wave-uniform): the header fields only, the payload
// comes straight from the encoder and is not hashed again.
__device__ __forceinline__ int32_t lz4c_check_block(const uint8_t* blocks, const uint64_t* block_off,
                                                    const int32_t* in_status, uint32_t b, uint8_t* slots,
                                                    uint64_t slots_cap, LzBlock& k) {
  if (in_status) {
    const int32_t s = in_status[b];
    if (s != ST_OK) return s;
  }
  const uint64_t o = block_off[b], e = block_off[b + 1];
  if (e < o || e - o < 4) return ST_TRUNCATED;
  k.base = blocks + (o & ~15ULL);
  const uint32_t hb = (uint32_t)(o & 15);
  HeaderInfo h;
  const int32_t st = check_header_fields(k.base, hb, e - o, h);
  if (st != ST_OK) return st;
  if ((uint64_t)h.data_length != e - o - kHdrLen) return ST_TRUNCATED;
  if (h.data_length != read_u32_unaligned(k.base, hb + 25)) return ST_UNSUPPORTED;  // already compressed
  if (h.data_length > kLzMaxInput) return ST_UNSUPPORTED;
  k.p0 = hb + kHdrLen;
  k.len = __builtin_amdgcn_readfirstlane(h.data_length);
  const uint64_t rel = o - block_off[0];
  const uint64_t s0 = lz4c_slot_start(rel, b);
  if (o < block_off[0] || s0 + lz4c_stream_bound(k.len) + 4 > slots_cap) return ST_BAD_ARG;  // workspace sized for fewer bytes
  k.slot = slots + s0;
  return ST_OK;
}

// Length extension bytes of a token nibble of 15: rem = length - 15.
__device__ __forceinline__ uint32_t lz4c_emit_ext(uint8_t* out, uint32_t op, uint32_t rem, uint32_t lane) {
  const uint32_t full = rem / 255;
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
  for (uint32_t j = lane; j < full; j += 64) out[op + j] = 255;
  if (lane == 0) out[op + full] = (uint8_t)(rem - full * 255);
  return op + full + 1;
}

// n literal bytes, a byte per lane and round.  (Left to itself the compiler unrolls and
// versions this loop for runs of thousands of bytes; a sequence's run is mostly < 64.)
__device__ __forceinline__ void lz4c_copy_literals(uint8_t* out, const uint8_t* in, uint32_t n, uint32_t lane) {
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
  for (uint32_t j = lane; j < n; j += 64) out[j] = in[j];
}

// One table entry per storing lane, several lanes may share an entry: the
// entry ends as the largest (kMax) or smallest stored position, whatever
// order the stores land in.  `act`: this lane stores.  Returns the entry.
template <bool kMax, class PosT>
__device__ __forceinline__ uint32_t lz4c_store_converge(PosT* tab, uint32_t slot, uint32_t pos, bool act) {
  if (act) tab[slot] = (PosT)pos;
  for (;;) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const uint32_t cur = act ? (uint32_t)tab[slot] : pos;
    const bool again = kMax ? cur < pos : cur > pos;
    if (__ballot(again) == 0) return cur;
    if (again) tab[slot] = (PosT)pos;
  }
}

// Match-table insert of this step's positions.  32-bit entries: an LDS atomic max, nothing to
// wait for (the next step's read follows it in the wave's LDS order).  16-bit entries (LDS
// has no 16-bit atomics): the store / read-back loop.
__device__ __forceinline__ void lz4c_insert(uint32_t* tab, uint32_t slot, uint32_t pos, bool act) {
  if (act) atomicMax(&tab[slot], pos);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}
__device__ __forceinline__ void lz4c_insert(uint16_t* tab, uint32_t slot, uint32_t pos, bool act) {
  lz4c_store_converge<true>(tab, slot, pos, act);
}

// The earliest position of this step (p .. p + 63, lane i at p + i) stored in the lane's
// step-table entry, or q where the entry holds none.  32-bit entries: one atomic max of
// (epoch, 63 - lane), epoch = the step's number from 1 (a cleared or older entry never
// matches it), then one read.  16-bit entries: the store / read-back loop; an entry of an
// earlier step that lies in this step's window is a position this step stores itself.
constexpr uint32_t kLzEpochs = 1u << 26;
__device__ __forceinline__ uint32_t lz4c_step_earliest(uint32_t* step, uint32_t slot, uint32_t p, uint32_t q,
                                                       uint32_t epoch, uint32_t lane, bool act) {
  if (act) atomicMax(&step[slot], (epoch << 6) | (63u - lane));
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  const uint32_t cur = act ? step[slot] : 0;
  return (cur >> 6) == epoch ? p + 63u - (cur & 63u) : q;
}
__device__ __forceinline__ uint32_t lz4c_step_earliest(uint16_t* step, uint32_t slot, uint32_t p, uint32_t q,
                                                       uint32_t epoch, uint32_t lane, bool act) {
  return lz4c_store_converge<false>(step, slot, q, act);
}

// The wave-step LZ4 block compressor.  in = base + p0 (base 4-byte aligned,
// readable 8 bytes past the payload), n payload bytes, out = room for
// lz4c_stream_bound(n) bytes, tab[1 << kBits] and step[kStep] cleared.
// PosT holds any position of the payload.  Returns the stream's length.
template <class PosT, uint32_t kBits, uint32_t kStep>
__device__ __forceinline__ uint32_t lz4_wave_compress(const uint8_t* base, uint32_t p0, uint32_t n, uint8_t* out,
                                                      PosT* tab, PosT* step, uint32_t lane) {
  const uint8_t* in = base + p0;
  uint32_t anchor = 0, op = 0;
  if (n >= 13) {
    const uint32_t mflimit = n - 12;  // the last position a match may start at
    const uint32_t mend = n - 5;      // a match ends at or before it
    uint32_t p = 0, epoch = 0;
    while (p <= mflimit) {
      if (++epoch == kLzEpochs) {  // (32-bit step table: 2^26 steps and the epochs start over)
        for (uint32_t w = lane; w < kStep; w += 64) step[w] = 0;
        epoch = 1;
      }
      const uint32_t q = p + lane;
      const bool act = q <= mflimit;
      const uint32_t v = act ? read_u32_unaligned(base, p0 + q) : 0;
      const uint32_t h = (v * 2654435761u) >> (32 - kBits);
      const uint32_t c1 = act ? (uint32_t)tab[h] : 0;  // the state before this step
      const uint32_t c2 = lz4c_step_earliest(step, h & (kStep - 1), p, q, epoch, lane, act);
      // candidates are read back at min(c, q): inside the payload whatever the tables hold
      // (and at 0 for a lane past the last position)
      const uint32_t v2 = read_u32_unaligned(base, p0 + (act ? min(c2, q) : 0));
      const uint32_t v1 = read_u32_unaligned(base, p0 + (act ? min(c1, q) : 0));
      const bool m2 = act && c2 < q && v2 == v;
      const bool m1 = act && c1 < q && q - c1 <= kLzMaxOffset && v1 == v;
      const uint64_t hit = __ballot(m1 || m2);
      if (hit == 0) {
        lz4c_insert(tab, h, q, act);
        p += 64;
        continue;
      }
      const uint32_t w = (uint32_t)__builtin_ctzll(hit);  // the lowest lane with a match wins
      lz4c_insert(tab, h, q, act && lane <= w);  // positions up to the match start stay inserted
      uint32_t cand = (uint32_t)__builtin_amdgcn_readlane((int)(m2 ? c2 : c1), (int)w);
      uint32_t ms = p + w;
      const uint32_t off = ms - cand;
      {  // backwards to the anchor while the bytes are equal
        const uint32_t kmax = min(ms - anchor, cand);
        uint32_t k = 0;
        while (k < kmax) {
          const uint32_t j = k + lane;
          const bool ok = j < kmax && in[ms - 1 - min(j, kmax - 1)] == in[cand - 1 - min(j, kmax - 1)];
          const uint64_t bad = __ballot(!ok);
          if (bad) {
            k += (uint32_t)__builtin_ctzll(bad);
            break;
          }
          k += 64;
        }
        ms -= k;
        cand -= k;
      }
      uint32_t end = p + w + 4;
      for (;;) {  // forwards, 64 bytes per round, up to n - 5
        const uint32_t x = end + lane;
        const uint32_t xc = min(x, mend - 1);  // (mend - 1 >= end - 1 >= off: xc - off stays inside the payload)
        const bool ok = x < mend && in[xc] == in[xc - off];
        const uint64_t bad = __ballot(!ok);
        if (bad) {
          end += (uint32_t)__builtin_ctzll(bad);
          break;
        }
        end += 64;
      }
      // the sequence: token, literal length, literals, offset, match length
      const uint32_t lit = ms - anchor, ml = end - ms - 4;
      if (lane == 0) out[op] = (uint8_t)((min(lit, 15u) << 4) | min(ml, 15u));
      op += 1;
      if (lit >= 15) op = lz4c_emit_ext(out, op, lit - 15, lane);
      lz4c_copy_literals(out + op, in + anchor, lit, lane);
      op += lit;
      if (lane == 0) {
        out[op] = (uint8_t)off;
        out[op + 1] = (uint8_t)(off >> 8);
      }
      op += 2;
      if (ml >= 15) op = lz4c_emit_ext(out, op, ml - 15, lane);
      if (lane == 0) {  // position end - 2, as liblz4 (later than every entry: a plain store)
        const uint32_t ve = read_u32_unaligned(base, p0 + end - 2);
        tab[(ve * 2654435761u) >> (32 - kBits)] = (PosT)(end - 2);
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      anchor = p = end;
    }
  }
  // the last sequence: literals only
  const uint32_t lit = n - anchor;
  if (lane == 0) out[op] = (uint8_t)(min(lit, 15u) << 4);
  op += 1;
  if (lit >= 15) op = lz4c_emit_ext(out, op, lit - 15, lane);
  lz4c_copy_literals(out + op, in + anchor, lit, lane);
  return op + lit;
}

// Coalesced dword copy of the payload's bytes into an LDS stage; returns the
// payload's position in the stage (0..3).
__device__ __forceinline__ uint32_t lz4c_stage(const LzBlock& k, uint32_t* lin, uint32_t lane) {
  const uint32_t a0 = k.p0 & ~3u, sh = k.p0 - a0;
  const uint32_t words = (sh + k.len + 3) / 4;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(k.base + a0);
  for (uint32_t w = lane; w < words; w += 64) lin[w] = src[w];
  return sh;
}

__device__ __forceinline__ void lz4c_clear(uint32_t* p, uint32_t words, uint32_t lane) {
  for (uint32_t w = lane; w < words; w += 64) p[w] = 0;
}

constexpr uint32_t kLzSmallStage = kLzSmallMax + 16;  // shift + the 8-byte over-read

__global__ __launch_bounds__(256) void lz4c_small_kernel(const uint8_t* __restrict__ blocks,
                                                         const uint64_t* __restrict__ block_off, uint32_t n,
                                                         const int32_t* in_status,
                                                         uint8_t* __restrict__ slots, uint64_t slots_cap,
                                                         uint32_t* __restrict__ sizes, int32_t* status) {
  __shared__ uint32_t s_in[4][kLzSmallStage / 4];  // 9,744 B per wave: four workgroups per CU
  __shared__ uint32_t s_tab[4][kLzSmallTab];
  __shared__ uint32_t s_step[4][kLzSmallStepTab];
  const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t b = blockIdx.x * 4 + wv;
  if (b >= n) return;
  LzBlock k;
  const int32_t st = lz4c_check_block(blocks, block_off, in_status, b, slots, slots_cap, k);
  if (st == ST_OK && k.len > kLzSmallMax) return;  // lz4c_big_kernel's
  uint32_t got = 0;
  if (st == ST_OK) {
    const uint32_t sh = lz4c_stage(k, s_in[wv], lane);
    lz4c_clear(s_tab[wv], kLzSmallTab, lane);
    lz4c_clear(s_step[wv], kLzSmallStepTab, lane);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    got = lz4_wave_compress<uint32_t, kLzSmallBits, kLzSmallStepTab>(reinterpret_cast<const uint8_t*>(s_in[wv]), sh,
                                                                     k.len, k.slot, s_tab[wv], s_step[wv], lane);
  }
  if (lane == 0) {
    sizes[b] = st == ST_OK ? kHdrLen + got : 0;
    status[b] = st;
  }
}

// Dynamic LDS of lz4c_big_kernel: the payload stage, then the two tables
// (16-bit positions; the HBM class lays its 32-bit tables over the stage).
constexpr uint32_t kLzBigStage = kLzStagedMax + 16;
constexpr uint32_t kLzBigLds = kLzBigStage + kLzTab * 2 + kLzStepTab * 2;
static_assert(kLzBigStage >= (kLzTab + kLzStepTab) * 4, "32-bit tables fit the stage");

// One block of lz4c_big_kernel (wave-uniform b): staged in LDS, or read from HBM.
__device__ __forceinline__ void lz4c_big_block(const uint8_t* blocks, const uint64_t* block_off, const int32_t* in_status,
                                               uint32_t b, uint8_t* slots, uint64_t slots_cap, uint32_t* sizes,
                                               int32_t* status, uint32_t* s_dyn, uint32_t lane) {
  LzBlock k;
  const int32_t st = lz4c_check_block(blocks, block_off, in_status, b, slots, slots_cap, k);
  if (st != ST_OK || k.len <= kLzSmallMax) return;  // lz4c_small_kernel's
  uint32_t got;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the previous block's LDS reads before these stores
  if (k.len <= kLzStagedMax) {
    uint16_t* tab = reinterpret_cast<uint16_t*>(s_dyn + kLzBigStage / 4);
    uint16_t* step = tab + kLzTab;
    const uint32_t sh = lz4c_stage(k, s_dyn, lane);
    lz4c_clear(reinterpret_cast<uint32_t*>(tab), (kLzTab + kLzStepTab) / 2, lane);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    got = lz4_wave_compress<uint16_t, kLzBits, kLzStepTab>(reinterpret_cast<const uint8_t*>(s_dyn), sh, k.len, k.slot,
                                                           tab, step, lane);
  } else {
    uint32_t* tab = s_dyn;
    uint32_t* step = tab + kLzTab;
    lz4c_clear(tab, kLzTab + kLzStepTab, lane);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    got = lz4_wave_compress<uint32_t, kLzBits, kLzStepTab>(k.base, k.p0, k.len, k.slot, tab, step, lane);
  }
  if (lane == 0) {
    sizes[b] = kHdrLen + got;
    status[b] = ST_OK;
  }
}

__global__ __launch_bounds__(64) void lz4c_big_kernel(const uint8_t* __restrict__ blocks,
                                                      const uint64_t* __restrict__ block_off, uint32_t n,
                                                      const int32_t* in_status,
                                                      uint8_t* __restrict__ slots, uint64_t slots_cap,
                                                      uint32_t* __restrict__ sizes, int32_t* status) {
  extern __shared__ uint32_t s_dyn[];
  const uint32_t lane = threadIdx.x;
  // Workgroup g takes the blocks g, g + G, g + 2 G, ...; 64 of them are sized at once (a lane
  // each), so a batch of small blocks costs this kernel one round of loads, not one per block.
  for (uint64_t r0 = 0; r0 * gridDim.x + blockIdx.x < n; r0 += 64) {
    const uint64_t cand = (r0 + lane) * gridDim.x + blockIdx.x;
    const bool big = cand < n && block_off[cand + 1] >= block_off[cand] &&
                     block_off[cand + 1] - block_off[cand] > (uint64_t)kHdrLen + kLzSmallMax;
    for (uint64_t todo = __ballot(big); todo; todo &= todo - 1)
      lz4c_big_block(blocks, block_off, in_status, (uint32_t)((r0 + (uint32_t)__builtin_ctzll(todo)) * gridDim.x + blockIdx.x),
                     slots, slots_cap, sizes, status, s_dyn, lane);
  }
}

struct LzOffOut {
  uint64_t* off;
  __device__ void operator()(uint64_t i, uint64_t prefix) const { off[i] = prefix; }
};

// Header' || stream at d_out[d_out_off[b] ..): one wave per block.
__global__ __launch_bounds__(256) void lz4c_pack_kernel(const uint8_t* __restrict__ blocks,
                                                        const uint64_t* __restrict__ block_off, uint32_t n,
                                                        const uint8_t* __restrict__ slots,
                                                        const uint32_t* __restrict__ sizes,
                                                        const uint64_t* __restrict__ out_off, uint8_t* __restrict__ out,
                                                        uint64_t out_cap, int32_t* __restrict__ status) {
  const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t b = blockIdx.x * 4 + wv;
  if (b >= n) return;
  if (__builtin_amdgcn_readfirstlane(status[b]) != ST_OK) return;  // rejected: 0 bytes, its status stands
  const uint64_t o0 = out_off[b], o1 = out_off[b + 1];
  if (o1 > out_cap) {  // no byte of it is written
    if (lane == 0) status[b] = ST_OVERFLOW;
    return;
  }
  const uint32_t len = __builtin_amdgcn_readfirstlane(sizes[b]) - kHdrLen;
  const uint64_t o = block_off[b];
  const uint8_t* src = slots + lz4c_slot_start(o - block_off[0], b);
  uint64_t lo, hi;
  xxh3_128_wave(src, 0, len, &kLongSecret, lo, hi);
  uint8_t* dst = out + o0;
  if (lane == 0) {
    const uint8_t* base = blocks + (o & ~15ULL);
    const uint32_t hb = (uint32_t)(o & 15);
    uint32_t h[12] = {0};  // 29 header bytes + the readers' over-read
    uint8_t* hp = reinterpret_cast<uint8_t*>(h);
    for (uint32_t j = 0; j < 5; ++j) hp[j] = base[hb + j];  // magic, type
    for (uint32_t j = 0; j < 8; ++j) {
      hp[5 + j] = (uint8_t)(lo >> (8 * j));
      hp[13 + j] = (uint8_t)(hi >> (8 * j));
    }
    const uint32_t raw = read_u32_unaligned(base, hb + 25);
    for (uint32_t j = 0; j < 4; ++j) {
      hp[21 + j] = (uint8_t)(len >> (8 * j));
      hp[25 + j] = (uint8_t)(raw >> (8 * j));
    }
    uint64_t clo, chi;
    xxh3_128_short(29, BaseReader8{hp, 0}, BaseReader64{hp, 0}, clo, chi);
    for (uint32_t j = 0; j < 4; ++j) hp[29 + j] = (uint8_t)(clo >> (8 * j));
    for (uint32_t j = 0; j < kHdrLen; ++j) dst[j] = hp[j];
  }
  // the stream: head bytes up to the first aligned dword of the destination,
  // dwords built from two aligned slot dwords, then the tail bytes
  uint8_t* d = dst + kHdrLen;
  uint32_t head = (4u - (uint32_t)((uintptr_t)d & 3)) & 3u;
  if (head > len) head = len;
  if (lane < head) d[lane] = src[lane];
  const uint32_t body = (len - head) >> 2, s = head & 3u;
  const uint32_t* s32 = reinterpret_cast<const uint32_t*>(src);
  uint32_t* d32 = reinterpret_cast<uint32_t*>(d + head);
  for (uint32_t w = lane; w < body; w += 64) d32[w] = s ? alignbyte(s32[w + 1], s32[w], s) : s32[w];
  for (uint32_t j = head + 4 * body + lane; j < len; j += 64) d[j] = src[j];
}

}  // namespace lsmgpu

using namespace lsmgpu;

extern "C" uint64_t lsm_lz4_compress_bound(uint64_t blocks_bytes, uint32_t n_blocks) {
  // per block 33 + len + len / 255 + 16, and the blocks' bytes are the sum of 33 + len
  return blocks_bytes + blocks_bytes / 255 + 16 * (uint64_t)n_blocks;
}

namespace {
struct LzLayout {
  size_t sizes, tiles, slots, total;
};
LzLayout lz4c_layout(uint32_t n_blocks, uint64_t blocks_bytes) {
  Carver c;
  LzLayout l;
  l.sizes = c.take((size_t)n_blocks * 4);
  l.tiles = c.take(scan_tiles(n_blocks ? n_blocks : 1) * 8);
  l.slots = c.take(lz4c_slots_bytes(blocks_bytes, n_blocks));
  l.total = c.total();
  return l;
}
}  // namespace

extern "C" size_t lsm_lz4_compress_workspace_size(uint32_t n_blocks, uint64_t blocks_bytes) {
  return lz4c_layout(n_blocks, blocks_bytes).total;
}

extern "C" int lsm_lz4_compress_blocks(const uint8_t* d_blocks, const uint64_t* d_block_off, uint32_t n_blocks,
                                       const int32_t* d_in_status, uint8_t* d_out, uint64_t out_cap,
                                       uint64_t* d_out_off, int32_t* d_status, void* d_workspace,
                                       size_t workspace_bytes, void* stream) {
  if (n_blocks == 0) return LSM_OK;
  if (!d_blocks || !d_block_off || !d_out || !d_out_off || !d_status || !d_workspace || ((uintptr_t)d_blocks & 15) ||
      ((uintptr_t)d_block_off & 7) || ((uintptr_t)d_out_off & 7) || ((uintptr_t)d_status & 3) ||
      ((uintptr_t)d_in_status & 3) || ((uintptr_t)d_workspace & 255) ||
      workspace_bytes < lsm_lz4_compress_workspace_size(n_blocks, 0))
    return LSM_BAD_ARG;
  const hipStream_t st = (hipStream_t)stream;
  const LzLayout l = lz4c_layout(n_blocks, 0);  // (the slot region is last: it takes what the workspace has)
  uint8_t* ws = (uint8_t*)d_workspace;
  uint32_t* sizes = (uint32_t*)(ws + l.sizes);
  uint64_t* tiles = (uint64_t*)(ws + l.tiles);
  uint8_t* slots = ws + l.slots;
  const uint64_t slots_cap = workspace_bytes - l.slots;
  static uint64_t attr_done = 0;
  hipError_t e = set_lds_attr((const void*)lz4c_big_kernel, kLzBigLds, &attr_done);
  if (e != hipSuccess) return hip_status(e, "lsm_lz4_compress_blocks");
  hipLaunchKernelGGL(lz4c_small_kernel, dim3((n_blocks + 3) / 4), dim3(256), 0, st, d_blocks, d_block_off, n_blocks,
                     d_in_status, slots, slots_cap, sizes, d_status);
  const uint32_t grid = n_blocks < 1024 ? n_blocks : 1024;
  hipLaunchKernelGGL(lz4c_big_kernel, dim3(grid), dim3(64), kLzBigLds, st, d_blocks, d_block_off, n_blocks,
                     d_in_status, slots, slots_cap, sizes, d_status);
  if ((e = launch_excl_scan(sizes, n_blocks, tiles, LzOffOut{d_out_off}, st)) != hipSuccess)
    return hip_status(e, "lsm_lz4_compress_blocks");
  hipLaunchKernelGGL(lz4c_pack_kernel, dim3((n_blocks + 3) / 4), dim3(256), 0, st, d_blocks, d_block_off, n_blocks,
                     slots, sizes, d_out_off, d_out, out_cap, d_status);
  return hip_status(hipGetLastError(), "lsm_lz4_compress_blocks");
}
