// gather.hpp — byte gathers shared by the merge, the index-entry and the
// materialize-items kernels: a wave assembles the contiguous output span of its
// 64 items in LDS and stores it 16 B per lane at any alignment (gather_field =
// lds_put + span_store, or gather_direct); long items are copied by the whole
// wave (wave_copy).  Sources are read through 16-B aligned windows,
// so a source arena must be readable LSM_INPUT_PADDING bytes past its end.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.hpp"

namespace lsmgpu {

constexpr uint32_t kGatherBuf = 8192;   // LDS bytes of one gather step (64 values of up to 128 B)
constexpr uint32_t kGatherLong = 256;   // keys / values from this length on are copied by the whole wave

// Bytes m .. m + 16 of the 32 bytes (q0 q1 | q2 q3), m in 0..15.
__device__ __forceinline__ void shift128(uint64_t q0, uint64_t q1, uint64_t q2, uint64_t q3, uint32_t m, uint64_t& lo,
                                         uint64_t& hi) {
  if (m & 8) {
    q0 = q1;
    q1 = q2;
    q2 = q3;
  }
  const uint32_t sh = (m & 7) * 8;
  lo = sh ? (q0 >> sh) | (q1 << (64 - sh)) : q0;
  hi = sh ? (q1 >> sh) | (q2 << (64 - sh)) : q1;
}
__device__ __forceinline__ uint64_t pack64(uint32_t a, uint32_t b) { return (uint64_t)a | ((uint64_t)b << 32); }

// Wave-cooperative copy of len bytes (all arguments wave-uniform): byte
// granular up to the first 16-byte boundary of dst and after the last, 16 B
// per lane between them from two aligned source windows.
__device__ __forceinline__ void wave_copy(const uint8_t* src, uint8_t* dst, uint64_t len, uint32_t lane) {
  const uint64_t head = min(len, (16 - ((uint64_t)(uintptr_t)dst & 15)) & 15);
  if (lane < head) dst[lane] = src[lane];
  const uint8_t* sb = src + head;
  uint8_t* db = dst + head;
  const uint64_t nb = (len - head) >> 4;
  const uint32_t m = (uint32_t)((uint64_t)(uintptr_t)sb & 15);
  const u32x4* sw = reinterpret_cast<const u32x4*>(sb - m);
  for (uint64_t c = lane; c < nb; c += 64) {
    const u32x4 a = gload(sw, c);
    u32x4 o = a;
    if (m) {
      const u32x4 b = gload(sw, c + 1);
      uint64_t lo, hi;
      shift128(pack64(a.x, a.y), pack64(a.z, a.w), pack64(b.x, b.y), pack64(b.z, b.w), m, lo, hi);
      o = u32x4{(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
    }
    gstore(reinterpret_cast<u32x4*>(db), c, o);
  }
  const uint64_t done = head + 16 * nb;
  if (done + lane < len) dst[done + lane] = src[done + lane];
}

// Lane-private part of a gather step: src[0 .. len) -> LDS d[0 .. len), 16 source
// bytes at a time through aligned global windows (reads up to 31 bytes past src + len).
__device__ __forceinline__ void lds_put(const uint8_t* src, uint32_t len, uint8_t* d) {
  if (len) {
    const uint64_t sa = (uint64_t)(uintptr_t)src;
    const uint32_t m = (uint32_t)(sa & 15);
    const u32x4* w = reinterpret_cast<const u32x4*>(sa & ~15ULL);
    u32x4 cur = gload(w, 0);
    for (uint32_t c = 0; 16 * c < len; ++c) {
      const u32x4 nxt = gload(w, (uint64_t)c + 1);
      uint64_t lo, hi;
      shift128(pack64(cur.x, cur.y), pack64(cur.z, cur.w), pack64(nxt.x, nxt.y), pack64(nxt.z, nxt.w), m, lo, hi);
      const uint32_t cnt = min(16u, len - 16 * c);
      uint8_t* dd = d + 16 * c;
#pragma unroll
      for (uint32_t t = 0; t < 16; ++t)
        if (t < cnt) dd[t] = (uint8_t)((t < 8 ? lo : hi) >> (8 * (t & 7)));
      cur = nxt;
    }
  }
}

// Wave part of a gather step: the span out[o0 .. o1), assembled by the lanes in
// bf at its global alignment (bf[pad ..), pad = (out + o0) & 15), goes out 16 B
// per lane, the partial pieces at both ends byte-wise.  Wave barriers on both sides.
__device__ __forceinline__ void span_store(uint8_t* out, uint64_t o0, uint64_t o1, uint32_t pad, const uint8_t* bf,
                                           uint32_t lane) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
  // copy-out: whole 16-B pieces, then the partial ones at both ends
  uint8_t* gdst = out + o0 - pad;  // 16-B aligned
  const uint32_t end = pad + (uint32_t)(o1 - o0);
  const uint32_t q0 = (pad + 15) >> 4, q1 = end >> 4;
  for (uint32_t q = q0 + lane; q < q1; q += 64)
    gstore(reinterpret_cast<u32x4*>(gdst), q, reinterpret_cast<const u32x4*>(bf)[q]);
  if (lane == 0)
    for (uint32_t x = pad; x < min(16 * q0, end); ++x) gdst[x] = bf[x];
  if (lane == 1 && q1 >= q0)
    for (uint32_t x = 16 * q1; x < end; ++x) gdst[x] = bf[x];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
}

// Straight to global, for a step that holds a long item or overflows the LDS
// buffer: long items by the whole wave, the others byte-wise by their lane.
__device__ __forceinline__ void gather_direct(const uint8_t* src, uint32_t len, uint8_t* dst, uint32_t lane) {
  uint64_t longs = __ballot(len >= kGatherLong);
  while (longs) {
    const uint32_t l = (uint32_t)__builtin_ctzll(longs);
    longs &= longs - 1;
    const uint64_t sa = wave_readlane_u64((uint64_t)(uintptr_t)src, l);
    const uint64_t da = wave_readlane_u64((uint64_t)(uintptr_t)dst, l);
    const uint32_t ll = wave_readlane_u32(len, l);
    wave_copy(reinterpret_cast<const uint8_t*>((uintptr_t)sa), reinterpret_cast<uint8_t*>((uintptr_t)da), ll, lane);
  }
  if (len < kGatherLong)
    for (uint32_t t = 0; t < len; ++t) dst[t] = src[t];
}

// One field (keys or values) of one step: lane's item is src[0 .. len) ->
// out[o .. o + len) (len 0 for dropped and idle lanes); the step's outputs are
// the contiguous span out[o0 .. o1).
__device__ __forceinline__ void gather_field(const uint8_t* src, uint32_t len, uint8_t* out, uint64_t o, uint64_t o0,
                                             uint64_t o1, uint8_t* bf, uint32_t lane) {
  if (o1 == o0) return;
  const uint32_t pad = (uint32_t)(((uint64_t)(uintptr_t)out + o0) & 15);
  if (__ballot(len >= kGatherLong) || o1 - o0 + pad > kGatherBuf) {
    gather_direct(src, len, out + o, lane);
    return;
  }
  lds_put(src, len, bf + (uint32_t)(o - o0) + pad);
  span_store(out, o0, o1, pad, bf, lane);
}

}  // namespace lsmgpu
