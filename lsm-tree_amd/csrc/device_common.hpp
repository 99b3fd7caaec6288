// device_common.hpp — gfx950 device building blocks for the SST block codec.
//
// * Format constants and statuses, explicit global-address-space access.
// * Unaligned 16-byte windows over LDS or global bytes (aligned dword reads +
//   v_alignbyte_b32).
// * LEB128 (varint-rs) decoding from a 16-byte register window.
// * Wave scans, broadcasts and the wave minimum.
// * XXH3-64 / XXH3-128: xxh3.hpp, included at the end of this file.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lds_dma.hpp"

namespace lsmgpu {

constexpr int kWave = 64;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// Explicit global-address-space access.  Generic (flat) pointers compile to
// flat_load/flat_store, which count on lgkmcnt as well as vmcnt: every LDS
// wait after a flat store would also wait for the store to reach memory.
template <class T>
__device__ __forceinline__ void gstore(T* p, uint64_t i, T v) {
  ((__attribute__((address_space(1))) T*)p)[i] = v;
}
template <class T>
__device__ __forceinline__ T gload(const T* p, uint64_t i) {
  return ((const __attribute__((address_space(1))) T*)p)[i];
}
// A trivially copyable struct element by explicit global loads (gload cannot
// copy a struct through an address-space-qualified lvalue).
template <class T>
__device__ __forceinline__ T gload_pod(const T* p, uint64_t i) {
  static_assert(sizeof(T) % 8 == 0, "8-byte multiple");
  T r;
  const __attribute__((address_space(1))) uint64_t* src = (const __attribute__((address_space(1))) uint64_t*)(p + i);
  uint64_t* dst = reinterpret_cast<uint64_t*>(&r);
#pragma unroll
  for (uint32_t k = 0; k < sizeof(T) / 8; ++k) dst[k] = src[k];
  return r;
}
constexpr uint32_t kHdrLen = 33;
constexpr uint32_t kTrailerLen = 31;
constexpr uint8_t kTrailerMarker = 0xFF;
constexpr uint8_t kHashFree = 254;
constexpr uint8_t kHashConflict = 255;
constexpr uint32_t kHashMaxPointers = 254;

enum : int32_t {
  ST_OK = 0, ST_BAD_MAGIC = 1, ST_BAD_TYPE = 2, ST_HDR_CKSUM = 3, ST_CKSUM = 4, ST_PARSE = 5,
  ST_OVERFLOW = 6, ST_TYPE_MISMATCH = 7, ST_TRUNCATED = 8, ST_UNSUPPORTED = 9, ST_BAD_ARG = 10,
  ST_INCOMPLETE = 13  // LSM_INCOMPLETE: a streamed chain gave up waiting; the fallback pass re-verifies the block
};

// ------------------------------------------------- byte access (LDS / global)
// `base` is 16-byte aligned (an LDS image base or a global span base); all
// reads are aligned dwords, unaligned views are assembled with v_alignbyte.
__device__ __forceinline__ uint32_t ld32(const uint8_t* base, uint32_t aligned_off) {
  return *reinterpret_cast<const uint32_t*>(base + aligned_off);
}
__device__ __forceinline__ uint32_t alignbyte(uint32_t hi, uint32_t lo, uint32_t shift) {
  return __builtin_amdgcn_alignbyte(hi, lo, shift);
}

struct Win16 {
  uint64_t lo, hi;
};
// 16 bytes at base[pos..pos+16) (reads up to 4 bytes past pos+16).
__device__ __forceinline__ Win16 read_win16(const uint8_t* base, uint32_t pos) {
  const uint32_t a = pos & ~3u, s = pos & 3u;
  uint32_t d0 = ld32(base, a), d1 = ld32(base, a + 4), d2 = ld32(base, a + 8),
           d3 = ld32(base, a + 12), d4 = ld32(base, a + 16);
  uint32_t e0 = alignbyte(d1, d0, s), e1 = alignbyte(d2, d1, s), e2 = alignbyte(d3, d2, s),
           e3 = alignbyte(d4, d3, s);
  return {(uint64_t)e0 | ((uint64_t)e1 << 32), (uint64_t)e2 | ((uint64_t)e3 << 32)};
}
// read_win16 with the dword-aligned offset a and the shift s split out, for
// loops that step a window by whole dwords: a + constant folds into the
// ds_read offsets, and the alignment is computed once per loop, not per window.
__device__ __forceinline__ Win16 read_win16_split(const uint8_t* base, uint32_t a, uint32_t s) {
  const uint32_t d0 = ld32(base, a), d1 = ld32(base, a + 4), d2 = ld32(base, a + 8), d3 = ld32(base, a + 12),
                 d4 = ld32(base, a + 16);
  return {(uint64_t)alignbyte(d1, d0, s) | ((uint64_t)alignbyte(d2, d1, s) << 32),
          (uint64_t)alignbyte(d3, d2, s) | ((uint64_t)alignbyte(d4, d3, s) << 32)};
}
// The same from an LDS pointer (explicit address space: ds_read even where
// the compiler cannot tell that a generic pointer is LDS).
__device__ __forceinline__ Win16 read_win16_lds(const uint8_t* base_generic, uint32_t pos) {
  const __attribute__((address_space(3))) uint32_t* b =
      (const __attribute__((address_space(3))) uint32_t*)(const __attribute__((address_space(3))) uint8_t*)base_generic;
  const uint32_t a = pos >> 2, s = pos & 3u;
  const uint32_t d0 = b[a], d1 = b[a + 1], d2 = b[a + 2], d3 = b[a + 3], d4 = b[a + 4];
  return {(uint64_t)alignbyte(d1, d0, s) | ((uint64_t)alignbyte(d2, d1, s) << 32),
          (uint64_t)alignbyte(d3, d2, s) | ((uint64_t)alignbyte(d4, d3, s) << 32)};
}
__device__ __forceinline__ uint32_t read_u32_unaligned(const uint8_t* base, uint32_t pos) {
  const uint32_t a = pos & ~3u, s = pos & 3u;
  return alignbyte(ld32(base, a + 4), ld32(base, a), s);
}
__device__ __forceinline__ uint64_t read_u64_unaligned(const uint8_t* base, uint32_t pos) {
  const uint32_t a = pos & ~3u, s = pos & 3u;
  const uint32_t d0 = ld32(base, a), d1 = ld32(base, a + 4), d2 = ld32(base, a + 8);
  return (uint64_t)alignbyte(d1, d0, s) | ((uint64_t)alignbyte(d2, d1, s) << 32);
}
__device__ __forceinline__ uint16_t read_u16_unaligned(const uint8_t* base, uint32_t pos) {
  return (uint16_t)(read_u32_unaligned(base, pos) & 0xFFFF);
}

// Drop the low n bytes (0 <= n <= 16) of a 128-bit window.
__device__ __forceinline__ void win_shift(Win16& w, uint32_t n) {
  if (n >= 16) {
    w.lo = w.hi = 0;
    return;
  }
  if (n >= 8) {
    w.lo = w.hi;
    w.hi = 0;
    n -= 8;
  }
  if (n) {
    w.lo = (w.lo >> (8 * n)) | (w.hi << (64 - 8 * n));
    w.hi >>= 8 * n;
  }
}

// LEB128 (varint-rs VarintReader) from the low bytes of a window.
// Returns the byte length (1..max_bytes) or 0 if the varint does not
// terminate within min(max_bytes, avail) bytes.  Value is truncated to the
// type width by the caller's mask (`as $type` in varint-rs).
__device__ __forceinline__ uint32_t leb_decode(const Win16& w, uint32_t max_bytes, uint32_t avail,
                                                uint64_t& v) {
  const uint64_t msb = 0x8080808080808080ULL;
  uint64_t stop = ~w.lo & msb;
  uint32_t n;
  if (stop) {
    n = (uint32_t)(__builtin_ctzll(stop) >> 3) + 1;  // 1..8
  } else {
    uint64_t stop2 = ~w.hi & 0x8080ULL;              // bytes 9, 10
    n = stop2 ? 9 + (uint32_t)(__builtin_ctzll(stop2) >> 3) : 99;
  }
  if (n > max_bytes || n > avail) return 0;
  uint64_t x = w.lo;
  if (n < 8) x &= (1ULL << (8 * n)) - 1;
  // compact 7-bit groups: 8 x 7 -> 56 bits
  x = ((x & 0x7F007F007F007F00ULL) >> 1) | (x & 0x007F007F007F007FULL);
  x = ((x & 0x3FFF00003FFF0000ULL) >> 2) | (x & 0x00003FFF00003FFFULL);
  x = ((x & 0x0FFFFFFF00000000ULL) >> 4) | (x & 0x000000000FFFFFFFULL);
  if (n > 8) {
    x |= (w.hi & 0x7FULL) << 56;
    if (n > 9) x |= (w.hi & 0x7F00ULL) << 55;  // bits 63..69 (only bit 63 survives)
  }
  v = x;
  return n;
}

// ------------------------------------------------------------ wave helpers
__device__ __forceinline__ uint32_t wave_incl_scan_u32(uint32_t v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    uint32_t t = __shfl_up((int)v, d);
    if (lane >= d) v += t;
  }
  return v;
}
__device__ __forceinline__ uint64_t wave_incl_scan_u64(uint64_t v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    uint32_t lo = __shfl_up((int)(uint32_t)v, d), hi = __shfl_up((int)(uint32_t)(v >> 32), d);
    uint64_t t = (uint64_t)lo | ((uint64_t)hi << 32);
    if (lane >= d) v += t;
  }
  return v;
}
__device__ __forceinline__ uint32_t wave_bcast_u32(uint32_t v, int src) { return __shfl((int)v, src); }
__device__ __forceinline__ uint64_t wave_bcast_u64(uint64_t v, int src) {
  uint32_t lo = __shfl((int)(uint32_t)v, src), hi = __shfl((int)(uint32_t)(v >> 32), src);
  return (uint64_t)lo | ((uint64_t)hi << 32);
}
// per-lane source lane (ds_bpermute)
__device__ __forceinline__ uint64_t wave_shfl_u64(uint64_t v, int src) { return wave_bcast_u64(v, src); }
// wave-uniform source lane (v_readlane -> SGPR)
__device__ __forceinline__ uint32_t wave_readlane_u32(uint32_t v, uint32_t src) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)src);
}
__device__ __forceinline__ uint64_t wave_readlane_u64(uint64_t v, uint32_t src) {
  return (uint64_t)wave_readlane_u32((uint32_t)v, src) | ((uint64_t)wave_readlane_u32((uint32_t)(v >> 32), src) << 32);
}
// wave-wide minimum, wave-uniform (SGPR); every lane must be active.  Four DPP
// steps inside the 16-lane rows (quad perms and row mirrors read an in-range
// lane for every lane), then the four rows by v_readlane: no LDS round trip.
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
  v = min(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
  v = min(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, true));   // quad_perm [2,3,0,1]
  v = min(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x141, 0xF, 0xF, true));  // row_half_mirror
  v = min(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x140, 0xF, 0xF, true));  // row_mirror
  const uint32_t r0 = wave_readlane_u32(v, 0), r1 = wave_readlane_u32(v, 16);
  const uint32_t r2 = wave_readlane_u32(v, 32), r3 = wave_readlane_u32(v, 48);
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)min(min(r0, r1), min(r2, r3)));
}

}  // namespace lsmgpu

#include "xxh3.hpp"  // (after the byte windows it reads through)
