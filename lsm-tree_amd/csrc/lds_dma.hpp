// lds_dma.hpp — LDS-DMA issue (global_load_lds_*) and counted vmcnt waits for
// loader waves on gfx950.
//
// The loader DMA (dma16) is inline asm on purpose: hipcc's waitcnt pass drains
// an LDS-DMA it knows about (vmcnt(0)) before every later LDS access of the
// issuing wave, which would serialise a loader that polls LDS flags between
// issues.  Asm loads are invisible to that pass, so the issuing wave counts
// them itself (vm_wait_n) — cdna_hip_programming.md, "LDS-DMA recipe".
// Whole stages that are waited for at once go through the builtin
// (stage_to_lds).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lsmgpu {

// 16 bytes per lane HBM -> LDS (M0 = wave-uniform LDS base; lane l lands at +16 l).
// Inline asm so the compiler neither drains it nor counts it: the loader
// waits for it with its own counted vmcnt (cdna_hip_programming.md, LDS-DMA recipe).
template <bool kNt>
__device__ __forceinline__ void dma16(const uint8_t* src, uint32_t lds_dst) {
  uint32_t keep;
  if constexpr (kNt)
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(src), "s"(lds_dst) : "memory");
  else
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(src), "s"(lds_dst) : "memory");
}
template <int N>
__device__ __forceinline__ void vm_wait() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// s_waitcnt vmcnt(n) for a run-time n (clamped to 63: loads retire in order,
// so <= 63 outstanding also means every older load has landed).
__device__ __forceinline__ void vm_wait_n(uint32_t n) {
  n = n > 63 ? 63 : n;
  switch (n) {
#define LSM_VMW(i) case i: vm_wait<i>(); break;
#define LSM_VMW8(i) LSM_VMW(i) LSM_VMW(i + 1) LSM_VMW(i + 2) LSM_VMW(i + 3) LSM_VMW(i + 4) LSM_VMW(i + 5) LSM_VMW(i + 6) LSM_VMW(i + 7)
    LSM_VMW8(0) LSM_VMW8(8) LSM_VMW8(16) LSM_VMW8(24) LSM_VMW8(32) LSM_VMW8(40) LSM_VMW8(48) LSM_VMW8(56)
#undef LSM_VMW8
#undef LSM_VMW
    default: vm_wait<0>();
  }
}
// s_waitcnt vmcnt(0) lgkmcnt(0) (simm16 0x0070 on gfx9: vmcnt = 0, expcnt = 7
// (no wait), lgkmcnt = 0): every load and store of this wave has completed,
// the stage DMA and the item fields it was issued for, and its LDS
// and scalar-memory accesses as well.
__device__ __forceinline__ void vm_lgkm_wait0() { __builtin_amdgcn_s_waitcnt(0x0070); }

// Stage copy HBM -> LDS through the compiler's own LDS-DMA builtin (the
// compiler counts these: for stages that are waited for as a whole).  The n16
// 16-byte pieces of src (16-aligned) go to lds_dst in runs of 64, one run
// (1 KiB, lane l its piece l) per instruction: this wave issues runs first,
// first + step, ...; a wave that copies alone passes first = 0, step = 1.
__device__ __forceinline__ void stage_to_lds(const uint8_t* src, uint8_t* lds_dst, uint32_t n16, uint32_t first,
                                             uint32_t step, int lane) {
  typedef __attribute__((address_space(3))) void lds_void_t;
  typedef const __attribute__((address_space(1))) void gbl_void_t;
  const uint8_t* s = src + 16 * lane;
  for (uint32_t i = first; i * 64 < n16; i += step)
    if (i * 64 + lane < n16)
      __builtin_amdgcn_global_load_lds((gbl_void_t*)(s + 1024 * i), (lds_void_t*)(lds_dst + 1024 * i), 16, 0, 0);
}

}  // namespace lsmgpu
