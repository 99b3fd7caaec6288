// items_gather.hpp — the wave that copies 64 consecutive output rows of an
// lsm_items-shaped SoA (key = prefix || suffix, value), shared by
// mi_gather_kernel (materialize_items.hip: rows named by a decode's parsed SoA)
// and rr_gather_kernel (table_range_rows.hip: rows named by the descriptors its
// rows pass left in the workspace).  The body is written over a row source:
//   void locate(uint64_t R, uint64_t i0, uint64_t i)   wave-uniform control flow; before row()
//   MiRow row(uint64_t i)                              the row's three byte ranges
//   uint64_t seqno(uint64_t i), uint8_t vtype(uint64_t i)   read when kMeta
//   static constexpr bool kMeta                        the gather stores seqno / vtype too
#pragma once

#include "gather.hpp"
#include "lsmgpu.h"

namespace lsmgpu {

// One row as the gather copies it.  A rejected row has ok = false and all
// lengths 0.
struct MiRow {
  const uint8_t* pre;  // prefix_len bytes of the restart head's key
  const uint8_t* suf;  // key_len bytes
  const uint8_t* val;
  uint32_t pl, kl, vl;
  bool ok;
};

// The cursor and the outputs of one gather: d_base / d_end as u64[3] {items, key
// bytes, value bytes}, the offsets the plan wrote, the arenas and their capacities.
struct ItemsOut {
  const uint64_t* base;  // null = zeros
  const uint64_t* end;
  const uint64_t* out_key_off;
  const uint64_t* out_val_off;
  uint64_t item_cap, key_cap, val_cap;
  uint8_t* out_keys;
  uint8_t* out_vals;
  uint64_t* out_seqno;
  uint8_t* out_vtype;
  int32_t* result;
};

constexpr uint32_t kMiWaves = 4;
// The gather's LDS buffer per wave: half of kGatherBuf, which doubles the waves per
// CU (the kernel waits on dependent loads: block search, row, source bytes); a
// tile of 64-byte values still fits when it starts 16-byte aligned.
constexpr uint32_t kMiBuf = 4096;

// gather_field through the smaller buffer: the tile's span at once when it fits,
// else its two half tiles one after the other, each through the buffer when it
// fits and straight to global when not.
__device__ __forceinline__ void mi_field(const uint8_t* src, uint32_t len, uint8_t* out, uint64_t o, uint64_t o0,
                                         uint64_t o1, uint32_t nrow, uint8_t* bf, uint32_t lane) {
  if (o1 == o0) return;
  if (__ballot(len >= kGatherLong)) {
    gather_direct(src, len, out + o, lane);
    return;
  }
  const uint32_t pad = (uint32_t)(((uint64_t)(uintptr_t)out + o0) & 15);
  if (o1 - o0 + pad <= kMiBuf) {
    lds_put(src, len, bf + (uint32_t)(o - o0) + pad);
    span_store(out, o0, o1, pad, bf, lane);
    return;
  }
  const uint32_t h = nrow / 2;
  const uint64_t om = wave_readlane_u64(o, h);
#pragma unroll
  for (uint32_t half = 0; half < 2; ++half) {
    const uint64_t a = half ? om : o0, e = half ? o1 : om;
    const uint32_t l = (half ? lane >= h : lane < h) ? len : 0;
    const uint32_t p = (uint32_t)(((uint64_t)(uintptr_t)out + a) & 15);
    if (e == a) continue;
    if (e - a + p <= kMiBuf) {
      lds_put(src, l, bf + (uint32_t)(o - a) + p);
      span_store(out, a, e, p, bf, lane);
    } else {
      gather_direct(src, l, out + o, lane);
    }
  }
}

// The body of a gather kernel of kMiWaves * 64 threads: wave w of workgroup
// blockIdx.x copies the rows [i0, i0 + 64) of the source's rows (clipped to the
// cursor's row count), i0 = (blockIdx.x * kMiWaves + w) * 64.  rows = the
// source's row count; null = a row that names no bytes.
template <class Src>
__device__ __forceinline__ void items_gather_tile(Src& S, const ItemsOut& O, uint64_t rows, const uint8_t* null,
                                                  uint8_t (*buf)[kMiBuf + 32]) {
  const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t base0 = O.base ? O.base[0] : 0, base1 = O.base ? O.base[1] : 0, base2 = O.base ? O.base[2] : 0;
  const uint64_t end0 = O.end[0], end1 = O.end[1], end2 = O.end[2];
  // all rows or none (the caller sized the outputs without a host sync)
  const bool fits = end0 <= O.item_cap && end1 <= O.key_cap && end2 <= O.val_cap && base0 <= end0 &&
                    base1 <= end1 && base2 <= end2;
  if (blockIdx.x == 0 && threadIdx.x == 0) *O.result = fits ? LSM_OK : LSM_OVERFLOW;
  if (!fits) return;
  const uint64_t R = min(rows, end0 - base0);
  const uint64_t i0 = ((uint64_t)blockIdx.x * kMiWaves + w) * 64;
  if (i0 >= R) return;
  const uint32_t nrow = (uint32_t)min((uint64_t)64, R - i0);
  const bool live = lane < nrow;
  const uint64_t i = i0 + lane;
  S.locate(R, i0, i);
  MiRow r{null, null, null, 0, 0, 0, false};
  uint64_t ko = 0, vo = 0;
  if (live) {
    r = S.row(i);
    ko = O.out_key_off[base0 + i];
    vo = O.out_val_off[base0 + i];
  }
  // the tile's output spans [ko0, ko1) and [vo0, vo1): contiguous, rows in order
  // (64-bit broadcasts go through uint32_t halves: an offset with bit 31 set is not sign-filled)
  const uint32_t klen = r.pl + r.kl;
  const uint64_t ko0 = wave_readlane_u64(ko, 0), ko1 = wave_readlane_u64(ko + klen, nrow - 1);
  const uint64_t vo0 = wave_readlane_u64(vo, 0), vo1 = wave_readlane_u64(vo + r.vl, nrow - 1);
  // offsets that are not this plan's (a span outside the cursor's range, a row outside its span): no store
  const bool stray = live && (ko < ko0 || ko + klen > ko1 || vo < vo0 || vo + r.vl > vo1);
  if (__ballot(stray) || ko0 < base1 || ko1 > end1 || vo0 < base2 || vo1 > end2) return;
  uint8_t* bf = buf[w];
  if (ko1 > ko0) {
    const uint32_t pad = (uint32_t)(((uint64_t)(uintptr_t)O.out_keys + ko0) & 15);
    if (__ballot(r.pl >= kGatherLong || r.kl >= kGatherLong) || ko1 - ko0 + pad > kMiBuf) {
      gather_direct(r.pre, r.pl, O.out_keys + ko, lane);
      gather_direct(r.suf, r.kl, O.out_keys + ko + r.pl, lane);
    } else {
      uint8_t* d = bf + (uint32_t)(ko - ko0) + pad;
      lds_put(r.pre, r.pl, d);
      lds_put(r.suf, r.kl, d + r.pl);
      span_store(O.out_keys, ko0, ko1, pad, bf, lane);
    }
  }
  mi_field(r.val, r.vl, O.out_vals, vo, vo0, vo1, nrow, bf, lane);
  if (Src::kMeta && live) {
    gstore(O.out_seqno, base0 + i, (uint64_t)(r.ok ? S.seqno(i) : 0));
    gstore(O.out_vtype, base0 + i, (uint8_t)(r.ok ? S.vtype(i) : 0));
  }
}

}  // namespace lsmgpu
