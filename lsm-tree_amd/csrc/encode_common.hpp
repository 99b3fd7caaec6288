// encode_common.hpp — what more than one stage of the encode path uses (encode.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <type_traits>

#include "block_format.hpp"
#include "encode.hpp"
#include "host_common.hpp"
#include "scan.hpp"
#include "fill.hpp"

namespace lsmgpu {

// Block classes: blocks that fit the group kernel's budget (group_fits) are
// written by encode_group_kernel; the others are listed by the size scan and
// written, by the LDS image they need (e2_need), by 1-wave workgroups with a
// 20 KiB image (medium), by workgroups of kListBigWaves waves with a 96 KiB
// image (big), or straight in HBM (E3, huge).  plan_block (encode_plan.hpp)
// is where a block gets its class.
constexpr uint32_t kPlanHuge = 1, kPlanBad = 2, kPlanMedium = 4, kPlanBig = 8;
constexpr uint32_t kPlanHugeGpu = 16;  // a huge block the whole-GPU E3 path took over (not the one-workgroup E3)
constexpr uint32_t kImgMedium = 20 * 1024;
constexpr uint32_t kImgBig = 96 * 1024;
constexpr uint32_t kListBigWaves = 8;  // waves per listed big block
constexpr uint32_t kE3HashChunk = 4096;    // buckets per LDS pass in E3
constexpr uint64_t kListedOne = 1ULL << 40, kOffMask = kListedOne - 1;

struct alignas(16) BlockPlan {
  uint32_t recs;      // bytes of all records
  uint32_t bin_len;   // restart heads
  uint32_t hash_w;    // buckets written (0 = no hash index in the block)
  uint32_t step_flags;  // step (2|4) | flags << 8
};

__device__ __forceinline__ uint32_t leb_len(uint64_t v) {
  const uint32_t bits = 64 - __builtin_clzll(v | 1);
  return (bits + 6) / 7;
}

// hash_index/builder.rs:39-63: (item_count as f32 * ratio) as u32, at least 1
__device__ __host__ __forceinline__ uint32_t bucket_count(uint64_t n, float ratio) {
  if (!(ratio > 0.0f)) return 0;
  const float prod = (float)n * ratio;
  uint32_t b;
  if (!(prod > 0.0f)) b = 0;
  else if (prod >= 4294967296.0f) b = 0xFFFFFFFFu;
  else b = (uint32_t)prod;
  return b < 1 ? 1 : b;
}

// EncodeParams::diag (lsm_block_params.reserved, a u8): honoured by diagnostic builds only
// (kDiagBuild), 0 in normal use.  The decode path's bits are in decode_common.hpp.
constexpr uint32_t kDiagNoRecordStores = 1;   // group loop: no record is written to the image
constexpr uint32_t kDiagNoHash = 2;           // no payload checksum and no header (group loop, listed blocks)
constexpr uint32_t kDiagNoCopyOut = 4;        // no copy-out of the image (group loop, listed blocks)
constexpr uint32_t kDiagNoRecordsTails = 8;   // group loop: no records, no tails, no checksum
constexpr uint32_t kDiagNoNextDma = 16;       // group loop: the next group's stage DMA is not issued
// The u8 has no unused bit, so two meanings share 0x20: the fused instantiation of the group
// kernel, the only one with a look-back, has no wave-per-block loop, and the others have no look-back.
constexpr uint32_t kDiagLookbackGiveUp = 0x20;  // fused: every run but the first gives up its look-back at
                                                // once (tests/test_gpu_encode_fused.py: the poison path)
constexpr uint32_t kDiagNoWaveBlocks = 0x20;    // the others: every run takes the group loop
constexpr uint32_t kDiagRecPhases = 0x40;     // per-phase cycle totals of encode_huge_records_kernel
constexpr uint32_t kDiagGroupPhases = 0x80;   // per-phase cycle totals of the group loop (lsm_diag_encode_phases)
// any ablation or timer bit of the group loop: such a run stays off the wave-per-block loop
constexpr uint32_t kDiagGroupLoopBits = kDiagNoRecordStores | kDiagNoHash | kDiagNoCopyOut | kDiagNoRecordsTails |
                                        kDiagNoNextDma | kDiagGroupPhases;
static_assert(kDiagGroupLoopBits == 0x9F, "diag bits");

struct EncodeParams {
  lsm_items it;
  const uint32_t* starts;
  uint32_t n_blocks;
  uint32_t ri;
  float ratio;
  uint32_t type;
  uint32_t diag;  // lsm_block_params.reserved: diagnostic ablations (0 in normal use)
  uint32_t plan_bpw;  // blocks per plan workgroup (<= kPlanBlocks), see plan_blocks_per_wg
  uint8_t* out;
  uint64_t out_cap;
  uint64_t* block_off;
  int32_t* status;
  uint64_t* kspan;      // [n_blocks + 1] key_off of each block's first item (E1 -> E2 stage spans)
  uint64_t* vspan;      // [n_blocks + 1] val_off of each block's first item
  uint64_t* sizes;      // [n_blocks] block bytes (E1) -> exclusive scan -> block_off
  BlockPlan* plans;     // [n_blocks]
  uint32_t* lists;      // [n_blocks]: the listed blocks in block order (from the size scan)
  uint32_t* list_count; // [1]
  uint32_t* erec;       // [n_items] E1 -> E2, see kErec*
  uint16_t* hbucket;    // [n_items] E1 -> E2 (hash-index batches, when hb_valid): the key's bucket
                        // in its block (kNoBucket for blocks of >= kNeedHash buckets, never group-class)
  uint32_t hb_valid;
  uint32_t hb_sh;       // hbucket holds every non-head item's shared prefix length (E1p ran)
  uint32_t* hb_fix;     // [1] set by E1 when it left keys of more than 16 bytes (kNeedHash)
  unsigned long long* phase;  // diagnostic builds: per-phase cycle totals [16]
  uint32_t* pfirst;     // [n_blocks + 1] E1p: each block's first record prefix (low 32 bits); [n_blocks] the total
  uint32_t* e1p_flag;   // [1] E1p: the item_start array is not monotone
  uint64_t* wpart;      // [2 per wave of items] E1p: record totals of the blocks crossing a wave's ends
  uint8_t* huge_pool;   // workspace past encode_workspace_size (null: E3 one workgroup per block)
  uint64_t huge_pool_bytes;
  uint32_t huge_cap;    // huge-list entries the pool's layout provides
  uint32_t off32;       // it.key_off / it.val_off hold u32 offsets (lsm_encode_blocks32, lsm_items32)
};

__device__ __forceinline__ bool is_index(const EncodeParams& P) { return P.type == 1; }

// Key / value offset i: u64 arrays (lsm_items) or u32 arrays (lsm_items32: SURVEY 8(d)'s 4 + 4 B
// per item, arenas < 4 GiB).  kOW: the width in bytes when the kernel is instantiated for one
// (the hot plan and group kernels: straight-line loads), 0 = the batch-wide P.off32 at run time
// (a scalar branch per load site: the cold kernels).
template <int kOW = 0>
__device__ __forceinline__ bool off_w32(const EncodeParams& P) {
  return kOW == 4 || (kOW == 0 && P.off32);
}
template <int kOW = 0>
__device__ __forceinline__ uint64_t off_at(const EncodeParams& P, const uint64_t* a, uint64_t i) {
  return off_w32<kOW>(P) ? (uint64_t)gload(reinterpret_cast<const uint32_t*>(a), i) : gload(a, i);
}
template <int kOW = 0>
__device__ __forceinline__ uint64_t koff(const EncodeParams& P, uint64_t i) { return off_at<kOW>(P, P.it.key_off, i); }
template <int kOW = 0>
__device__ __forceinline__ uint64_t voff(const EncodeParams& P, uint64_t i) { return off_at<kOW>(P, P.it.val_off, i); }
// offset base + t with a wave-uniform base (SGPR pointer) and a per-lane t < 2^29 (32-bit byte offsets)
template <int kOW = 0>
__device__ __forceinline__ uint64_t off_rel(const EncodeParams& P, const uint64_t* a, uint64_t base, uint32_t t) {
  if (off_w32<kOW>(P))
    return *reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(reinterpret_cast<const uint32_t*>(a) + base) + 4u * t);
  return *reinterpret_cast<const uint64_t*>(reinterpret_cast<const uint8_t*>(a + base) + 8u * t);
}

// d_block_item_start[i] as E1 walks it: clamped to n_items, so no item field
// past the arenas is read (the reference takes &[InternalValue],
// data_block/mod.rs:523-549, so its block ranges are in bounds by type; the
// C ABI checks).  A block whose end is past n_items is rejected (ST_BAD_ARG).
__device__ __forceinline__ uint32_t clamped_start(const EncodeParams& P, uint32_t i) {
  const uint32_t v = P.starts[i];
  return (uint64_t)v > P.it.n_items ? (uint32_t)P.it.n_items : v;
}
__device__ __forceinline__ bool start_past_items(const EncodeParams& P, uint32_t i) {
  return (uint64_t)P.starts[i] > P.it.n_items;
}

// ------------------------------------------------------ E2: LDS write pass
// Wave-local ordering of LDS traffic between lanes (no workgroup barrier:
// the waves of a workgroup write independent blocks).
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
}

// One item's fields, loaded once per lane (all loads independent).
struct ItemMeta {
  uint64_t ko, vo, seq;
  uint32_t klen, vl, vt, sh;
  uint32_t e;   // E2 only: the plan's erec word
  uint32_t hb;  // E2 only: the plan's hash bucket (kNoBucket: none)
};
constexpr uint32_t kNoBucket = 0xFFFF;

constexpr uint32_t kNeedHash = 0xFFFE;  // E1 left this key (> 16 bytes) to encode_bucket_fixup_kernel

// An item's fields exactly as loaded (E2's one-group-ahead prefetch).  The
// offsets keep the width they were loaded with (RawItemT<4>: u32), so nothing
// widens them before cook_item consumes them: a zero-extension at the load
// made the compiler wait for the prefetched loads right there (the u32 group
// kernel ran 5 % slower with u64 fields here).
template <int kOW = 0, bool kIdx = false>
struct RawItemT {
  typedef typename std::conditional<kOW == 4, uint32_t, uint64_t>::type off_t;
  typedef typename std::conditional<kOW == 4 && !kIdx, uint32_t, uint64_t>::type voff_t;  // (index: handle offset)
  off_t ko, ko1;
  voff_t vo, vo1;  // (vo1: the index handle size for index blocks)
  uint64_t seq;
  uint32_t vt, e, hb;
};
typedef RawItemT<0> RawItem;

// Plain loads of item i's fields (no arithmetic, so no wait is forced here).
template <bool kIndex, int kOW = 0>
__device__ __forceinline__ RawItemT<kOW, kIndex> load_raw(const EncodeParams& P, uint64_t i) {
  RawItemT<kOW, kIndex> r;
  if (kOW == 4) {
    r.ko = gload(reinterpret_cast<const uint32_t*>(P.it.key_off), i);
    r.ko1 = gload(reinterpret_cast<const uint32_t*>(P.it.key_off), i + 1);
  } else {
    r.ko = koff<kOW>(P, i);
    r.ko1 = koff<kOW>(P, i + 1);
  }
  r.seq = P.it.seqno[i];
  r.e = 0;
  r.hb = kNoBucket;
  if (kIndex) {
    r.vo = P.it.handle_off[i];
    r.vo1 = P.it.handle_size[i];
    r.vt = 0;
  } else {
    if (kOW == 4) {
      r.vo = gload(reinterpret_cast<const uint32_t*>(P.it.val_off), i);
      r.vo1 = gload(reinterpret_cast<const uint32_t*>(P.it.val_off), i + 1);
    } else {
      r.vo = voff<kOW>(P, i);
      r.vo1 = voff<kOW>(P, i + 1);
    }
    r.vt = P.it.vtype[i];
  }
  return r;
}

// The same from a wave-uniform base item and a per-lane offset t < 2^29:
// base pointers in SGPRs and 32-bit byte offsets (one VGPR per address).
template <bool kIndex>
__device__ __forceinline__ RawItem load_raw_rel(const EncodeParams& P, uint64_t base, uint32_t t) {
  auto at64 = [&](const uint64_t* a, uint32_t k) {
    return *reinterpret_cast<const uint64_t*>(reinterpret_cast<const uint8_t*>(a + base) + 8u * k);
  };
  RawItem r;
  r.ko = off_rel(P, P.it.key_off, base, t);
  r.ko1 = off_rel(P, P.it.key_off, base, t + 1);
  r.seq = at64(P.it.seqno, t);
  r.e = 0;
  r.hb = kNoBucket;
  if (kIndex) {
    r.vo = at64(P.it.handle_off, t);
    r.vo1 = (P.it.handle_size + base)[t];
    r.vt = 0;
  } else {
    r.vo = off_rel(P, P.it.val_off, base, t);
    r.vo1 = off_rel(P, P.it.val_off, base, t + 1);
    r.vt = (P.it.vtype + base)[t];
  }
  return r;
}

// Derived fields of a raw item and the writer's argument checks (key length
// <= u16, a known value type, value length <= u32).
template <bool kIndex, class R>
__device__ __forceinline__ ItemMeta cook_item(const R& r, bool& bad) {
  ItemMeta m;
  const uint64_t kl = (uint64_t)r.ko1 - (uint64_t)r.ko;  // (widened first: a decreasing pair is bad at any width)
  if (kl > 0xFFFF) bad = true;
  m.ko = r.ko;
  m.klen = (uint32_t)min(kl, (uint64_t)0xFFFF);
  m.seq = r.seq;
  m.vo = r.vo;
  m.vt = r.vt;
  m.sh = 0;
  m.e = r.e;
  m.hb = r.hb;
  if (kIndex) {
    m.vl = (uint32_t)r.vo1;
  } else {
    const uint64_t vl = (uint64_t)r.vo1 - (uint64_t)r.vo;
    if (!valid_vtype(m.vt)) bad = true;
    if (!is_tombstone(m.vt) && vl > 0xFFFFFFFFULL) bad = true;
    m.vl = (uint32_t)vl;
  }
  return m;
}

__device__ __forceinline__ uint32_t head_len(const EncodeParams& P, const ItemMeta& m, bool head) {
  if (is_index(P)) return 1 + leb_len(m.vo) + leb_len(m.vl) + leb_len(m.seq) + leb_len(m.klen);
  return 1 + leb_len(m.seq) + (head ? leb_len(m.klen) : leb_len(m.sh) + leb_len(m.klen - m.sh));
}

__device__ __forceinline__ uint64_t item_record_len(const EncodeParams& P, const ItemMeta& m, bool head) {
  uint64_t rec = head_len(P, m, head) + m.klen - (head ? 0 : m.sh);
  if (!is_index(P) && !is_tombstone(m.vt)) rec += leb_len(m.vl) + (uint64_t)m.vl;
  return rec;
}

// Byte stores of a LEB128 (varint-rs write_*_varint) / single bytes.
template <class D>
__device__ __forceinline__ uint32_t put_leb(D* dst, uint32_t pos, uint64_t v) {
  while (v >= 0x80) {
    dst[pos++] = (uint8_t)(v | 0x80);
    v >>= 7;
  }
  dst[pos++] = (uint8_t)v;
  return pos;
}

template <class D>
__device__ __forceinline__ void store_le(D* dst, uint32_t pos, uint64_t v, uint32_t n) {
  for (uint32_t k = 0; k < n; ++k) dst[pos + k] = (uint8_t)(v >> (8 * k));
}

// Hash-index bucket of a key (hash_index/mod.rs:35-41), key bytes from HBM.
__device__ __forceinline__ uint32_t key_bucket(const EncodeParams& P, uint64_t ko, uint32_t klen, uint32_t buckets) {
  const uint64_t ka = (uint64_t)(uintptr_t)P.it.keys + ko;
  const uint8_t* kb = reinterpret_cast<const uint8_t*>(ka & ~15ULL);
  const uint32_t kq = (uint32_t)(ka & 15);
  const uint64_t h = xxh3_64_any(klen, BaseReader8{kb, kq}, BaseReader64{kb, kq});
  return (uint32_t)(h % buckets);
}

// Marker, binary index entries are written by the record loop; this writes
// the hash-index bytes (given final min/max per bucket) and the trailer.
__device__ __forceinline__ uint32_t bucket_byte(uint32_t lo, uint32_t hi) {
  return lo == 0xFFFFFFFFu ? kHashFree : (lo == hi ? lo : kHashConflict);
}

__device__ __forceinline__ void write_trailer_bytes(uint8_t* dst, uint32_t tp, uint32_t ri, uint32_t step,
                                                    uint32_t bin_len, uint32_t bin_off, uint32_t hash_w,
                                                    uint32_t hash_off, uint32_t items) {
  // trailer.rs:118-163, lanes 0..30 write one byte each
  const int lane = threadIdx.x & 63;
  if (lane >= (int)kTrailerLen) return;
  uint32_t v;
  const int k = lane;
  if (k == 0) v = ri;
  else if (k == 1) v = step;
  else if (k < 6) v = bin_len >> (8 * (k - 2));
  else if (k < 10) v = bin_off >> (8 * (k - 6));
  else if (k < 14) v = hash_w >> (8 * (k - 10));
  else if (k < 18) v = hash_off >> (8 * (k - 14));
  else if (k == 18) v = 1;       // prefix truncation on
  else if (k < 27) v = 0;        // fixed key/value size (unused)
  else v = items >> (8 * (k - 27));
  dst[tp + k] = (uint8_t)v;
}

// Header::encode_into (header.rs:80-112): lanes 0..32 write one byte each.
__device__ __forceinline__ void write_header_bytes(uint8_t* dst, uint32_t hp, uint32_t type, uint64_t ck_lo,
                                                   uint64_t ck_hi, uint32_t plen) {
  uint64_t w0 = 0x034D534CULL | ((uint64_t)type << 32) | (ck_lo << 40);
  uint64_t w1 = (ck_lo >> 24) | (ck_hi << 40);
  uint64_t w2 = (ck_hi >> 24) | ((uint64_t)plen << 40);
  uint64_t w3 = ((uint64_t)plen >> 24) | ((uint64_t)plen << 8);
  auto r64 = [&](uint32_t o) -> uint64_t {  // LE u64 at byte o of w0..w3 (o <= 24)
    const uint32_t q = o >> 3, sft = (o & 7) * 8;
    const uint64_t a = q == 0 ? w0 : q == 1 ? w1 : q == 2 ? w2 : w3;
    const uint64_t b = q == 0 ? w1 : q == 1 ? w2 : q == 2 ? w3 : 0;
    return sft ? (a >> sft) | (b << (64 - sft)) : a;
  };
  auto r8 = [&](uint32_t o) -> uint32_t { return (uint32_t)(r64(o) & 0xFF); };
  uint64_t hlo, hhi;
  xxh3_128_short(29, r8, r64, hlo, hhi);
  const int lane = threadIdx.x & 63;
  if (lane < 29) dst[hp + lane] = (uint8_t)r8(lane);
  else if (lane < 33) dst[hp + lane] = (uint8_t)((uint32_t)hlo >> (8 * (lane - 29)));
}

// The same header written by a lane quad (lane q of the quad: bytes
// [8q, 8q + 8), lane 0 also byte 32), every lane computing the 29-byte
// checksum itself.  BytePtr: uint8_t* (an LDS image, or any memory) or a global-
// address-space byte pointer (the wave-per-block loop's deferred headers, which
// go straight to the output).
template <class BytePtr>
__device__ __forceinline__ void write_header_quad(BytePtr dst, uint32_t hp, uint32_t type, uint64_t ck_lo,
                                                  uint64_t ck_hi, uint32_t plen, int q) {
  const uint64_t w0 = 0x034D534CULL | ((uint64_t)type << 32) | (ck_lo << 40);
  const uint64_t w1 = (ck_lo >> 24) | (ck_hi << 40);
  const uint64_t w2 = (ck_hi >> 24) | ((uint64_t)plen << 40);
  const uint64_t w3 = ((uint64_t)plen >> 24) | ((uint64_t)plen << 8);
  auto r64 = [&](uint32_t o) -> uint64_t {  // LE u64 at byte o of w0..w3 (o <= 24)
    const uint32_t qq = o >> 3, sft = (o & 7) * 8;
    const uint64_t a = qq == 0 ? w0 : qq == 1 ? w1 : qq == 2 ? w2 : w3;
    const uint64_t b = qq == 0 ? w1 : qq == 1 ? w2 : qq == 2 ? w3 : 0;
    return sft ? (a >> sft) | (b << (64 - sft)) : a;
  };
  auto r8 = [&](uint32_t o) -> uint32_t { return (uint32_t)(r64(o) & 0xFF); };
  uint64_t hlo, hhi;
  xxh3_128_short(29, r8, r64, hlo, hhi);
  // bytes 29..32: the low 4 bytes of the header checksum
  const uint64_t w = q == 0 ? w0 : q == 1 ? w1 : q == 2 ? w2 : (w3 & 0xFFFFFFFFFFULL) | (hlo << 40);
  const uint32_t at = hp + 8 * q;
#pragma unroll
  for (uint32_t i = 0; i < 8; ++i) dst[at + i] = (uint8_t)(w >> (8 * i));
  if (q == 0) dst[hp + 32] = (uint8_t)(hlo >> 24);
}

// Per-item word from E1 to E2 (read for group-class blocks, whose payload is
// < 32 KiB and whose items are < 2^16): bits 0-14 the record's offset in the
// block payload, bit 15 restart head, bits 16-31 the restart index (heads)
// or the shared-prefix length (keys are < 2^16 bytes).
constexpr uint32_t kErecHead = 0x8000u;

// Group write kernel (E2) budget, see encode_group_kernel.
constexpr uint32_t kGWaves = 4, kGThreads = kGWaves * kWave;
constexpr uint32_t kGRun = 32;          // blocks per workgroup (<= 63: one lane each)
constexpr uint32_t kGRunFused = 32;  // the same with the fused run-level plan (48 / 63: r06_experiments ab6h)
constexpr uint64_t kFusedAutoItems = 128;  // items per block from which the fused plan is taken
static_assert(kGRunFused <= 63, "one lane per block and one for the run's end");
constexpr uint32_t kGBlocks = 16;    // blocks per group
constexpr uint32_t kGItems = kGThreads;        // items per group (one thread each)
constexpr uint32_t kGSlack = 48;               // readable bytes past each staged span
// group LDS budget (four configs[1] blocks by default)
constexpr uint32_t kGKeys = 4096, kGVals = 14400, kGImg = 15872;
constexpr uint32_t kGUnits = kGImg / 1024 + kGBlocks + 1;  // hash units per group
constexpr uint32_t kGUnion = 4096;      // hash votes | hash contributions
constexpr uint32_t kGHash = kGUnion / 8;       // vote pairs
static_assert(kGUnits * 64 <= kGUnion, "hash contributions");
static_assert((kGUnits + 4) * 64 <= kGUnion, "the chain's batched reads stay inside L.uni");


__device__ __host__ __forceinline__ bool group_fits(uint64_t n, uint64_t kspan, uint64_t vspan, uint64_t total,
                                                    uint32_t hash_w) {
  return n <= kGItems && kspan + 15 <= kGKeys && vspan + 15 <= kGVals && total + 15 <= kGImg && hash_w <= kGHash;
}

// blocks per workgroup: longer-lived workgroups (16 -> 128: 0.80 -> 0.68 ms per 1 M blocks)
constexpr uint32_t kPlanBlocks = 128;
static_assert(kPlanBlocks <= 255, "thread nb loads the run's end: nb < 256 threads");
constexpr uint32_t kE1pMaxBpw = 4;  // E1p for batches of >= 4 Ki items per block on average

// ------------------------------------------- the whole-GPU E3's pool (encode_large.hip)
// The huge-block pool header's collected-block count (EncHugeHdr::count), as a u32 index.
constexpr uint32_t kEncHugeCountWord = 2;

struct EncHuge {
  uint64_t dst_off;
  uint64_t acc[8];
  uint32_t b, s, n, total;
  uint32_t nbk, nru, accepted, done;
  uint32_t ipu, pad;  // items per record unit
};
static_assert(sizeof(EncHuge) % 16 == 0, "EncHuge layout");
struct EncHugeHdr {
  uint64_t total_kib;
  uint32_t count;      // collected (atomic; may exceed the capacity: the rest stay with the one-workgroup E3)
  uint32_t n3;         // planned entries
  uint64_t total_units;
};
static_assert(offsetof(EncHugeHdr, count) == 4 * kEncHugeCountWord, "E1p clears the count by index");
// Pool: [hdr | 256][list u32 x cap][kpre u64 x (cap + 1)][upre u64 x (cap + 1)][EncHuge x cap]
// [contributions, 64 B per KiB block][done flags, 1 B per KiB block]
struct EncHugeLayout {
  EncHugeHdr* hdr;
  uint32_t* list;
  uint64_t* kpre;
  uint64_t* upre;
  EncHuge* rec;
  uint64_t* contrib;
  uint8_t* kdone;  // KiB block's contribution computed by the records kernel (from its LDS image)
  uint64_t cap_kib;
};
__host__ __device__ __forceinline__ uint64_t enc_huge_fixed_bytes(uint64_t cap) {
  return (256 + ((4 * cap + 15) & ~15ULL) + 16 * (cap + 1) + sizeof(EncHuge) * cap + 255) & ~255ULL;
}
// The pool at b (pool_bytes bytes, cap huge-list entries).  The host takes the addresses the size
// scan writes from it (hdr->count, list); the kernels take all of it.
__host__ __device__ __forceinline__ EncHugeLayout enc_huge_layout(uint8_t* b, uint64_t pool_bytes, uint64_t cap) {
  EncHugeLayout L;
  L.hdr = reinterpret_cast<EncHugeHdr*>(b);
  L.list = reinterpret_cast<uint32_t*>(b + 256);
  L.kpre = reinterpret_cast<uint64_t*>(b + 256 + ((4 * cap + 15) & ~15ULL));
  L.upre = L.kpre + (cap + 1);
  L.rec = reinterpret_cast<EncHuge*>(L.upre + (cap + 1));
  const uint64_t fixed = enc_huge_fixed_bytes(cap);
  L.contrib = reinterpret_cast<uint64_t*>(b + fixed);
  L.cap_kib = (pool_bytes - fixed) / 65;
  L.kdone = reinterpret_cast<uint8_t*>(L.contrib + 8 * L.cap_kib);
  return L;
}
__host__ __device__ __forceinline__ EncHugeLayout enc_huge_layout(const EncodeParams& P) {
  return enc_huge_layout(P.huge_pool, P.huge_pool_bytes, P.huge_cap);
}

// ------------------------------------------------------------ host: the workspace
// The regions of the caller's workspace for a batch of n_items items in n_blocks blocks, each
// 256-byte aligned: byte offsets from the workspace's start, in layout order, and their sum.
// encode_workspace_size() returns `total` and launch_encode() takes every pointer from here.
struct EncodeWorkspace {
  size_t kspan, vspan;  // u64 [n_blocks + 1] each
  size_t sizes;         // u64 [n_blocks]
  size_t plans;         // BlockPlan [n_blocks]
  size_t lists;         // u32 [n_blocks]
  size_t counts;        // one cell: u32 list_count, u32 e1p_flag
  size_t tiles;         // u64 scan tile sums (the size scan over blocks, E1p's over items)
  size_t erec;          // u32 [n_items]
  size_t hbucket;       // u16 [n_items]
  size_t hb_fix;        // one cell: u32
  size_t pfirst;        // u32 [n_blocks + 1]
  size_t wpart;         // u64 [2 per wave of items]
  size_t total;
  EncodeWorkspace(uint64_t n_items, uint32_t n_blocks) {
    Carver c;
    const size_t nb = n_blocks, ni = (size_t)n_items;
    kspan = c.take((nb + 1) * 8);
    vspan = c.take((nb + 1) * 8);
    sizes = c.take(nb * 8);
    plans = c.take(nb * sizeof(BlockPlan));
    lists = c.take(nb * 4);
    counts = c.take(256);
    tiles = c.take(std::max<uint64_t>(scan_tiles(n_blocks), scan_tiles(std::max<uint64_t>(n_items, 1))) * 8);
    erec = c.take(ni * 4);
    hbucket = c.take(ni * 2);
    hb_fix = c.take(256);
    pfirst = c.take((nb + 1) * 4);
    wpart = c.take((ni / 64 + 1) * 16);
    total = c.total();
  }
  // where the whole-GPU E3's pool starts in a workspace that carries one (lsm_encode_workspace_size_ex)
  size_t pool_base() const { return round256(total); }
};

// ------------------------------------------------------- host: the stage launchers
// Each launches its stage's kernels on st, in order; launch_encode (encode.hip) calls them.
// Calls f(std::integral_constant<int, W>()) with W the batch's offset width in bytes, 4 or 8:
// the launchers name a kernel that is instantiated per width once, as K<..., decltype(w)::value>.
template <class F>
inline auto by_offset_width(const EncodeParams& P, F&& f) {
  return P.off32 ? f(std::integral_constant<int, 4>()) : f(std::integral_constant<int, 8>());
}
// (the plan stage's kernel that is defined in encode_large.hip: see there)
__global__ __launch_bounds__(256) void encode_bucket_fixup_kernel(EncodeParams P);
// E1 / E1p and the size scan (not the scan with the fused plan).  Sets P.hb_valid and P.hb_sh.
hipError_t launch_encode_plan(EncodeParams& P, bool e1p, bool fused, uint64_t* tiles, hipStream_t st);
// E2
void launch_encode_group(const EncodeParams& P, bool fused, hipStream_t st);
// the listed blocks: medium, big, and the huge ones (across the GPU with the pool, the rest one workgroup each)
hipError_t launch_encode_large(const EncodeParams& P, hipStream_t st);

}  // namespace lsmgpu
