// decode_common.hpp — what more than one stage of the decode path uses (decode.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "block_format.hpp"
#include "decode.hpp"
#include "host_common.hpp"
#include "lds_dma.hpp"

namespace lsmgpu {

// Diagnostic-only flags (lsm_decode_tuning.flags high bits, honoured only by
// -DLSM_DIAG builds; the release library rejects them with LSM_BAD_ARG): drop
// one phase to price it in a profile.  Outputs are NOT valid with them set.
constexpr uint32_t kDiagSkipHash = 0x100, kDiagSkipParse = 0x200, kDiagSkipStore = 0x400, kDiagSkipPhaseB = 0x800;
// (group kernel, stage-only profiling: outputs and statuses invalid) no header / trailer wave; no stage DMA
constexpr uint32_t kDiagSkipHeader = 0x1000, kDiagSkipDma = 0x2000;
// (huge-block pool, streamed chains) every chain wave gives up its first wait at once, as the
// 5 ms no-progress guard would; the fallback chain pass is skipped (LSM_INCOMPLETE stays)
constexpr uint32_t kDiagStreamGiveUp = 0x4000, kDiagNoChainFallback = 0x8000;
static_assert(kDecodeDiagMask == (kDiagSkipHash | kDiagSkipParse | kDiagSkipStore | kDiagSkipPhaseB | kDiagSkipHeader |
                                  kDiagSkipDma | kDiagStreamGiveUp | kDiagNoChainFallback),
              "the bits the ABI lets through");

// (16 blocks x 80 B of block metadata: the LDS this frees lets the stage hold
// two 17 KB blocks of the 16 KiB random-key class, or nine 4 KiB blocks,
// inside the 40 KiB that keeps four workgroups per CU)
constexpr uint32_t kMaxGroup = 16;  // blocks per staged group
// Internal status: the block needs the general path (index block, a record
// shape the straight-line parsers do not take, a block larger than the
// stage).  The group kernel lists it for decode_big_kernel, which hands on
// what it cannot take (index blocks, rare shapes, blocks beyond its stage) to
// decode_deferred_staged_kernel, the general path with the LEB cursor; that
// one writes the final status.
constexpr int32_t ST_DEFER = 0x7F;
constexpr uint32_t kStagePad = 256;  // readable LDS bytes past the span (fast parsers read <= 138)

// Record descriptor (one u64 per group item, LDS), written by phase A, read
// by phase B: image offsets of the record start, of where it must end (the
// next record's start, or the interval's end for its last record) and of its
// restart head's key; [48,53) group block, 53 restart head, 54 valid,
// [55,58) seqno bytes and [58,60) shared bytes of a header shape phase A has
// verified (0 = not verified: phase B decodes the header itself).
// Two layouts: kWide = false for stages < 64 KiB (16-bit image offsets),
// kWide = true for the big-block kernel's stage (17-bit offsets; the end is
// kept as its distance from the start, clamped to 2^15 - 1: longer than any
// record the straight-line parsers take, so a clamped end can only mismatch).
template <bool kWide>
struct RecLayout {
  static constexpr int kPosBits = kWide ? 17 : 16;
  static constexpr uint32_t kPosMask = (1u << kPosBits) - 1;
  static constexpr int kKeyShift = 32, kBlockShift = 32 + kPosBits;
  static constexpr uint64_t kRestart = 1ULL << (kBlockShift + 5), kValid = 1ULL << (kBlockShift + 6);
  static constexpr int kN1Shift = kBlockShift + 7, kN2Shift = kBlockShift + 10;
  __device__ static __forceinline__ uint32_t lo(uint32_t a, uint32_t end) {
    return kWide ? a | (min(end - a, 0x7FFFu) << 17) : a | (end << 16);
  }
  __device__ static __forceinline__ uint32_t start(uint64_t d) { return (uint32_t)d & kPosMask; }
  __device__ static __forceinline__ uint32_t end(uint64_t d) {
    return kWide ? ((uint32_t)d & kPosMask) + (((uint32_t)d >> 17) & 0x7FFF) : (uint32_t)d >> 16;
  }
};
static_assert(RecLayout<true>::kN2Shift + 2 <= 64 && RecLayout<false>::kN2Shift + 2 <= 64, "descriptor bits");

struct alignas(16) BlockMeta {
  // first 16 bytes: what phase B needs per record (one ds_read_b128)
  uint32_t p0;        // image / span offset of the payload (header offset + 33)
  uint32_t rec_end;   // image / span offset of the 0xFF trailer marker
  int32_t st;         // lsm_status
  uint32_t type;
  uint64_t ck_lo, ck_hi;
  uint32_t hb;        // byte offset of the header in the image / span
  uint32_t len;       // handle size (header + payload)
  uint32_t ri, step, bin_len, bin_off, item_count;
  uint32_t item0;     // first output index relative to the group base
  uint32_t chain0;    // exclusive prefix of restart intervals in the group
  int32_t hdr_st;     // header-level status before the header checksum (gates hashing)
  uint16_t ck_bad;    // payload checksum mismatch
  uint16_t hck_bad;   // header checksum mismatch
};
static_assert(sizeof(BlockMeta) == 80, "BlockMeta layout");

// The kernel's DecodeParams in the kernarg segment.  Out-of-line helpers take
// this pointer: taking the address of the by-value kernel parameter instead
// makes the compiler copy it to scratch and reload its fields from there
// (vmcnt waits in the hot loops).
typedef const __attribute__((address_space(4))) DecodeParams* KArgs;
__device__ __forceinline__ KArgs kargs() { return (KArgs)__builtin_amdgcn_kernarg_segment_ptr(); }
__device__ __forceinline__ DecodeParams load_params(KArgs Pk) {
  DecodeParams P;
  __builtin_memcpy(&P, (const void*)Pk, sizeof(P));
  return P;
}

__device__ __forceinline__ void wave_sync() {
  // Single-wave workgroups: LDS operations of a wave complete in order, so a
  // compiler barrier is all cross-lane LDS hand-offs need (no s_barrier, and
  // no vmcnt(0) drain of the output stores as __syncthreads would imply).
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Workgroup barrier for LDS hand-offs only: waits for this wave's LDS ops
// (lgkmcnt), not for its global stores, which __syncthreads' release fence
// would drain (vmcnt(0)) before every phase.
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// compact (lsm_decode_blocks16): key_off / val_off / val_len are uint16_t
// arrays; every block that reaches a store has a payload <= 65535 bytes
// (meta_trailer), so the payload-relative values fit.
__device__ __forceinline__ void emit_global(const lsm_parsed_items& o, uint64_t i, const ItemFields& f,
                                            uint64_t seqno_add, bool compact) {
  if (o.seqno) gstore(o.seqno, i, f.seqno + seqno_add);
  if (compact) {
    if (o.key_off) gstore(reinterpret_cast<uint16_t*>(o.key_off), i, (uint16_t)f.key_off);
    if (o.val_off) gstore(reinterpret_cast<uint16_t*>(o.val_off), i, (uint16_t)f.val_off);
    if (o.val_len) gstore(reinterpret_cast<uint16_t*>(o.val_len), i, (uint16_t)f.val_len);
  } else {
    if (o.key_off) gstore(o.key_off, i, f.key_off);
    if (o.val_off) gstore(o.val_off, i, f.val_off);
    if (o.val_len) gstore(o.val_len, i, f.val_len);
  }
  if (o.key_len) gstore(o.key_len, i, f.key_len);
  if (o.prefix_len) gstore(o.prefix_len, i, f.prefix_len);
  if (o.vtype) gstore(o.vtype, i, f.vtype);
  if (o.handle_off) gstore(o.handle_off, i, f.handle_off);
}

// Lane-level: header checks in oracle order (header.rs:116-169).
__device__ __forceinline__ void meta_header(const uint8_t* base, uint32_t hb, uint64_t len, BlockMeta& m) {
  HeaderInfo h;
  m.hb = hb;
  m.p0 = hb + kHdrLen;
  m.rec_end = 0;
  m.len = (uint32_t)len;
  m.st = (len > 0xFFFFFF00ULL) ? ST_TRUNCATED : check_header(base, hb, len, h);
  m.ck_lo = h.ck_lo;
  m.ck_hi = h.ck_hi;
  m.type = h.type;
  m.item_count = h.data_length;  // stash data_length until meta_trailer
  m.chain0 = 0;
}

// Staged kernel: the same without the header checksum (the hash waves check it).
__device__ __forceinline__ void meta_header_fields(const uint8_t* base, uint32_t hb, uint64_t len, BlockMeta& m) {
  HeaderInfo h;
  m.hb = hb;
  m.p0 = hb + kHdrLen;
  m.rec_end = 0;
  m.len = (uint32_t)len;
  m.st = (len > 0xFFFFFF00ULL) ? ST_TRUNCATED : check_header_fields(base, hb, len, h);
  m.ck_lo = h.ck_lo;
  m.ck_hi = h.ck_hi;
  m.type = h.type;
  m.item_count = h.data_length;  // stash data_length until meta_trailer
  m.chain0 = 0;
}

// After the payload checksum: data_length, expected type, trailer structure.
// compact output (lsm_decode_blocks16): index blocks (u64 handle offsets) and
// payloads over 65535 bytes cannot be stored in 16 bits: LSM_UNSUPPORTED,
// decided here, after every header check and before the trailer is read.
__device__ __forceinline__ void meta_trailer(const uint8_t* base, int32_t expect_type, uint32_t cap, BlockMeta& m,
                                             bool compact, const uint8_t* mbase = nullptr) {
  if (m.st != ST_OK) return;
  const uint32_t plen = m.len - kHdrLen;
  if (m.item_count != plen) { m.st = ST_TRUNCATED; return; }   // data_length vs handle
  if (expect_type >= 0 && (int32_t)m.type != expect_type) { m.st = ST_TYPE_MISMATCH; return; }
  if (m.type == 2) { m.st = ST_UNSUPPORTED; return; }          // filter blocks are not KV blocks
  if (compact && (m.type == 1 || plen > 0xFFFFu)) { m.st = ST_UNSUPPORTED; return; }
  TrailerInfo t;
  int32_t st = read_trailer(base, m.hb + kHdrLen, plen, t, mbase);
  if (st == ST_OK && m.type == 1 && t.ri != 1) st = ST_PARSE;   // index blocks: restart interval 1
  if (st == ST_OK && t.item_count > cap) st = ST_OVERFLOW;
  m.st = st;
  if (st != ST_OK) return;
  m.ri = t.ri; m.step = t.step; m.bin_len = t.bin_len; m.bin_off = t.bin_off;
  m.item_count = t.item_count; m.rec_end = m.p0 + t.rec_end;
}

__device__ __forceinline__ TrailerInfo trailer_of(const BlockMeta& m) {
  TrailerInfo t;
  t.ri = m.ri; t.step = m.step; t.bin_len = m.bin_len; t.bin_off = m.bin_off;
  t.item_count = m.item_count; t.rec_end = m.rec_end - m.p0;
  t.hash_len = 0; t.hash_off = 0;
  return t;
}

// Rare record shapes (long varints) through the general LEB cursor; kept out
// of line so the hot loops stay small in the instruction cache.
__device__ __noinline__ bool parse_data_slow(const uint8_t* base, uint32_t p0, uint32_t pos, uint32_t end,
                                             bool restart, uint32_t base_key, ItemFields* f, uint32_t* next) {
  Cursor c;
  c.init(base, p0, pos, end);
  if (!parse_data_record(c, restart, base_key, *f)) return false;
  *next = c.pos;
  return true;
}
__device__ __noinline__ bool parse_index_slow(const uint8_t* base, uint32_t p0, uint32_t pos, uint32_t end,
                                              ItemFields* f, uint32_t* next) {
  Cursor c;
  c.init(base, p0, pos, end);
  if (!parse_index_record(c, *f)) return false;
  *next = c.pos;
  return true;
}

// Full parse of one record at pos; returns next position or false.
__device__ __forceinline__ bool parse_record(const uint8_t* base, uint32_t p0, uint32_t pos, const TrailerInfo& t,
                                             uint32_t type, bool restart, uint32_t base_key, ItemFields& f,
                                             uint32_t& next) {
  ItemFields tmp;  // only the out-of-line paths take an address (keeps f in registers)
  uint32_t tnext;
  bool ok;
  if (type == 1) {
    ok = parse_index_slow(base, p0, pos, t.rec_end, &tmp, &tnext);
  } else {
    const int rc = parse_data_fast(base, p0, pos, t.rec_end, restart, base_key, f, next);
    if (rc > 0) return true;
    if (rc < 0) return false;
    ok = parse_data_slow(base, p0, pos, t.rec_end, restart, base_key, &tmp, &tnext);
  }
  f = tmp;
  next = tnext;
  return ok;
}

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
  return v;
}

template <class RL>
__device__ __forceinline__ uint64_t rec_desc(uint32_t a, uint32_t end, uint32_t key, uint64_t tag) {
  return (uint64_t)RL::lo(a, end) | ((uint64_t)key << RL::kKeyShift) | tag;
}

// Predicted header shape of a non-restart record: n1 seqno bytes, n2 shared
// bytes, 1 key-length byte.  msk = MSB bits of header bytes 1..hdr-1, pat =
// where their LEB terminators must be; a record matches iff (~h & msk) == pat.
struct Shape {
  uint32_t hdr, kshift;
  uint64_t msk, pat;
  uint64_t bits;  // descriptor shape bits
};
template <class RL>
__device__ __forceinline__ Shape make_shape(uint32_t n1, uint32_t n2) {
  Shape s;
  s.bits = ((uint64_t)n1 << RL::kN1Shift) | ((uint64_t)n2 << RL::kN2Shift);
  s.hdr = n1 + n2 + 2;  // <= 8
  s.kshift = 8 * (s.hdr - 1);
  s.msk = 0x8080808080808000ULL & (s.hdr >= 8 ? ~0ULL : ((1ULL << (8 * s.hdr)) - 1));
  s.pat = (0x80ULL << (8 * n1)) | (0x80ULL << (8 * (n1 + n2))) | (0x80ULL << (8 * (s.hdr - 1)));
  return s;
}

// Value length from the two bytes z after the key; ok = 1-2 byte varint.
__device__ __forceinline__ void rec_value(uint32_t vt, uint32_t z, uint32_t& n4, uint32_t& vl, bool& ok) {
  const bool tomb = vt - 1u < 2u;
  const bool two = (z & 0x80) != 0;
  ok = tomb || (z & 0x8080) != 0x8080;
  n4 = tomb ? 0 : (two ? 2 : 1);
  vl = tomb ? 0 : (two ? ((z & 0x7F) | ((z >> 1) & 0x3F80)) : (z & 0x7F));
}

// Record length from the key length and the two bytes z after the key
// (1-2 byte value length; tombstones carry none).
__device__ __forceinline__ uint32_t rec_len(uint32_t vt, uint32_t q, uint32_t z) {
  const bool tomb = vt - 1u < 2u;
  const bool two = (z & 0x80) != 0;
  const uint32_t vl = two ? ((z & 0x7F) | ((z >> 1) & 0x3F80)) : (z & 0x7F);
  return q + (tomb ? 0u : vl + 1u + (two ? 1u : 0u));
}

// Phase A: lane = restart interval.  Walks record BOUNDARIES only and writes
// one descriptor per record; phase B parses every record in full and checks
// that it ends exactly where its descriptor says, so a boundary computed
// here from a malformed record can only turn into a PARSE status.  The step
// is kept short because it runs as one wave's serial instruction stream:
// the key length is read at the PREDICTED header length (the previous
// record's shape, checked with one mask compare) and the value length from
// the same 16-byte LDS window; only a shape change, a long key suffix or a
// long varint leaves the straight path.  The loop is wave-uniform: lanes
// past their interval's end store to rec[dummy].
template <bool kWide = false>
__device__ __forceinline__ void phase_a(const uint8_t* img, BlockMeta* meta, const uint8_t* owner, uint64_t* rec,
                                        uint32_t c_first, uint32_t c_step, uint32_t total, uint32_t dummy) {
  typedef RecLayout<kWide> RL;
  const int lane = threadIdx.x & (kWave - 1);
  for (uint32_t c0 = c_first; c0 < total; c0 += c_step) {
    const uint32_t c = c0 + lane;
    const bool live = c < total;
    const uint32_t j = live ? owner[c] : 0;
    const BlockMeta& m = meta[j];
    const TrailerInfo t = trailer_of(m);
    const uint32_t p0 = m.p0, rec_end = m.rec_end;
    const uint32_t r = live ? c - m.chain0 : 0;
    const bool last_iv = r + 1 == t.bin_len;
    const uint32_t s_rel = bin_get(img, p0, t, r);
    const uint32_t e_rel = last_iv ? t.rec_end : bin_get(img, p0, t, r + 1);
    // records lie before the marker; the first one at payload offset 0
    bool ok = s_rel < t.rec_end && e_rel <= t.rec_end && (r != 0 || s_rel == 0);
    const uint32_t count = (live && ok) ? (last_iv ? t.item_count - r * t.ri : t.ri) : 0;
    if (live && !ok) atomicCAS(&meta[j].st, ST_OK, ST_PARSE);
    const uint32_t ib0 = m.item0 + r * t.ri;
    const uint64_t tag = ((uint64_t)j << RL::kBlockShift) | RL::kValid;
    const uint32_t stop = p0 + e_rel;
    uint32_t a = p0 + (ok ? s_rel : 0), key = a;
    const uint32_t max_count = __builtin_amdgcn_readfirstlane(wave_max_u32(count));
    if (!max_count) continue;
    Shape sp;
    bool defer = false;  // a record shape the straight path does not take: whole block to the general path
    {  // restart head (full key: the value length is read separately)
      const Win16 w = read_win16(img, a);
      const RecHead hd = rec_head(w.lo, true);
      const uint32_t nxt = a + rec_len(hd.vt, hd.q, read_u16_unaligned(img, a + hd.q));
      key = a + hd.hdr;
      sp = make_shape<RL>(min(hd.e1 >> 3, 5u), 1);
      defer = count > 1 && !(hd.ok && valid_vtype(hd.vt));
      const bool act = count > 0 && !defer;
      if (count > 1 && act) ok = nxt < rec_end;
      const uint64_t rbits = (count > 1) ? ((uint64_t)(hd.e1 >> 3) << RL::kN1Shift) : 0;  // verified only if walked
      rec[act ? ib0 : dummy] = rec_desc<RL>(a, count == 1 ? stop : nxt, key, tag | RL::kRestart | rbits);
      a = (act && ok) ? nxt : a;
    }
    // The straight-line step, kept short because it is one wave's serial
    // instruction stream: the key length is read at the header length of the
    // previous record's shape and the value length at its key end (both
    // loads issued together); a shape or key-length change takes the rare
    // branch.  No bounds bookkeeping here: positions are clamped to the
    // marker and phase B rejects any record that does not end where its
    // descriptor says.
    uint32_t qp = 0;
    uint32_t hi = (uint32_t)((((uint64_t)key << RL::kKeyShift) | tag | sp.bits) >> 32);
    const uint32_t dmy = dummy;
    for (uint32_t jj = 1; jj < max_count; ++jj) {
      const uint64_t h = read_u64_unaligned(img, a);
      uint32_t z = read_u16_unaligned(img, a + qp);
      const uint32_t klen = (uint32_t)(h >> sp.kshift) & 0x7F;
      uint32_t q = sp.hdr + klen;
      uint32_t vt = (uint32_t)h & 0xFF;
      if (((~h & sp.msk) != sp.pat) | (q != qp)) {  // rare: header shape or key length changed
        const RecHead hd = rec_head(h, false);
        if (hd.ok) sp = make_shape<RL>(hd.e1 >> 3, (hd.e2 - hd.e1) >> 3);
        defer = defer || (jj < count && !hd.ok);  // seqno >= 2^49, shared >= 2^21 or key length >= 128
        q = hd.q;
        z = read_u16_unaligned(img, a + q);
        qp = q;
        hi = (uint32_t)((((uint64_t)key << RL::kKeyShift) | tag | sp.bits) >> 32);
      }
      const uint32_t nxt = min(a + rec_len(vt, q, z), rec_end);
      const bool act = jj < count && !defer;
      const uint32_t end = jj + 1 == count ? stop : nxt;
      rec[act ? ib0 + jj : dmy] = ((uint64_t)hi << 32) | (uint64_t)RL::lo(a, end);
      a = act ? nxt : a;
    }
    if (defer) meta[j].st = ST_DEFER;                             // wins over PARSE
    else if (count && !ok) atomicCAS(&meta[j].st, ST_OK, ST_PARSE);  // walked off the record area
  }
}


// parse_data_fast for a record whose header shape (n1 seqno bytes, n2 shared
// bytes, 1-byte key length) phase A has already verified bit for bit.
__device__ __forceinline__ int parse_data_shape(const uint8_t* base, uint32_t p0, uint32_t pos, uint32_t end,
                                                bool restart, uint32_t base_key_off, uint32_t n1, uint32_t n2,
                                                ItemFields& f, uint32_t& next) {
  const uint64_t h = read_u64_unaligned(base, p0 + pos);
  const uint32_t hdr = n1 + (restart ? 0u : n2) + 2;
  const uint32_t klen = (uint32_t)(h >> (8 * (hdr - 1))) & 0x7F;
  const uint32_t q = hdr + klen;
  const uint32_t vt = (uint32_t)h & 0xFF;
  uint32_t n4, vl;
  bool vl_ok;
  rec_value(vt, read_u16_unaligned(base, p0 + min(pos + q, end)), n4, vl, vl_ok);
  const uint32_t shared = restart ? 0u : (uint32_t)leb_val8(h >> (8 * (n1 + 1)), n2) & 0xFFFF;
  const uint32_t val_off = pos + q + n4;
  f.seqno = leb_val8(h >> 8, n1);
  f.handle_off = 0;
  f.key_off = pos + hdr;
  f.key_len = (uint16_t)klen;
  f.prefix_len = (uint16_t)shared;
  f.val_off = val_off;
  f.val_len = vl;
  f.vtype = (uint8_t)vt;
  next = val_off + vl;
  const bool bad = (pos + q + n4 > end) || ((uint64_t)val_off + vl > end) ||
                   (!restart && (uint64_t)base_key_off + shared > end);
  return !valid_vtype(vt) ? -1 : (!vl_ok ? 0 : (bad ? -1 : 1));
}

// The seven data-block fields present (handle_off is an index-block field,
// stored only when requested).
__host__ __device__ __forceinline__ bool all_fields(const lsm_parsed_items& o) {
  return o.seqno && o.key_off && o.val_off && o.val_len && o.key_len && o.prefix_len && o.vtype;
}

template <bool kCompact>
__device__ __forceinline__ void store_fields(const DecodeParams& P, bool all_fields, uint64_t gi,
                                             const ItemFields& f) {
  if (all_fields) {  // every output array present: no per-field null checks
    gstore(P.out.seqno, gi, f.seqno + P.seqno_add);
    if (kCompact) {  // 19 B/item: 16-bit payload offsets and lengths
      gstore(reinterpret_cast<uint16_t*>(P.out.key_off), gi, (uint16_t)f.key_off);
      gstore(reinterpret_cast<uint16_t*>(P.out.val_off), gi, (uint16_t)f.val_off);
      gstore(reinterpret_cast<uint16_t*>(P.out.val_len), gi, (uint16_t)f.val_len);
    } else {
      gstore(P.out.key_off, gi, f.key_off);
      gstore(P.out.val_off, gi, f.val_off);
      gstore(P.out.val_len, gi, f.val_len);
    }
    gstore(P.out.key_len, gi, f.key_len);
    gstore(P.out.prefix_len, gi, f.prefix_len);
    gstore(P.out.vtype, gi, f.vtype);
    if (P.out.handle_off) gstore(P.out.handle_off, gi, f.handle_off);
  } else {
    emit_global(P.out, gi, f, P.seqno_add, kCompact);
  }
}

// Phase B: thread = record.  Full parse + validation of every descriptor
// (the oracle's parse_data_item checks, and the record must end exactly at
// the descriptor's end), then coalesced stores of all fields.
template <bool kAllFields, bool kCompact, bool kWide = false>
__device__ __forceinline__ void phase_b(const DecodeParams& P, const uint8_t* img, BlockMeta* meta,
                                        const uint64_t* rec, uint32_t n_items, uint32_t g_item0, uint32_t tid,
                                        uint32_t nthr) {
  typedef RecLayout<kWide> RL;
  constexpr bool all_fields = kAllFields;
  const bool store = !(kDiagBuild && (P.flags & kDiagSkipStore));
  for (uint32_t i0 = 0; i0 < n_items; i0 += nthr) {
    const uint32_t i = i0 + tid;
    if (i >= n_items) break;
    const uint64_t d = rec[i];
    if (!(d & RL::kValid)) continue;  // not reached: its block has failed
    const uint32_t j = (uint32_t)(d >> RL::kBlockShift) & 31;
    const u32x4 hot = *reinterpret_cast<const u32x4*>(&meta[j]);  // p0, rec_end, st, type
    const uint32_t p0 = hot.x, end = hot.y - p0;
    if ((int32_t)hot.z != ST_OK) continue;  // block already failed: outputs unspecified
    const uint32_t a = RL::start(d) - p0;
    const uint32_t want = RL::end(d) - p0;
    const uint32_t base_key = ((uint32_t)(d >> RL::kKeyShift) & RL::kPosMask) - p0;
    const bool restart = (d & RL::kRestart) != 0;
    const uint64_t gi = (uint64_t)g_item0 + i;
    ItemFields f;
    uint32_t next;
    const uint32_t n1 = (uint32_t)(d >> RL::kN1Shift) & 7, n2 = (uint32_t)(d >> RL::kN2Shift) & 3;
    const int rc = n1 ? parse_data_shape(img, p0, a, end, restart, base_key, n1, n2, f, next)
                      : parse_data_fast(img, p0, a, end, restart, base_key, f, next);
    if (rc > 0 && store) store_fields<kCompact>(P, all_fields, gi, f);
    if (rc == 0) meta[j].st = ST_DEFER;  // wins over PARSE
    else if (rc < 0 || next != want) atomicCAS(&meta[j].st, ST_OK, ST_PARSE);
  }
}

// Records of restart interval r, [start, stop) payload-relative (the binary
// index's entries r, r + 1), parsed from `base`; emit(j, fields).
template <class Emit>
__device__ __forceinline__ bool walk_interval_at(const uint8_t* base, uint32_t p0, const BlockMeta& m,
                                                 const TrailerInfo& t, uint32_t r, uint32_t start, uint32_t stop,
                                                 Emit emit) {
  const bool last = r + 1 == t.bin_len;
  const uint32_t count = last ? t.item_count - r * t.ri : t.ri;
  if (start > t.rec_end || stop > t.rec_end || (r == 0 && start != 0)) return false;
  uint32_t base_key = 0, pos = start;
  ItemFields f;
  for (uint32_t j = 0; j < count; ++j) {
    uint32_t next;
    if (!parse_record(base, p0, pos, t, m.type, j == 0, base_key, f, next)) return false;
    if (j == 0) base_key = f.key_off;
    emit(r * t.ri + j, f);
    pos = next;
  }
  return pos == stop;
}

// Interval walk straight from a span (direct path); emit(j, fields).
template <class Emit>
__device__ __forceinline__ bool walk_interval(const uint8_t* base, uint32_t p0, const BlockMeta& m, uint32_t r,
                                              Emit emit) {
  const TrailerInfo t = trailer_of(m);
  const bool last = r + 1 == t.bin_len;
  const uint32_t start = bin_get(base, p0, t, r);
  const uint32_t stop = last ? t.rec_end : bin_get(base, p0, t, r + 1);
  return walk_interval_at(base, p0, m, t, r, start, stop, emit);
}

// One block straight from HBM (blocks larger than the LDS stage).
__device__ __forceinline__ void decode_block_direct(const DecodeParams& P, uint32_t b, BlockMeta* meta) {
  const int lane = threadIdx.x;
  const uint64_t off = gload(P.block_off, b), end = gload(P.block_off, b + 1);
  const uint8_t* base = P.blocks + (off & ~15ULL);
  const uint32_t hb = (uint32_t)(off & 15);
  const uint64_t len = end >= off ? end - off : 0;
  const uint64_t item_base = gload(P.item_start, b);
  const uint32_t cap = gload(P.item_start, b + 1) - gload(P.item_start, b);
  if (lane == 0) meta_header(base, hb, len, meta[0]);
  wave_sync();
  if (meta[0].st == ST_OK && !(P.flags & LSM_DECODE_PAYLOAD_VERIFIED)) {
    uint64_t lo, hi;
    xxh3_128_wave(base, hb + kHdrLen, meta[0].len - kHdrLen, &kLongSecret, lo, hi);
    if (lane == 0 && (lo != meta[0].ck_lo || hi != meta[0].ck_hi)) meta[0].st = ST_CKSUM;
  }
  wave_sync();
  if (lane == 0) meta_trailer(base, P.expect_type, cap, meta[0], P.compact);
  wave_sync();
  const BlockMeta m = meta[0];
  if (m.st == ST_OK) {
    bool ok = true;
    for (uint32_t r = lane; r < m.bin_len; r += kWave) {
      ok &= walk_interval(base, hb + kHdrLen, m, r,
                          [&](uint32_t j, const ItemFields& f) { emit_global(P.out, item_base + j, f, P.seqno_add, P.compact); });
    }
    if (!ok) atomicCAS(&meta[0].st, ST_OK, ST_PARSE);
  }
  wave_sync();
  if (lane == 0) gstore(P.status, b, meta[0].st);
  wave_sync();
}

// Hand-off lists in the workspace: a count and the block indices (u32 x n_blocks).
__device__ __forceinline__ void defer_block(const DecodeParams& P, uint32_t b) {
  const uint32_t slot = atomicAdd(P.defer_count, 1u);
  gstore(P.defer_list, slot, b);
}
// Wave-level: lanes with `pred` list block b (one atomic per wave, not per block).
__device__ __forceinline__ void defer_blocks_wave(const DecodeParams& P, bool pred, uint32_t b) {
  const uint64_t m = __ballot(pred);
  if (!m) return;
  const int lane = threadIdx.x & (kWave - 1);
  uint32_t base = 0;
  if (lane == (int)__builtin_ctzll(m)) base = atomicAdd(P.defer_count, (uint32_t)__builtin_popcountll(m));
  base = (uint32_t)__shfl((int)base, (int)__builtin_ctzll(m));
  const uint32_t rank = (uint32_t)__builtin_popcountll(m & ((1ULL << lane) - 1));
  if (pred) gstore(P.defer_list, base + rank, b);
}

__device__ __forceinline__ void defer2_block(const DecodeParams& P, uint32_t b) {
  const uint32_t slot = atomicAdd(P.defer2_count, 1u);
  gstore(P.defer2_list, slot, b);
}

__device__ __forceinline__ void defer3_block(const DecodeParams& P, uint32_t b) {
  const uint32_t slot = atomicAdd(P.defer3_count, 1u);
  gstore(P.defer3_list, slot, b);
}

// Diagnostic builds with timers (-DLSM_DIAG without -DLSM_DIAG_NOTIME): per-phase s_memtime
// totals of the group, big-block and huge kernels, read by lsm_diag_decode_phases (decode.hip).
// A kernel adds into a 32-entry array of its own unit (the library has no relocatable device
// code): the big-block kernel into entries 0..7, the huge kernel into 8..14, both their block /
// unit counts into 15, the group kernel into 16..31; decode_*_phases adds a unit's array into
// sum32 and clears it.
#if defined(LSM_DIAG) && !defined(LSM_DIAG_NOTIME)
#define DEC_PHASE(i)                                  \
  {                                                   \
    const uint64_t t_ = __builtin_amdgcn_s_memtime(); \
    ph[i] += t_ - t_last;                             \
    t_last = t_;                                      \
  }
// Role timer: time since the last phase mark into ph[i], one count into ph[i + 1].
#define DEC_ROLE(i)                                   \
  {                                                   \
    ph[i] += __builtin_amdgcn_s_memtime() - t_last;   \
    ph[(i) + 1] += 1;                                 \
  }
template <class Sym>
inline hipError_t take_dec_phases(const Sym& sym, uint64_t* sum32) {
  uint64_t v[32];
  static const uint64_t z[32] = {};
  hipError_t e = hipMemcpyFromSymbol(v, HIP_SYMBOL(sym), sizeof(v));
  if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(sym), z, sizeof(z));
  for (int i = 0; i < 32 && e == hipSuccess; ++i) sum32[i] += v[i];
  return e;
}
hipError_t decode_group_phases(uint64_t* sum32);
hipError_t decode_large_phases(uint64_t* sum32);  // the big-block and the huge kernel
#else
#define DEC_PHASE(i)
#define DEC_ROLE(i)
#endif

// ------------------------------------------------------- host: the stage launchers
// Each launches its stage's kernels on st; launch_decode (decode.hip) calls them in this order.
// variant: bit 0 every data-block field is asked for (all_fields), bit 1 P.compact.
hipError_t launch_decode_group(const DecodeParams& P, int variant, hipStream_t st);
// the blocks the group kernel listed; *bgrid: the workgroups launched (0: none)
hipError_t launch_decode_big(const DecodeParams& P, int variant, uint32_t* bgrid, hipStream_t st);
// with the pool: the huge blocks the big-block kernel listed (rejects go to the general path's list)
hipError_t launch_decode_huge_plan(const DecodeParams& P, hipStream_t st);
// the general path over the defer2 list
hipError_t launch_decode_general(const DecodeParams& P, hipStream_t st);
// with the pool: the unit table, the units with the streamed chains, the chain pass
hipError_t launch_decode_huge(const DecodeParams& P, bool all, hipStream_t st);
// The pool's bytes for a batch of blocks_bytes bytes in n_blocks blocks, and the least a pool holds.
size_t decode_huge_pool_bytes(uint32_t n_blocks, uint64_t blocks_bytes);
size_t decode_huge_pool_min_bytes();

}  // namespace lsmgpu
