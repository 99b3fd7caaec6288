// point_read.hpp — the per-block body of DataBlock::point_read
// (src/table/data_block/mod.rs:412-472) and the key compares it is built on,
// shared by point_read_kernel (point_read.hip) and table_get_kernel
// (table_get.hip), and the per-block body of the data-block iterator's range
// seeks (data_block/iter.rs:37-176), shared by seek_kernel (point_read.hip)
// and table_range_kernel (table_range.hip).  One lane per query, block bytes
// straight from HBM through the aligned-window readers.
#pragma once

#include "block_format.hpp"
#include "lsmgpu.h"

namespace lsmgpu {

__device__ __forceinline__ uint32_t win_byte(const Win16& w, uint32_t i) {
  return (uint32_t)((i < 8 ? w.lo >> (8 * i) : w.hi >> (8 * (i - 8))) & 0xFF);
}

// Lexicographic compare of a[ap .. ap+an) with b[bp .. bp+bn) (both bases
// 4-byte aligned, 16-byte windows; both spans readable up to 20 bytes past).
__device__ __forceinline__ int cmp_span(const uint8_t* ab, uint32_t ap, uint32_t an, const uint8_t* bb, uint32_t bp,
                                        uint32_t bn) {
  const uint32_t n = min(an, bn);
  for (uint32_t k = 0; k < n; k += 16) {
    const Win16 wa = read_win16(ab, ap + k), wb = read_win16(bb, bp + k);
    const uint32_t m = min(16u, n - k);
    uint64_t x0 = wa.lo ^ wb.lo, x1 = wa.hi ^ wb.hi;
    if (m < 8) {
      x0 &= (1ULL << (8 * m)) - 1;
      x1 = 0;
    } else if (m < 16) {
      x1 &= m == 8 ? 0ULL : (1ULL << (8 * (m - 8))) - 1;
    }
    if (x0 | x1) {
      const uint32_t i = x0 ? (uint32_t)__builtin_ctzll(x0) >> 3 : 8 + ((uint32_t)__builtin_ctzll(x1) >> 3);
      return win_byte(wa, i) < win_byte(wb, i) ? -1 : 1;
    }
  }
  return an < bn ? -1 : (an > bn ? 1 : 0);
}

// compare_prefixed_slice(prefix, suffix, needle), src/table/util.rs:133-167.
__device__ __forceinline__ int cmp_prefixed(const uint8_t* kb, uint32_t pre, uint32_t pn, uint32_t suf, uint32_t sn,
                                            const uint8_t* nb, uint32_t np, uint32_t nn) {
  if (nn == 0) return (pn + sn) > 0 ? 1 : 0;
  const uint32_t m = min(pn, nn);
  const int c = cmp_span(kb, pre, m, nb, np, m);
  if (c) return c;
  if (pn > nn) return 1;
  return cmp_span(kb, suf, sn, nb, np + pn, nn - pn);
}

// DataBlock::point_read on the payload base[p0 .. p0+plen) whose trailer is t:
// the hash-index probe (FREE = not found, CONFLICT or no hash index = the
// restart-head binary search, else the head the bucket names), then the linear
// MVCC scan (first item with key == needle and seqno < snap).  found = the
// item's index in the block (hit = its fields), -1 = None.  Returns ST_OK or
// ST_PARSE.
__device__ __forceinline__ int32_t point_read_block(const uint8_t* base, uint32_t p0, uint32_t plen,
                                                    const TrailerInfo& t, const uint8_t* nb, uint32_t np,
                                                    uint32_t nn, uint64_t snap, int64_t& found, ItemFields& hit) {
  int32_t st = ST_OK;
  bool search = true, miss = false;
  uint32_t start = 0;
  if (t.hash_len > 0) {
    if ((uint64_t)t.hash_off + t.hash_len > (uint64_t)plen - kTrailerLen) {  // bucket bytes precede the trailer
      st = ST_PARSE;
    } else {
      const uint64_t hv = xxh3_64_any(nn, BaseReader8{nb, np}, BaseReader64{nb, np});
      const uint32_t m = read_u32_unaligned(base, p0 + t.hash_off + (uint32_t)(hv % t.hash_len)) & 0xFF;
      if (m == kHashFree) {
        miss = true;
      } else if (m != kHashConflict) {
        if (m >= t.bin_len) st = ST_PARSE;
        start = m;
        search = false;
      }
    }
  }
  if (st == ST_OK && !miss && search) {  // last restart head with key < needle
    uint32_t lo = 0, hi = t.bin_len;
    while (lo < hi && st == ST_OK) {
      const uint32_t mid = lo + (hi - lo) / 2;
      Cursor c;
      c.init(base, p0, bin_get(base, p0, t, mid), t.rec_end);
      ItemFields f;
      if (!parse_data_record(c, true, 0, f)) {
        st = ST_PARSE;
        break;
      }
      if (cmp_span(base, p0 + f.key_off, f.key_len, nb, np, nn) < 0) lo = mid + 1;
      else hi = mid;
    }
    start = lo == 0 ? 0 : lo - 1;
  }
  if (st == ST_OK && !miss) {  // linear scan from restart head `start`
    Cursor c;
    c.init(base, p0, bin_get(base, p0, t, start), t.rec_end);
    uint32_t head_key = 0;
    for (uint64_t i = (uint64_t)start * t.ri; i < t.item_count; ++i) {
      const bool restart = i % t.ri == 0;
      ItemFields f;
      if (!parse_data_record(c, restart, head_key, f)) {
        st = ST_PARSE;
        break;
      }
      int cmp;
      if (restart) {
        head_key = f.key_off;
        cmp = cmp_span(base, p0 + f.key_off, f.key_len, nb, np, nn);
      } else {
        cmp = cmp_prefixed(base, p0 + head_key, f.prefix_len, p0 + f.key_off, f.key_len, nb, np, nn);
      }
      if (cmp > 0) break;
      if (cmp < 0) continue;
      if (f.seqno >= snap) continue;
      found = (int64_t)i;
      hit = f;
      break;
    }
  }
  return st;
}

// ---------------------------------------------------------------- seek
// partition_point over the restart heads: pred = head < needle (or <= with le).
__device__ __forceinline__ int32_t seek_partition(const uint8_t* base, uint32_t p0, const TrailerInfo& t,
                                                  const uint8_t* nb, uint32_t np, uint32_t nn, bool le,
                                                  uint32_t& iv) {
  uint32_t lo = 0, hi = t.bin_len;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    Cursor c;
    c.init(base, p0, bin_get(base, p0, t, mid), t.rec_end);
    ItemFields f;
    if (!parse_data_record(c, true, 0, f)) return ST_PARSE;
    const int cmp = cmp_span(base, p0 + f.key_off, f.key_len, nb, np, nn);
    if (le ? cmp <= 0 : cmp < 0) lo = mid + 1;
    else hi = mid;
  }
  iv = lo == 0 ? 0 : lo - 1;
  return ST_OK;
}

// Forward scan from restart interval iv: index of the first item that stops
// it (key >= needle, or key > needle with `past_equal`), item_count if none;
// eq = that item's key equals the needle.
__device__ __forceinline__ int32_t seek_scan(const uint8_t* base, uint32_t p0, const TrailerInfo& t, uint32_t iv,
                                             const uint8_t* nb, uint32_t np, uint32_t nn, bool past_equal,
                                             uint32_t& at, bool& eq, bool& prev_eq) {
  Cursor c;
  c.init(base, p0, bin_get(base, p0, t, iv), t.rec_end);
  uint32_t head_key = 0;
  at = t.item_count;
  eq = prev_eq = false;
  for (uint32_t i = iv * t.ri; i < t.item_count; ++i) {
    const bool restart = i % t.ri == 0;
    ItemFields f;
    if (!parse_data_record(c, restart, head_key, f)) return ST_PARSE;
    int cmp;
    if (restart) {
      head_key = f.key_off;
      cmp = cmp_span(base, p0 + f.key_off, f.key_len, nb, np, nn);
    } else {
      cmp = cmp_prefixed(base, p0 + head_key, f.prefix_len, p0 + f.key_off, f.key_len, nb, np, nn);
    }
    if (cmp > 0 || (cmp == 0 && !past_equal)) {
      at = i;
      eq = cmp == 0;
      return ST_OK;
    }
    prev_eq = cmp == 0;
  }
  return ST_OK;
}

// The bound arenas of a batch of range queries (lsm_seek_blocks, lsm_table_range):
// query q's lower bound is lo[lo_off[q] .. lo_off[q+1]), its upper bound likewise.
struct SeekBounds {
  const uint8_t* lo;
  const uint64_t* lo_off;
  const uint8_t* hi;
  const uint64_t* hi_off;
};

// Both seeks of query q (flags fl, LSM_SEEK_*) on the data block whose payload
// is base[p0 ..) with trailer t: the item range [first, end) and the seeks'
// return values (found bit 0 lower, bit 1 upper).  Returns ST_OK or ST_PARSE.
__device__ __forceinline__ int32_t seek_block(const uint8_t* base, uint32_t p0, const TrailerInfo& t,
                                              const SeekBounds& B, uint32_t q, uint32_t fl, uint32_t& first,
                                              uint32_t& end, uint32_t& found) {
  int32_t st = ST_OK;
  first = 0;
  end = t.item_count;
  if (fl & LSM_SEEK_LO) {  // Iter::seek (iter.rs:37-76) / seek_exclusive (iter.rs:115-145)
    const uint64_t o = B.lo_off[q];
    const uint32_t nn = (uint32_t)min(B.lo_off[q + 1] - o, (uint64_t)0xFFFFFFFFu);
    const uint8_t* nb = B.lo + (o & ~15ULL);
    const uint32_t np = (uint32_t)(o & 15);
    const bool excl = (fl & LSM_SEEK_LO_EXCLUSIVE) != 0;
    uint32_t iv = 0;
    bool eq = false, prev_eq = false;
    st = seek_partition(base, p0, t, nb, np, nn, false, iv);
    if (st == ST_OK) st = seek_scan(base, p0, t, iv, nb, np, nn, excl, first, eq, prev_eq);
    if (excl ? first < t.item_count : eq) found |= 1;
  }
  if (st == ST_OK && (fl & LSM_SEEK_HI)) {  // Iter::seek_upper (iter.rs:78-113) / seek_upper_exclusive (:147-176)
    const uint64_t o = B.hi_off[q];
    const uint32_t nn = (uint32_t)min(B.hi_off[q + 1] - o, (uint64_t)0xFFFFFFFFu);
    const uint8_t* nb = B.hi + (o & ~15ULL);
    const uint32_t np = (uint32_t)(o & 15);
    const bool excl = (fl & LSM_SEEK_HI_EXCLUSIVE) != 0;
    uint32_t iv = 0;
    bool eq = false, prev_eq = false;
    // inclusive: end = first key > needle (heads <= needle); exclusive: first key >= needle (heads < needle)
    st = seek_partition(base, p0, t, nb, np, nn, !excl, iv);
    if (st == ST_OK) st = seek_scan(base, p0, t, iv, nb, np, nn, !excl, end, eq, prev_eq);
    if (excl ? end > 0 : (end > 0 && prev_eq)) found |= 2;
  }
  if (first > end) first = end;  // the two scanners crossed: empty range
  return st;
}

}  // namespace lsmgpu
