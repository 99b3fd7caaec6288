// encode_large.hip — the blocks the group kernel does not take: the listed medium / big blocks and
// the huge ones (E3, one workgroup per block or across the GPU); see encode.hip.
#include "encode_group.hpp"

namespace lsmgpu {

__device__ __forceinline__ Win16 read_win16_at(const uint8_t* base, uint64_t off) {
  return read_win16(base + (off & ~3ULL), (uint32_t)(off & 3));
}

// longest_shared_prefix_length, src/table/util.rs:125-130.  Up to 48 bytes
// per step with all six windows in flight together (one HBM round trip for
// the keys of every BASELINE shape).
__device__ __forceinline__ uint32_t lcp_global(const uint8_t* keys, uint64_t a, uint64_t b, uint32_t n) {
  uint32_t k = 0;
  while (k < n) {
    Win16 wa[3], wb[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      wa[i] = wb[i] = Win16{0, 0};
      if (i == 0 || k + 16 * i < n) {
        wa[i] = read_win16_at(keys, a + k + 16 * i);
        wb[i] = read_win16_at(keys, b + k + 16 * i);
      }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const uint32_t kk = k + 16 * i;
      if (kk >= n) return n;
      const uint64_t x0 = wa[i].lo ^ wb[i].lo, x1 = wa[i].hi ^ wb[i].hi;
      if (x0) return min(n, kk + (uint32_t)(__builtin_ctzll(x0) >> 3));
      if (x1) return min(n, kk + 8 + (uint32_t)(__builtin_ctzll(x1) >> 3));
    }
    k += 48;
  }
  return n;
}

// ------------------------------------------------------- record assembly
// Destination pointers of the record writers: LDS images (lds8_t) or HBM
// (gbl8_t), explicit so that the stores compile to ds_write / global_store
// (a generic pointer gives flat stores, which also count on lgkmcnt: every
// later LDS wait then waits for the loads in flight too).
typedef __attribute__((address_space(3))) uint8_t lds8_t;
typedef __attribute__((address_space(1))) uint8_t gbl8_t;
__device__ __forceinline__ void st_u32(lds8_t* p, uint32_t v) { *(__attribute__((address_space(3))) uint32_t*)p = v; }
__device__ __forceinline__ void st_u32(gbl8_t* p, uint32_t v) { *(__attribute__((address_space(1))) uint32_t*)p = v; }
__device__ __forceinline__ void st_u32(uint8_t* p, uint32_t v) { *reinterpret_cast<uint32_t*>(p) = v; }
__device__ __forceinline__ lds8_t* as_lds(uint8_t* p) { return (lds8_t*)p; }
__device__ __forceinline__ gbl8_t* as_gbl(uint8_t* p) { return (gbl8_t*)p; }

// Span copy src (HBM, any alignment) -> dst[d .. d + n) (any alignment), in
// two steps so that all loads of a record are issued before its stores:
// load() reads the aligned 16-B windows that hold bytes of the span (the
// first K in registers; longer spans stream the rest at store time) and the
// at most 3 + 3 edge bytes; store() writes the destination dwords wholly
// inside the span (dword q, counted from d & ~3, is source bytes
// [base + 4q, base + 4q + 4) relative to the first window, base = (src & 15)
// - (d & 3), assembled with v_alignbyte) and the edge bytes, which share
// their dword with the neighbouring record.
template <int K>
struct SpanCopy {
  const __attribute__((address_space(1))) u32x4* W;
  uint32_t n, d, rel, nwin, h, tl, hb, tb;
  u32x4 w[K];
  __device__ __forceinline__ void load(const uint8_t* src, uint32_t n_, uint32_t d_) {
    const uint64_t a = (uint64_t)(uintptr_t)src;
    W = (const __attribute__((address_space(1))) u32x4*)(a & ~15ULL);
    n = n_;
    d = d_;
    rel = (uint32_t)(a & 15);
    nwin = n_ ? ((rel + n_ - 1) >> 4) + 1 : 0;
#pragma unroll
    for (int k = 0; k < K; ++k) w[k] = (uint32_t)k < nwin ? W[k] : u32x4{0, 0, 0, 0};
    h = min(n_, (4u - (d_ & 3u)) & 3u);
    tl = n_ > h ? (d_ + n_) & 3u : 0u;
    hb = tb = 0;
    const gbl8_t* gs = (const gbl8_t*)src;
    for (uint32_t k = 0; k < h; ++k) hb |= (uint32_t)gs[k] << (8 * k);
    for (uint32_t k = 0; k < tl; ++k) tb |= (uint32_t)gs[n_ - tl + k] << (8 * k);
  }
  template <class D>
  __device__ __forceinline__ void emit(D* dst, int wi, const u32x4& cw, uint32_t next0, int t0, uint32_t sh,
                                       uint32_t da, int qa, int qb) const {
    const uint32_t c[5] = {cw.x, cw.y, cw.z, cw.w, next0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int q = 4 * wi + j - t0;
      if (q >= qa && q <= qb) st_u32(dst + da + 4 * q, alignbyte(c[j + 1], c[j], sh));
    }
  }
  template <class D>
  __device__ __forceinline__ void store(D* dst) const {
    for (uint32_t k = 0; k < h; ++k) dst[d + k] = (uint8_t)(hb >> (8 * k));
    for (uint32_t k = 0; k < tl; ++k) dst[d + n - tl + k] = (uint8_t)(tb >> (8 * k));
    const int qa = (d & 3) ? 1 : 0;
    const int qb = (int)((d + n) >> 2) - (int)(d >> 2) - 1;
    if (!n || qb < qa) return;
    const int base = (int)rel - (int)(d & 3);
    const int t0 = base >> 2;  // -1 when the destination phase runs ahead of the source
    const uint32_t sh = (uint32_t)base & 3u;
    const uint32_t da = d & ~3u;
    // (t0 = -1 only when d & 3 > rel, and then dword 0 is an edge dword)
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if ((uint32_t)k < nwin) {
        uint32_t nx = 0;
        if (k + 1 < K) nx = w[k + 1].x;
        else if ((uint32_t)(k + 1) < nwin) nx = W[k + 1].x;
        emit(dst, k, w[k], nx, t0, sh, da, qa, qb);
      }
    }
    for (uint32_t k = K; k < nwin; ++k) {  // spans longer than K windows
      const u32x4 cw = W[k];
      const uint32_t nx = k + 1 < nwin ? W[k + 1].x : 0;
      emit(dst, (int)k, cw, nx, t0, sh, da, qa, qb);
    }
  }
};

// 16-B copy-out store of the list / huge-block kernels (non-temporal: plain stores measured
// 0 to +2 % slower for the configs[4] classes, profiles/r06_experiments.txt; the group
// kernel's copy-out is plain)
__device__ __forceinline__ void copy_store16(u32x4* dst, const u32x4& v) { __builtin_nontemporal_store(v, dst); }

template <int kOW = 0>
__device__ __forceinline__ ItemMeta load_item(const EncodeParams& P, uint64_t i, bool& bad) {
  ItemMeta m;
  m.ko = koff<kOW>(P, i);  // (global loads, not flat ones)
  const uint64_t kl = koff<kOW>(P, i + 1) - m.ko;
  if (kl > 0xFFFF) bad = true;
  m.klen = (uint32_t)min(kl, (uint64_t)0xFFFF);
  m.seq = gload(P.it.seqno, i);
  m.sh = 0;
  m.e = 0;
  if (is_index(P)) {
    m.vo = gload(P.it.handle_off, i);
    m.vl = gload(P.it.handle_size, i);
    m.vt = 0;
  } else {
    m.vo = voff<kOW>(P, i);
    const uint64_t vl = voff<kOW>(P, i + 1) - m.vo;
    m.vt = gload(P.it.vtype, i);
    if (!valid_vtype(m.vt)) bad = true;
    if (!is_tombstone(m.vt) && vl > 0xFFFFFFFFULL) bad = true;
    m.vl = (uint32_t)vl;
  }
  return m;
}

// Item j of the block starting at item s, with its shared prefix against the
// restart head (encoder.rs:140-143, util.rs:125-130).
template <int kOW = 0>
__device__ __forceinline__ ItemMeta load_item_lcp(const EncodeParams& P, uint32_t s, uint32_t j, uint32_t ri,
                                                  bool& bad) {
  const uint64_t i = (uint64_t)s + j;
  ItemMeta m = load_item<kOW>(P, i, bad);
  if (!is_index(P) && j % ri != 0) {
    const uint64_t h = (uint64_t)s + (j / ri) * ri;
    const uint64_t hko = koff<kOW>(P, h);
    const uint32_t hkl = (uint32_t)min(koff<kOW>(P, h + 1) - hko, (uint64_t)0xFFFF);
    m.sh = lcp_global(P.it.keys, hko, m.ko, min(hkl, m.klen));
  }
  return m;
}

// One record at dpos: issue() loads the key (suffix) and value spans, store()
// writes the record (encode_full_into / encode_truncated_into,
// data_block/mod.rs:195-264; index: block_handle.rs:134-156).
struct RecordCopy {
  SpanCopy<2> key;
  SpanCopy<5> val;
  uint32_t dpos;
  __device__ __forceinline__ void issue(const EncodeParams& P, const ItemMeta& m, bool head, uint32_t dpos_) {
    dpos = dpos_;
    const uint32_t kfrom = head ? 0 : m.sh;
    const uint32_t kpos = dpos_ + head_len(P, m, head);
    key.load(P.it.keys + m.ko + kfrom, m.klen - kfrom, kpos);
    const bool has_val = !is_index(P) && !is_tombstone(m.vt);
    const uint32_t vpos = kpos + m.klen - kfrom + leb_len(m.vl);
    val.load(P.it.vals + (has_val ? m.vo : 0), has_val ? m.vl : 0, vpos);
  }
  template <class D>
  __device__ __forceinline__ void store(const EncodeParams& P, const ItemMeta& m, bool head, D* dst) const {
    uint32_t pos = dpos;
    if (is_index(P)) {
      dst[pos++] = 0;
      pos = put_leb(dst, pos, m.vo);
      pos = put_leb(dst, pos, m.vl);
      pos = put_leb(dst, pos, m.seq);
      put_leb(dst, pos, m.klen);
    } else {
      dst[pos++] = (uint8_t)m.vt;
      pos = put_leb(dst, pos, m.seq);
      if (head) {
        put_leb(dst, pos, m.klen);
      } else {
        pos = put_leb(dst, pos, m.sh);
        put_leb(dst, pos, m.klen - m.sh);
      }
      if (!is_tombstone(m.vt)) put_leb(dst, key.d + key.n, m.vl);
    }
    key.store(dst);
    val.store(dst);
  }
};

// ------------------------------------------- the stages of a listed / huge block
// Where a block's parts lie.  The block is assembled in an image whose byte 0 is 16-byte aligned:
// an LDS image that is copied out to gdst, or gdst itself (the huge blocks, straight in HBM).
struct ListedGeom {
  uint32_t s, n;               // first item, items
  uint32_t ri, step;           // restart interval, bytes per binary-index entry
  uint32_t total, plen;        // block bytes with and without the header
  uint32_t pad, p0;            // image offsets of the header and of the payload
  uint32_t bin_off, hash_off;  // payload offsets of the binary index and of the hash index (0: none)
  uint8_t* gdst;               // the block's place in the output, rounded down to 16 bytes
  bool overflow;               // the block ends past out_cap: nothing of it is written
};
__device__ __forceinline__ ListedGeom listed_geom(const EncodeParams& P, const BlockPlan& pl, uint32_t s, uint32_t n,
                                                  uint64_t dst_off, uint32_t total, bool overflow) {
  ListedGeom g;
  g.s = s;
  g.n = n;
  g.ri = is_index(P) ? 1 : P.ri;
  g.step = pl.step_flags & 0xFF;
  g.total = total;
  g.plen = total - kHdrLen;
  const uint64_t dabs = (uint64_t)(uintptr_t)P.out + dst_off;
  g.pad = (uint32_t)(dabs & 15);
  g.p0 = g.pad + kHdrLen;
  g.bin_off = pl.recs + 1;
  g.hash_off = pl.hash_w ? g.bin_off + pl.bin_len * g.step : 0;
  g.gdst = reinterpret_cast<uint8_t*>(dabs & ~15ULL);
  g.overflow = overflow;
  return g;
}
// Block b with plan pl, from the batch's offsets.
__device__ __forceinline__ ListedGeom listed_geom(const EncodeParams& P, uint32_t b, const BlockPlan& pl) {
  const uint32_t s = P.starts[b], e = P.starts[b + 1];
  const uint64_t dst_off = P.block_off[b], dst_end = P.block_off[b + 1];
  return listed_geom(P, pl, s, e - s, dst_off, (uint32_t)(dst_end - dst_off), dst_end > P.out_cap);
}

// A block the whole-GPU E3 accepted (it ends inside the output: encode_huge_plan_kernel).
__device__ __forceinline__ ListedGeom listed_geom(const EncodeParams& P, const EncHuge& h, const BlockPlan& pl) {
  return listed_geom(P, pl, h.s, h.n, h.dst_off, h.total, false);
}

// Exclusive prefix of rec over the workgroup's kWaves * 64 threads, in thread order, and the sum.
// One barrier, behind the psum stores: a caller that scans again puts its own behind the use.
template <uint32_t kWaves>
__device__ __forceinline__ uint32_t wg_excl_scan(uint32_t rec, uint32_t* psum, uint32_t* total) {
  const uint32_t incl = wave_incl_scan_u32(rec);
  if constexpr (kWaves == 1) {  // the wave scan alone (psum is not used)
    *total = wave_bcast_u32(incl, kWave - 1);
    return incl - rec;
  } else {
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    if ((threadIdx.x & (kWave - 1)) == kWave - 1) psum[wave] = incl;
    __syncthreads();
    // (two loops, not one with a select per wave: with that form the 8-wave listed writer took 173
    // VGPRs and ran 0.35 % slower than with its own copy of the scan, with this one 157 and 0.5 %
    // faster, profiles/encode_large_refactor_ab.txt)
    uint32_t base = 0, tot = 0;
    for (uint32_t w = 0; w < kWaves; ++w) tot += psum[w];
    for (uint32_t w = 0; w < wave; ++w) base += psum[w];
    *total = tot;
    return base + incl - rec;
  }
}

// The barrier between the stages of a kLW-wave block writer.
template <uint32_t kLW>
__device__ __forceinline__ void writer_sync() {
  if constexpr (kLW == 1) wave_lds_sync();
  else __syncthreads();
}

// Hash index of a block whose image is in HBM: the votes of all n keys in LDS passes of
// kE3HashChunk buckets (hlo / hhi), each pass's bytes to img.  Every thread of the kThreads calls it.
template <uint32_t kThreads, int kOW>
__device__ __forceinline__ void hash_index_passes(const EncodeParams& P, uint32_t s, uint32_t n, uint32_t ri,
                                                  uint32_t hash_w, uint8_t* img, uint32_t p0, uint32_t hash_off,
                                                  uint32_t* hlo, uint32_t* hhi) {
  const uint32_t tid = threadIdx.x;
  for (uint32_t base = 0; base < hash_w; base += kE3HashChunk) {
    const uint32_t lim = min(kE3HashChunk, hash_w - base);
    for (uint32_t k = tid; k < lim; k += kThreads) {
      hlo[k] = 0xFFFFFFFFu;
      hhi[k] = 0;
    }
    __syncthreads();
    for (uint32_t j = tid; j < n; j += kThreads) {
      const uint64_t i = (uint64_t)s + j;
      const uint64_t ko = koff<kOW>(P, i);
      const uint32_t bk = key_bucket(P, ko, (uint32_t)(koff<kOW>(P, i + 1) - ko), hash_w);
      if (bk >= base && bk < base + lim) {
        atomicMin(&hlo[bk - base], j / ri);
        atomicMax(&hhi[bk - base], j / ri);
      }
    }
    __syncthreads();
    for (uint32_t k = tid; k < lim; k += kThreads) img[p0 + hash_off + base + k] = (uint8_t)bucket_byte(hlo[k], hhi[k]);
    __syncthreads();
  }
}

// Image bytes [pad, pad + total) to gdst in 16-byte pieces, the ragged first and last piece by bytes.
template <uint32_t kThreads>
__device__ __forceinline__ void copy_out_image(const uint8_t* img, uint8_t* gdst, uint32_t pad, uint32_t total) {
  const uint32_t chunks = (pad + total + 15) >> 4;
  for (uint32_t c = threadIdx.x; c < chunks; c += kThreads) {
    const uint32_t lo = c * 16, hi = lo + 16;
    if (lo >= pad && hi <= pad + total) {
      copy_store16(reinterpret_cast<u32x4*>(gdst) + c, reinterpret_cast<const u32x4*>(img)[c]);
    } else {
      for (uint32_t k = max(lo, pad); k < min(hi, pad + total); ++k) gdst[k] = img[k];
    }
  }
}

// Listed block b (any item count) by the kLW waves of a workgroup, assembled in the LDS image at
// `smem` (16-B aligned, at least e2_need bytes) and copied out to its place in the packed output:
// items in chunks of kLW * 64 (shared prefixes recomputed from the keys, record offsets from a
// scan), then marker / hash-index bytes / trailer, the payload xxh3_128 and the header, and the
// copy-out.  With more than one wave the hash is xxh3_128_workgroup's (psum and contrib are
// theirs alone); one wave per 20-96 KiB block ran the 64 KiB classes at 0.18 TB/s.  Every thread
// of the workgroup calls it; the overflow return is uniform.
template <uint32_t kLW, int kOW>
__device__ __forceinline__ void write_listed_block(const EncodeParams& P, uint32_t b, uint8_t* smem, uint32_t* psum,
                                                   uint64_t* contrib) {
  constexpr uint32_t kT = kLW * kWave;
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  const BlockPlan pl = P.plans[b];
  const ListedGeom g = listed_geom(P, b, pl);
  if (g.overflow) {
    if (tid == 0) P.status[b] = ST_OVERFLOW;
    return;
  }
  uint8_t* img = smem;
  uint32_t* hlo = reinterpret_cast<uint32_t*>(smem + ((g.pad + g.total + 15) & ~15u) + 32);
  uint32_t* hhi = hlo + ((pl.hash_w + 3) & ~3u);
  for (uint32_t k = tid; k < pl.hash_w; k += kT) {
    hlo[k] = 0xFFFFFFFFu;
    hhi[k] = 0;
  }
  writer_sync<kLW>();
  const uint32_t s = g.s, n = g.n, ri = g.ri, step = g.step, p0 = g.p0, bin_off = g.bin_off;
  uint32_t carry = 0;
  for (uint32_t c = 0; c < n; c += kT) {
    const uint32_t j = c + tid;
    const bool head = j % ri == 0;
    ItemMeta m;
    RecordCopy rc;
    uint32_t rec = 0;
    if (j < n) {
      bool bad = false;
      m = load_item_lcp<kOW>(P, s, j, ri, bad);
      rec = (uint32_t)item_record_len(P, m, head);
    }
    uint32_t tot;
    const uint32_t roff = carry + wg_excl_scan<kLW>(rec, psum, &tot);
    if (j < n) {
      rc.issue(P, m, head, p0 + roff);
      rc.store(P, m, head, img);
      if (head) store_le(img, p0 + bin_off + (j / ri) * step, roff, step);
      if (pl.hash_w) {
        const uint32_t bk = key_bucket(P, m.ko, m.klen, pl.hash_w);
        atomicMin(&hlo[bk], j / ri);
        atomicMax(&hhi[bk], j / ri);
      }
    }
    carry += tot;
    if constexpr (kLW > 1) __syncthreads();  // (psum is rewritten by the next chunk; the votes are complete)
  }
  if constexpr (kLW == 1) wave_lds_sync();  // (one wave: no barrier per chunk)
  if (tid == 0) img[p0 + pl.recs] = kTrailerMarker;
  for (uint32_t k = tid; k < pl.hash_w; k += kT) img[p0 + g.hash_off + k] = (uint8_t)bucket_byte(hlo[k], hhi[k]);
  if (wave == 0)
    write_trailer_bytes(img, p0 + g.plen - kTrailerLen, ri, step, pl.bin_len, bin_off, pl.hash_w, g.hash_off, n);
  writer_sync<kLW>();
  if (!(kDiagBuild && (P.diag & kDiagNoHash))) {
    uint64_t lo, hi;
    if constexpr (kLW == 1) xxh3_128_wave(img, p0, g.plen, &kLongSecret, lo, hi);
    else xxh3_128_workgroup<true>(img, p0, g.plen, contrib, wave, kLW, lo, hi);
    if (wave == 0) write_header_bytes(img, g.pad, P.type, lo, hi, g.plen);
  }
  writer_sync<kLW>();
  if (!(kDiagBuild && (P.diag & kDiagNoCopyOut))) copy_out_image<kT>(img, g.gdst, g.pad, g.total);
  if (tid == 0) P.status[b] = ST_OK;
  if constexpr (kLW > 1) __syncthreads();  // (the next block reuses the image)
}

// Listed medium blocks: one wave per workgroup, grid-stride over the list.
template <int kOW>
__global__ __launch_bounds__(kWave) void encode_write_list_kernel(EncodeParams P, uint32_t plan_flag) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const uint32_t count = P.list_count[0];
  for (uint32_t li = blockIdx.x; li < count; li += gridDim.x) {
    const uint32_t b = P.lists[li];
    if ((P.plans[b].step_flags >> 8) == plan_flag) write_listed_block<1, kOW>(P, b, smem, nullptr, nullptr);
  }
}

// Listed big blocks: kLW waves per block.
template <uint32_t kLW, int kOW>
__global__ __launch_bounds__(kLW * kWave) void encode_write_list_mw_kernel(EncodeParams P, uint32_t plan_flag) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  __shared__ uint32_t psum[kLW];
  __shared__ uint64_t contrib[8 * 64];
  const uint32_t count = P.list_count[0];
  for (uint32_t li = blockIdx.x; li < count; li += gridDim.x) {
    const uint32_t b = P.lists[li];
    if ((P.plans[b].step_flags >> 8) == plan_flag) write_listed_block<kLW, kOW>(P, b, smem, psum, contrib);
  }
}

// ----------------------------------------------------- E3: HBM write pass
// Blocks larger than the list kernels' 96 KiB image (data blocks up to the
// writer's 4 MiB target, writer/mod.rs:193-198), one 8-wave workgroup per
// block, straight in HBM:
//   records  thread = item, at the record offset E1 left in erec (blocks of
//            more than kGItems items) or from a workgroup scan (fewer items);
//            the shared prefix is recomputed from the keys
//   hash     hash-index votes in LDS passes of kE3HashChunk buckets
//   tail     marker, trailer (wave 0)
//   xxh3     of the bytes just written: per 64 KiB, every wave reduces KiB
//            blocks into LDS contributions, then wave 0 carries the scramble
//            chain (as decode_chunked), the tail merge and the header.
constexpr uint32_t kE3Waves = 8, kE3Threads = kE3Waves * kWave;
template <int kOW>
__global__ __launch_bounds__(kE3Threads) void encode_large_kernel(EncodeParams P) {
  __shared__ uint32_t hlo[kE3HashChunk], hhi[kE3HashChunk];
  __shared__ uint64_t contrib[8 * 64];
  __shared__ uint32_t psum[kE3Waves];
  const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1);
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  const uint32_t count = P.list_count[0];
  for (uint32_t li = blockIdx.x; li < count; li += gridDim.x) {
    const uint32_t b = P.lists[li];
    const BlockPlan pl = P.plans[b];
    if ((pl.step_flags >> 8) != kPlanHuge) continue;
    const ListedGeom g = listed_geom(P, b, pl);
    if (g.overflow) {
      if (tid == 0) P.status[b] = ST_OVERFLOW;
      continue;
    }
    const uint32_t s = g.s, n = g.n, ri = g.ri, step = g.step, p0 = g.p0, bin_off = g.bin_off;
    uint8_t* img = g.gdst;
    const bool scan = n <= kGItems;  // (uniform) else erec holds each record's offset
    const uint32_t pf = P.hb_sh ? P.pfirst[b] : 0u;  // (after E1p erec holds huge blocks' record prefixes)
    for (uint32_t j = tid; j < (scan ? kE3Threads : n); j += kE3Threads) {
      const bool head = j % ri == 0;
      ItemMeta m;
      uint32_t roff = 0;
      if (j < n) {
        bool bad = false;
        m = load_item_lcp<kOW>(P, s, j, ri, bad);
        if (!scan) roff = P.erec[s + j] - pf;  // (after E1p: the record prefix, see encode_e1p_offsets_kernel)
      }
      if (scan) {  // n <= kGItems <= kE3Threads: one pass
        uint32_t tot;
        roff = wg_excl_scan<kE3Waves>(j < n ? (uint32_t)item_record_len(P, m, head) : 0u, psum, &tot);
      }
      if (j < n) {
        RecordCopy rc;
        rc.issue(P, m, head, p0 + roff);
        rc.store(P, m, head, img);
        if (head) store_le(img, p0 + bin_off + (j / ri) * step, roff, step);
      }
    }
    hash_index_passes<kE3Threads, kOW>(P, s, n, ri, pl.hash_w, img, p0, g.hash_off, hlo, hhi);
    if (wave == 0) {
      if (lane == 0) img[p0 + pl.recs] = kTrailerMarker;
      write_trailer_bytes(img, p0 + g.plen - kTrailerLen, ri, step, pl.bin_len, bin_off, pl.hash_w, g.hash_off, n);
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");  // the block's bytes, for this workgroup's re-reads below
    __syncthreads();
    uint64_t lo, hi;
    xxh3_128_workgroup<false>(img, p0, g.plen, contrib, wave, kE3Waves, lo, hi);
    if (wave == 0) {
      write_header_bytes(img, g.pad, P.type, lo, hi, g.plen);
      if (lane == 0) P.status[b] = ST_OK;
    }
    __syncthreads();
  }
}

// ---------------------------------------- E3 across the GPU (workspace pool)
// The one-workgroup E3 above writes a 1-4 MiB block's records with 512
// threads and carries its XXH3 chain on one wave, 64 KiB at a time.  With the
// pool (lsm_encode_workspace_size_ex) the huge blocks are collected by the
// size scan and cut into units any workgroup takes:
//   plan     (one workgroup) per collected block its record units, KiB-block
//            count and the prefix sums of both; accepted blocks are re-flagged
//            kPlanHugeGpu (the one-workgroup E3 passes them over)
//   records  record units of kEHugeItems items (thread per item at its E1
//            offset; blocks of <= kGItems items: one unit with a workgroup
//            scan), then one tail unit per block (hash-index votes, marker,
//            trailer)
//            (the contributions of the KiB blocks wholly inside a unit's LDS
//            image come from the image, flagged done)
//   chain    a workgroup per block: three waves hash the KiB blocks the
//            records kernel left into the pool while the fourth runs the eight
//            accumulator chains on lanes 0..7 behind them, then the tail merge,
//            the header and the status
constexpr uint32_t kEHugeItems = 1024;  // items per record unit, at most (four per thread)
constexpr uint32_t kEHugeImg = 2 * 4 * kE3HashChunk;  // LDS image of a record unit (the tail unit's vote arrays)
constexpr uint32_t kEHugeWaves = 4, kEHugeThreads = kEHugeWaves * kWave;  // encode_huge_records_kernel's workgroup
constexpr uint32_t kEHugeWgsPerCU = 4;  // encode_huge_records_kernel's residency (4 waves per SIMD, 32 KB of LDS)

__device__ __forceinline__ uint32_t last_le_u64(const uint64_t* a, uint32_t n, uint64_t v) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a[mid] <= v) lo = mid;
    else hi = mid;
  }
  return lo;
}

// One workgroup of 1024 threads.
__global__ __launch_bounds__(1024) void encode_huge_plan_kernel(EncodeParams P) {
  __shared__ uint64_t sh[40];
  const EncHugeLayout L = enc_huge_layout(P);
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t n = min(L.hdr->count, P.huge_cap);
  if (tid == 0) sh[32] = 0, sh[33] = 0;
  __syncthreads();
  for (uint32_t c = 0; c < n; c += 1024) {
    const uint32_t i = c + tid;
    uint64_t nbk = 0, nu = 0;
    bool acc = false;
    EncHuge h{};
    if (i < n) {
      h.b = L.list[i];
      h.dst_off = P.block_off[h.b];
      const uint64_t dst_end = P.block_off[h.b + 1];
      h.s = P.starts[h.b];
      h.n = P.starts[h.b + 1] - h.s;
      h.total = (uint32_t)(dst_end - h.dst_off);
      acc = dst_end <= P.out_cap;  // (else the one-workgroup E3 reports the overflow)
      nbk = (h.total - kHdrLen - 1) / 1024;  // (payload > 96 KiB: the long path)
      // items per record unit: 7/8 of the LDS image at the block's mean record size (a unit over
      // the image goes straight to HBM and leaves its hash to the contrib kernel: the margin keeps
      // nearly every unit staged)
      const uint32_t recs = P.plans[h.b].recs;
      h.ipu = (uint32_t)min<uint64_t>(kEHugeItems, max<uint64_t>(64, (uint64_t)(kEHugeImg * 7 / 8) * h.n / max(recs, 1u)));
      h.nru = h.n <= kGItems ? 1 : (h.n + h.ipu - 1) / h.ipu;
      nu = acc ? h.nru + 1 : 0;
      nbk = acc ? nbk : 0;
    }
    const uint64_t ik = wave_incl_scan_u64(nbk), iu = wave_incl_scan_u64(nu);
    if (lane == 63) sh[wave] = ik, sh[16 + wave] = iu;
    __syncthreads();
    uint64_t bk = sh[32], bu = sh[33], tk = 0, tu = 0;
    for (uint32_t w = 0; w < 16; ++w) {
      bk += w < wave ? sh[w] : 0;
      bu += w < wave ? sh[16 + w] : 0;
      tk += sh[w];
      tu += sh[16 + w];
    }
    const uint64_t kp = bk + ik - nbk;
    if (i < n) {
      acc = acc && kp + nbk <= L.cap_kib;  // (the pool holds the contributions of a prefix of the list)
      h.nbk = (uint32_t)nbk;
      h.accepted = acc;
      h.done = 0;
      L.rec[i] = h;
      L.kpre[i] = kp;
      L.upre[i] = bu + iu - nu;
      if (acc) P.plans[h.b].step_flags = (P.plans[h.b].step_flags & 0xFF) | (kPlanHugeGpu << 8);
    }
    __syncthreads();
    if (tid == 0) sh[32] += tk, sh[33] += tu;
    __syncthreads();
  }
  if (tid == 0) {
    L.kpre[n] = sh[32];
    L.upre[n] = sh[33];
    L.hdr->total_kib = sh[32];
    L.hdr->total_units = sh[33];
    L.hdr->n3 = n;
  }
  // the records kernel's done flags start clear (the numbers of accepted blocks' KiB blocks are < cap_kib)
  const uint64_t nf = min(sh[32], L.cap_kib);
  for (uint64_t x = tid; 16 * x < nf; x += 1024) {
    if (16 * x + 16 <= nf) reinterpret_cast<u32x4*>(L.kdone)[x] = u32x4{0, 0, 0, 0};
    else
      for (uint64_t y = 16 * x; y < nf; ++y) L.kdone[y] = 0;
  }
}

// Record units (u < nru of a block) and the tail unit (u == nru).
template <int kOW>
__global__ __launch_bounds__(kEHugeThreads) __attribute__((amdgpu_waves_per_eu(4))) void encode_huge_records_kernel(EncodeParams P) {
  __shared__ __attribute__((aligned(16))) uint32_t lbuf[2 * kE3HashChunk];  // record image | vote arrays
  uint32_t* hlo = lbuf;
  uint32_t* hhi = lbuf + kE3HashChunk;
  __shared__ uint32_t psum[kEHugeWaves];
  const EncHugeLayout L = enc_huge_layout(P);
  const uint32_t n3 = L.hdr->n3;
  if (!n3) return;
  const uint64_t units = L.hdr->total_units;
  const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // a run of consecutive units per workgroup: one block search per run
  const uint64_t per = (units + gridDim.x - 1) / gridDim.x;
  const uint64_t u_begin = (uint64_t)blockIdx.x * per, u_end = min(units, u_begin + per);
  uint32_t i = u_begin < u_end ? last_le_u64(L.upre, n3, u_begin) : 0;
#ifdef LSM_DIAG  // diagnostic per-phase s_memtime totals of wave 0 (kDiagRecPhases)
  uint32_t ph_acc[8] = {}, ph_n = 0;
  uint64_t t_last = __builtin_amdgcn_s_memtime();
#define REC_PHASE(k)                                   \
  if (P.diag & kDiagRecPhases) {                                 \
    const uint64_t t_ = __builtin_amdgcn_s_memtime();  \
    ph_acc[k] += (uint32_t)(t_ - t_last);              \
    t_last = t_;                                       \
  }
#else
#define REC_PHASE(k)
#endif
  for (uint64_t u = u_begin; u < u_end; ++u) {
    REC_PHASE(6);
    while (i + 1 < n3 && gload(L.upre, i + 1) <= u) ++i;
    const EncHuge h = gload_pod(L.rec, i);
    if (!h.accepted) continue;  // (uniform; rejected blocks own no units)
    const uint32_t k = (uint32_t)(u - gload(L.upre, i));
    const BlockPlan pl = gload_pod(P.plans, h.b);
    const uint32_t ri = is_index(P) ? 1 : P.ri;
    REC_PHASE(0);
    if (k < h.nru) {
      // (the geometry is built in each arm, not once above them: built there, this kernel, which is
      // held to 128 VGPRs, spilled 32 bytes per lane more)
      const ListedGeom g = listed_geom(P, h, pl);
      const uint32_t step = g.step, p0 = g.p0, bin_off = g.bin_off;
      uint8_t* img = g.gdst;
      if (h.n <= kGItems) {  // one pass: record offsets from a workgroup scan
        const uint32_t j = tid;
        const bool head = j % ri == 0;
        ItemMeta m;
        bool bad = false;
        if (j < h.n) m = load_item_lcp<kOW>(P, h.s, j, ri, bad);
        uint32_t tot;
        const uint32_t rec = j < h.n ? (uint32_t)item_record_len(P, m, head) : 0u;
        const uint32_t roff = wg_excl_scan<kEHugeWaves>(rec, psum, &tot);
        if (j < h.n) {
          RecordCopy rc;
          rc.issue(P, m, head, p0 + roff);
          rc.store(P, m, head, as_gbl(img));
          if (head) store_le(as_gbl(img), p0 + bin_off + (j / ri) * step, roff, step);
        }
        __syncthreads();  // (psum is rewritten by the next unit)
      } else {
        // records [j0, j1) assembled in LDS (image bytes [a0, a0 + lend)), then copied
        // out in 16-B pieces; a unit larger than the image writes straight to HBM
        const uint32_t j0 = k * h.ipu, j1 = min(h.n, j0 + h.ipu);
        // (after E1p erec holds a huge block's record prefixes: offsets relative to its first)
        const uint32_t pf = P.hb_sh ? gload(P.pfirst, h.b) : 0u;
        const uint32_t rb = gload(P.erec, (uint64_t)h.s + j0) - pf;
        const uint32_t re = j1 < h.n ? gload(P.erec, (uint64_t)h.s + j1) - pf : pl.recs;
        const uint32_t a0 = (p0 + rb) & ~15u, lend = p0 + re - a0;
        const bool staged = lend + 32 <= kEHugeImg;  // (uniform)
        uint8_t* limg = reinterpret_cast<uint8_t*>(lbuf) - a0;  // image offset x -> LDS limg + x
        auto put = [&](auto* dst) {  // (two call sites: LDS and global stores)
          for (uint32_t j = j0 + tid; j < j1; j += 256) {
            const bool head = j % ri == 0;
            bool bad = false;
            // (after E1p the shared prefix is in hbucket: no key reads before the copy)
            ItemMeta m = P.hb_sh ? load_item<kOW>(P, (uint64_t)h.s + j, bad) : load_item_lcp<kOW>(P, h.s, j, ri, bad);
            if (P.hb_sh && !head) m.sh = gload(P.hbucket, (uint64_t)h.s + j);
            const uint32_t roff = gload(P.erec, (uint64_t)h.s + j) - pf;
            RecordCopy rc;
            rc.issue(P, m, head, p0 + roff);
            rc.store(P, m, head, dst);
            if (head) store_le(as_gbl(img), p0 + bin_off + (j / ri) * step, roff, step);
          }
        };
        if (staged) put(as_lds(limg));
        else put(as_gbl(img));
        REC_PHASE(1);
        if (staged) {
          __syncthreads();
          REC_PHASE(2);
          if (h.nbk) {  // the KiB blocks wholly inside these records: contributions from the image
            const uint32_t g0 = (rb + 1023) / 1024, g1 = min(h.nbk, re / 1024);
            if (g1 > g0) {
              const uint64_t kg = gload(L.kpre, i) + g0;
              xxh3_kib_contribs(reinterpret_cast<const uint8_t*>(lbuf), p0 + 1024 * g0 - a0, (g1 - g0) * 1024 + 1,
                                &kLongSecret, L.contrib + 8 * kg, wave, kEHugeWaves);  // (lbuf-relative: ds_read, not flat)
              for (uint32_t g = tid; g < g1 - g0; g += 256) L.kdone[kg + g] = 1;
            }
          }
          REC_PHASE(3);
          const uint32_t lo = (p0 + rb) - a0, c0 = (lo + 15) >> 4, c1 = lend >> 4;
          const u32x4* src = reinterpret_cast<const u32x4*>(lbuf);
          u32x4* dst = reinterpret_cast<u32x4*>(img + a0);
          for (uint32_t c = c0 + tid; c < c1; c += 256) copy_store16(dst + c, src[c]);
          // the partial pieces at both ends (shared with the neighbouring units' records)
          auto* gb = (__attribute__((address_space(1))) uint8_t*)(img + a0);
          const uint8_t* lb = reinterpret_cast<const uint8_t*>(lbuf);
          if (tid == 0)
            for (uint32_t x = lo; x < min(16 * c0, lend); ++x) gb[x] = lb[x];
          if (tid == kWave && c1 >= c0)
            for (uint32_t x = 16 * c1; x < lend; ++x) gb[x] = lb[x];
          __syncthreads();  // (the next unit rewrites the image)
          REC_PHASE(4);
        }
      }
#ifdef LSM_DIAG
      ++ph_n;
#endif
      continue;
    }
    // tail unit: hash-index votes (LDS passes), marker, trailer
    const ListedGeom g = listed_geom(P, h, pl);
    const uint32_t step = g.step, p0 = g.p0, bin_off = g.bin_off;
    uint8_t* img = g.gdst;
    hash_index_passes<kEHugeThreads, kOW>(P, h.s, h.n, ri, pl.hash_w, img, p0, g.hash_off, hlo, hhi);
    if (wave == 0) {
      if (lane == 0) img[p0 + pl.recs] = kTrailerMarker;
      write_trailer_bytes(img, p0 + g.plen - kTrailerLen, ri, step, pl.bin_len, bin_off, pl.hash_w, g.hash_off, h.n);
    }
    REC_PHASE(5);
  }
#ifdef LSM_DIAG
  if ((P.diag & kDiagRecPhases) && tid == 0) {
    for (int k = 0; k < 7; ++k) atomicAdd(&P.phase[k], (unsigned long long)ph_acc[k]);
    atomicAdd(&P.phase[15], (unsigned long long)ph_n);
  }
#endif
#undef REC_PHASE
}

// A four-wave workgroup per block.  Waves 1..3 hash the KiB blocks the records
// kernel left (kdone clear: across two record units, into the index / trailer,
// units over the LDS image, one-pass blocks) from the written payload: helper h
// takes the 64-row chunks h, h + 3, ... in order and publishes each in LDS.
// Wave 0 runs the eight accumulator chains on lanes 0..7 (xxh3_chain8), fetching
// a chunk's rows once its helper has published it, then the tail merge, the
// header (Header::encode_into) and the status.  The contributions cross a
// kernel boundary (an agent-scope fence per unit would write back the XCD's
// whole L2).
constexpr uint32_t kEChainRing = 16;
constexpr uint32_t kEChainHelpers = 3;
__global__ __launch_bounds__(256) void encode_huge_chain_kernel(EncodeParams P) {
  __shared__ __attribute__((aligned(16))) uint8_t ring[kEChainRing * 1024];
  __shared__ uint32_t prog[4];  // helper h: 64-row chunks of this block done (h, h + 3, ... in order)
  const EncHugeLayout L = enc_huge_layout(P);
  const uint32_t n3 = L.hdr->n3;
  if (!n3) return;
  const uint32_t tid = threadIdx.x, lane = tid & 63, k = lane & 7, q = lane & 3;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (tid < 4) prog[tid] = 0;
  __syncthreads();
  for (uint32_t i = blockIdx.x; i < n3; i += gridDim.x) {
    const EncHuge* r = L.rec + i;
    if (!r->accepted) continue;  // (uniform)
    const uint32_t nbk = r->nbk;
    const uint64_t kp = L.kpre[i];
    if (wave > 0) {
      const uint32_t h = wave - 1;
      const uint64_t dabs = (uint64_t)(uintptr_t)P.out + r->dst_off;
      const uint8_t* img = reinterpret_cast<const uint8_t*>(dabs & ~15ULL);
      const uint32_t p0 = (uint32_t)(dabs & 15) + kHdrLen;
      const uint64_t k0 = kLongSecret.acc[(lane >> 2) + 2 * q], k1 = kLongSecret.acc[(lane >> 2) + 2 * q + 1];
      uint32_t done = 0;
      for (uint32_t c = h; 64 * c < nbk; c += kEChainHelpers) {
        const uint32_t g = 64 * c + lane;
        uint64_t m = __ballot(g < nbk && !L.kdone[kp + g]);
        while (m) {  // four rows at a time (independent loads and sums)
          uint32_t gs[4];
          bool live[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            live[j] = m != 0;
            gs[j] = live[j] ? 64 * c + (uint32_t)__builtin_ctzll(m) : 64 * c;
            m &= m - 1;
          }
          Win16 w[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) w[j] = live[j] ? read_win16(img, p0 + 1024 * gs[j] + 16 * lane) : Win16{0, 0};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            uint64_t c0 = 0, c1 = 0;
            stripe_part(w[j], k0, k1, c0, c1);
            c0 = quad_group_sum64(c0);
            c1 = quad_group_sum64(c1);
            if (live[j] && lane < 4) {
              L.contrib[8 * (kp + gs[j]) + 2 * q] = c0;
              L.contrib[8 * (kp + gs[j]) + 2 * q + 1] = c1;
            }
          }
        }
        vm_wait<0>();  // (the rows' stores, before the chain wave's DMA reads them)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        if (lane == 0) __hip_atomic_store(&prog[h], ++done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      __syncthreads();  // (the chain wave's end of this block)
      __syncthreads();
      continue;
    }
    uint64_t a0, a1;
    xxh3_acc_init((int)(k >> 1), a0, a1);
    uint64_t x = (k & 1) ? a1 : a0;
    // chunk qq of 16 rows lies in 64-row chunk qq / 4, helper (qq / 4) % 3's (qq / 4) / 3 + 1-th
    auto wait = [&](uint64_t qq) {
      const uint32_t c = (uint32_t)(qq / 4);
      while (__hip_atomic_load(&prog[c % kEChainHelpers], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) <
             c / kEChainHelpers + 1)
        __builtin_amdgcn_s_sleep(1);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    };
    if (nbk) x = xxh3_chain8<kEChainRing>(L.contrib + 8 * kp, nbk, x, kLongSecret.acc[16 + k], ring, wait);
    // lane quad position q takes accumulators 2q, 2q + 1 (lanes 2q, 2q + 1 hold them)
    const uint64_t c0 = wave_shfl_u64(x, (int)(2 * q)), c1 = wave_shfl_u64(x, (int)(2 * q + 1));
    const uint64_t dabs = (uint64_t)(uintptr_t)P.out + r->dst_off;
    uint8_t* img = reinterpret_cast<uint8_t*>(dabs & ~15ULL);
    const uint32_t pad = (uint32_t)(dabs & 15), plen = r->total - kHdrLen;
    uint64_t lo, hi;
    xxh3_wave_tail_merge(img, pad + kHdrLen, plen, &kLongSecret, c0, c1, lo, hi);
    write_header_bytes(img, pad, P.type, lo, hi, plen);
    if (lane == 0) P.status[r->b] = ST_OK;
    __syncthreads();  // every helper is past its last chunk of this block
    if (lane < 4) prog[lane] = 0;
    __syncthreads();
  }
}

// ------------------------------------- the other kernels that hash whole keys
// xxh3_64_long_lane (xxh3.hpp; keys of more than 240 bytes) is a __noinline__ function, and the
// device compiler specialises such a callee to the callers its unit has.  Every kernel of the encode
// path that calls it (through key_bucket or xxh3_64_any) is therefore compiled in this one unit, which
// keeps the callee, and with it the callers, as they are with the whole path in one unit: the listed
// and huge blocks' kernels above, the group kernel without plan-pass buckets, and the plan stage's
// bucket fixup (launched by launch_encode_group and launch_encode_plan).
template __global__ void encode_group_kernel<false, true, false, 4, false>(EncodeParams);
template __global__ void encode_group_kernel<false, true, false, 8, false>(EncodeParams);

// The buckets of the keys E1 left (more than 16 bytes): a wave per block,
// grid-stride; exits at once when E1 left none.
__global__ __launch_bounds__(256) void encode_bucket_fixup_kernel(EncodeParams P) {
  if (!P.hb_fix[0]) return;
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t w0 = (blockIdx.x * blockDim.x + threadIdx.x) / kWave, nw = gridDim.x * blockDim.x / kWave;
  for (uint32_t b = w0; b < P.n_blocks; b += nw) {
    // blocks E1 rejected (non-monotone or out-of-range starts, over-long keys,
    // bad value types) are skipped by E2: their hbucket entries may be stale
    if ((P.plans[b].step_flags >> 8) & kPlanBad) continue;
    const uint32_t s = P.starts[b], e = P.starts[b + 1];  // (E1 checked s < e <= n_items)
    const uint32_t n = e - s, buckets = bucket_count(n, P.ratio);
    const uint32_t hw = (buckets > 0 && (n + P.ri - 1) / P.ri <= kHashMaxPointers) ? buckets : 0;
    if (!hw || hw >= kNeedHash) continue;
    for (uint32_t i = s + lane; i < e; i += kWave) {
      if (P.hbucket[i] != kNeedHash) continue;
      const uint64_t ko = koff(P, i);
      // (E1 checked every key of a good block: <= 0xFFFF bytes; the cap is the same as E1's)
      const uint32_t klen = (uint32_t)min(koff(P, i + 1) - ko, (uint64_t)0xFFFF);
      const uint64_t hv = xxh3_64_any(klen, BaseReader8{P.it.keys + ko, 0}, BaseReader64{P.it.keys + ko, 0});
      P.hbucket[i] = (uint16_t)(hv % hw);
    }
  }
}

hipError_t launch_encode_large(const EncodeParams& P, hipStream_t st) {
  // (the cold kernels too are instantiated per offset width: a run-time width branch per
  // item load cost the 1 / 4 MiB encodes 5-6 %, profiles/r06_experiments.txt)
  return by_offset_width(P, [&](auto w) -> hipError_t {
    constexpr int kOW = decltype(w)::value;
    hipError_t e;
    static uint64_t attr_done = 0, attr_mw = 0;  // (per width: one pair per instantiation of this lambda)
    if ((e = set_lds_attr((const void*)encode_write_list_kernel<kOW>, kImgBig, &attr_done)) != hipSuccess) return e;
    if ((e = set_lds_attr((const void*)encode_write_list_mw_kernel<kListBigWaves, kOW>, kImgBig, &attr_mw)) !=
        hipSuccess)
      return e;
    // medium blocks (<= 20 KiB images): one wave each, eight workgroups per CU, was
    // faster than four waves each (2.26 vs 2.40 ms for the 16 KiB random-key class)
    hipLaunchKernelGGL(encode_write_list_kernel<kOW>, dim3(2048), dim3(kWave), kImgMedium, st, P, kPlanMedium);
    hipLaunchKernelGGL((encode_write_list_mw_kernel<kListBigWaves, kOW>), dim3(512), dim3(kListBigWaves * kWave),
                       kImgBig, st, P, kPlanBig);
    if (P.huge_pool) {  // huge blocks across the GPU (the ones it does not take stay flagged for E3 below)
      hipLaunchKernelGGL(encode_huge_plan_kernel, dim3(1), dim3(1024), 0, st, P);
      // one resident wave of record workgroups (no partly filled last wave: 256 KiB encode
      // 0.459 -> 0.424 ms against a 2048-workgroup grid)
      int n_cu = 0;
      if ((e = device_cu_count(&n_cu)) != hipSuccess) return e;
      hipLaunchKernelGGL(encode_huge_records_kernel<kOW>, dim3(kEHugeWgsPerCU * (uint32_t)n_cu), dim3(kEHugeThreads), 0,
                         st, P);
      hipLaunchKernelGGL(encode_huge_chain_kernel, dim3(min(P.n_blocks, 1024u)), dim3(256), 0, st, P);
    }
    hipLaunchKernelGGL(encode_large_kernel<kOW>, dim3(512), dim3(kE3Threads), 0, st, P);
    return hipSuccess;
  });
}

}  // namespace lsmgpu
