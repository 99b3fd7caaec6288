// merge.hip — Merger + CompactionStream on the device (src/merge.rs:34-100,
// src/compaction/stream.rs:46-221, InternalKey order src/key.rs:59-72): the
// step between lsm_scan_table and lsm_encode_blocks.  Sorted runs in, one
// merged, garbage-collected lsm_items-shaped SoA out.  Plain launches only: no
// atomics, no waits between workgroups.
//   0. merge_setup_kernel   one wave: run_start checked, segment bases (a
//                           segment = 64 consecutive items of one run)
//   1. merge_heads_kernel   lane per item: first 16 key bytes as two
//                           byte-swapped u64 (integer order = byte order)
//   2. merge_check_kernel   lane per item: item i - 1 <= item i inside a run
//   3. merge_split_kernel   thread per (segment, run): the segment's last item
//                           searched in the whole other run
//   4. merge_rank_kernel    wave per segment: every item searched in the other
//                           runs inside its segment's bracket; perm[pos] = i
//   5. merge_gc_kernel      lane per merged position: the per-item GC rule
//   6. three exclusive scans (keep flags, key lengths, value lengths)
//   7. merge_gather_kernel  wave per 64 merged positions: keys and values
//                           assembled in LDS and stored 16 B per lane; long
//                           values (>= kGatherLong) copied by the whole wave
// Tie rule: of two items with equal (key, seqno) the lower run comes first
// (lower bound in higher runs, upper bound in lower runs).
// lsm_merge_read (the reader's merge of per-query runs, range.rs:99-235) shares
// the heads, scan and gather stages; its own kernels are listed further down.
#include <hip/hip_runtime.h>

#include "device_common.hpp"
#include "gather.hpp"
#include "host_common.hpp"
#include "lsmgpu.h"
#include "scan.hpp"

namespace lsmgpu {

constexpr uint32_t kMergeSeg = 64;     // items per segment (splitter stride)
constexpr uint32_t kMergeWaves = 4;

struct MergeHdr {
  uint32_t bad;                            // a run_start fault: no run is looked at
  uint32_t unsorted;                       // some run is not sorted (either one: nothing is emitted)
  uint32_t pad[14];
  uint32_t seg_base[LSM_MERGE_MAX_RUNS + 1];  // first segment of each run
};

struct MergeParams {
  const uint8_t* keys;
  const uint64_t* key_off;
  const uint8_t* vals;
  const uint64_t* val_off;
  const uint64_t* seqno;
  const uint8_t* vtype;
  uint64_t n;
  const uint64_t* run_start;
  uint32_t n_runs;
  uint64_t thr;
  uint32_t flags;
  uint8_t* out_keys;
  uint64_t* out_key_off;
  uint8_t* out_vals;
  uint64_t* out_val_off;
  uint64_t* out_seqno;
  uint8_t* out_vtype;
  uint32_t* out_src;
  uint64_t* n_out;
  int32_t* status;
  // workspace
  MergeHdr* hdr;
  uint64_t* heads;   // [n][2]
  uint32_t* perm;    // [n] merged position -> input index
  uint32_t* keep;    // [n]
  uint32_t* oidx;    // [n + 1] merged position -> output index
  uint32_t* klen;    // [n] 0 when dropped
  uint32_t* vlen;    // [n]
  uint64_t* koff;    // [n + 1] output key offset of each merged position
  uint64_t* voff;    // [n + 1]
  uint32_t* table;   // [segments][n_runs] rank of each segment's last item in every run
};

// ---------------------------------------------------------------- key access
// 16 bytes at p (any alignment) from two aligned 16-byte loads (reads up to 31 bytes past p).
__device__ __forceinline__ void load16(const uint8_t* p, uint64_t& lo, uint64_t& hi) {
  const uint64_t a = (uint64_t)(uintptr_t)p;
  const u32x4* w = reinterpret_cast<const u32x4*>(a & ~15ULL);
  const u32x4 w0 = gload(w, 0), w1 = gload(w, 1);
  shift128(pack64(w0.x, w0.y), pack64(w0.z, w0.w), pack64(w1.x, w1.y), pack64(w1.z, w1.w), (uint32_t)(a & 15), lo, hi);
}
// 8 bytes at p (any alignment) from two aligned 8-byte loads (reads up to 15 bytes past p).
__device__ __forceinline__ uint64_t load8(const uint8_t* p) {
  const uint64_t a = (uint64_t)(uintptr_t)p;
  const uint64_t* w = reinterpret_cast<const uint64_t*>(a & ~7ULL);
  const uint64_t q0 = gload(w, 0), q1 = gload(w, 1);
  const uint32_t sh = (uint32_t)(a & 7) * 8;
  return sh ? (q0 >> sh) | (q1 << (64 - sh)) : q0;
}

struct MergeItem {
  uint64_t h0, h1;  // first 16 key bytes, big-endian, zero-filled past the key
  uint64_t len;
  uint64_t seq;
  const uint8_t* key;
};

__device__ __forceinline__ MergeItem load_item(const MergeParams& P, uint64_t i) {
  MergeItem x;
  const uint64_t o = gload(P.key_off, i);
  x.len = gload(P.key_off, i + 1) - o;
  x.key = P.keys + o;
  x.h0 = gload(P.heads, 2 * i);
  x.h1 = gload(P.heads, 2 * i + 1);
  x.seq = gload(P.seqno, i);
  return x;
}

// User keys of a and b beyond their (equal) heads: <0, 0, >0.
__device__ __forceinline__ int cmp_key_tail(const uint8_t* ka, uint64_t la, const uint8_t* kb, uint64_t lb) {
  const uint64_t ml = la < lb ? la : lb;
  for (uint64_t t = 16; t < ml; t += 8) {
    uint64_t a = load8(ka + t), b = load8(kb + t);
    const uint64_t rem = ml - t;
    if (rem < 8) {
      const uint64_t mask = (1ULL << (8 * rem)) - 1;
      a &= mask;
      b &= mask;
    }
    if (a != b) return __builtin_bswap64(a) < __builtin_bswap64(b) ? -1 : 1;
  }
  return la < lb ? -1 : la > lb ? 1 : 0;
}

// InternalKey order of input item m against x (key.rs:69-71): user key ascending, seqno descending.
__device__ __forceinline__ int cmp_probe(const MergeParams& P, uint64_t m, const MergeItem& x) {
  const uint64_t m0 = gload(P.heads, 2 * m), m1 = gload(P.heads, 2 * m + 1);
  if (m0 != x.h0) return m0 < x.h0 ? -1 : 1;
  if (m1 != x.h1) return m1 < x.h1 ? -1 : 1;
  const uint64_t o = gload(P.key_off, m);
  const uint64_t lm = gload(P.key_off, m + 1) - o;
  const int c = cmp_key_tail(P.keys + o, lm, x.key, x.len);
  if (c) return c;
  const uint64_t sm = gload(P.seqno, m);
  return sm > x.seq ? -1 : sm < x.seq ? 1 : 0;
}

__device__ __forceinline__ bool same_user_key(const MergeItem& a, const MergeItem& b) {
  return a.h0 == b.h0 && a.h1 == b.h1 && a.len == b.len && cmp_key_tail(a.key, a.len, b.key, b.len) == 0;
}

// Number of items of [base + lo, base + hi) before x: strictly before (lower
// bound), or before-or-equal (upper bound).  Returns lo + that count.
__device__ __forceinline__ uint32_t rank_in(const MergeParams& P, const MergeItem& x, uint64_t base, uint32_t lo,
                                            uint32_t hi, bool upper) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    const int c = cmp_probe(P, base + mid, x);
    if (upper ? c <= 0 : c < 0) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// Largest r with arr[r] <= v (arr non-decreasing, arr[0] <= v, cnt + 1 entries).
template <class T>
__device__ __forceinline__ uint32_t upper_slot(const T* arr, uint32_t cnt, uint64_t v) {
  uint32_t lo = 0, hi = cnt;  // answer in [lo, hi)
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if ((uint64_t)gload(arr, mid) <= v) lo = mid;
    else hi = mid;
  }
  return lo;
}

// ------------------------------------------------------------------ kernels
__global__ __launch_bounds__(64) void merge_setup_kernel(MergeParams P) {
  const uint32_t r = threadIdx.x;
  uint64_t s = 0, e = 0;
  bool ok = true;
  if (r < P.n_runs) {
    s = P.run_start[r];
    e = P.run_start[r + 1];
    ok = s <= e && e <= P.n && (r != 0 || s == 0) && (r + 1 != P.n_runs || e == P.n);
  }
  const bool bad = __ballot(!ok) != 0;
  const uint32_t segs = (r < P.n_runs && ok) ? (uint32_t)((e - s + kMergeSeg - 1) / kMergeSeg) : 0;
  const uint32_t incl = wave_incl_scan_u32(segs);
  if (r < P.n_runs) {
    P.status[r] = ok ? LSM_OK : LSM_BAD_ARG;
    P.hdr->seg_base[r + 1] = incl;
  }
  if (r == 0) {
    P.hdr->seg_base[0] = 0;
    P.hdr->bad = bad ? 1u : 0u;
    P.hdr->unsorted = 0;
  }
}

__global__ __launch_bounds__(256) void merge_heads_kernel(MergeParams P) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= P.n) return;
  const uint64_t o = gload(P.key_off, i);
  const uint64_t len = gload(P.key_off, i + 1) - o;
  uint64_t lo, hi;
  load16(P.keys + o, lo, hi);
  if (len < 8) lo &= (1ULL << (8 * len)) - 1;
  if (len <= 8) hi = 0;
  else if (len < 16) hi &= (1ULL << (8 * (len - 8))) - 1;
  gstore(P.heads, 2 * i, (uint64_t)__builtin_bswap64(lo));
  gstore(P.heads, 2 * i + 1, (uint64_t)__builtin_bswap64(hi));
}

__global__ __launch_bounds__(256) void merge_check_kernel(MergeParams P) {
  if (P.hdr->bad) return;
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= P.n || i == 0) return;
  const uint32_t r = upper_slot(P.run_start, P.n_runs, i);
  if (i == gload(P.run_start, r)) return;  // first item of its run
  const MergeItem x = load_item(P, i);
  if (cmp_probe(P, i - 1, x) > 0) {
    P.status[r] = LSM_BAD_ARG;
    P.hdr->unsorted = 1;
  }
}

__global__ __launch_bounds__(256) void merge_split_kernel(MergeParams P) {
  if (P.hdr->bad | P.hdr->unsorted) return;
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t g = (uint32_t)(t / P.n_runs), q = (uint32_t)(t % P.n_runs);
  if (g >= P.hdr->seg_base[P.n_runs]) return;
  const uint32_t r = upper_slot(P.hdr->seg_base, P.n_runs, g);
  if (q == r) return;
  const uint64_t rs = gload(P.run_start, r), len = gload(P.run_start, r + 1) - rs;
  const uint64_t local = min((uint64_t)(g - P.hdr->seg_base[r]) * kMergeSeg + (kMergeSeg - 1), len - 1);
  const MergeItem x = load_item(P, rs + local);
  const uint64_t qs = gload(P.run_start, q);
  const uint32_t qlen = (uint32_t)(gload(P.run_start, q + 1) - qs);
  P.table[(uint64_t)g * P.n_runs + q] = rank_in(P, x, qs, 0, qlen, q < r);
}

__global__ __launch_bounds__(kMergeWaves * 64) void merge_rank_kernel(MergeParams P) {
  if (P.hdr->bad | P.hdr->unsorted) return;
  const uint32_t g = blockIdx.x * kMergeWaves + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (g >= P.hdr->seg_base[P.n_runs]) return;
  const uint32_t r = upper_slot(P.hdr->seg_base, P.n_runs, g);
  const uint32_t s = g - P.hdr->seg_base[r];
  const uint64_t rs = gload(P.run_start, r), len = gload(P.run_start, r + 1) - rs;
  const uint64_t local = (uint64_t)s * kMergeSeg + lane;
  if (local >= len) return;
  const uint64_t i = rs + local;
  const MergeItem x = load_item(P, i);
  uint64_t pos = local;
  for (uint32_t q = 0; q < P.n_runs; ++q) {
    if (q == r) continue;
    const uint64_t qs = gload(P.run_start, q);
    const uint32_t lo = s ? gload(P.table, (uint64_t)(g - 1) * P.n_runs + q) : 0;
    const uint32_t hi = gload(P.table, (uint64_t)g * P.n_runs + q);
    pos += rank_in(P, x, qs, lo, hi, q < r);
  }
  if (pos < P.n) gstore(P.perm, pos, (uint32_t)i);
}

// The per-item form of CompactionStream::next (stream.rs:145-219): seqnos do
// not increase inside a key, so whether position j is drained, a dropped head
// or an emitted head depends on its two neighbours only.
__global__ __launch_bounds__(256) void merge_gc_kernel(MergeParams P) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= P.n) return;
  bool keep = false;
  uint32_t kl = 0, vl = 0;
  if (!(P.hdr->bad | P.hdr->unsorted)) {
    const uint32_t i = gload(P.perm, j);
    const MergeItem x = load_item(P, i);
    const uint32_t t = gload(P.vtype, (uint64_t)i);
    const bool evict = P.flags & LSM_MERGE_EVICT_TOMBSTONES;
    const bool prev_same = j > 0 && same_user_key(load_item(P, gload(P.perm, j - 1)), x);
    if (prev_same && x.seq < P.thr) {
      keep = false;  // in a drained tail
    } else {
      const bool tomb = t == LSM_TOMBSTONE || t == LSM_WEAK_TOMBSTONE;
      bool next_same = false;
      uint32_t in = 0;
      if (j + 1 < P.n) {
        in = gload(P.perm, j + 1);
        next_same = same_user_key(x, load_item(P, in));
      }
      if (!next_same) {
        keep = !(tomb && evict);
      } else if (gload(P.seqno, (uint64_t)in) < P.thr) {
        const bool drop = (t == LSM_TOMBSTONE && evict) ||
                          (t == LSM_WEAK_TOMBSTONE && gload(P.vtype, (uint64_t)in) == LSM_VALUE);
        keep = !drop;
      } else {
        keep = true;
      }
    }
    if (keep) {
      kl = (uint32_t)x.len;
      vl = (uint32_t)(gload(P.val_off, (uint64_t)i + 1) - gload(P.val_off, (uint64_t)i));
    }
  }
  gstore(P.keep, j, keep ? 1u : 0u);
  gstore(P.klen, j, kl);
  gstore(P.vlen, j, vl);
}

struct KeepOut {  // scan of the keep flags: output index of every merged position, and the count
  uint32_t* oidx;
  uint64_t* n_out;
  uint64_t n;
  __device__ void operator()(uint64_t j, uint64_t prefix) const {
    oidx[j] = (uint32_t)prefix;
    if (j == n) *n_out = prefix;
  }
};
struct OffOut {  // scan of the lengths: arena offset of every merged position, and the output's last offset
  uint64_t* woff;  // (the gather kernel copies the kept positions' offsets to the output arrays)
  uint64_t* out_off;
  const uint32_t* oidx;
  uint64_t n;
  __device__ void operator()(uint64_t j, uint64_t prefix) const {
    woff[j] = prefix;
    if (j == n) out_off[oidx[n]] = prefix;
  }
};

__global__ __launch_bounds__(kMergeWaves * 64) void merge_gather_kernel(MergeParams P) {
  __shared__ __attribute__((aligned(16))) uint8_t buf[kMergeWaves][kGatherBuf + 32];
  const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t c = ((uint64_t)blockIdx.x * kMergeWaves + w) * 64;
  if (c >= P.n) return;
  const uint64_t j = c + lane;
  const uint64_t ce = min(c + 64, P.n);
  const bool live = j < P.n && gload(P.keep, j) != 0;
  uint32_t kl = 0, vl = 0;
  uint64_t ko = 0, vo = 0;
  const uint8_t *ks = P.keys, *vs = P.vals;
  if (live) {
    const uint64_t i = gload(P.perm, j);
    const uint64_t o = gload(P.oidx, j);
    kl = gload(P.klen, j);
    vl = gload(P.vlen, j);
    ko = gload(P.koff, j);
    vo = gload(P.voff, j);
    ks = P.keys + gload(P.key_off, i);
    vs = P.vals + gload(P.val_off, i);
    const uint64_t s = gload(P.seqno, i);
    gstore(P.out_key_off, o, ko);
    gstore(P.out_val_off, o, vo);
    gstore(P.out_seqno, o, ((P.flags & LSM_MERGE_ZERO_SEQNOS) && s < P.thr) ? (uint64_t)0 : s);
    gstore(P.out_vtype, o, gload(P.vtype, i));
    if (P.out_src) gstore(P.out_src, o, (uint32_t)i);
  }
  gather_field(ks, kl, P.out_keys, ko, P.koff[c], P.koff[ce], buf[w], lane);
  gather_field(vs, vl, P.out_vals, vo, P.voff[c], P.voff[ce], buf[w], lane);
}

// ---------------------------------------------------------------- workspace
struct MergeWorkspace {
  size_t hdr, heads, perm, keep, oidx, klen, vlen, koff, voff, tiles, table, total;
  MergeWorkspace(uint64_t n_items, uint32_t n_runs) {
    const uint64_t n = n_items ? n_items : 1;
    Carver c;
    hdr = c.take(sizeof(MergeHdr));
    heads = c.take(n * 16);
    perm = c.take(n * 4);
    keep = c.take(n * 4);
    oidx = c.take((n + 1) * 4);
    klen = c.take(n * 4);
    vlen = c.take(n * 4);
    koff = c.take((n + 1) * 8);
    voff = c.take((n + 1) * 8);
    tiles = c.take(scan_tiles(n + 1) * 8);
    table = c.take((n / kMergeSeg + n_runs) * (uint64_t)n_runs * 4);
    total = c.total();
  }
};

// ------------------------------------------------- read merge (lsm_merge_read)
// Q independent merges of S runs each, with the reader's rule in place of the
// compaction's (range.rs:99-235: seqno_filter per source, Merger, MvccStream,
// the tombstone filter).  Run s * n_groups + g is source s of group g.  The heads
// kernel, the three scans and the gather kernel are the ones above (thr = 0,
// flags = 0); the kernels here stand where setup, check, split + rank and gc do:
//   read_runs_kernel    lane per run: run_start checked (a fault is the whole call's)
//   read_groups_kernel  lane per group: the group's item total, d_in_status folded
//                       into d_status[g]; then a scan gives the groups' bases
//   read_check_kernel   lane per item: item i - 1 <= item i inside a run; a fault
//                       is its group's (d_status[g], one value, plain store)
//   read_rank_kernel    lane per item: searched in the group's other runs, whole
//   read_rule_kernel    lane per merged position: visible, first visible of its
//                       key in its group, not a tombstone
//   read_starts_kernel  lane per group: d_out_group_start[g] = oidx[gbase[g]]
struct ReadParams {
  MergeParams M;  // n_runs = n_sources * n_groups, status = d_status [n_groups], n_out = &d_out_group_start[n_groups]
  uint32_t n_groups, n_sources;
  uint64_t snapshot;
  const uint64_t* group_seqno;  // or null
  const int32_t* in_status;     // or null
  uint32_t keep_tombstones;
  uint64_t* out_group_start;
  // workspace
  uint32_t* bad;    // [1] a run_start fault (zeroed by the call before read_runs_kernel)
  uint32_t* glen;   // [n_groups] items of each group
  uint32_t* gbase;  // [n_groups + 1] first merged position of each group
};

__global__ __launch_bounds__(256) void read_runs_kernel(ReadParams R) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= R.M.n_runs) return;
  const uint64_t s = gload(R.M.run_start, r), e = gload(R.M.run_start, r + 1);
  const bool ok = s <= e && e <= R.M.n && (r != 0 || s == 0) && (r + 1 != R.M.n_runs || e == R.M.n);
  if (!ok) gstore(R.bad, 0, 1u);
}

__global__ __launch_bounds__(256) void read_groups_kernel(ReadParams R) {
  const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= R.n_groups) return;
  uint64_t total = 0;
  int32_t fault = LSM_OK;
  if (gload(R.bad, 0)) {
    fault = LSM_BAD_ARG;
  } else {
    for (uint32_t s = 0; s < R.n_sources; ++s) {
      const uint64_t r = (uint64_t)s * R.n_groups + g;
      total += gload(R.M.run_start, r + 1) - gload(R.M.run_start, r);
      if (R.in_status && fault == LSM_OK) fault = gload(R.in_status, r);  // the lowest source's
    }
  }
  gstore(R.glen, g, (uint32_t)total);
  gstore(R.M.status, g, fault);
}

struct BaseOut {  // scan of the group totals
  uint32_t* gbase;
  __device__ void operator()(uint64_t g, uint64_t prefix) const { gbase[g] = (uint32_t)prefix; }
};

__global__ __launch_bounds__(256) void read_check_kernel(ReadParams R) {
  if (gload(R.bad, 0)) return;
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= R.M.n || i == 0) return;
  const uint32_t r = upper_slot(R.M.run_start, R.M.n_runs, i);
  if (i == gload(R.M.run_start, r)) return;  // first item of its run
  const uint32_t g = r % R.n_groups;
  if (gload(R.M.status, g) != LSM_OK) return;  // an input status stands; an unsorted mark is already there
  const MergeItem x = load_item(R.M, i);
  if (cmp_probe(R.M, i - 1, x) > 0) gstore(R.M.status, g, (int32_t)LSM_BAD_ARG);
}

__global__ __launch_bounds__(256) void read_rank_kernel(ReadParams R) {
  if (gload(R.bad, 0)) return;
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= R.M.n) return;
  const uint32_t r = upper_slot(R.M.run_start, R.M.n_runs, i);
  const uint32_t s = r / R.n_groups, g = r % R.n_groups;
  if (gload(R.M.status, g) != LSM_OK) return;  // nothing of a faulted group is emitted
  const MergeItem x = load_item(R.M, i);
  uint64_t pos = (uint64_t)gload(R.gbase, g) + (i - gload(R.M.run_start, r));
  for (uint32_t q = 0; q < R.n_sources; ++q) {
    if (q == s) continue;
    const uint64_t qr = (uint64_t)q * R.n_groups + g;
    const uint64_t qs = gload(R.M.run_start, qr);
    const uint32_t qlen = (uint32_t)(gload(R.M.run_start, qr + 1) - qs);
    pos += rank_in(R.M, x, qs, 0, qlen, q < s);
  }
  if (pos < R.M.n) gstore(R.M.perm, pos, (uint32_t)i);
}

// The per-item form of seqno_filter + MvccStream::next + the tombstone filter
// (range.rs:22-24,215-228, mvcc_stream.rs:45-52): seqnos do not increase inside a
// key, so a key's invisible versions come first and position j is the key's
// emitted head iff it is visible and its predecessor in the group is another
// key or invisible.
__global__ __launch_bounds__(256) void read_rule_kernel(ReadParams R) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= R.M.n) return;
  bool keep = false;
  uint32_t kl = 0, vl = 0;
  if (!gload(R.bad, 0)) {
    const uint32_t g = upper_slot(R.gbase, R.n_groups, j);
    if (gload(R.M.status, g) == LSM_OK) {
      const uint64_t snap = R.group_seqno ? gload(R.group_seqno, g) : R.snapshot;
      const uint32_t i = gload(R.M.perm, j);
      const MergeItem x = load_item(R.M, i);
      if (x.seq < snap) {
        bool head = j == gload(R.gbase, g);
        if (!head) {
          const MergeItem y = load_item(R.M, gload(R.M.perm, j - 1));
          head = !(y.seq < snap) || !same_user_key(y, x);
        }
        const uint32_t t = gload(R.M.vtype, (uint64_t)i);
        const bool tomb = t == LSM_TOMBSTONE || t == LSM_WEAK_TOMBSTONE;
        keep = head && (!tomb || R.keep_tombstones);
      }
      if (keep) {
        kl = (uint32_t)x.len;
        vl = (uint32_t)(gload(R.M.val_off, (uint64_t)i + 1) - gload(R.M.val_off, (uint64_t)i));
      }
    }
  }
  gstore(R.M.keep, j, keep ? 1u : 0u);
  gstore(R.M.klen, j, kl);
  gstore(R.M.vlen, j, vl);
}

__global__ __launch_bounds__(256) void read_starts_kernel(ReadParams R) {
  const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= R.n_groups) return;
  gstore(R.out_group_start, g, (uint64_t)gload(R.M.oidx, (uint64_t)gload(R.gbase, g)));
}

struct MergeReadWorkspace {
  size_t bad, heads, perm, keep, oidx, klen, vlen, koff, voff, tiles, glen, gbase, total;
  MergeReadWorkspace(uint64_t n_items, uint32_t n_groups, uint32_t /*n_sources*/) {
    const uint64_t n = n_items ? n_items : 1;
    const uint64_t q = n_groups ? n_groups : 1;
    Carver c;
    bad = c.take(4);
    heads = c.take(n * 16);
    perm = c.take(n * 4);
    keep = c.take(n * 4);
    oidx = c.take((n + 1) * 4);
    klen = c.take(n * 4);
    vlen = c.take(n * 4);
    koff = c.take((n + 1) * 8);
    voff = c.take((n + 1) * 8);
    tiles = c.take(scan_tiles((n > q ? n : q) + 1) * 8);
    glen = c.take(q * 4);
    gbase = c.take((q + 1) * 4);
    total = c.total();
  }
};

}  // namespace lsmgpu

using namespace lsmgpu;

extern "C" size_t lsm_merge_workspace_size(uint64_t n_items, uint32_t n_runs) {
  return MergeWorkspace(n_items, n_runs ? n_runs : 1).total;
}

extern "C" int lsm_merge_runs(const lsm_items* d_in, const uint64_t* d_run_start, uint32_t n_runs,
                              uint64_t gc_seqno_threshold, uint32_t flags, uint8_t* d_out_keys,
                              uint64_t* d_out_key_off, uint8_t* d_out_vals, uint64_t* d_out_val_off,
                              uint64_t* d_out_seqno, uint8_t* d_out_vtype, uint32_t* d_out_src, uint64_t* d_n_out,
                              int32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream) {
  if (!d_in || !d_run_start || !d_n_out || !d_status || !d_workspace) return LSM_BAD_ARG;
  if (n_runs < 1 || n_runs > LSM_MERGE_MAX_RUNS) return LSM_BAD_ARG;
  if (flags & ~(LSM_MERGE_EVICT_TOMBSTONES | LSM_MERGE_ZERO_SEQNOS)) return LSM_BAD_ARG;
  if (d_in->n_items > 0xFFFFFFFEULL) return LSM_BAD_ARG;
  if (!d_in->keys || !d_in->key_off || !d_in->vals || !d_in->val_off || !d_in->seqno || !d_in->vtype)
    return LSM_BAD_ARG;
  if (!d_out_keys || !d_out_key_off || !d_out_vals || !d_out_val_off || !d_out_seqno || !d_out_vtype)
    return LSM_BAD_ARG;
  const uint64_t n = d_in->n_items;
  const MergeWorkspace W(n, n_runs);
  if (workspace_bytes < W.total) return LSM_BAD_ARG;
  const hipStream_t st = (hipStream_t)stream;
  uint8_t* ws = (uint8_t*)d_workspace;
  MergeParams P;
  P.keys = d_in->keys;
  P.key_off = d_in->key_off;
  P.vals = d_in->vals;
  P.val_off = d_in->val_off;
  P.seqno = d_in->seqno;
  P.vtype = d_in->vtype;
  P.n = n;
  P.run_start = d_run_start;
  P.n_runs = n_runs;
  P.thr = gc_seqno_threshold;
  P.flags = flags;
  P.out_keys = d_out_keys;
  P.out_key_off = d_out_key_off;
  P.out_vals = d_out_vals;
  P.out_val_off = d_out_val_off;
  P.out_seqno = d_out_seqno;
  P.out_vtype = d_out_vtype;
  P.out_src = d_out_src;
  P.n_out = d_n_out;
  P.status = d_status;
  P.hdr = (MergeHdr*)(ws + W.hdr);
  P.heads = (uint64_t*)(ws + W.heads);
  P.perm = (uint32_t*)(ws + W.perm);
  P.keep = (uint32_t*)(ws + W.keep);
  P.oidx = (uint32_t*)(ws + W.oidx);
  P.klen = (uint32_t*)(ws + W.klen);
  P.vlen = (uint32_t*)(ws + W.vlen);
  P.koff = (uint64_t*)(ws + W.koff);
  P.voff = (uint64_t*)(ws + W.voff);
  P.table = (uint32_t*)(ws + W.table);
  uint64_t* tiles = (uint64_t*)(ws + W.tiles);
  const char* where = "lsm_merge_runs";
  hipLaunchKernelGGL(merge_setup_kernel, dim3(1), dim3(64), 0, st, P);
  if (n == 0) {  // nothing to merge: the count and the first offsets
    hipError_t e = hipMemsetAsync(d_n_out, 0, 8, st);
    if (e == hipSuccess) e = hipMemsetAsync(d_out_key_off, 0, 8, st);
    if (e == hipSuccess) e = hipMemsetAsync(d_out_val_off, 0, 8, st);
    if (e != hipSuccess) return hip_status(e, where);
    return hip_status(hipGetLastError(), where);
  }
  const uint32_t item_blocks = (uint32_t)((n + 255) / 256);
  const uint64_t segs = n / kMergeSeg + n_runs;  // bound of the segment count (it stays on the device)
  hipLaunchKernelGGL(merge_heads_kernel, dim3(item_blocks), dim3(256), 0, st, P);
  hipLaunchKernelGGL(merge_check_kernel, dim3(item_blocks), dim3(256), 0, st, P);
  if (n_runs > 1)
    hipLaunchKernelGGL(merge_split_kernel, dim3((uint32_t)((segs * n_runs + 255) / 256)), dim3(256), 0, st, P);
  hipLaunchKernelGGL(merge_rank_kernel, dim3((uint32_t)((segs + kMergeWaves - 1) / kMergeWaves)),
                     dim3(kMergeWaves * 64), 0, st, P);
  hipLaunchKernelGGL(merge_gc_kernel, dim3(item_blocks), dim3(256), 0, st, P);
  hipError_t e = launch_excl_scan(P.keep, n, tiles, KeepOut{P.oidx, d_n_out, n}, st);
  if (e == hipSuccess) e = launch_excl_scan(P.klen, n, tiles, OffOut{P.koff, d_out_key_off, P.oidx, n}, st);
  if (e == hipSuccess) e = launch_excl_scan(P.vlen, n, tiles, OffOut{P.voff, d_out_val_off, P.oidx, n}, st);
  if (e != hipSuccess) return hip_status(e, where);
  hipLaunchKernelGGL(merge_gather_kernel, dim3((uint32_t)((n + kMergeWaves * 64 - 1) / (kMergeWaves * 64))),
                     dim3(kMergeWaves * 64), 0, st, P);
  return hip_status(hipGetLastError(), where);
}

extern "C" size_t lsm_merge_read_workspace_size(uint64_t n_items, uint32_t n_groups, uint32_t n_sources) {
  return MergeReadWorkspace(n_items, n_groups, n_sources).total;
}

extern "C" int lsm_merge_read(const lsm_items* d_in, const uint64_t* d_run_start, uint32_t n_groups,
                              uint32_t n_sources, uint64_t snapshot_seqno, const uint64_t* d_group_seqno,
                              const int32_t* d_in_status, uint32_t flags, uint8_t* d_out_keys,
                              uint64_t* d_out_key_off, uint8_t* d_out_vals, uint64_t* d_out_val_off,
                              uint64_t* d_out_seqno, uint8_t* d_out_vtype, uint32_t* d_out_src,
                              uint64_t* d_out_group_start, int32_t* d_status, void* d_workspace,
                              size_t workspace_bytes, void* stream) {
  if (!d_in || !d_run_start || !d_out_group_start || !d_status || !d_workspace) return LSM_BAD_ARG;
  if (n_sources < 1 || n_sources > LSM_MERGE_MAX_RUNS) return LSM_BAD_ARG;
  if (flags & ~LSM_MERGE_READ_KEEP_TOMBSTONES) return LSM_BAD_ARG;
  const uint64_t n = d_in->n_items;
  if (n > 0xFFFFFFFEULL) return LSM_BAD_ARG;
  if (n_groups == 0 && n != 0) return LSM_BAD_ARG;
  const uint64_t n_runs = (uint64_t)n_sources * n_groups;
  if (n_runs > 0xFFFFFFFEULL) return LSM_BAD_ARG;
  if (!d_in->keys || !d_in->key_off || !d_in->vals || !d_in->val_off || !d_in->seqno || !d_in->vtype)
    return LSM_BAD_ARG;
  if (!d_out_keys || !d_out_key_off || !d_out_vals || !d_out_val_off || !d_out_seqno || !d_out_vtype)
    return LSM_BAD_ARG;
  const MergeReadWorkspace W(n, n_groups, n_sources);
  if (workspace_bytes < W.total) return LSM_BAD_ARG;
  const hipStream_t st = (hipStream_t)stream;
  const char* where = "lsm_merge_read";
  hipError_t e;
  if (n_groups == 0) {  // no query: the one entry of d_out_group_start
    if ((e = hipMemsetAsync(d_out_group_start, 0, 8, st)) != hipSuccess) return hip_status(e, where);
    return LSM_OK;
  }
  uint8_t* ws = (uint8_t*)d_workspace;
  ReadParams R;
  MergeParams& P = R.M;
  P.keys = d_in->keys;
  P.key_off = d_in->key_off;
  P.vals = d_in->vals;
  P.val_off = d_in->val_off;
  P.seqno = d_in->seqno;
  P.vtype = d_in->vtype;
  P.n = n;
  P.run_start = d_run_start;
  P.n_runs = (uint32_t)n_runs;
  P.thr = 0;
  P.flags = 0;
  P.out_keys = d_out_keys;
  P.out_key_off = d_out_key_off;
  P.out_vals = d_out_vals;
  P.out_val_off = d_out_val_off;
  P.out_seqno = d_out_seqno;
  P.out_vtype = d_out_vtype;
  P.out_src = d_out_src;
  P.n_out = d_out_group_start + n_groups;
  P.status = d_status;
  P.hdr = nullptr;
  P.heads = (uint64_t*)(ws + W.heads);
  P.perm = (uint32_t*)(ws + W.perm);
  P.keep = (uint32_t*)(ws + W.keep);
  P.oidx = (uint32_t*)(ws + W.oidx);
  P.klen = (uint32_t*)(ws + W.klen);
  P.vlen = (uint32_t*)(ws + W.vlen);
  P.koff = (uint64_t*)(ws + W.koff);
  P.voff = (uint64_t*)(ws + W.voff);
  P.table = nullptr;
  R.n_groups = n_groups;
  R.n_sources = n_sources;
  R.snapshot = snapshot_seqno;
  R.group_seqno = d_group_seqno;
  R.in_status = d_in_status;
  R.keep_tombstones = flags & LSM_MERGE_READ_KEEP_TOMBSTONES;
  R.out_group_start = d_out_group_start;
  R.bad = (uint32_t*)(ws + W.bad);
  R.glen = (uint32_t*)(ws + W.glen);
  R.gbase = (uint32_t*)(ws + W.gbase);
  uint64_t* tiles = (uint64_t*)(ws + W.tiles);
  const uint32_t group_blocks = (uint32_t)(((uint64_t)n_groups + 255) / 256);
  if ((e = hipMemsetAsync(R.bad, 0, 4, st)) != hipSuccess) return hip_status(e, where);
  hipLaunchKernelGGL(read_runs_kernel, dim3((uint32_t)((n_runs + 255) / 256)), dim3(256), 0, st, R);
  hipLaunchKernelGGL(read_groups_kernel, dim3(group_blocks), dim3(256), 0, st, R);
  if (n == 0) {  // nothing to merge: the statuses stand, every start and the first offsets are 0
    e = hipMemsetAsync(d_out_group_start, 0, ((size_t)n_groups + 1) * 8, st);
    if (e == hipSuccess) e = hipMemsetAsync(d_out_key_off, 0, 8, st);
    if (e == hipSuccess) e = hipMemsetAsync(d_out_val_off, 0, 8, st);
    if (e != hipSuccess) return hip_status(e, where);
    return hip_status(hipGetLastError(), where);
  }
  const uint32_t item_blocks = (uint32_t)((n + 255) / 256);
  e = launch_excl_scan(R.glen, n_groups, tiles, BaseOut{R.gbase}, st);
  if (e != hipSuccess) return hip_status(e, where);
  hipLaunchKernelGGL(merge_heads_kernel, dim3(item_blocks), dim3(256), 0, st, P);
  hipLaunchKernelGGL(read_check_kernel, dim3(item_blocks), dim3(256), 0, st, R);
  hipLaunchKernelGGL(read_rank_kernel, dim3(item_blocks), dim3(256), 0, st, R);
  hipLaunchKernelGGL(read_rule_kernel, dim3(item_blocks), dim3(256), 0, st, R);
  e = launch_excl_scan(P.keep, n, tiles, KeepOut{P.oidx, P.n_out, n}, st);
  if (e == hipSuccess) e = launch_excl_scan(P.klen, n, tiles, OffOut{P.koff, d_out_key_off, P.oidx, n}, st);
  if (e == hipSuccess) e = launch_excl_scan(P.vlen, n, tiles, OffOut{P.voff, d_out_val_off, P.oidx, n}, st);
  if (e != hipSuccess) return hip_status(e, where);
  hipLaunchKernelGGL(read_starts_kernel, dim3(group_blocks), dim3(256), 0, st, R);
  hipLaunchKernelGGL(merge_gather_kernel, dim3((uint32_t)((n + kMergeWaves * 64 - 1) / (kMergeWaves * 64))),
                     dim3(kMergeWaves * 64), 0, st, P);
  return hip_status(hipGetLastError(), where);
}
