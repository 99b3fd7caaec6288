// bloom.hpp — reading the standard Bloom filter image on the device
// (StandardBloomFilterReader, src/table/filter/standard_bloom/mod.rs:36-120),
// shared by bloom_contains_kernel (bloom.hip) and table_get_kernel
// (table_get.hip).
#pragma once

#include "device_common.hpp"
#include "lsmgpu.h"

namespace lsmgpu {

constexpr uint32_t kBloomHdr = LSM_BLOOM_HEADER;  // magic 4 + filter type 1 + hash type 1 + m u64 + k u64
constexpr uint64_t kBloomMaxK = LSM_BLOOM_MAX_K;

__device__ __forceinline__ uint64_t bloom_secondary(uint64_t h1) {  // builder.rs:10-13
  return (h1 >> 32) * 0x517cc1b727220a95ULL;
}

// StandardBloomFilterReader::new (mod.rs:36-86) on the image filter[0 .. len),
// len >= kBloomHdr: m and k, and whether the header is well formed and the bit
// array lies inside the image.  k is not bounded here.
__device__ __forceinline__ bool bloom_read_header(const uint8_t* __restrict__ filter, uint64_t len, uint64_t& m,
                                                  uint64_t& k) {
  m = 0;
  k = 0;
#pragma unroll
  for (int b = 7; b >= 0; --b) {
    m = (m << 8) | filter[6 + b];
    k = (k << 8) | filter[14 + b];
  }
  return filter[0] == 'L' && filter[1] == 'S' && filter[2] == 'M' && filter[3] == 3 && filter[4] == 0 &&
         filter[5] == 0 && m > 0 && (m + 7) / 8 <= len - kBloomHdr;
}

// contains_hash (mod.rs:100-120) over the bit array: k double-hashed
// positions, early exit on a clear bit.  k <= kBloomMaxK (bounded loop).
__device__ __forceinline__ bool bloom_probe(const uint8_t* __restrict__ bits, uint64_t m, uint64_t k, uint64_t h1) {
  uint64_t h2 = bloom_secondary(h1);
  for (uint64_t i = 1; i <= k; ++i) {
    const uint64_t idx = h1 % m;
    if (!(bits[idx >> 3] & (0x80u >> (idx & 7)))) return false;
    h1 += h2;
    h2 *= i;
  }
  return true;
}

}  // namespace lsmgpu
