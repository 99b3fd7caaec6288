// host_common.hpp — host-side helpers every stage's launch code shares.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "lsmgpu.h"

namespace lsmgpu {

// Diagnostic builds (-DLSM_DIAG, `make variant`) honour ablation bits in
// lsm_decode_tuning.flags / lsm_block_params.reserved that skip parts of the
// work (outputs invalid); the release library rejects them (LSM_BAD_ARG).
// The bits: decode_common.hpp (decode), encode_common.hpp (encode).
#ifdef LSM_DIAG
constexpr bool kDiagBuild = true;
#else
constexpr bool kDiagBuild = false;
#endif

// hipSuccess -> LSM_OK; else LSM_HIP_ERROR with the message kept for lsm_last_error().
int hip_status(hipError_t e, const char* where);

// The > 64 KiB dynamic-LDS attribute acts on the CURRENT device: set it once
// per device (a process may drive several GPUs, one host thread per device).
inline hipError_t set_lds_attr(const void* fn, uint32_t bytes, uint64_t* done_mask) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const uint64_t bit = dev < 64 ? 1ULL << dev : 0;
  if (bit && (__atomic_load_n(done_mask, __ATOMIC_ACQUIRE) & bit)) return hipSuccess;
  e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess && bit) __atomic_fetch_or(done_mask, bit, __ATOMIC_RELEASE);
  return e;
}

// Compute units of the current device, asked for once per device.
inline hipError_t device_cu_count(int* n_cu) {
  static int cu_count[64] = {};  // per device (benign race: every writer stores the same count)
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  *n_cu = dev < 64 ? __atomic_load_n(&cu_count[dev], __ATOMIC_RELAXED) : 0;
  if (!*n_cu) {
    if ((e = hipDeviceGetAttribute(n_cu, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess) return e;
    if (dev < 64) __atomic_store_n(&cu_count[dev], *n_cu, __ATOMIC_RELAXED);
  }
  return hipSuccess;
}

// The block handle (off, size) holds a header and lies in a file of file_len
// bytes: the test of both handle kernels of table_scan.hip and, on the TLI's
// handle, of the tables' entry points (load_block of table_index.hpp spells it out).
__host__ __device__ inline bool handle_in_file(uint64_t off, uint32_t size, uint64_t file_len) {
  return size >= LSM_HEADER_LEN && off + size >= off && off + size <= file_len;
}
inline bool tli_in_file(const lsm_table_scan& table, uint64_t file_len) {
  return handle_in_file(table.tli_off, table.tli_size, file_len);
}

// Workspace regions are 256-byte aligned.
constexpr size_t round256(size_t bytes) { return (bytes + 255) / 256 * 256; }

// Carves a workspace into such regions, in layout order: take() returns the
// region's byte offset from the workspace's start, total() the bytes taken.
class Carver {
 public:
  size_t take(size_t bytes) {
    const size_t o = at_;
    at_ += round256(bytes);
    return o;
  }
  size_t total() const { return at_; }

 private:
  size_t at_ = 0;
};

}  // namespace lsmgpu
