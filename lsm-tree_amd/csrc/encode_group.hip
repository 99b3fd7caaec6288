// encode_group.hip — the group write kernel's instantiations and launch (E2); see encode.hip.
#include "encode_group.hpp"

namespace lsmgpu {

void launch_encode_group(const EncodeParams& P, bool fused, hipStream_t st) {
  const dim3 ggrid((P.n_blocks + kGRun - 1) / kGRun), gblock(kGThreads);
  // (kernels instantiated per offset width: straight-line item loads)
  by_offset_width(P, [&](auto w) {
    constexpr int kOW = decltype(w)::value;
    if (P.type == 1)
      hipLaunchKernelGGL((encode_group_kernel<true, false, false, kOW>), ggrid, gblock, 0, st, P);
    else if (P.ratio > 0.0f && P.hb_valid)  // buckets from the plan pass
      hipLaunchKernelGGL((encode_group_kernel<false, true, true, kOW>), ggrid, gblock, 0, st, P);
    else if (P.ratio > 0.0f)
      hipLaunchKernelGGL((encode_group_kernel<false, true, false, kOW>), ggrid, gblock, 0, st, P);
    else if (fused)
      hipLaunchKernelGGL((encode_group_kernel<false, false, false, kOW, true>),
                         dim3((P.n_blocks + kGRunFused - 1) / kGRunFused), gblock, 0, st, P);
    else
      hipLaunchKernelGGL((encode_group_kernel<false, false, false, kOW>), ggrid, gblock, 0, st, P);
  });
}

}  // namespace lsmgpu
