// k_kspace_maskgrad -- gradient of the TB_OP_MASK round trip with respect to the mask (maskgrad.h):
// per (mask channel slot, tile of spectrum columns), one H transform of the tiles of S_x and S_g in LDS,
// Re(X conj G) accumulated over the launch group's volumes in registers, one write per element of dM.
// Per radix set (-DTB_RS).  Resource report (both radix sets): 226 VGPRs, no scratch, two workgroups per CU
// with the next volume's loads held in registers across the transform; without them 204 VGPRs and the
// same two workgroups, so the loads in flight cost no occupancy.
// k_kspace_cmaskgrad -- the same unit for the complex mask of TB_OP_CMASK (maskgrad.h, CX): a second
// accumulator per coefficient, complex stores.  232 VGPRs, no scratch, the same tile and two workgroups per CU.
#include "kernels.h"

namespace tb {
namespace {
template <int NT, int RS>
__global__ __launch_bounds__(NT) void k_kspace_maskgrad(MaskGradArgs) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const MaskGradArgs& a = kargs<MaskGradArgs>();
  DevCtx ctx{(int)threadIdx.x, NT};
  cf xa[MG_NE], ga[MG_NE];
  float acc[MG_NE];
  maskgrad_unit<DevCtx, RS, MG_NE, true>(ctx, reinterpret_cast<cf*>(smem), a, (int)blockIdx.y, (int)blockIdx.x, MG_NE,
                                              xa, ga, acc);
}
// the complex gradient (a.cplx): the same unit with the second accumulator
template <int NT, int RS>
__global__ __launch_bounds__(NT) void k_kspace_cmaskgrad(MaskGradArgs) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const MaskGradArgs& a = kargs<MaskGradArgs>();
  DevCtx ctx{(int)threadIdx.x, NT};
  cf xa[MG_NE], ga[MG_NE];
  float acc[MG_NE], acc2[MG_NE];
  maskgrad_unit<DevCtx, RS, MG_NE, true, true>(ctx, reinterpret_cast<cf*>(smem), a, (int)blockIdx.y, (int)blockIdx.x,
                                                    MG_NE, xa, ga, acc, acc2);
}
}  // namespace

template <int RS>
hipError_t launch_kspace_maskgrad(const MaskGradArgs& a, dim3 grid, size_t lds, hipStream_t st) {
  static_assert(MG_NE * NT_TILE == MG_MAX_TILE, "tile slots per workgroup");
  if (a.cplx) {
    hipError_t e = allow_lds(k_kspace_cmaskgrad<NT_TILE, RS>, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_kspace_cmaskgrad<NT_TILE, RS>), grid, dim3(NT_TILE), lds, st, a);
    return hipGetLastError();
  }
  hipError_t e = allow_lds(k_kspace_maskgrad<NT_TILE, RS>, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((k_kspace_maskgrad<NT_TILE, RS>), grid, dim3(NT_TILE), lds, st, a);
  return hipGetLastError();
}
template hipError_t launch_kspace_maskgrad<TB_RS>(const MaskGradArgs& a, dim3 grid, size_t lds, hipStream_t st);
}  // namespace tb
