// k_kspace_ampmix / k_kspace_ampmix_bwd -- amplitude mixing in k-space and its gradients (ampmix.h): per
// (volume, tile of spectrum columns), one H transform of the tiles of S_x and S_y[partner] (and S_g) side
// by side in LDS, the per-coefficient closed form with the mask gathered at s(f) and s(-f), one inverse H
// transform of the result columns, one write per output element, no atomics.  Per radix set (-DTB_RS).
// One unit per workgroup, nothing held in registers across the transforms (as k_kspace_export /
// k_kspace_import): the next tile's loads in flight are those of the other workgroups of the CU -- the
// forward's 32 KB tile leaves four per CU by LDS, the backward's three-wide 48 KB tile three.  The
// registers allow four workgroups per CU with radix set 0 and two with radix set 1, so the three-wide tile
// costs at most one workgroup (radix set 0: three instead of four) and never goes below two; two DIF
// rounds over a two-wide tile would win that workgroup back for a second set of barriers per unit.
// Resource report (radix set 0 / 1), scratch 0 everywhere, dynamic LDS only:
//   k_kspace_ampmix               119 / 176 VGPRs, 4 / 2 waves per SIMD
//   k_kspace_ampmix_bwd, with Gy  117 / 176 VGPRs, 4 / 2 waves per SIMD
//   k_kspace_ampmix_bwd, no Gy    119 / 176 VGPRs, 4 / 2 waves per SIMD
#include "kernels.h"

namespace tb {
namespace {
template <int NT, int RS>
__global__ __launch_bounds__(NT) void k_kspace_ampmix(AmpMixArgs) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const AmpMixArgs& a = kargs<AmpMixArgs>();
  DevCtx ctx{(int)threadIdx.x, NT};
  ampmix_fwd_unit<DevCtx, RS>(ctx, reinterpret_cast<cf*>(smem), a, a.bc0 + (int)blockIdx.y, (int)blockIdx.x);
}

template <int NT, int RS, bool GY>
__global__ __launch_bounds__(NT) void k_kspace_ampmix_bwd(AmpMixArgs) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const AmpMixArgs& a = kargs<AmpMixArgs>();
  DevCtx ctx{(int)threadIdx.x, NT};
  ampmix_bwd_unit<DevCtx, RS, GY>(ctx, reinterpret_cast<cf*>(smem), a, a.bc0 + (int)blockIdx.y, (int)blockIdx.x);
}

template <class K>
hipError_t launch(K kern, const AmpMixArgs& a, dim3 grid, size_t lds, hipStream_t st) {
  hipError_t e = allow_lds(kern, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, grid, dim3(NT_TILE), lds, st, a);
  return hipGetLastError();
}
}  // namespace

template <int RS>
hipError_t launch_kspace_ampmix(const AmpMixArgs& a, dim3 grid, size_t lds, hipStream_t st) {
  return launch(k_kspace_ampmix<NT_TILE, RS>, a, grid, lds, st);
}
template <int RS>
hipError_t launch_kspace_ampmix_bwd(const AmpMixArgs& a, dim3 grid, size_t lds, hipStream_t st) {
  if (a.need_gy) return launch(k_kspace_ampmix_bwd<NT_TILE, RS, true>, a, grid, lds, st);
  return launch(k_kspace_ampmix_bwd<NT_TILE, RS, false>, a, grid, lds, st);
}
template hipError_t launch_kspace_ampmix<TB_RS>(const AmpMixArgs& a, dim3 grid, size_t lds, hipStream_t st);
template hipError_t launch_kspace_ampmix_bwd<TB_RS>(const AmpMixArgs& a, dim3 grid, size_t lds, hipStream_t st);
}  // namespace tb
