// k_kspace_export / k_kspace_import -- the centred complex spectrum out of and into the library
// (spectrum.h): per (volume, tile of spectrum columns), one H transform of the tile in LDS; the export
// stores every coefficient to f and its conjugate to -f (one write per element of K), the import gathers
// K(f) and K(-f), symmetrises and writes the tile of the half spectrum pass C reads.  Per radix set
// (-DTB_RS).  One unit per workgroup, nothing held in registers across the transform: the 32 KB tile and
// the registers leave four workgroups per CU, whose loads and stores cover each other's transforms.
// Resource report: export 109 / 121 VGPRs (radix set 0 / 1), import 119 / 176 (radix set 1: two
// workgroups per CU), no scratch.
#include "kernels.h"

namespace tb {
namespace {
template <int NT, int RS>
__global__ __launch_bounds__(NT) void k_kspace_export(SpectrumArgs) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const SpectrumArgs& a = kargs<SpectrumArgs>();
  DevCtx ctx{(int)threadIdx.x, NT};
  export_unit<DevCtx, RS>(ctx, reinterpret_cast<cf*>(smem), a, a.bc0 + (int)blockIdx.y, (int)blockIdx.x);
}

template <int NT, int RS>
__global__ __launch_bounds__(NT) void k_kspace_import(SpectrumArgs) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const SpectrumArgs& a = kargs<SpectrumArgs>();
  DevCtx ctx{(int)threadIdx.x, NT};
  import_unit<DevCtx, RS>(ctx, reinterpret_cast<cf*>(smem), a, a.bc0 + (int)blockIdx.y, (int)blockIdx.x);
}
}  // namespace

template <int RS>
hipError_t launch_kspace_export(const SpectrumArgs& a, dim3 grid, size_t lds, hipStream_t st) {
  hipError_t e = allow_lds(k_kspace_export<NT_TILE, RS>, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((k_kspace_export<NT_TILE, RS>), grid, dim3(NT_TILE), lds, st, a);
  return hipGetLastError();
}
template <int RS>
hipError_t launch_kspace_import(const SpectrumArgs& a, dim3 grid, size_t lds, hipStream_t st) {
  hipError_t e = allow_lds(k_kspace_import<NT_TILE, RS>, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((k_kspace_import<NT_TILE, RS>), grid, dim3(NT_TILE), lds, st, a);
  return hipGetLastError();
}
template hipError_t launch_kspace_export<TB_RS>(const SpectrumArgs& a, dim3 grid, size_t lds, hipStream_t st);
template hipError_t launch_kspace_import<TB_RS>(const SpectrumArgs& a, dim3 grid, size_t lds, hipStream_t st);
}  // namespace tb
