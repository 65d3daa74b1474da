// k_radial_grad / k_radial_power -- shell-binned reductions of the spectrum (radial.h): per (slot, run of
// tiles of spectrum columns), one H transform of the tile(s) in LDS, Re(X conj G) -- |X|^2 for the power
// spectrum -- accumulated over the launch group's volumes in registers, then reduced into the K radial
// bins in a fixed order (values written back over the tile, thread k scans the groups of entries that
// can hold bin k, in float64).  No dM is stored, no floating-point atomics.  Per radix set (-DTB_RS).
// k_radial_sum -- the partials of each (slot, k) added in unit order in float64, scaled, written as float32.
// k_radial_expand, k_radial_bin -- the dense pair: profile -> centred mask, real centred array -> bins.
// Resource report (scripts/resource_usage.py), next to k_kspace_maskgrad's 226 VGPRs and two workgroups
// per CU: k_radial_grad 233 VGPRs, k_radial_power 187 (radix set 1), no scratch, two workgroups per CU
// each; the dense kernels use at most 32 VGPRs.
#include "kernels.h"

namespace tb {
namespace {
template <int NT, int RS>
__global__ __launch_bounds__(NT) void k_radial_grad(RadialArgs) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const RadialArgs& a = kargs<RadialArgs>();
  DevCtx ctx{(int)threadIdx.x, NT};
  cf xa[MG_NE], ga[MG_NE];
  float acc[MG_NE];
  radial_unit<DevCtx, RS, MG_NE, true, false>(ctx, reinterpret_cast<cf*>(smem), a, (int)blockIdx.y, (int)blockIdx.x,
                                              (int)gridDim.y, MG_NE, xa, ga, acc);
}
template <int NT, int RS>
__global__ __launch_bounds__(NT) void k_radial_power(RadialArgs) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const RadialArgs& a = kargs<RadialArgs>();
  DevCtx ctx{(int)threadIdx.x, NT};
  cf xa[MG_NE];
  float acc[MG_NE];
  radial_unit<DevCtx, RS, MG_NE, true, true>(ctx, reinterpret_cast<cf*>(smem), a, (int)blockIdx.y, (int)blockIdx.x,
                                             (int)gridDim.y, MG_NE, xa, nullptr, acc);
}

#if TB_RS == 0
constexpr int NT_RSUM = 256;  // RSUM_SEG runs x 16 outputs
__global__ __launch_bounds__(NT_RSUM) void k_radial_sum(RadialSumArgs a) {
  __shared__ double red[RSUM_SEG][NT_RSUM / RSUM_SEG];
  const int jj = threadIdx.x % (NT_RSUM / RSUM_SEG), seg = threadIdx.x / (NT_RSUM / RSUM_SEG);
  const int j = (int)blockIdx.x * (NT_RSUM / RSUM_SEG) + jj;
  red[seg][jj] = j < a.n ? radial_sum_seg(a, j, seg) : 0.0;
  __syncthreads();
  if (seg == 0 && j < a.n) {
    double s = 0.0;
    for (int q = 0; q < RSUM_SEG; ++q) s += red[q][jj];
    radial_sum_store(a, j, s);
  }
}

__global__ __launch_bounds__(NT_TILE) void k_radial_bin(RadialDenseArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  DevCtx ctx{(int)threadIdx.x, NT_TILE};
  RadEnt* ent = reinterpret_cast<RadEnt*>(smem);
  double* bins = reinterpret_cast<double*>(smem + sizeof(RadEnt) * RB_CHUNK);
  RadRange* rng = reinterpret_cast<RadRange*>(bins + a.K);
  radial_bin_unit(ctx, ent, bins, rng, a, (int)blockIdx.y, (int)blockIdx.x);
}

// V elements per thread along D (V = 4: D % 4 = 0, one 16-B store)
template <int V>
__global__ __launch_bounds__(256) void k_radial_expand(RadialDenseArgs a) {
  const int64_t N = (int64_t)a.H * a.W * a.D;
  const int64_t s = ((int64_t)blockIdx.x * 256 + threadIdx.x) * V;
  if (s >= N) return;
  const int c = (int)blockIdx.y;
  const float* p = a.src + (int64_t)c * a.K;
  float* M = a.M + (int64_t)c * N;
  if (V == 4) {
    float4 v;
    v.x = radial_expand_at(a, p, s);
    v.y = radial_expand_at(a, p, s + 1);
    v.z = radial_expand_at(a, p, s + 2);
    v.w = radial_expand_at(a, p, s + 3);
    *reinterpret_cast<float4*>(M + s) = v;
  } else {
    M[s] = radial_expand_at(a, p, s);
  }
}
#endif
}  // namespace

template <int RS>
hipError_t launch_radial(const RadialArgs& a, bool self, dim3 grid, size_t lds, hipStream_t st) {
  static_assert(MG_NE * NT_TILE == MG_MAX_TILE, "tile slots per workgroup");
  if (self) {
    hipError_t e = allow_lds(k_radial_power<NT_TILE, RS>, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_radial_power<NT_TILE, RS>), grid, dim3(NT_TILE), lds, st, a);
    return hipGetLastError();
  }
  hipError_t e = allow_lds(k_radial_grad<NT_TILE, RS>, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((k_radial_grad<NT_TILE, RS>), grid, dim3(NT_TILE), lds, st, a);
  return hipGetLastError();
}
template hipError_t launch_radial<TB_RS>(const RadialArgs& a, bool self, dim3 grid, size_t lds, hipStream_t st);

#if TB_RS == 0
hipError_t launch_radial_sum(const RadialSumArgs& a, hipStream_t st) {
  constexpr int per = NT_RSUM / RSUM_SEG;
  hipLaunchKernelGGL(k_radial_sum, dim3((a.n + per - 1) / per), dim3(NT_RSUM), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_radial_bin(const RadialDenseArgs& a, int units, hipStream_t st) {
  const size_t lds = sizeof(RadEnt) * RB_CHUNK + sizeof(double) * (size_t)a.K + sizeof(RadRange) * (RB_CHUNK / RAD_GRP);
  hipError_t e = allow_lds(k_radial_bin, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_radial_bin, dim3(units, a.Cm), dim3(NT_TILE), lds, st, a);
  return hipGetLastError();
}

hipError_t launch_radial_expand(const RadialDenseArgs& a, hipStream_t st) {
  const int64_t N = (int64_t)a.H * a.W * a.D;
  if (a.D % 4 == 0) {
    hipLaunchKernelGGL(k_radial_expand<4>, dim3((unsigned)((N / 4 + 255) / 256), a.Cm), dim3(256), 0, st, a);
  } else {
    hipLaunchKernelGGL(k_radial_expand<1>, dim3((unsigned)((N + 255) / 256), a.Cm), dim3(256), 0, st, a);
  }
  return hipGetLastError();
}
#endif
}  // namespace tb
