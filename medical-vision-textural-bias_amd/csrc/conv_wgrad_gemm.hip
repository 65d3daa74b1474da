// conv_wgrad_gemm.hip -- the weight gradients of the U-Net's deepest levels as one implicit GEMM on the
// f32 matrix cores.
//
// The reference's MONAI UNet (10_scripts/20_Gibbs_filters/stylized_gibbs12p5.py:192-199; module tree
// source_code/test.ipynb:754-1010) ends in a 15 x 15 x 10 level at the C3 shape: the stride-2 entry
// 64 -> 128 (twice: the unit and its residual), Conv3d 128 -> 128, the bottom unit (128 -> 256,
// 256 -> 256, a 1x1x1 128 -> 256 residual) and the ConvTranspose3d 384 -> 64 back up.  Rows of 10 floats
// give the z-marching kernels of conv_wgrad.hip nothing to march over, so these weight gradients stayed on
// MIOpen / CK (im2col + rocBLAS, NCDHW <-> NDHWC transposes around CK; ~45 TFLOP/s).  As a GEMM
//
//   dW[m][c][t] = sum_{n, o} G[n][m][o] X[n][c][S o + tap_t - pad]          (zero outside X)
//
// is D[m][j] = sum_q A[m][q] B[j][q] with rows m = G channels, columns j = (tap t, X channel c) and the
// reduction q = (n, oz, oy, ox): both operands are contiguous along q (the forward GEMM of conv_gemm.hip
// gathers one scalar per (position, channel) instead).  A ConvTranspose3d passes G = layer input, X = output
// gradient, so dW comes out as [Cin][Cout][27], the way the module holds it.
//
// A column tile holds BP channels of ONE tap, so the tap's shift and every q's validity are per (stage, q),
// never per element.  A 256-thread block computes a BM x BP tile over stages of 32 q: thread (q lane =
// tid & 31, row group = tid >> 5) loads rows rg, rg + 8, .. of both operands at its q -- a wave reads two
// 128-B row segments per load -- through buffer descriptors whose range check returns 0 for a masked q
// (offset 2^31), a row past the tensor's end, and the tail of a sample, without selects on loaded values.
// Rows past M / C inside the range read some other channel; they only feed output rows / columns that are
// never stored.  Everything after the stagers is the tile pipeline of gemm_core.h.
//
// The reduction is cut into slices of whole stages that never straddle a sample; every block writes its
// partial tile to the caller's workspace [slice][m][t C + c], and k_wgg_reduce sums the slices in order
// (deterministic, no float atomics) and transposes to [m][c][t] through LDS.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gemm_core.h"
#include "num_cu.h"
#include "texbias.h"

namespace {

using namespace tb::gemm;

constexpr int RC = 64;  // X channels per reduce block

struct WGArgs {
  const float* g;
  const float* x;
  float* part;
  float* dw;
  int64_t gsn, xsn;        // batch strides (floats)
  int64_t gbytes, xbytes;  // descriptor ranges
  int M, C, T;             // G channels, X channels, taps (27 or 1)
  int Do, Ho, Wo, Di, Hi, Wi;
  int S, pad;
  int Q, XS;               // positions per sample of G, voxels per channel of X
  int mtiles, ctiles;      // row tiles, column tiles per tap
  int sps, spb;            // slices per sample, stages per slice
  int nsplit;              // N sps
};

template <int BM, int BP>
__global__ __launch_bounds__(NTH) void k_conv_wgrad_gemm(const WGArgs a) {
  using TileT = Tile<BM, BP, 2>;
  constexpr int AR = BM / 8, BR = BP / 8;  // rows per thread per stage
  extern __shared__ __attribute__((aligned(16))) float lds_dyn[];
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ql = tid & 31, rg = tid >> 5;
  // slices slowest: one XCD's L2 then serves the few slices its blocks share
  int b = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int mt = b % a.mtiles;
  b /= a.mtiles;
  const int ct = b % a.ctiles;
  b /= a.ctiles;
  const int t = b % a.T, slice = b / a.T;
  const int n = slice / a.sps, sb = (slice - n * a.sps) * a.spb;  // first stage of the slice in sample n
  const int Q = a.Q;
  const int nst = min(a.spb, (Q + KC - 1) / KC - sb);
  const int m0 = mt * BM, c0 = ct * BP;
  const int dz = a.T == 27 ? t / 9 - a.pad : 0, dy = a.T == 27 ? (t / 3) % 3 - a.pad : 0,
            dx = a.T == 27 ? t % 3 - a.pad : 0;

  const uint32_t gbytes = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.gbytes);
  const uint32_t xbytes = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.xbytes);
  const __amdgpu_buffer_rsrc_t gr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.g), 0, (int)gbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, (int)xbytes, 0x00020000);
  // byte offsets of this thread's first row at q = 0 / voxel 0; rows 8 apart (every offset goes through the
  // descriptor's range check: the host keeps row steps and ranges below 2^30 / 2^31 bytes, so nothing wraps)
  const uint32_t abase = 4u * ((uint32_t)(n * a.gsn) + (uint32_t)(m0 + rg) * (uint32_t)Q);
  const uint32_t bbase = 4u * ((uint32_t)(n * a.xsn) + (uint32_t)(c0 + rg) * (uint32_t)a.XS);
  const uint32_t arow = 32u * (uint32_t)Q, brow = 32u * (uint32_t)a.XS;

  // the stagers' two register slots (gemm_core.h); stage s holds q = 32 (sb + s) .. + 31 of sample n, and
  // a stage past the slice or a q past the sample reads zeros
  float ra[2][AR], rb[2][BR];
  auto gload = [&](auto SL, int s) {
    constexpr int sl = decltype(SL)::value;
    const int q = (sb + s) * KC + ql;
    const bool ok = s < nst && q < Q;
    int r = q;
    const int ox = r % a.Wo;
    r /= a.Wo;
    const int oy = r % a.Ho, oz = r / a.Ho;
    const int iz = a.S * oz + dz, iy = a.S * oy + dy, ix = a.S * ox + dx;
    const bool v = ok && (unsigned)iz < (unsigned)a.Di && (unsigned)iy < (unsigned)a.Hi && (unsigned)ix < (unsigned)a.Wi;
    const uint32_t av = ok ? abase + 4u * (uint32_t)q : 0x80000000u;
    const uint32_t bv = v ? bbase + 4u * (uint32_t)((iz * a.Hi + iy) * a.Wi + ix) : 0x80000000u;
#pragma unroll
    for (int i = 0; i < AR; ++i)
      ra[sl][i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(gr, (int)(av + i * arow), 0, 0));
#pragma unroll
    for (int i = 0; i < BR; ++i)
      rb[sl][i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xr, (int)(bv + i * brow), 0, 0));
  };
  auto store = [&](auto SL) {
    constexpr int sl = decltype(SL)::value;
    float* L = lds_dyn + sl * TileT::LBUF + rg * RS + ql;
#pragma unroll
    for (int i = 0; i < AR; ++i) L[8 * i * RS] = ra[sl][i];
#pragma unroll
    for (int i = 0; i < BR; ++i) L[(BM + 8 * i) * RS] = rb[sl][i];
  };

  TileT tile(w, lane);
  __builtin_assume(nst > 0);  // a slice starts inside its sample (make_plan): no guard round the prologue
  tile.run(lds_dyn, nst, gload, store);

  // column = X channel, row = G channel
  const int M = a.M, C = a.C, J = a.T * C;
  tile.epilogue([&](int col) {
    const int c = c0 + col;
    float* dst = a.part + (int64_t)slice * M * J + t * C + c;
    return [=](int row, float v) {
      const int m = m0 + row;
      if (c < C && m < M) dst[(int64_t)m * J] = v;
    };
  });
}

// dW[m][c][t] = the slices' partials [slice][m][t C + c] summed in slice order; block (m, 64 channels):
// coalesced reads along c, the (c, t) transpose through LDS, one contiguous run of 64 T floats out
__global__ __launch_bounds__(256) void k_wgg_reduce(const WGArgs a) {
  __shared__ float sh[RC * 27];
  const int m = (int)blockIdx.x, cb = (int)blockIdx.y * RC;
  const int T = a.T, J = a.T * a.C;
  const int nc = min(RC, a.C - cb);
  const int64_t per = (int64_t)a.M * J;
  for (int i = (int)threadIdx.x; i < T * RC; i += 256) {
    const int t = i / RC, cl = i - t * RC;
    if (cl >= nc) continue;
    const float* src = a.part + (int64_t)m * J + t * a.C + cb + cl;
    float s = 0.f;
    for (int k = 0; k < a.nsplit; ++k) s += src[k * per];
    sh[cl * T + t] = s;
  }
  __syncthreads();
  float* dst = a.dw + ((int64_t)m * a.C + cb) * T;
  for (int i = (int)threadIdx.x; i < nc * T; i += 256) dst[i] = sh[i];
}

struct Plan {
  WGArgs a;
  int BM, BP;
  int64_t blocks;
  size_t part_floats;
};

// Geometry and tiling of a call (no device pointers).  force_sps > 0 overrides the planned slices per sample.
int make_plan(int N, int M, int C, int Do, int Ho, int Wo, int Di, int Hi, int Wi, int stride, int ksize,
              int force_sps, Plan& pl) {
  if (N < 1 || M < 1 || C < 1 || Do < 1 || Ho < 1 || Wo < 1 || Di < 1 || Hi < 1 || Wi < 1) return TB_ERR_INVALID_ARG;
  if ((ksize != 3 && ksize != 1) || (stride != 1 && stride != 2) || (ksize == 1 && stride != 1))
    return TB_ERR_INVALID_ARG;
  WGArgs& a = pl.a;
  a = WGArgs{};
  a.M = M, a.C = C, a.T = ksize * ksize * ksize;
  a.Do = Do, a.Ho = Ho, a.Wo = Wo, a.Di = Di, a.Hi = Hi, a.Wi = Wi;
  a.S = stride, a.pad = ksize == 3 ? 1 : 0;
  const int64_t Q = (int64_t)Do * Ho * Wo, XS = (int64_t)Di * Hi * Wi;
  // 32-bit byte offsets with room for a tile's rows past the end (see the kernel's abase / arow)
  if (Q >= (1 << 21) || XS >= (1 << 21)) return TB_ERR_UNSUPPORTED_SIZE;
  if ((int64_t)N * M * Q >= (int64_t)1 << 29 || (int64_t)N * C * XS >= (int64_t)1 << 29) return TB_ERR_UNSUPPORTED_SIZE;
  if ((int64_t)M * C * a.T >= (int64_t)1 << 31) return TB_ERR_UNSUPPORTED_SIZE;
  a.Q = (int)Q, a.XS = (int)XS;
  pl.BM = M <= 64 ? 64 : 128;
  pl.BP = C <= 64 ? 64 : 128;
  a.mtiles = (M + pl.BM - 1) / pl.BM;
  a.ctiles = (C + pl.BP - 1) / pl.BP;
  const int64_t tiles = (int64_t)a.mtiles * a.ctiles * a.T;
  const int stages = (int)((Q + KC - 1) / KC);
  // slices per sample: the most loaded CU's blocks x (stages per block + a fixed per-block cost of ~3
  // stages) at the matrix-core rate of one BM x BP stage (two blocks per CU hide each other's LDS phases,
  // one does not), plus the partials written once and read once at ~3 TB/s; ties keep the smaller split
  const int ncu = tb::num_cu();
  const double t_stage = (double)pl.BM * pl.BP * 2 * KC / 614e3;  // us at a CU's f32 MFMA peak
  const double part_us = (double)N * M * a.T * C * 8 / 3.0e6;     // per slice per sample
  double best = 1e30;
  int sps = 1;
  for (int s = 1; s <= 32 && s <= stages; ++s) {
    const int spb = (stages + s - 1) / s;
    const int se = (stages + spb - 1) / spb;
    const int64_t per_cu = (tiles * N * se + ncu - 1) / ncu;
    const double cost = (double)per_cu * (spb + 3) * t_stage / (per_cu >= 2 ? 0.8 : 0.6) + se * part_us;
    if (cost < best * 0.97) best = cost, sps = se;
  }
  if (force_sps > 0) sps = force_sps < stages ? force_sps : stages;
  a.spb = (stages + sps - 1) / sps;
  a.sps = (stages + a.spb - 1) / a.spb;
  a.nsplit = N * a.sps;
  pl.blocks = tiles * a.nsplit;
  if (pl.blocks >= (int64_t)1 << 31) return TB_ERR_UNSUPPORTED_SIZE;
  pl.part_floats = (size_t)a.nsplit * M * a.T * C;
  return TB_OK;
}

template <int BM, int BP>
hipError_t launch(const WGArgs& a, int64_t nb, hipStream_t st) {
  return launch_tile<&k_conv_wgrad_gemm<BM, BP>>(lds_bytes(BM, BP), nb, a, st);
}

}  // namespace

size_t tb_conv3d_wgrad_gemm_ws_bytes_ex(int N, int M, int C, int Do, int Ho, int Wo, int Di, int Hi, int Wi, int stride,
                                        int ksize, int sps) {
  Plan pl;
  if (make_plan(N, M, C, Do, Ho, Wo, Di, Hi, Wi, stride, ksize, sps, pl) != TB_OK) return 0;
  return 4 * pl.part_floats + 256;
}

size_t tb_conv3d_wgrad_gemm_ws_bytes(int N, int M, int C, int Do, int Ho, int Wo, int Di, int Hi, int Wi, int stride,
                                     int ksize) {
  return tb_conv3d_wgrad_gemm_ws_bytes_ex(N, M, C, Do, Ho, Wo, Di, Hi, Wi, stride, ksize, 0);
}

int tb_conv3d_wgrad_gemm_ex_f32(const float* G, int64_t gsn, const float* X, int64_t xsn, float* dW, int N, int M, int C,
                                int Do, int Ho, int Wo, int Di, int Hi, int Wi, int stride, int ksize, int sps, void* ws,
                                size_t ws_bytes, void* stream) {
  if (!G || !X || !dW) return TB_ERR_INVALID_ARG;
  Plan pl;
  const int rc = make_plan(N, M, C, Do, Ho, Wo, Di, Hi, Wi, stride, ksize, sps, pl);
  if (rc != TB_OK) return rc;
  WGArgs& a = pl.a;
  if (!ws || ws_bytes < 4 * pl.part_floats + 256) return TB_ERR_WORKSPACE;
  a.gsn = gsn > 0 ? gsn : (int64_t)M * a.Q;
  a.xsn = xsn > 0 ? xsn : (int64_t)C * a.XS;
  if (a.gsn < (int64_t)M * a.Q || a.xsn < (int64_t)C * a.XS) return TB_ERR_INVALID_ARG;
  a.gbytes = 4 * ((int64_t)(N - 1) * a.gsn + (int64_t)M * a.Q);
  a.xbytes = 4 * ((int64_t)(N - 1) * a.xsn + (int64_t)C * a.XS);
  if (a.gbytes >= (int64_t)1 << 31 || a.xbytes >= (int64_t)1 << 31) return TB_ERR_UNSUPPORTED_SIZE;
  a.g = G, a.x = X, a.dw = dW;
  a.part = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(ws) + 255) & ~uintptr_t(255));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipError_t e;
  if (pl.BM == 64 && pl.BP == 64) e = launch<64, 64>(a, pl.blocks, st);
  else if (pl.BM == 64) e = launch<64, 128>(a, pl.blocks, st);
  else if (pl.BP == 64) e = launch<128, 64>(a, pl.blocks, st);
  else e = launch<128, 128>(a, pl.blocks, st);
  if (e != hipSuccess) return TB_ERR_HIP;
  hipLaunchKernelGGL(k_wgg_reduce, dim3((unsigned)M, (unsigned)((C + RC - 1) / RC)), dim3(256), 0, st, a);
  return hipGetLastError() == hipSuccess ? TB_OK : TB_ERR_HIP;
}

int tb_conv3d_wgrad_gemm_f32(const float* G, int64_t gsn, const float* X, int64_t xsn, float* dW, int N, int M, int C,
                             int Do, int Ho, int Wo, int Di, int Hi, int Wi, int stride, int ksize, void* ws,
                             size_t ws_bytes, void* stream) {
  return tb_conv3d_wgrad_gemm_ex_f32(G, gsn, X, xsn, dW, N, M, C, Do, Ho, Wo, Di, Hi, Wi, stride, ksize, 0, ws, ws_bytes,
                                     stream);
}

int tb_conv3d_wgrad_gemm_config_ex(int N, int M, int C, int Do, int Ho, int Wo, int Di, int Hi, int Wi, int stride,
                                   int ksize, int sps, int64_t* cfg) {
  Plan pl;
  const int rc = make_plan(N, M, C, Do, Ho, Wo, Di, Hi, Wi, stride, ksize, sps, pl);
  if (rc != TB_OK || !cfg) return rc != TB_OK ? rc : TB_ERR_INVALID_ARG;
  cfg[0] = pl.BM, cfg[1] = pl.BP, cfg[2] = pl.a.nsplit, cfg[3] = (int64_t)pl.a.spb * KC, cfg[4] = pl.blocks;
  return TB_OK;
}

int tb_conv3d_wgrad_gemm_config(int N, int M, int C, int Do, int Ho, int Wo, int Di, int Hi, int Wi, int stride,
                                int ksize, int64_t* cfg) {
  return tb_conv3d_wgrad_gemm_config_ex(N, M, C, Do, Ho, Wo, Di, Hi, Wi, stride, ksize, 0, cfg);
}
