// conv_small.hip -- direct 3x3x3 convolution (stride 1, padding 1) for few channels (Cin, Cout <= 4).
//
// The U-Net the reference trains (MONAI UNet, 10_scripts/20_Gibbs_filters/stylized_gibbs12p5.py:192-199)
// ends in a full-resolution ResidualUnit(3, 3): a 3 -> 3 Conv3d over 2 x 240 x 240 x 160 voxels.
// With 3 channels the implicit-GEMM library kernels (CK via MIOpen) run at ~1 TFLOP/s (3.5 ms
// forward, 4.8 ms input gradient per step).  The layer is a stencil: each output needs 27 * Cin
// inputs and Cout * 27 * Cin FMAs, so a direct kernel is bound by one HBM sweep of x and y.
//
//   y[n][co][z][h][w] = b[co] + sum_{ci, tz, ty, tx} wt[co][ci][tz][ty][tx] x[n][ci][z+tz-1][h+ty-1][w+tx-1]
//
// The input gradient of the same layer is this convolution of dY with the flipped, transposed
// weights (wt'[ci][co][t] = wt[co][ci][26 - t]), prepared by the caller.
// Block = (n, z, 6 rows of h, all of w): the input tile x[ci][3 tz][8 rows][W + 2] is staged in LDS
// once; each thread owns 4 consecutive w outputs of one row for every co (12 accumulators for
// 3 -> 3), reads 6 inputs per (ci, tz, ty) row and applies 3 tx taps; the weights sit in LDS
// (every lane reads the same address: broadcast).
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "texbias.h"
#include "kernels.h"
#include "num_cu.h"

namespace {

constexpr int NT = 256;
constexpr int ROWS = 6;   // output rows (h) per block
constexpr int WPT = 4;    // consecutive w outputs per thread
constexpr int kSeg = 3;   // 64-lane segments per staged row: XP <= 192

template <int CI, int CO>
__global__ __launch_bounds__(NT) void k_conv3d_small(const float* __restrict__ x, const float* __restrict__ wt,
                                                     const float* __restrict__ bias, float* __restrict__ y, int D,
                                                     int H, int W, int XP, int nhb) {
  extern __shared__ __attribute__((aligned(16))) float xs[];  // [CI][3][ROWS + 2][XP], col 0 = w = -1
  static_assert(WPT == 4, "the input reads are one float4 + one float2");
  // weights after the input tile (broadcast LDS reads; 243 of them would spill SGPRs).  No static
  // LDS in this kernel: the dynamic base stays 16-B aligned for the float4 reads.
  float* ws = xs + CI * 3 * (ROWS + 2) * XP;
  const int tid = (int)threadIdx.x;
  for (int i = tid; i < CO * CI * 27; i += NT) ws[i] = wt[i];
  const int hb = (int)blockIdx.x % nhb, z = (int)blockIdx.x / nhb, n = (int)blockIdx.y;
  const int h0 = hb * ROWS;
  const int64_t plane = (int64_t)H * W, vol = (int64_t)D * plane;
  // stage: rows (ci, tz, r) of W floats at column 1, one wave per row (row bounds are scalar);
  // halo columns and out-of-range rows are zero
  constexpr int NR = CI * 3 * (ROWS + 2);
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  static_assert(NR % (NT / 64) == 0, "rows deal evenly to the waves");
#pragma unroll
  for (int row = wave; row < NR; row += NT / 64) {  // fully unrolled: every row's loads in flight
    const int ci = row / (3 * (ROWS + 2)), rem = row - ci * (3 * (ROWS + 2));
    const int tz = rem / (ROWS + 2), r = rem - tz * (ROWS + 2);
    const int zi = z + tz - 1, hi = h0 + r - 1;
    const bool ok = zi >= 0 && zi < D && hi >= 0 && hi < H;
    const float* src = x + ((int64_t)n * CI + ci) * vol + (ok ? (int64_t)zi * plane + (int64_t)hi * W : 0) - 1;
    float* dst = xs + row * XP;
#pragma unroll
    for (int sg = 0; sg < kSeg; ++sg) {
      const int col = lane + 64 * sg;
      const bool in = ok && col >= 1 && col <= W;
      const float v = src[in ? col : 1];
      if (col < XP) dst[col] = in ? v : 0.f;
    }
  }
  __syncthreads();
  const int tpr = (W + WPT - 1) / WPT;  // threads per output row
  const int r = tid / tpr, w0 = (tid - r * tpr) * WPT;
  if (r >= ROWS || h0 + r >= H) return;
  float acc[CO][WPT];
#pragma unroll
  for (int co = 0; co < CO; ++co) {
    const float b = bias ? bias[co] : 0.f;
#pragma unroll
    for (int k = 0; k < WPT; ++k) acc[co][k] = b;
  }
  // (ci, tz) not unrolled: only that slice's 9 * CO weights and 6 inputs per row are live
#pragma unroll 1
  for (int ct = 0; ct < CI * 3; ++ct) {
    const int ci = ct / 3, tz = ct - 3 * ci;
    {
#pragma unroll
      for (int ty = 0; ty < 3; ++ty) {
        const float* src = xs + (ct * (ROWS + 2) + r + ty) * XP + w0;  // column w0 = w0 - 1 + halo
        // 16-B aligned (XP % 4 == 0, w0 % 4 == 0): one ds_read_b128 + one ds_read_b64, no conflicts
        const float4 v4 = *reinterpret_cast<const float4*>(src);
        const float2 v2 = *reinterpret_cast<const float2*>(src + 4);
        const float v[WPT + 2] = {v4.x, v4.y, v4.z, v4.w, v2.x, v2.y};
#pragma unroll
        for (int co = 0; co < CO; ++co) {
#pragma unroll
          for (int tx = 0; tx < 3; ++tx) {
            const float wv = ws[(((co * CI + ci) * 3 + tz) * 3 + ty) * 3 + tx];
#pragma unroll
            for (int k = 0; k < WPT; ++k) acc[co][k] = fmaf(wv, v[k + tx], acc[co][k]);
          }
        }
      }
    }
  }
  const int h = h0 + r;
#pragma unroll
  for (int co = 0; co < CO; ++co) {
    float* dst = y + ((int64_t)n * CO + co) * vol + (int64_t)z * plane + (int64_t)h * W + w0;
#pragma unroll
    for (int k = 0; k < WPT; ++k)
      if (w0 + k < W) dst[k] = acc[co][k];
  }
}

// z-marching form: block = (n, zb consecutive output planes z, ROWS rows of h).  The input planes
// live in a 3-slot LDS ring ([slot][ci][ROWS + 2 rows][XP]): step z computes plane z from the slots of
// z - 1, z, z + 1 while plane z + 2 is on its way from memory into registers, and then puts it over
// plane z - 1, so every input row is read from memory once per block instead of three times (once per
// tz of each output plane).  Three slots are 48 KB at the C3 shape (3 channels, W = 160): three blocks
// per CU, where a fourth slot (no barrier between the FMAs and the LDS store) allowed two.
//
// What the step's schedule rests on:
//   * the next plane travels through registers (one wave per staged row, 4 bytes per lane, any W), is
//     not touched between its load and its LDS store at the END of the step, and takes its zeros for
//     out-of-range rows and planes in a select at that store.  (Fetched by global->LDS DMA the compiler
//     has to treat it as a pending LDS write and drains vmcnt(0) before the step's first LDS read: the
//     fetch, the residual loads and the previous step's stores were all waited for ahead of the FMAs.)
//   * the weights (scalar loads, SGPR operands of the packed FMAs) and the input rows (LDS reads) of
//     (channel, tz) group g + 1 are issued before group g's FMAs, and the one lgkmcnt(0) of a group
//     stands before that issue: scalar loads return out of order, so any wait on them is a full drain,
//     and placed there it only waits for what was issued a whole group of FMAs earlier.
//   * the outputs leave one step late, behind the next plane's loads, so the wait for those loads at
//     the LDS store never includes a store of the same step.
//   * the residual: `add == x` (RES = 2: the ResidualUnit's forward conv(x) + x and its input gradient
//     dconv(g) + g) is taken from the staged centre plane (channel co, row r + 1, columns w0 + 1 ..),
//     not loaded again; any other `add` (RES = 1) is loaded behind the plane.
#ifndef TB_SMALL_ZB
#define TB_SMALL_ZB 0
#endif
constexpr int ZB = TB_SMALL_ZB;  // output planes per block; 0: chosen per launch (zplanes below)
constexpr int NS = 3;            // ring slots: planes z - 1, z, z + 1; plane z + 2 replaces z - 1
typedef const __attribute__((address_space(4))) float* cfloat_sp;
typedef float f4v __attribute__((ext_vector_type(4)));
typedef float f2v __attribute__((ext_vector_type(2)));

template <int CI, int CO, int RES = 0>
__global__ __launch_bounds__(NT) void k_conv3d_small_z(const float* __restrict__ x, const float* __restrict__ wt,
                                                       const float* __restrict__ bias, float* __restrict__ y, int D,
                                                       int H, int W, int XP, int nhb, const float* __restrict__ add,
                                                       int vec, int zb) {
  static_assert(RES != 2 || CI == CO, "the aliased residual is the input itself");
  extern __shared__ __attribute__((aligned(16))) float xs[];  // [NS slots][CI][ROWS + 2][XP], col 0 = w = -1
  constexpr int RS = ROWS + 2, NR = CI * RS, NW = NT / 64;   // staged rows per plane, waves
  constexpr int NJ = NR / NW;                                // staged rows per wave
  constexpr int NG = CI * 3, GW = CO * 9;                    // (channel, tz) groups; weights per group
  static_assert(NR % NW == 0, "rows deal evenly to the waves");
  const int slot_f = CI * RS * XP;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int i = tid; i < NS * slot_f / 4; i += NT)  // XP % 4 == 0; halo columns stay zero
    reinterpret_cast<f4v*>(xs)[i] = f4v{0.f, 0.f, 0.f, 0.f};
  const int hb = (int)blockIdx.x % nhb, z0 = ((int)blockIdx.x / nhb) * zb, n = (int)blockIdx.y;
  const int h0 = hb * ROWS;
  const int64_t plane = (int64_t)H * W, vol = (int64_t)D * plane;
  const int zend = z0 + zb < D ? z0 + zb : D;
  // plane zi -> registers: row wave + NW j (channel j / 2, staged row wave + NW (j % 2)), columns
  // lane + 64 sg.  Every address is clamped into the tensor (plane, row and column) and every LDS store
  // below is unconditional, so no load or wait sits under a branch of its own: a load whose wait the
  // compiler sees skipped on some path is waited for wherever its register is next reused.
  static_assert(RS == 2 * NW, "a wave's rows: two per channel");
  int hoff[2], cof[kSeg], lcol[kSeg];
  unsigned lm[2][kSeg];  // all ones where (row, column) is inside the tensor
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int hi = h0 + wave + NW * q - 1;
#pragma unroll
    for (int sg = 0; sg < kSeg; ++sg) lm[q][sg] = ((hi >= 0) & (hi < H) & (lane + 64 * sg < W)) ? ~0u : 0u;
    hoff[q] = (hi < 0 ? 0 : hi >= H ? H - 1 : hi) * W;  // < H W <= 2^31 / 4 elements (launcher)
  }
#pragma unroll
  for (int sg = 0; sg < kSeg; ++sg) {
    cof[sg] = lane + 64 * sg < W ? lane + 64 * sg : W - 1;
    lcol[sg] = lane + 64 * sg < W ? lane + 64 * sg : XP - 2;
  }
  const float* xn = x + (int64_t)n * CI * vol;
  // (a plane past zend is not needed: its loads stay, all at the sample's first element -- one line --
  // so that no load and no LDS store of the march sits under a branch)
  auto load = [&](int zi, float (&rg)[NJ][kSeg]) {
    const bool need = zi <= zend;
    const float* xz = xn + (need ? (int64_t)(zi < 0 ? 0 : zi >= D ? D - 1 : zi) * plane : 0);
    const int64_t cv = need ? vol : 0;
    const int nm = need ? ~0 : 0;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const float* src = xz + (int64_t)(j >> 1) * cv + (hoff[j & 1] & nm);
#pragma unroll
      for (int sg = 0; sg < kSeg; ++sg) rg[j][sg] = src[cof[sg] & nm];
    }
  };
  // ... -> ring slot (zi - z0 + 1) % NS, zeros for rows and planes outside the tensor; the lanes past W
  // write a zero to column XP - 1, which nothing reads (the last thread's 6-wide read ends at W + 4)
  auto store = [&](int zi, const float (&rg)[NJ][kSeg]) {
    float* sl = xs + ((zi - z0 + 1) % NS) * slot_f + 1;
    const unsigned zm = ((zi >= 0) & (zi < D)) ? ~0u : 0u;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      float* dst = sl + (wave + NW * j) * XP;
#pragma unroll
      for (int sg = 0; sg < kSeg; ++sg)  // the zero-select as a bit mask: no branch, no wait but the value's own
        dst[lcol[sg]] = __uint_as_float(__float_as_uint(rg[j][sg]) & lm[j & 1][sg] & zm);
    }
  };
  float ra[NJ][kSeg], rb[NJ][kSeg], rc[NJ][kSeg];
  __syncthreads();  // zero fill before any plane store
  load(z0 - 1, ra);
  load(z0, rb);
  load(z0 + 1, rc);  // (z0 + 1 may be past D: clamped here, zeroed at the store)
  store(z0 - 1, ra);
  store(z0, rb);
  store(z0 + 1, rc);
  __syncthreads();
  const int tpr = (W + WPT - 1) / WPT;
  const int r = tid / tpr, w0 = (tid - r * tpr) * WPT;
  const bool act = r < ROWS && h0 + r < H;
  const int h = h0 + r;
  float bv[CO];
#pragma unroll
  for (int co = 0; co < CO; ++co) bv[co] = bias ? bias[co] : 0.f;
  const cfloat_sp wc = (cfloat_sp)wt;
  // group g = (ci, tz): its CO x 9 weights and the thread's 3 rows of 6 inputs
  auto issue = [&](int g, int zr, float (&wg)[GW], float (&vg)[3][WPT + 2]) {
    const int ci = g / 3, tz = g - 3 * ci;
#pragma unroll
    for (int co = 0; co < CO; ++co)
#pragma unroll
      for (int t = 0; t < 9; ++t) wg[co * 9 + t] = wc[((co * CI + ci) * 3 + tz) * 9 + t];
    const float* base = xs + ((zr + tz) % NS) * slot_f + (ci * RS + r) * XP + w0;  // column w0 = w0 - 1 + halo
#pragma unroll
    for (int ty = 0; ty < 3; ++ty) {
      // 16-B aligned (XP % 4 == 0, w0 % 4 == 0): one ds_read_b128 + one ds_read_b64, no conflicts
      const f4v v4 = *reinterpret_cast<const f4v*>(base + ty * XP);
      const f2v v2 = *reinterpret_cast<const f2v*>(base + ty * XP + 4);
      vg[ty][0] = v4.x, vg[ty][1] = v4.y, vg[ty][2] = v4.z, vg[ty][3] = v4.w, vg[ty][4] = v2.x, vg[ty][5] = v2.y;
    }
  };
  float prev[CO][WPT];
  auto put = [&](int zp) {
#pragma unroll
    for (int co = 0; co < CO; ++co) {
      float* o = y + ((int64_t)n * CO + co) * vol + (int64_t)zp * plane + (int64_t)h * W + w0;
      if (vec) {  // W % 4 == 0 and y 16-B aligned
        *reinterpret_cast<f4v*>(o) = f4v{prev[co][0], prev[co][1], prev[co][2], prev[co][3]};
      } else {
#pragma unroll
        for (int k = 0; k < WPT; ++k)
          if (w0 + k < W) o[k] = prev[co][k];
      }
    }
  };
  // step z: load plane z + 2 | (RES 1: load the residual) | store step z - 1's outputs | FMAs of plane z |
  // barrier | LDS store of plane z + 2 over plane z - 1 | barrier
  for (int z = z0; z < zend; ++z) {
    load(z + 2, ra);
    if (act) {
      float res[CO][WPT];
      if (RES == 1) {
#pragma unroll
        for (int co = 0; co < CO; ++co) {
          const float* s = add + ((int64_t)n * CO + co) * vol + (int64_t)z * plane + (int64_t)h * W + w0;
#pragma unroll
          for (int k = 0; k < WPT; ++k) res[co][k] = s[w0 + k < W ? k : 0];  // columns past W are not stored
        }
      }
      if (z > z0) put(z - 1);
      float acc[CO][WPT];
#pragma unroll
      for (int co = 0; co < CO; ++co)
#pragma unroll
        for (int k = 0; k < WPT; ++k) acc[co][k] = bv[co];
      float wg[2][GW], vg[2][3][WPT + 2];
      issue(0, z - z0, wg[0], vg[0]);
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const int ci = g / 3, tz = g - 3 * ci;
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): group g's operands, issued a group ago
        __builtin_amdgcn_sched_barrier(0);
        if (g + 1 < NG) issue(g + 1, z - z0, wg[(g + 1) & 1], vg[(g + 1) & 1]);  // (no load past the last group)
        __builtin_amdgcn_sched_barrier(0);
        const float(&w)[GW] = wg[g & 1];
        const float(&v)[3][WPT + 2] = vg[g & 1];
#pragma unroll
        for (int ty = 0; ty < 3; ++ty)
#pragma unroll
          for (int co = 0; co < CO; ++co)
#pragma unroll
            for (int tx = 0; tx < 3; ++tx)
#pragma unroll
              for (int k = 0; k < WPT; ++k) acc[co][k] = fmaf(w[co * 9 + ty * 3 + tx], v[ty][k + tx], acc[co][k]);
        if (RES == 2 && tz == 1) {  // the centre plane's row r + 1, columns w0 + 1 ..: x[ci] at the outputs
#pragma unroll
          for (int k = 0; k < WPT; ++k) res[ci < CO ? ci : 0][k] = v[1][k + 1];
        }
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int co = 0; co < CO; ++co)
#pragma unroll
        for (int k = 0; k < WPT; ++k) prev[co][k] = RES ? acc[co][k] + res[co][k] : acc[co][k];
    }
    __syncthreads();  // every wave is done with plane z - 1
    store(z + 2, ra);
    __syncthreads();
  }
  if (act) put(zend - 1);
}

__global__ __launch_bounds__(256) void k_add_inplace(float* __restrict__ y, const float* __restrict__ a, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) y[i] += a[i];
}

// Output planes per block of the z-march: `base` blocks per z segment, `per_cu` blocks resident per CU.
// A block of l planes takes about l + 2 plane steps (its first three planes arrive together); the
// segments run in rounds of per_cu x CUs blocks, and the fewest steps over all rounds win (C3: 27 planes,
// 720 blocks in one round of 768; the fixed 8 planes were 2400 blocks in four rounds).  No segment is
// shorter than 8 planes (or D): a block reads l + 2 planes for l, and the model does not count traffic.
int zplanes(int D, int base, int per_cu) {
  const int slots = (per_cu < 1 ? 1 : per_cu) * tb::num_cu();
  int best = 1 << 30, zl = D;
  for (int l = D; l >= (D < 8 ? D : 8); --l) {
    const int zs = (D + l - 1) / l, rounds = (base * zs + slots - 1) / slots, cost = rounds * (l + 2);
    if (cost < best) best = cost, zl = l;
  }
  return zl;
}

template <int CI, int CO>
int launch(const float* x, const float* w, const float* b, const float* add, float* y, int N, int D, int H, int W,
           hipStream_t st) {
  const int XP = (W + 2 + WPT + 3) / 4 * 4;  // halo, slack for the last thread's 6-wide read, 16-B rows
  const size_t lds = sizeof(float) * ((size_t)CI * 3 * (ROWS + 2) * XP + CO * CI * 27);
  if ((W + WPT - 1) / WPT * ROWS > NT || lds > 65536 || XP > 64 * kSeg || (int64_t)H * W > (1 << 29))
    return TB_ERR_UNSUPPORTED_SIZE;
  const int nhb = (H + ROWS - 1) / ROWS;
  const size_t lds_z = sizeof(float) * ((size_t)NS * CI * (ROWS + 2) * XP);
  if (lds_z <= 65536 * 2) {  // z-march
    void (*kern)(const float*, const float*, const float*, float*, int, int, int, int, int, const float*, int, int) =
        k_conv3d_small_z<CI, CO, 0>;
    if (add) kern = k_conv3d_small_z<CI, CO, 1>;
    if constexpr (CI == CO)
      if (add == x) kern = k_conv3d_small_z<CI, CO, 2>;  // conv(x) + x: the residual is the staged input
    if (tb::allow_full_lds(kern) != hipSuccess) return TB_ERR_HIP;  // once per kernel (kernels.h)
    const int vec = W % 4 == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0;  // 16-byte output stores
    const int zb = ZB ? ZB : zplanes(D, N * nhb, (int)(163840 / lds_z));
    hipLaunchKernelGGL(kern, dim3((unsigned)(nhb * ((D + zb - 1) / zb)), (unsigned)N), dim3(NT), lds_z, st, x, w, b, y,
                       D, H, W, XP, nhb, add, vec, zb);
    return hipGetLastError() == hipSuccess ? TB_OK : TB_ERR_HIP;
  }
  hipLaunchKernelGGL((k_conv3d_small<CI, CO>), dim3((unsigned)(nhb * D), (unsigned)N), dim3(NT), lds, st, x, w, b, y,
                     D, H, W, XP, nhb);
  if (add) {  // the plane-per-block kernel has no residual epilogue: a separate y += add pass
    const int64_t n = (int64_t)N * CO * D * H * W;
    hipLaunchKernelGGL(k_add_inplace, dim3((unsigned)((n + 1023) / 1024 < 8192 ? (n + 1023) / 1024 : 8192)), dim3(256),
                       0, st, y, add, n);
  }
  return hipGetLastError() == hipSuccess ? TB_OK : TB_ERR_HIP;
}

}  // namespace

int tb_conv3d_small_f32(const float* x, const float* w, const float* b, float* y, int N, int Cin, int Cout, int D,
                        int H, int W, void* stream) {
  return tb_conv3d_small_add_f32(x, w, b, nullptr, y, N, Cin, Cout, D, H, W, stream);
}

int tb_conv3d_small_add_f32(const float* x, const float* w, const float* b, const float* add, float* y, int N, int Cin,
                            int Cout, int D, int H, int W, void* stream) {
  if (!x || !w || !y || N < 1 || D < 1 || H < 1 || W < 1 || N > 65535) return TB_ERR_INVALID_ARG;
  if (Cin < 1 || Cin > 4 || Cout < 1 || Cout > 4) return TB_ERR_UNSUPPORTED_SIZE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define TB_CASE(ci, co) \
  if (Cin == ci && Cout == co) return launch<ci, co>(x, w, b, add, y, N, D, H, W, st);
#define TB_ROW(ci) TB_CASE(ci, 1) TB_CASE(ci, 2) TB_CASE(ci, 3) TB_CASE(ci, 4)
  TB_ROW(1) TB_ROW(2) TB_ROW(3) TB_ROW(4)
#undef TB_ROW
#undef TB_CASE
  return TB_ERR_UNSUPPORTED_SIZE;
}
