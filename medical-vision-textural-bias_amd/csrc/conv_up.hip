// conv_up.hip -- the U-Net's full-resolution stride-2 layers with few channels on one side.
//
// The reference's MONAI UNet (10_scripts/20_Gibbs_filters/stylized_gibbs12p5.py:192-199) enters with
// Conv3d(4 -> 16, stride 2) twice (the first unit and its residual) and leaves with
// ConvTranspose3d(32 -> 3, stride 2, output_padding 1).  MIOpen runs these through layout transposes
// and im2col / col2im GEMMs (467 us per forward of the entry conv, 1.17 ms for the transposed
// forward, 0.82 ms for its input gradient per C3 step).  All three are one of two stencils:
//
//   k_conv_s2_fewin    out[m][o] = b[m] + sum_{c, t} K[c][t][m] in[c][2 o + t - 1]      (c < CIN <= 4)
//     * Conv3d(4 -> 16, s2) forward: in = x, K[c][t][m] = W[m][c][t];
//     * the input gradient of ConvTranspose3d(32 -> 3, s2): in = dY (3 channels), out = dX (32),
//       K[c][t][m] = W[m][c][t] with W the transposed conv's [Cin = m][Cout = c] weight;
//   k_convT_fewout     y[m][2 j + p] = b[m] + sum_c sum_{(d, t) in S(p)} W[c][m][t] x[c][j + d]   (m < MO <= 4)
//     per axis S(0) = {(0, 1)}, S(1) = {(0, 2), (1, 0)}: the 8 output parities of one input position
//     from its 2 x 2 x 2 neighbourhood (sub-pixel form: every multiply-add is a real tap).
//
// Both march along z with the input planes staged in an LDS ring and the next step's planes in
// registers; one thread per output position (A) or input position (B) holds all output channels
// (A: its 27 CIN inputs in registers, packed FMAs per output pair; B: the 8 parities x MO channels);
// the weights are scalar loads (SGPR operands).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <type_traits>

#include "conv_host.h"
#include "split_bf16.h"
#include "texbias.h"

namespace {

typedef float f2v __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
// Weights are wave-uniform: read through the constant address space they become scalar loads and
// SGPR operands of the FMAs (as broadcast LDS reads they cost an LDS instruction per 2 FMAs: the
// first version of these kernels was LDS-bound at 8 % of the FMA rate).
typedef const __attribute__((address_space(4))) float* cfloat_p;
typedef const __attribute__((address_space(4))) f2v* cf2v_p;

// f(integral_constant<int, i>) for i = B .. N - 1: a loop that cannot stay rolled
template <int B, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (B < N) {
    f(std::integral_constant<int, B>{});
    static_for<B + 1, N>(f);
  }
}

// ------------------------------------------------------------------------------ stride-2 conv
struct S2Args {
  const float* in;
  const float* K;     // [MOUT / 2][CIN 27][2]: output channel pairs
  const float* bias;  // [MOUT] or null
  float* out;
  int Do, Ho, Wo, Di, Hi, Wi;
  int ZS, zlen, nyb;
  int PX, RR;  // LDS row pitch; rows per channel slab (2 TY + 1)
};

// NTH = 512: the two halves of the block share the positions and split the output pairs (registers of
// the 27 CIN inputs + half the accumulators: two waves per SIMD instead of one for CIN = 4, MOUT = 32)
template <int CIN, int MOUT, int TY, int WV, int NTH = 256>  // WV: most float4 per input row (Wi <= 4 WV)
__global__ __launch_bounds__(NTH) void k_conv_s2_fewin(S2Args a) {
  static_assert(MOUT % 2 == 0, "packed output pairs");
  constexpr int NHALF = NTH / 256, MP = MOUT / 2 / NHALF;  // output pairs per half
  constexpr int NR = 2 * TY + 1;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = (int)threadIdx.x;
  constexpr int PX = 4 * WV + 12, SS = CIN * NR * PX;  // row pitch (odd multiple of 4), slot stride
  // [3][CIN][NR][PX], input column xi at xi + 4: step z reads planes 2z - 1 .. 2z + 1; its first stores
  // put planes 2z, 2z + 1 over the slots of 2z - 3, 2z - 2 (three slots instead of five: 58 KB at the
  // C3 shapes, two blocks per CU)
  float* ring = smem;
  for (int i = tid; i < 3 * SS; i += NTH) ring[i] = 0.f;  // halos, padding rows stay 0
  int b = (int)blockIdx.x;
  const int zs = b % a.ZS;
  b /= a.ZS;
  const int yb = b % a.nyb, n = b / a.nyb;
  const int y0 = yb * TY;
  const int z0 = zs * a.zlen, z1 = min(a.Do, z0 + a.zlen);
  const int Di = a.Di, Hi = a.Hi, Wi = a.Wi;
  const int64_t iplane = (int64_t)Hi * Wi, iplane4 = iplane / 4;
  const float4* inb = reinterpret_cast<const float4*>(a.in + (int64_t)n * CIN * Di * iplane);
  // staging items of one plane: (c, r, q) -> input row 2 y0 - 1 + r, float4 q
  const int W4 = Wi >> 2;
  constexpr int NL = (CIN * NR * WV + NTH - 1) / NTH;
  int gof[NL], lof[NL];
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    const int i = tid + NTH * j;
    const int q = i % W4, t = i / W4, r = t % NR, c = t / NR;
    const int yi = 2 * y0 - 1 + r;
    const bool ok = c < CIN && yi >= 0 && yi < Hi;
    gof[j] = ok ? (int)((int64_t)c * Di * iplane4 + ((int64_t)yi * Wi + 4 * q) / 4) : -1;
    lof[j] = (c * NR + r) * PX + 4 + 4 * q;
  }
  float4 ra[NL], rb[NL];
  auto load = [&](int zi, float4 (&r)[NL]) {
    const bool in = zi >= 0 && zi < Di;
    const float4* src = inb + (int64_t)(in ? zi : 0) * iplane4;
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      r[j] = src[gof[j] < 0 ? 0 : gof[j]];  // zeroed at the store (a select here waits for the load)
    }
  };
  auto store = [&](int zi, const float4 (&r)[NL]) {
    float* d = ring + ((zi + 3) % 3) * SS;
    const bool in = zi >= 0 && zi < Di;
#pragma unroll
    for (int j = 0; j < NL; ++j)
      if (gof[j] >= 0) *reinterpret_cast<float4*>(d + lof[j]) = in ? r[j] : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  __syncthreads();  // zero fill before any slab store
  load(2 * z0 - 1, ra);
  store(2 * z0 - 1, ra);
  load(2 * z0, ra);
  load(2 * z0 + 1, rb);
  // this thread's output position: row y0 + oy, column ox; output pairs mh * MP .. + MP - 1
  const int pt = tid & 255, mh = __builtin_amdgcn_readfirstlane(tid >> 8);
  const int Wo = a.Wo, oy = pt / Wo, ox = pt - oy * Wo;
  const bool act = oy < TY && y0 + oy < a.Ho;
  const int roff = (2 * oy) * PX + 2 * ox + 3;  // + (ty PX + tx): input row 2 oy + ty, column 2 ox + tx - 1
  f2v bias2[MP];
#pragma unroll
  for (int mm = 0; mm < MP; ++mm) {
    const int m = mh * MP + mm;
    bias2[mm] = a.bias ? f2v{a.bias[2 * m], a.bias[2 * m + 1]} : f2v{0.f, 0.f};
  }
  const int64_t oplane = (int64_t)a.Ho * Wo;
  float* outb = a.out + (int64_t)n * MOUT * a.Do * oplane + (int64_t)(y0 + oy) * Wo + ox;
  // LATE (the 256-thread form): outputs leave one step late (pend), after the next planes' loads, so the
  // wait for those loads at the next step's LDS store never includes a store issued in the same step
  // (3 -> 32: 225 -> 212 us; the 512-thread 4 -> 32 form measured 278 -> 317 us with it: immediate stores)
  constexpr bool LATE = NTH == 256;
  f2v pend[MP];
  auto put = [&](int zp) {
    float* o = outb + (int64_t)zp * oplane;
#pragma unroll
    for (int mm = 0; mm < MP; ++mm) {
      const int m = mh * MP + mm;
      o[(int64_t)(2 * m) * a.Do * oplane] = pend[mm].x;
      o[(int64_t)(2 * m + 1) * a.Do * oplane] = pend[mm].y;
    }
  };
  for (int z = z0; z < z1; ++z) {
    store(2 * z, ra);
    store(2 * z + 1, rb);
    __syncthreads();
    if (LATE || z + 1 < z1) {  // (LATE: unconditionally; past the segment: never stored)
      load(2 * z + 2, ra);
      load(2 * z + 3, rb);
    }
    if (LATE && act && z > z0) put(z - 1);
    if (act) {
      // the position's 27 CIN inputs into registers, then one packed FMA chain per output pair
      float v[CIN * 27];
#pragma unroll
      for (int tz = 0; tz < 3; ++tz) {
        const float* sl = ring + ((2 * z - 1 + tz + 3) % 3) * SS + roff;
#pragma unroll
        for (int c = 0; c < CIN; ++c)
#pragma unroll
          for (int ty = 0; ty < 3; ++ty)
#pragma unroll
            for (int tx = 0; tx < 3; ++tx) v[c * 27 + tz * 9 + ty * 3 + tx] = sl[(c * NR + ty) * PX + tx];
      }
      // The thread's weights are one contiguous stream of NP = MP x CIN 27 pairs (pair-major over its output
      // pairs).  It goes through two SGPR buffers of BT pairs: lgkmcnt(0), then the NEXT batch's scalar loads,
      // then this batch's FMAs -- scalar loads return out of order, so a wait on them is always a full drain,
      // and placed here it only waits for loads issued a whole batch of FMAs earlier.  The last batch loads
      // only the pairs that exist.
      constexpr int KC = CIN * 27, NP = MP * KC, BT = 16, NB = (NP + BT - 1) / BT;
      const cf2v_p kp = (cf2v_p)(cfloat_p)a.K + mh * NP;
      f2v kb[2][BT];
      auto kload = [&](int b, f2v (&k)[BT]) {
#pragma unroll
        for (int i = 0; i < BT; ++i)
          if (b * BT + i < NP) k[i] = kp[b * BT + i];
      };
      kload(0, kb[0]);
      f2v acc = bias2[0];
      // (a compile-time loop: `#pragma unroll` gives up on NB batches of this size, and v[] goes to scratch)
      static_for<0, NB>([&](auto bc) {
        constexpr int b = decltype(bc)::value;
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0) (the first: the position's LDS reads as well)
        __builtin_amdgcn_sched_barrier(0);
        if (b + 1 < NB) kload(b + 1, kb[(b + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < BT; ++i) {
          const int p = b * BT + i, mm = p / KC, k = p - mm * KC;
          if (p < NP) {
            if (k == 0) acc = bias2[mm];
            acc = __builtin_elementwise_fma(f2v{v[k], v[k]}, kb[b & 1][i], acc);
            if (k == KC - 1) {
              if (LATE) {
                pend[mm] = acc;
              } else {
                const int m = mh * MP + mm;
                float* o = outb + (int64_t)z * oplane;
                o[(int64_t)(2 * m) * a.Do * oplane] = acc.x;
                o[(int64_t)(2 * m + 1) * a.Do * oplane] = acc.y;
              }
            }
          }
        }
      });
    }
    __syncthreads();  // every wave is done with this step's slots before the next step's stores
  }
  if (LATE && act && z1 > z0) put(z1 - 1);
}

// --------------------------------------------------------------- ConvTranspose3d, few outputs
struct TArgs {
  const float* x;
  const float* W;     // [Cin][MO][27] (the module's own weight layout)
  const float* bias;  // [MO] or null
  float* y;
  int Cin, Di, Hi, Wi;
  int ZS, zlen, nyb;
  int PX, CS;  // LDS row pitch, channel slab stride (TY + 1 rows)
};

template <int MO, int TY, int WV, int NTH = 256, int U = 1>  // U: input channels per FMA-loop iteration
__global__ __launch_bounds__(NTH) void k_convT_fewout(TArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = (int)threadIdx.x;
  constexpr int PX = 4 * WV + 8, CS = (TY + 1) * PX;
  const int Cin = a.Cin, SS = Cin * CS;
  // [2][Cin][TY + 1][PX], column xi at xi + 4 (xi = Wi: zero): step z reads planes z, z + 1; its first
  // store puts plane z + 1 over the slot of z - 1
  float* ring = smem;
  for (int i = tid; i < 2 * SS; i += NTH) ring[i] = 0.f;
  const cfloat_p wg = (cfloat_p)a.W;  // [Cin][MO][27], scalar loads
  int b = (int)blockIdx.x;
  const int zs = b % a.ZS;
  b /= a.ZS;
  const int yb = b % a.nyb, n = b / a.nyb;
  const int y0 = yb * TY;
  const int Di = a.Di, Hi = a.Hi, Wi = a.Wi;
  const int z0 = zs * a.zlen, z1 = min(Di, z0 + a.zlen);
  const int64_t iplane = (int64_t)Hi * Wi, iplane4 = iplane / 4;
  const float4* xb = reinterpret_cast<const float4*>(a.x + (int64_t)n * Cin * Di * iplane);
  const int W4 = Wi >> 2;
  // staging items of one plane: (c, r, q) -> input row y0 + r (r <= TY), float4 q; at most 32 channels
  constexpr int NL = (32 * (TY + 1) * WV + NTH - 1) / NTH;
  const int nitem = Cin * (TY + 1) * W4;
  int gof[NL], lof[NL];
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    const int i = tid + NTH * j;
    const int q = i % W4, t = i / W4, r = t % (TY + 1), c = t / (TY + 1);
    const int yi = y0 + r;
    const bool ok = i < nitem && yi < Hi;
    gof[j] = ok ? (int)((int64_t)c * Di * iplane4 + ((int64_t)yi * Wi + 4 * q) / 4) : -1;
    lof[j] = c * CS + r * PX + 4 + 4 * q;
  }
  float4 rg[NL];
  auto load = [&](int zi) {
    const bool in = zi < Di;
    const float4* src = xb + (int64_t)(in ? zi : 0) * iplane4;
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      rg[j] = src[gof[j] < 0 ? 0 : gof[j]];  // zeroed at the store (a select here waits for the load)
    }
  };
  auto store = [&](int zi) {
    float* d = ring + (zi & 1) * SS;
    const bool in = zi < Di;
#pragma unroll
    for (int j = 0; j < NL; ++j)
      if (gof[j] >= 0) *reinterpret_cast<float4*>(d + lof[j]) = in ? rg[j] : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  __syncthreads();
  load(z0);
  store(z0);
  load(z0 + 1);
  const int jy = tid / Wi, jx = tid - jy * Wi;
  const bool act = jy < TY && y0 + jy < Hi;
  const int roff = jy * PX + jx + 4;
  const int Ho = 2 * Hi, Wo = 2 * Wi, Do = 2 * Di;
  const int64_t oplane = (int64_t)Ho * Wo;
  float bia[MO];
#pragma unroll
  for (int m = 0; m < MO; ++m) bia[m] = a.bias ? a.bias[m] : 0.f;
  float* yb0 = a.y + (int64_t)n * MO * Do * oplane + (int64_t)(2 * (y0 + jy)) * Wo + 2 * jx;
  // (outputs one step late, as k_conv_s2_fewin's 256-thread form: 291 -> 317 us here, not taken)
  for (int z = z0; z < z1; ++z) {
    store(z + 1);  // plane z + 1 (zero past Di)
    __syncthreads();
    if (z + 1 < z1) load(z + 2);
    // acc[m][pz][py][px]
    float acc[MO][2][2][2];
#pragma unroll
    for (int m = 0; m < MO; ++m)
#pragma unroll
      for (int p = 0; p < 8; ++p) acc[m][p >> 2][(p >> 1) & 1][p & 1] = bia[m];
    if (act) {
      const float* s0 = ring + (z & 1) * SS + roff;
      const float* s1 = ring + ((z + 1) & 1) * SS + roff;
#pragma unroll U
      for (int c = 0; c < Cin; ++c) {
        float v[2][2][2];  // [dz][dy][dx]
        v[0][0][0] = s0[c * CS];
        v[0][0][1] = s0[c * CS + 1];
        v[0][1][0] = s0[c * CS + PX];
        v[0][1][1] = s0[c * CS + PX + 1];
        v[1][0][0] = s1[c * CS];
        v[1][0][1] = s1[c * CS + 1];
        v[1][1][0] = s1[c * CS + PX];
        v[1][1][1] = s1[c * CS + PX + 1];
        const cfloat_p wc = wg + c * MO * 27;
#pragma unroll
        for (int m = 0; m < MO; ++m) {
          const cfloat_p wk = wc + m * 27;
          // per axis: parity 0 <- (d 0, t 1); parity 1 <- (d 0, t 2) + (d 1, t 0)
#pragma unroll
          for (int pz = 0; pz < 2; ++pz)
#pragma unroll
            for (int py = 0; py < 2; ++py)
#pragma unroll
              for (int px = 0; px < 2; ++px) {
                float s = acc[m][pz][py][px];
#pragma unroll
                for (int dz = 0; dz <= pz; ++dz)
#pragma unroll
                  for (int dy = 0; dy <= py; ++dy)
#pragma unroll
                    for (int dx = 0; dx <= px; ++dx) {
                      const int tz = pz ? (dz ? 0 : 2) : 1, ty = py ? (dy ? 0 : 2) : 1, tx = px ? (dx ? 0 : 2) : 1;
                      s = fmaf(v[dz][dy][dx], wk[tz * 9 + ty * 3 + tx], s);
                    }
                acc[m][pz][py][px] = s;
              }
        }
      }
#pragma unroll
      for (int m = 0; m < MO; ++m)
#pragma unroll
        for (int pz = 0; pz < 2; ++pz)
#pragma unroll
          for (int py = 0; py < 2; ++py) {
            float* o = yb0 + ((int64_t)m * Do + 2 * z + pz) * oplane + (int64_t)py * Wo;
            *reinterpret_cast<float2*>(o) = make_float2(acc[m][pz][py][0], acc[m][pz][py][1]);
          }
    }
    __syncthreads();
  }
}

template <int CIN, int MOUT, int WV>
int launch_s2(S2Args& a, size_t lds, int N, hipStream_t st) {
  constexpr int TY = 3;
  // CIN = 4, MOUT = 32 (the stacked entry unit + residual): 512 threads splitting the output pairs
  constexpr int NT = (CIN == 4 && MOUT == 32) ? 512 : 256;
  const int per_cu = lds <= 81920 ? 2 : 1;
  a.zlen = tb::zseg(a.Do, N * a.nyb, per_cu, 1);
  a.ZS = (a.Do + a.zlen - 1) / a.zlen;
  return tb::launch_lds(k_conv_s2_fewin<CIN, MOUT, TY, WV, NT>, dim3((unsigned)(N * a.nyb * a.ZS)), dim3(NT), lds, st,
                        a);
}

}  // namespace

// Stride-2, padding-1 3x3x3 convolution with CIN <= 4 input channels and 16 or 32 output channels,
// input [N][CIN][2 Do][2 Ho][2 Wo], output [N][MOUT][Do][Ho][Wo], K = [MOUT / 2][CIN][27][2] (file header).
int tb_conv3d_s2_fewin_f32(const float* in, const float* K, const float* bias, float* out, int N, int Cin, int Mout,
                           int Do, int Ho, int Wo, void* stream) {
  if (!in || !K || !out || N < 1 || Do < 1 || Ho < 1 || Wo < 1) return TB_ERR_INVALID_ARG;
  if (Cin < 1 || Cin > 4 || (Mout != 16 && Mout != 32) || 3 * Wo > 256 || (2 * Wo) % 4 != 0 || 2 * Wo > 256 ||
      (reinterpret_cast<uintptr_t>(in) & 15) != 0)
    return TB_ERR_UNSUPPORTED_SIZE;
  constexpr int TY = 3;
  S2Args a{};
  a.in = in, a.K = K, a.bias = bias, a.out = out;
  a.Do = Do, a.Ho = Ho, a.Wo = Wo, a.Di = 2 * Do, a.Hi = 2 * Ho, a.Wi = 2 * Wo;
  const bool wide = a.Wi > 160;
  a.PX = 4 * (wide ? 64 : 40) + 12;  // = the kernel's compile-time pitch: data at column 4 .. Wi + 3
  a.RR = 2 * TY + 1;
  a.nyb = (Ho + TY - 1) / TY;
  const size_t lds = (size_t)4 * 3 * Cin * a.RR * a.PX;
  if (lds > 163840) return TB_ERR_UNSUPPORTED_SIZE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define TB_S2(CI, MO)                                                                                  \
  if (Cin == CI && Mout == MO) return wide ? launch_s2<CI, MO, 64>(a, lds, N, st) : launch_s2<CI, MO, 40>(a, lds, N, st);
  TB_S2(1, 16) TB_S2(2, 16) TB_S2(3, 16) TB_S2(4, 16) TB_S2(1, 32) TB_S2(2, 32) TB_S2(3, 32) TB_S2(4, 32)
#undef TB_S2
  return TB_ERR_UNSUPPORTED_SIZE;
}

// ConvTranspose3d(Cin -> Mout <= 4, kernel 3, stride 2, padding 1, output_padding 1): x [N][Cin][Di][Hi][Wi]
// -> y [N][Mout][2 Di][2 Hi][2 Wi], W = [Cin][Mout][27] (the module's layout), Cin <= 32.
int tb_convT3d_fewout_f32(const float* x, const float* W, const float* bias, float* y, int N, int Cin, int Mout, int Di,
                          int Hi, int Wi, void* stream) {
  if (!x || !W || !y || N < 1 || Di < 1 || Hi < 1 || Wi < 1) return TB_ERR_INVALID_ARG;
  if (Cin < 1 || Cin > 32 || Mout < 1 || Mout > 4 || Wi % 4 != 0 || Wi > 128 || (reinterpret_cast<uintptr_t>(x) & 15) != 0)
    return TB_ERR_UNSUPPORTED_SIZE;
  // 512 threads over 6 input rows where the two-slot ring of 7 rows fits (one block of 8 waves per CU,
  // two per SIMD, so the scalar weight loads of one wave hide under the other's FMAs); else 256 threads
  const bool big = Wi <= 80 && (size_t)4 * 2 * Cin * 7 * (4 * 20 + 8) <= 163840;
  const int TY = big ? 6 : 256 / Wi >= 3 ? 3 : 256 / Wi >= 2 ? 2 : 1;
  const int nth = big ? 512 : 256;
  TArgs a{};
  a.x = x, a.W = W, a.bias = bias, a.y = y;
  a.Cin = Cin, a.Di = Di, a.Hi = Hi, a.Wi = Wi;
  a.PX = 4 * (Wi <= 80 ? 20 : 32) + 8;  // = the kernel's compile-time pitch
  a.CS = (TY + 1) * a.PX;
  a.nyb = (Hi + TY - 1) / TY;
  const size_t lds = (size_t)4 * 2 * Cin * a.CS;
  if (lds > 163840) return TB_ERR_UNSUPPORTED_SIZE;
  const int per_cu = lds <= 81920 ? 2 : 1;
  a.zlen = tb::zseg(Di, N * a.nyb, per_cu, 1);
  a.ZS = (Di + a.zlen - 1) / a.zlen;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)(N * a.nyb * a.ZS));
  void (*kern)(TArgs) = nullptr;
#define TB_T(MO, T)                                                                    \
  if (Mout == MO && TY == T) kern = Wi <= 80 ? k_convT_fewout<MO, T, 20> : k_convT_fewout<MO, T, 32>;
  TB_T(1, 1) TB_T(1, 2) TB_T(1, 3) TB_T(2, 1) TB_T(2, 2) TB_T(2, 3) TB_T(3, 1) TB_T(3, 2) TB_T(3, 3) TB_T(4, 1)
  TB_T(4, 2) TB_T(4, 3)
#undef TB_T
  // (the 512-thread form takes one input channel per FMA-loop iteration: 1 / 2 / 4 measured 296 / 294 / 311 us
  // for the C3 32 -> 3 layer)
  if (big)
    kern = Mout == 1 ? k_convT_fewout<1, 6, 20, 512> : Mout == 2 ? k_convT_fewout<2, 6, 20, 512>
         : Mout == 3 ? k_convT_fewout<3, 6, 20, 512> : k_convT_fewout<4, 6, 20, 512>;
  if (!kern) return TB_ERR_UNSUPPORTED_SIZE;
  return tb::launch_lds(kern, grid, dim3(nth), lds, st, a);
}

// ------------------------------------------------- stride-1 3x3x3 conv, 16 -> 16 channels, on MFMA
// out[m][p] = b[m] + sum_{c, t} W[m][c][t] X[c][p + t - 1] (padding 1) as Out(16 m x 16 x) =
// W(16 m x 432 k) . X(432 k x 16 x) on mfma_f32_16x16x4f32, k = (tap, channel quad): the block's whole
// W lives in 108 A-fragment registers per lane for the kernel's life; B fragments are LDS reads of the
// staged input planes (lane = (x, channel within the quad): bank-distinct at a channel pitch of 16 mod 32).
// The block marches its (n, YB output rows, z segment) along z with a 3-slot plane ring (the next plane
// in registers, stored over the slot the previous step read last); each wave takes output tiles (row, 16 columns) two at a time (two accumulator chains
// sharing every A fragment).  The input gradient of the same layer is this kernel with
// W'[c][m][t] = W[m][c][26 - t].  Serves the 16-channel full-resolution units (120 x 120 x 80 at C3).
namespace {
struct F16Args {
  const float* x;
  const float* W;     // [16 m][16 c][27]
  const float* bias;  // [16] or null
  const float* add;   // [N][16][D][H][W] summed into y, or null
  float* y;
  int D, H, Wd;
  int ZS, zlen, nyb;
  int PX, RX;  // row pitch (data at column x + 4), channel pitch (= 16 mod 32)
  int flip;    // 1: W is the layer's weight and the call its input gradient: A = W[c][m][26 - t]
  int persist, ncol;  // k_conv3d_fwd16: persistent shares of the ncol = N nyb columns' steps
  int64_t addsn;      // floats between samples of `add` (0: 16 D H W, contiguous)
};

// NS: plane-ring slots.  3: a step's MFMAs read planes z - 1 .. z + 1, plane z + 2 goes over plane z - 1's
// slot after a barrier; 4 (when it fits): plane z + 2 goes into the slot plane z - 2 held, which no wave
// reads in step z -- one barrier per step instead of two.
template <int YB, int NXT, int NTH, bool ADD = false, bool PF = false, int NS = 3>  // output rows per block;
__global__ __launch_bounds__(NTH) void k_conv3d_fwd16(F16Args a) {  // 16-column tiles per row (W = 16 NXT);
                                            // threads; `add` summed into the store; PF: B reads a tap ahead
  constexpr int NWV = NTH / 64;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NR = YB + 2, W4 = 4 * NXT;  // staged rows; float4 per row
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int D = a.D, H = a.H, Wd = a.Wd, PX = a.PX, RX = a.RX, SS = 16 * RX;
  float* ring = smem;  // [NS][16 c][NR][PX]
  for (int i = tid; i < NS * SS; i += NTH) ring[i] = 0.f;
  // A fragments: lane (m = l & 15, ks = l >> 4); k-step kk = 4 t + cq covers channel 4 cq + ks at tap t
  const int li = lane & 15, ks = lane >> 4;
  float af[108];
#pragma unroll
  for (int kk = 0; kk < 108; ++kk) {
    const int c = 4 * (kk & 3) + ks, t = kk >> 2;
    af[kk] = a.flip ? a.W[(c * 16 + li) * 27 + 26 - t] : a.W[(li * 16 + c) * 27 + t];
  }
  const float bm[4] = {a.bias ? a.bias[4 * ks] : 0.f, a.bias ? a.bias[4 * ks + 1] : 0.f,
                       a.bias ? a.bias[4 * ks + 2] : 0.f, a.bias ? a.bias[4 * ks + 3] : 0.f};
  // the block's steps: (n, row block, plane) linearised as column (n, yb) major, plane minor.  a.persist: a
  // contiguous 1/gridDim share of all of them (one block per CU, every CU busy, a share spans at most a
  // few columns, each marched on its own); else the (n, yb, z segment) of blockIdx
  int64_t s_beg, s_end;
  if (a.persist) {
    const int64_t T = (int64_t)a.ncol * D;
    s_beg = T * blockIdx.x / gridDim.x, s_end = T * (blockIdx.x + 1) / gridDim.x;
  } else {
    int b = (int)blockIdx.x;
    const int zs = b % a.ZS;
    b /= a.ZS;
    const int zb = zs * a.zlen;
    s_beg = (int64_t)b * D + zb, s_end = (int64_t)b * D + min(D, zb + a.zlen);
  }
  for (int64_t sg = s_beg; sg < s_end;) {
  const int col = (int)(sg / D), z0 = (int)(sg - (int64_t)col * D);
  const int z1 = (int)min((int64_t)D, z0 + (s_end - sg));
  sg += z1 - z0;
  const int yb = col % a.nyb, n = col / a.nyb;
  const int y0 = yb * YB;
  const int64_t plane = (int64_t)H * Wd, plane4 = plane / 4;
  const float4* xb = reinterpret_cast<const float4*>(a.x + (int64_t)n * 16 * D * plane);
  constexpr int NL = (16 * NR * W4 + NTH - 1) / NTH;
  int gof[NL], lof[NL];
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    const int i = tid + NTH * j;
    const int q = i % W4, t = i / W4, r = t % NR, c = t / NR;
    const int yi = y0 - 1 + r;
    const bool ok = i < 16 * NR * W4 && yi >= 0 && yi < H;
    gof[j] = ok ? (int)((int64_t)c * D * plane4 + ((int64_t)yi * Wd + 4 * q) / 4) : -1;
    // rows outside the volume store zeros over their (zero) staging rows; slots past the staged block
    // store zeros over the first four pad columns -- every lane stores, so that no path skips the wait for
    // the plane loads (a skippable wait makes the compiler wait again, for the output stores too, before
    // the next plane's loads reuse the registers)
    lof[j] = i < 16 * NR * W4 ? c * RX + r * PX + 4 + 4 * q : 0;
  }
  float4 rg[NL];
  auto load = [&](int zi) {
    const bool in = zi >= 0 && zi < D;
    const float4* src = xb + (int64_t)(in ? zi : 0) * plane4;
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      rg[j] = src[gof[j] < 0 ? 0 : gof[j]];  // zeroed at the store (a select here waits for the load)
    }
  };
  auto store = [&](int zi) {
    float* d = ring + ((zi + NS) % NS) * SS;
    const bool in = zi >= 0 && zi < D;
#pragma unroll
    for (int j = 0; j < NL; ++j)
      *reinterpret_cast<float4*>(d + lof[j]) = in && gof[j] >= 0 ? rg[j] : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  __syncthreads();
  load(z0 - 1);
  store(z0 - 1);
  load(z0);
  store(z0);
  load(z0 + 1);
  store(z0 + 1);
  // every start-up load (A fragments, bias, the first planes) retired here, so that the compiler does not
  // wait for the loop's plane loads (vmcnt(0)) before a step's first MFMA
  __builtin_amdgcn_s_waitcnt(0x0F70);
  __syncthreads();
  // B lane base: channel 4 cq + ks (cq added per k-step), column x = li of the tile (+ tx - 1 at + 4)
  const int bl = ks * RX + li + 3;
  const int64_t oplane = plane;
  float* yb0 = a.y + (int64_t)n * 16 * D * oplane;
  const float* ab0 = ADD ? a.add + (int64_t)n * (a.addsn ? a.addsn : 16 * D * oplane) : nullptr;
  constexpr int NT = YB * NXT;                        // tiles per step
  constexpr int NIT = (NT + 2 * NWV - 1) / (2 * NWV);  // tile pairs per wave
  // step z: fetch plane z + 2 (registers) | MFMAs over planes z - 1 .. z + 1 | barrier | plane z + 2 into
  // the slot plane z - 1 held | the step's output stores | barrier.  The output stores come after the
  // plane's LDS store, so the wait for the plane loads never includes an output store's write-back.
  for (int z = z0; z < z1; ++z) {
    const bool more = z + 1 < z1;
    if (more) load(z + 2);
    // ADD: the step's `add` values fetched now, summed at the stores after the MFMAs (loaded at the store
    // they would be waited for there)
    float av[NIT][2][4];
    if constexpr (ADD) {
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int t0 = wave + 2 * NWV * it;
        if (t0 >= NT) break;
        const int t1 = t0 + NWV < NT ? t0 + NWV : t0;
        const int yy0 = t0 / NXT, x00 = 16 * (t0 - yy0 * NXT);
        const int yy1 = t1 / NXT, x01 = 16 * (t1 - yy1 * NXT);
        const int ya = min(y0 + yy0, H - 1), yc = min(y0 + yy1, H - 1);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = 4 * ks + r;
          av[it][0][r] = ab0[((int64_t)m * D + z) * oplane + (int64_t)ya * Wd + x00 + li];
          av[it][1][r] = ab0[((int64_t)m * D + z) * oplane + (int64_t)yc * Wd + x01 + li];
        }
      }
    }
    const float* s0 = ring + ((z + NS - 1) % NS) * SS + bl;  // tz = 0: plane z - 1
    const float* s1 = ring + (z % NS) * SS + bl;
    const float* s2 = ring + ((z + 1) % NS) * SS + bl;
    f32x4 acc[NIT][2];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {  // tiles t0 and t0 + NWV of this wave
      const int t0 = wave + 2 * NWV * it;
      if (t0 >= NT) break;
      const int t1 = t0 + NWV < NT ? t0 + NWV : t0;
      const int yy0 = t0 / NXT, x00 = 16 * (t0 - yy0 * NXT);
      const int yy1 = t1 / NXT, x01 = 16 * (t1 - yy1 * NXT);
      const int o0 = yy0 * PX + x00, o1 = yy1 * PX + x01;
      f32x4 acc0 = {bm[0], bm[1], bm[2], bm[3]}, acc1 = acc0;
      if constexpr (PF) {  // the next tap's 8 B fragments read while this tap's 8 MFMAs run
        float bq[2][8];
        auto ldb = [&](int t, float (&q)[8]) {
          const int tz = t / 9, ty = (t / 3) % 3, tx = t % 3;
          const float* sl = tz == 0 ? s0 : tz == 1 ? s1 : s2;
#pragma unroll
          for (int cq = 0; cq < 4; ++cq) {
            const int off = 4 * cq * RX + ty * PX + tx;
            q[2 * cq] = sl[o0 + off], q[2 * cq + 1] = sl[o1 + off];
          }
        };
        ldb(0, bq[0]);
#pragma unroll
        for (int t = 0; t < 27; ++t) {
          if (t + 1 < 27) ldb(t + 1, bq[(t + 1) & 1]);
#pragma unroll
          for (int cq = 0; cq < 4; ++cq) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(af[4 * t + cq], bq[t & 1][2 * cq], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(af[4 * t + cq], bq[t & 1][2 * cq + 1], acc1, 0, 0, 0);
          }
        }
        // schedule: one MFMA, then one LDS read (the next tap's), alternating
#pragma unroll
        for (int i = 0; i < 216; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
      } else {
#pragma unroll
      for (int tz = 0; tz < 3; ++tz) {
        const float* sl = tz == 0 ? s0 : tz == 1 ? s1 : s2;
#pragma unroll
        for (int ty = 0; ty < 3; ++ty)
#pragma unroll
          for (int tx = 0; tx < 3; ++tx) {
            const int t = tz * 9 + ty * 3 + tx;
#pragma unroll
            for (int cq = 0; cq < 4; ++cq) {
              const int off = 4 * cq * RX + ty * PX + tx;
              const float b0 = sl[o0 + off], b1 = sl[o1 + off];
              acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(af[4 * t + cq], b0, acc0, 0, 0, 0);
              acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(af[4 * t + cq], b1, acc1, 0, 0, 0);
            }
          }
      }
      }
      acc[it][0] = acc0, acc[it][1] = acc1;
    }
    if constexpr (NS == 3) __syncthreads();
    store(z + 2);  // unconditionally (after the last step a dead slot): no path skips the loads' wait
#pragma unroll
    for (int it = 0; it < NIT; ++it) {  // C: column x = li, rows m = 4 ks + r
      const int t0 = wave + 2 * NWV * it;
      if (t0 >= NT) break;
      const int t1 = t0 + NWV < NT ? t0 + NWV : t0;
      const int yy0 = t0 / NXT, x00 = 16 * (t0 - yy0 * NXT);
      const int yy1 = t1 / NXT, x01 = 16 * (t1 - yy1 * NXT);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = 4 * ks + r;
        const int64_t o0 = ((int64_t)m * D + z) * oplane + (int64_t)(y0 + yy0) * Wd + x00 + li;
        const int64_t o1 = ((int64_t)m * D + z) * oplane + (int64_t)(y0 + yy1) * Wd + x01 + li;
        if (y0 + yy0 < H) yb0[o0] = ADD ? acc[it][0][r] + av[it][0][r] : acc[it][0][r];
        if (t1 != t0 && y0 + yy1 < H) yb0[o1] = ADD ? acc[it][1][r] + av[it][1][r] : acc[it][1][r];
      }
    }
    __syncthreads();
  }
  }
}
}  // namespace

// (Round 6: the DMA-staged plane variant (439 vs 382 us) was measured, rejected and removed; the
// split-precision bf16 variant k_conv16_x3 of that round (no gain in the step: its staging, not its
// MFMAs, set its time) came back in round 15 as k_conv16_split below; DESIGN.md records both.)

// ------------------------------------------------- the same layer in split precision on the bf16 matrix cores
// f32 operands as three bf16 parts and six products per 32-k step (split_bf16.h): 96 matrix-core cycles
// per 32 k where the f32 MFMA takes 256.  k = (tap, channel): a 32-k step q is two taps x 16 channels; lane
// group g = lane >> 4 holds tap 2 q + (g >> 1) (tap 27: zero weights), channels 8 (g & 1) .. + 7, so its B
// operand is 8 channels of ONE input position.  The staged planes are channel-innermost bf16,
// [part][row][position][16] (position = x + 1, pitch 32 B: the lanes of a ds_read_b128 group hit distinct
// banks), one 16-B read per part; the row holds W + 5 positions, a pitch of 8 dwords mod 32, so that the
// staging writes of a half wave (4 channel quads x rows) spread over the banks.  The block's A operand
// (14 steps x 3 parts) lives in registers for the kernel's life.  Staging: thread (channel quad, row,
// x quad) loads four float4 (one per channel, 16 B along x) a step ahead, untouched until it splits them
// at the LDS store: 12 ds_write_b64 (4 positions x 3 parts x 4 channels), rows and planes outside the
// volume masked to zero there; idle threads write zeros to the row's spare positions -- no branch stands
// around a load or a store.  Each wave takes one 16-column tile at a time (tiles wave, wave + 8, ..), the
// B fragments of step q + 1 read ahead of step q's six MFMAs.  Block march, plane ring (4 slots and one
// barrier per step where they fit, W <= 80; 3 slots up to W = 96), persistent shares: as k_conv3d_fwd16.
namespace {
struct X16Args {
  const float* x;
  const float* W;     // [16 m][16 c][27]
  const float* bias;  // [16] or null
  const float* add;   // [N][16][D][H][W] summed into y, or null
  float* y;
  int D, H, Wd;
  int ZS, zlen, nyb;
  int flip;           // 1: the input gradient, A = W[c][m][26 - t]
  int persist, ncol;  // as F16Args
  int64_t addsn;
};

constexpr int x16_pxp(int W) { return W + 5; }                     // positions per staged row (1 mod 4)
constexpr size_t x16_slot(int W) { return (size_t)3 * 5 * x16_pxp(W) * 32; }  // bytes per plane slot

template <int NXT, bool ADD, int NS>
__global__ __launch_bounds__(512) void k_conv16_split(X16Args a) {
  using tb::bf16x8;
  constexpr int YB = 3, NR = YB + 2, NTH = 512, NWV = NTH / 64, W = 16 * NXT, W4 = 4 * NXT;
  constexpr int RPB = x16_pxp(W) * 32, SPL = NR * RPB, SLOT = 3 * SPL;  // bytes: row, part, plane slot
  constexpr int NTASK = 4 * NR * W4;  // staging tasks (channel quad, row, x quad)
  static_assert(NTASK <= NTH && 2 * SPL + RPB < 65536 && (size_t)SLOT == x16_slot(W), "one task per thread");
  extern __shared__ __attribute__((aligned(16))) char ring16[];  // [NS][3 parts][NR][W + 5][16] bf16
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int D = a.D, H = a.H;
  for (int i = tid; i < NS * SLOT / 16; i += NTH) reinterpret_cast<uint4*>(ring16)[i] = make_uint4(0, 0, 0, 0);
  // A: lane (m = l & 15, g = l >> 4), step q: tap 2 q + (g >> 1), channels 8 (g & 1) + j
  const int li = lane & 15, g = lane >> 4, hi = g >> 1;
  bf16x8 af[14][3];
  const int wsm = a.flip ? 27 : 16 * 27, wsc = a.flip ? 16 * 27 : 27;  // W[m][c][t], flipped W[c][m][26 - t]
  const float* wl = a.W + li * wsm + 8 * (g & 1) * wsc;
#pragma unroll
  for (int q = 0; q < 14; ++q) {
    const int t = 2 * q + hi, tc = t < 27 ? t : 26;
    const float* wq = wl + (a.flip ? 26 - tc : tc);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = wq[j * wsc];
    if (q == 13) {  // tap 27 does not exist: zero weights (the B operand there is tap 26's, finite)
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = hi ? 0.f : v[j];
    }
    tb::split3(v, af[q][0], af[q][1], af[q][2]);
  }
  const float bm[4] = {a.bias ? a.bias[4 * g] : 0.f, a.bias ? a.bias[4 * g + 1] : 0.f,
                       a.bias ? a.bias[4 * g + 2] : 0.f, a.bias ? a.bias[4 * g + 3] : 0.f};
  int64_t s_beg, s_end;  // the block's steps, as in k_conv3d_fwd16
  if (a.persist) {
    const int64_t T = (int64_t)a.ncol * D;
    s_beg = T * blockIdx.x / gridDim.x, s_end = T * (blockIdx.x + 1) / gridDim.x;
  } else {
    int b = (int)blockIdx.x;
    const int zs = b % a.ZS;
    b /= a.ZS;
    const int zb = zs * a.zlen;
    s_beg = (int64_t)b * D + zb, s_end = (int64_t)b * D + min(D, zb + a.zlen);
  }
  // this thread's staging task; threads past the last task load the sample's first floats and write zeros
  // over the spare positions W + 1 .. W + 4 of row 0 (W + 1 is the right halo: zero anyway)
  const bool act = tid < NTASK;
  const int cq = tid & 3, rr = act ? (tid >> 2) % NR : 0, q4 = act ? (tid >> 2) / NR : 0;
  const int lof = act ? rr * RPB + (4 * q4 + 1) * 32 + cq * 8 : (W + 1) * 32;
  // B lane base: position li (+ tx), channel half g & 1
  const int lb = li * 32 + 16 * (g & 1);
  constexpr int NT = YB * NXT;                // tiles per step
  constexpr int NIT = (NT + NWV - 1) / NWV;   // tiles per wave
  for (int64_t sg = s_beg; sg < s_end;) {
    const int col = (int)(sg / D), z0 = (int)(sg - (int64_t)col * D);
    const int z1 = (int)min((int64_t)D, z0 + (s_end - sg));
    sg += z1 - z0;
    const int yb = col % a.nyb, n = col / a.nyb;
    const int y0 = yb * YB;
    const int64_t plane = (int64_t)H * W, plane4 = plane / 4, chq = (int64_t)D * plane4;
    const float4* xb = reinterpret_cast<const float4*>(a.x + (int64_t)n * 16 * D * plane);
    const int yi = y0 - 1 + rr;
    const bool rowok = act && yi >= 0 && yi < H;
    // per-lane byte offsets (32 bits: the host keeps a sample below 2 GiB) on wave-uniform bases
    const unsigned gof = rowok ? (unsigned)(16 * (4 * cq * chq) + 4 * ((int64_t)yi * W + 4 * q4)) : 0u;  // clamped into the tensor
    const unsigned lo = (unsigned)(4 * ((int64_t)4 * g * D * plane + li));  // output: rows m = 4 g + r, column li
    float4 rg[4];
    auto load = [&](int zi) {  // nothing conditional; zeroed by the mask at the store
      const char* src = reinterpret_cast<const char*>(xb + (int64_t)(zi < 0 ? 0 : zi >= D ? D - 1 : zi) * plane4);
#pragma unroll
      for (int c = 0; c < 4; ++c) rg[c] = *reinterpret_cast<const float4*>(src + 16 * c * chq + gof);
    };
    auto store = [&](int zi) {
      char* d = ring16 + ((zi + NS) % NS) * SLOT + lof;
      const unsigned m = 0u - (unsigned)(rowok && zi >= 0 && zi < D);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c)
          v[c] = __uint_as_float(__float_as_uint(e == 0 ? rg[c].x : e == 1 ? rg[c].y : e == 2 ? rg[c].z : rg[c].w) & m);
        unsigned p[3][2];
        tb::split3_pk(v[0], v[1], p[0][0], p[1][0], p[2][0]);
        tb::split3_pk(v[2], v[3], p[0][1], p[1][1], p[2][1]);
#pragma unroll
        for (int s = 0; s < 3; ++s) *reinterpret_cast<uint2*>(d + s * SPL + e * 32) = make_uint2(p[s][0], p[s][1]);
      }
    };
    __syncthreads();
    load(z0 - 1);
    store(z0 - 1);
    load(z0);
    store(z0);
    load(z0 + 1);
    store(z0 + 1);
    // every start-up load (weights, bias, the first planes) retired here: no vmcnt(0) ahead of a step's MFMAs
    __builtin_amdgcn_s_waitcnt(0x0F70);
    __syncthreads();
    float* yb0 = a.y + (int64_t)n * 16 * D * plane;
    const float* ab0 = ADD ? a.add + (int64_t)n * (a.addsn ? a.addsn : 16 * D * plane) : nullptr;
    // step z: fetch plane z + 2 (registers) | per tile: MFMAs over planes z - 1 .. z + 1, output stores |
    // (3 slots: barrier) | plane z + 2 split into the slot plane z - 2 (3 slots: z - 1) held | barrier
    for (int z = z0; z < z1; ++z) {
      load(z + 2);
      int hv = hi;  // opaque: the per-step B offsets it selects are recomputed, not kept in 14 registers
      asm volatile("" : "+v"(hv));
      int sb[3];  // byte offsets of planes z - 1, z, z + 1
#pragma unroll
      for (int tz = 0; tz < 3; ++tz) sb[tz] = ((z + tz + NS - 1) % NS) * SLOT;
      // the wave's last tile is stored after the plane's LDS store: the wait for the plane loads then has
      // only stores a tile old behind it
      tb::f32x4s cl = {0.f, 0.f, 0.f, 0.f};
      float avl[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int t = wave + NWV * it;
        if (t < NT) {
          const int yy = t / NXT, x0 = 16 * (t - yy * NXT);
          // ADD: the tile's `add` values fetched ahead of its MFMAs, summed at its stores
          const int64_t ou = ((int64_t)z * plane + (int64_t)min(y0 + yy, H - 1) * W + x0) * 4;
          float av[4];
          if constexpr (ADD) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
              av[r] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(ab0) + ou + 4 * r * D * plane + lo);
          }
          const char* rb = ring16 + yy * RPB + x0 * 32 + lb;
          bf16x8 bq[2][3];
          auto ldb = [&](int q, bf16x8 (&b)[3]) {  // read in the order the products take them: parts 1, 2, 0
            const int t0 = 2 * q, t1 = 2 * q + 1 < 27 ? 2 * q + 1 : 26;
            const int c0 = ((t0 / 3) % 3) * RPB + (t0 % 3) * 32, c1 = ((t1 / 3) % 3) * RPB + (t1 % 3) * 32;
            const int o = t0 / 9 == t1 / 9 ? sb[t0 / 9] + (hv ? c1 : c0) : hv ? sb[t1 / 9] + c1 : sb[t0 / 9] + c0;
            b[1] = *reinterpret_cast<const bf16x8*>(rb + o + SPL);
            b[2] = *reinterpret_cast<const bf16x8*>(rb + o + 2 * SPL);
            b[0] = *reinterpret_cast<const bf16x8*>(rb + o);
          };
          tb::f32x4s c = {0.f, 0.f, 0.f, 0.f}, cs = c;  // leading / small products; the bias joins at the store
          ldb(0, bq[0]);
#pragma unroll
          for (int q = 0; q < 14; ++q) {
            if (q + 1 < 14) ldb(q + 1, bq[(q + 1) & 1]);
            tb::mfma_split6(af[q], bq[q & 1], c, cs);
          }
          c += cs;
#pragma unroll
          for (int r = 0; r < 4; ++r) c[r] += bm[r];
          // schedule: (the `add` loads,) step q + 1's three reads, then step q's six MFMAs
          if constexpr (ADD) __builtin_amdgcn_sched_group_barrier(0x020, 4, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);
#pragma unroll
          for (int q = 0; q < 13; ++q) {
            __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 6, 0);
          }
          __builtin_amdgcn_sched_group_barrier(0x008, 6, 0);
          if constexpr (ADD) {  // waited for on every path (a skippable wait comes back ahead of the next loads)
#pragma unroll
            for (int r = 0; r < 4; ++r) asm volatile("" : "+v"(av[r]));
          }
          if (it == NIT - 1) {
            cl = c;
            if constexpr (ADD) {
#pragma unroll
              for (int r = 0; r < 4; ++r) avl[r] = av[r];
            }
          } else if (y0 + yy < H) {  // C: column x = li, rows m = 4 g + r
#pragma unroll
            for (int r = 0; r < 4; ++r)
              *reinterpret_cast<float*>(reinterpret_cast<char*>(yb0) + ou + 4 * r * D * plane + lo) = ADD ? c[r] + av[r] : c[r];
          }
        }
      }
      if constexpr (NS == 3) __syncthreads();
      store(z + 2);  // unconditionally (after the last step a dead slot)
      {
        const int t = wave + NWV * (NIT - 1);
        const int yy = t / NXT, x0 = 16 * (t - yy * NXT);
        if (t < NT && y0 + yy < H) {
          const int64_t ou = ((int64_t)z * plane + (int64_t)(y0 + yy) * W + x0) * 4;
#pragma unroll
          for (int r = 0; r < 4; ++r)
            *reinterpret_cast<float*>(reinterpret_cast<char*>(yb0) + ou + 4 * r * D * plane + lo) = ADD ? cl[r] + avl[r] : cl[r];
        }
      }
      __syncthreads();
    }
  }
}
}  // namespace


// Conv3d(16 -> 16, 3, stride 1, padding 1) forward: x [N][16][D][H][W] -> y [N][16][D][H][W], W % 16 == 0,
// W <= 128; weight [16][16][27], bias [16] or NULL.  (csrc/conv_up.hip, k_conv3d_fwd16)
int tb_conv3d_fwd16_f32(const float* x, const float* W, const float* bias, float* y, int N, int D, int H, int Wd,
                        void* stream) {
  return tb_conv3d_fwd16_add_f32(x, W, bias, nullptr, y, N, D, H, Wd, stream);
}

static int fwd16_call(const float* x, const float* W, const float* bias, const float* add, float* y, int N, int D, int H,
                      int Wd, int flip, void* stream, int64_t add_sn = 0);

int tb_conv3d_fwd16_add_f32(const float* x, const float* W, const float* bias, const float* add, float* y, int N, int D,
                            int H, int Wd, void* stream) {
  return fwd16_call(x, W, bias, add, y, N, D, H, Wd, 0, stream);
}

int tb_conv3d_fwd16_dgrad_f32(const float* gy, const float* W, const float* add, int64_t add_sn, float* dx, int N, int D,
                              int H, int Wd, void* stream) {
  return fwd16_call(gy, W, nullptr, add, dx, N, D, H, Wd, 1, stream, add_sn);
}

static int split16_call(const float* x, const float* W, const float* bias, const float* add, float* y, int N, int D,
                        int H, int Wd, int flip, void* stream, int64_t add_sn) {
  X16Args a{};
  a.x = x, a.W = W, a.bias = bias, a.add = add, a.y = y, a.D = D, a.H = H, a.Wd = Wd;
  a.flip = flip;
  a.addsn = add_sn;
  a.nyb = (H + 2) / 3;
  const int NS = 4 * x16_slot(Wd) <= 163840 ? 4 : 3;  // 4-slot plane ring where it fits (W <= 80)
  const size_t lds = NS * x16_slot(Wd);
  a.zlen = tb::zseg(D, N * a.nyb, 1, 2);  // 8 waves at 2 per SIMD: one block per CU
  a.ZS = (D + a.zlen - 1) / a.zlen;
  void (*kern)(X16Args) = nullptr;
#define TB_X16(NX, S) \
  case NX: kern = add ? k_conv16_split<NX, true, S> : k_conv16_split<NX, false, S>; break;
  switch (Wd / 16) {
    TB_X16(1, 4) TB_X16(2, 4) TB_X16(3, 4) TB_X16(4, 4) TB_X16(5, 4) TB_X16(6, 3)
    default: return TB_ERR_UNSUPPORTED_SIZE;
  }
#undef TB_X16
  if (NS != (Wd <= 80 ? 4 : 3)) return TB_ERR_UNSUPPORTED_SIZE;
  // persistent shares when the (n, yb, z segment) grid leaves CUs idle, as for k_conv3d_fwd16
  a.ncol = N * a.nyb;
  unsigned nblk = (unsigned)(N * a.nyb * a.ZS);
  a.persist = (int64_t)a.ncol * D >= 8LL * tb::num_cu() && nblk % tb::num_cu() != 0;
  if (a.persist) nblk = (unsigned)tb::num_cu();
  return tb::launch_lds(kern, dim3(nblk), dim3(512), lds, reinterpret_cast<hipStream_t>(stream), a);
}

static int fwd16_call(const float* x, const float* W, const float* bias, const float* add, float* y, int N, int D, int H,
                      int Wd, int flip, void* stream, int64_t add_sn) {
  if (!x || !W || !y || N < 1 || D < 1 || H < 1 || Wd < 1) return TB_ERR_INVALID_ARG;
  if (Wd % 16 != 0 || Wd > 128 || (reinterpret_cast<uintptr_t>(x) & 15) != 0) return TB_ERR_UNSUPPORTED_SIZE;
  // rows whose split-bf16 plane ring fits the LDS (W <= 96), samples below 2 GiB (32-bit byte offsets):
  // k_conv16_split; the others stay on the f32 MFMA
  if (3 * x16_slot(Wd) <= 163840 && (int64_t)16 * D * H * Wd < (1LL << 29)) return split16_call(x, W, bias, add, y, N, D, H, Wd, flip, stream, add_sn);
  // output rows per block (C3, W = 80: YB 2 / 3 / 4 = 478 / 419 / 482 us -- the YB x 5 tiles of a step
  // over 4 waves x 2 chains: 10 of 16, 15 of 16, 20 of 24 slots used; YB = 2's second block per CU did not
  // make up for it): only YB = 3 is instantiated
  constexpr int YB = 3;
  F16Args a{};
  a.x = x, a.W = W, a.bias = bias, a.add = add, a.y = y, a.D = D, a.H = H, a.Wd = Wd;
  a.flip = flip;
  a.addsn = add_sn;
  a.PX = Wd + 8;
  a.RX = (YB + 2) * a.PX;
  while ((a.RX & 31) != 16) ++a.RX;
  a.nyb = (H + YB - 1) / YB;
  const int NS = (size_t)4 * 4 * 16 * a.RX <= 163840 ? 4 : 3;  // 4-slot plane ring where it fits
  const size_t lds = (size_t)NS * 4 * 16 * a.RX;
  if (lds > 163840) return TB_ERR_UNSUPPORTED_SIZE;
  const int per_cu = 163840 / (int)lds >= 2 ? 2 : 1;
  a.zlen = tb::zseg(D, N * a.nyb, per_cu, 2);
  a.ZS = (D + a.zlen - 1) / a.zlen;
  void (*kern)(F16Args) = nullptr;
  // 512 threads per block: 8 waves, 2 per SIMD sharing the matrix core, hide the B-fragment LDS reads the
  // compiler issues only 1-3 ahead (YB = 3: 421 -> 365 us per C3 call against 256 threads).
  // W = 80 takes the PF form: the B fragments read a tap ahead of their MFMAs, interleaved one LDS read per
  // MFMA (sched_group_barrier) and a 4-slot plane ring, one barrier per step (C3, by
  // scripts/diag/conv_kern_bench.py: forward 385 -> 374 us, input gradient 361 -> 353 us against the earlier
  // form, which the other widths keep)
#define TB_F16(X, PF)                                                                                             \
  case X:                                                                                                         \
    kern = add ? (NS == 4 ? k_conv3d_fwd16<YB, X, 512, true, PF, 4> : k_conv3d_fwd16<YB, X, 512, true, PF, 3>)     \
               : (NS == 4 ? k_conv3d_fwd16<YB, X, 512, false, PF, 4> : k_conv3d_fwd16<YB, X, 512, false, PF, 3>);  \
    break;
  switch (Wd / 16) {
    TB_F16(1, false) TB_F16(2, false) TB_F16(3, false) TB_F16(4, false) TB_F16(5, true) TB_F16(6, false)
    TB_F16(7, false) TB_F16(8, false)
    default: return TB_ERR_UNSUPPORTED_SIZE;
  }
#undef TB_F16
  // persistent shares when the (n, yb, z segment) grid leaves CUs idle (C3: 240 blocks of 256)
  a.ncol = N * a.nyb;
  unsigned nblk = (unsigned)(N * a.nyb * a.ZS);
  a.persist = per_cu == 1 && (int64_t)a.ncol * D >= 8LL * tb::num_cu() && nblk % tb::num_cu() != 0;
  if (a.persist) nblk = (unsigned)tb::num_cu();
  return tb::launch_lds(kern, dim3(nblk), dim3(512), lds, reinterpret_cast<hipStream_t>(stream), a);
}

// ------------------------------------------------- ConvTranspose3d(64 -> 16, 3, s2, p1, op1) on MFMA
// Sub-pixel form (as k_convT_fewout): input position i = (z, y, x) gives the 8 outputs 2 i + p, p in
// {0, 1}^3; per axis parity 0 takes tap 1 at offset 0, parity 1 takes tap 2 at offset 0 and tap 0 at
// offset +1, so the 27 taps split over the 8 parities and each is a real multiply-add.  As products:
// Out_p(16 m x 16 positions) = sum over p's taps and the 64 channels of W[c][m][t] X[c][i + delta(t)],
// on mfma_f32_16x16x4f32 with k = (tap, channel quad).  Wave g holds the A fragments of channel group
// g (channels 16 g .. 16 g + 15: 108 registers) and accumulates all 8 parities of a 16-position tile
// (positions = flattened (row, column) of the block's YB input rows); the four groups' partial tiles
// meet in LDS (double-buffered, one barrier per tile), where wave w sums parities (w >> 1, w & 1, 0 / 1)
// and writes them as (px = 0, 1) float2 pairs.  The block marches (n, YB rows, z segment) along z with
// a 2-slot input plane ring (plane z and z + 1; the next plane in registers).  Replaces MIOpen's
// col2im GEMM pair for the U-Net's up1 ConvTranspose3d (64 -> 16, 60 x 60 x 40 -> 120 x 120 x 80 at C3).
namespace {
struct T64Args {
  const float* x;     // [N][64][Di][Hi][Wi]
  const float* W;     // [64 c][16 m][27]
  const float* bias;  // [16] or null
  const float* add;   // summed into y (y's layout within a sample, samples addsn floats apart), or null
  float* y;           // [N][16][2 Di][2 Hi][2 Wi], samples ysn floats apart
  int Di, Hi, Wi;
  int ZS, zlen, nyb;
  int PX, RX;         // staged row pitch (data at columns 0 .. Wi - 1, zeros after), channel pitch (16 mod 32)
  int64_t ysn, addsn;
};

// G channel groups (Cin = 16 G): with G = 2 the waves (g, h) also split the position tiles (h = tile parity).
template <int G, int YB, int NL>  // NL: float4 staging pieces per thread (Cin (YB + 1) Wi / 4 <= 256 NL)
__global__ __launch_bounds__(256) void k_convT_mfma64(T64Args a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NR = YB + 1;  // staged rows: y0 .. y0 + YB
  constexpr int CIN = 16 * G, HT = 4 / G;
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = w % G, h = w / G;  // channel group, tile phase of this wave
  const int Di = a.Di, Hi = a.Hi, Wi = a.Wi, PX = a.PX, RX = a.RX, SS = CIN * RX;
  float* ring = smem;                   // [2][Cin][NR][PX]
  float* part = smem + 2 * SS;          // [2 buf][4 waves][8 parities][16 m][16 pos]
  for (int i = tid; i < 2 * SS; i += 256) ring[i] = 0.f;
  int b = (int)blockIdx.x;
  const int zs = b % a.ZS;
  b /= a.ZS;
  const int yb = b % a.nyb, n = b / a.nyb;
  const int y0 = yb * YB;
  const int z0 = zs * a.zlen, z1 = min(Di, z0 + a.zlen);
  const int li = lane & 15, ks = lane >> 4;
  float af[108];  // k-step 4 t + cq: channel 16 g + 4 cq + ks, tap t, output channel li
#pragma unroll
  for (int kk = 0; kk < 108; ++kk) af[kk] = a.W[((16 * g + 4 * (kk & 3) + ks) * 16 + li) * 27 + (kk >> 2)];
  const int64_t plane = (int64_t)Hi * Wi;
  const float* xb = a.x + (int64_t)n * CIN * Di * plane;
  // staging: float4 pieces of (channel, row, column quad); Wi % 4 == 0.  gof: offset in the
  // channel-plane's floats (-1: a row past Hi, staged as zeros), lof: LDS offset
  const int W4 = Wi >> 2, per_c = NR * W4, total = CIN * per_c;
  const int64_t cstride = (int64_t)Di * plane;
  int gof[NL], lof[NL], gch[NL];
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    const int i = tid + 256 * j;
    const int c = i / per_c, r2 = i - c * per_c, r = r2 / W4, q = r2 - r * W4;
    const int yi = y0 + r;
    lof[j] = i < total ? c * RX + r * PX + 4 * q : Wi;  // past the block: zeros over row 0's pad columns
    gof[j] = (i < total && yi < Hi) ? yi * Wi + 4 * q : -1;
    gch[j] = i < total ? c : 0;
  }
  float4 rg[NL];
  auto load = [&](int zi) {
    const bool in = zi < Di;
    const float* src = xb + (int64_t)(in ? zi : 0) * plane;
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const bool ok = in && gof[j] >= 0;  // zeroed at the store (a select here waits for the load)
      rg[j] = *reinterpret_cast<const float4*>(src + gch[j] * cstride + (ok ? gof[j] : 0));
    }
  };
  auto store = [&](int zi) {  // every lane stores (see k_conv3d_fwd16: no path skips the loads' wait)
    float* d = ring + (zi & 1) * SS;
    const bool in = zi < Di;
#pragma unroll
    for (int j = 0; j < NL; ++j)
      *reinterpret_cast<float4*>(d + lof[j]) = (in && gof[j] >= 0) ? rg[j] : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  float bm[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) bm[r] = a.bias ? a.bias[4 * ks + r] : 0.f;
  __syncthreads();
  load(z0);
  store(z0);
  load(z0 + 1);
  store(z0 + 1);
  __builtin_amdgcn_s_waitcnt(0x0F70);  // start-up loads retired (as in k_conv3d_fwd16)
  __syncthreads();
  const int npos = YB * Wi, ntile = (npos + 15) / 16;
  const int64_t oplane = 4 * plane, orow = 2 * Wi;
  float* yb0 = a.y + (int64_t)n * a.ysn;
  // `add` (a wave-uniform branch: this kernel is the fall-back of k_convT_split, which fetches its add values
  // ahead of the MFMAs; here they are read at the head of the sum phase, ahead of the partials' LDS reads)
  const float* ab0 = a.add ? a.add + (int64_t)n * a.addsn : nullptr;
  // (tile phase h', parity pair (pz, py, 0 / 1)) combos over the waves: the G groups' partials summed
  auto sums = [&](int z, int t0, int pb) {
    const float* pr = part + pb * 4 * 8 * 256;
    for (int k = w; k < 4 * HT; k += 4) {
      const int hq = k >> 2, pz = (k >> 1) & 1, py = k & 1, q0 = pz * 4 + py * 2;
      const int pq = 16 * (t0 + hq) + li, yq = pq / Wi, xq = pq - yq * Wi;
      const bool okp = t0 + hq < ntile && pq < npos && y0 + yq < Hi;
      float2 av[4];
      if (ab0) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          av[r] = okp ? *reinterpret_cast<const float2*>(ab0 + ((int64_t)(4 * ks + r) * (2 * Di) + 2 * z + pz) * oplane +
                                                         (int64_t)(2 * (y0 + yq) + py) * orow + 2 * xq)
                      : make_float2(0.f, 0.f);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = 4 * ks + r, e = m * 16 + li;
        float v0 = bm[r], v1 = bm[r];
#pragma unroll
        for (int v = 0; v < G; ++v) {
          v0 += pr[((hq * G + v) * 8 + q0) * 256 + e];
          v1 += pr[((hq * G + v) * 8 + q0 + 1) * 256 + e];
        }
        if (ab0) v0 += av[r].x, v1 += av[r].y;
        if (okp)
          *reinterpret_cast<float2*>(yb0 + ((int64_t)m * (2 * Di) + 2 * z + pz) * oplane +
                                     (int64_t)(2 * (y0 + yq) + py) * orow + 2 * xq) = make_float2(v0, v1);
      }
    }
  };
  int buf = 0;
  // step z: fetch plane z + 2 | per tile: MFMAs, partials, barrier, the previous tile's sums and stores |
  // plane z + 2 over plane z's slot | the last tile's sums and stores | barrier.  The plane's LDS store
  // waits for its loads and the stores of all but the last tile (issued a tile earlier), never for the
  // stores just issued.
  for (int z = z0; z < z1; ++z) {
    if (z + 1 < z1) load(z + 2);
    const float* sz[2] = {ring + (z & 1) * SS, ring + ((z + 1) & 1) * SS};
    for (int t0 = 0; t0 < ntile; t0 += HT) {
      const int tI = t0 + h;
      const int p = 16 * tI + li, pc = p < npos ? p : npos - 1;
      const int yy = pc / Wi, xx = pc - yy * Wi;
      const int bl = (16 * g + ks) * RX + yy * PX + xx;
      f32x4 acc[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int tz = 0; tz < 3; ++tz)
#pragma unroll
        for (int ty = 0; ty < 3; ++ty)
#pragma unroll
          for (int tx = 0; tx < 3; ++tx) {
            const int t = tz * 9 + ty * 3 + tx;
            const int par = (tz != 1) * 4 + (ty != 1) * 2 + (tx != 1);
            const float* s = sz[tz == 0] + bl + (ty == 0) * PX + (tx == 0);
#pragma unroll
            for (int cq = 0; cq < 4; ++cq)
              acc[par] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[4 * t + cq], s[4 * cq * RX], acc[par], 0, 0, 0);
          }
      // partial tiles: C layout column = position li, rows m = 4 ks + r
      float* pw = part + (buf * 4 + w) * 8 * 256;
#pragma unroll
      for (int q = 0; q < 8; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) pw[q * 256 + (4 * ks + r) * 16 + li] = acc[q][r];
      __syncthreads();
      if (t0 > 0) sums(z, t0 - HT, buf ^ 1);
      buf ^= 1;
    }
    store(z + 2);  // slot (z + 2) & 1 = plane z's, read by no wave after the last tile's barrier; unconditional
    sums(z, ((ntile - 1) / HT) * HT, buf ^ 1);
    __syncthreads();
  }
}
}  // namespace

// ------------------------------------------------- the same product in split precision on the bf16 matrix cores
// k_convT_mfma64's sub-pixel product (Cin = 64) on v_mfma_f32_16x16x32_bf16 (split_bf16.h), staged as
// k_conv_mfma_split stages.  A 32-k step is two taps of ONE parity class x the 16 channels of one channel
// group; the classes (pz py px) own 1, 2, 2, 4, 2, 4, 4, 8 taps (tap_of(kind = 2) of conv_gemm.hip), the
// single-tap class 0 is padded with a zero-weight tap: 14 steps per group.  8 waves: wave w takes channel group
// w & 3 and one half of the steps, w >> 2 -- classes 7, 3, 0 (4 + 2 + 1 steps) or 5, 6, 1, 2, 4 (2 + 2 + 1 + 1 + 1)
// -- so it holds 7 steps x 3 parts = 84 A registers (split once at start-up), not 168, the two waves of a SIMD
// share every B position, and one 16-position tile at a time is in flight: its partials [group][class][lane]
// float4 are 32 KiB, double-buffered 64 KiB, one barrier per tile.  Each class runs its own (hi, lo)
// accumulator pair; hi + lo is added once and goes to the partials.  After the barrier wave w sums classes
// (w & 3) * 2 + {0, 1} (px = 0, 1) for rows 4 g4 + 2 (w >> 2) + {0, 1}: the four groups in order, then the bias,
// then `add` (fetched ahead of the tile's MFMAs), then one float2 store per row.  No atomics.
// LDS: a 2-slot plane ring (planes z, z + 1) of bf16 part images [slot][part][group][row 0..YB][position
// 0..Wi][16 ch], position = x, position Wi the zero right neighbour: Wi + 1 positions are 1 mod 4, a row pitch
// of 8 dwords mod 32 as k_conv_mfma_split's Wi + 5, and at Wi = 40, YB = 2 the ring is 94 464 B, with the
// partials 160 000 B of the 163 840.  A staging task (channel quad, row, x quad, group) loads four float4 a
// step ahead, nothing conditional on them, and splits them at the LDS store, rows and planes outside the volume
// masked to zero there; threads past the last task repeat an earlier one (the same values to the same place).
namespace {
struct TSArgs {
  const float* x;     // [N][64][Di][Hi][Wi]
  const float* W;     // [64 c][16 m][27]
  const float* bias;  // [16] or null
  const float* add;   // summed into y (y's layout within a sample, samples addsn floats apart), or null
  float* y;           // [N][16][2 Di][2 Hi][2 Wi], samples ysn floats apart
  int Di, Hi, Wi, YB;
  int ZS, zlen, nyb;
  int ntile;          // position tiles per step: ceil(YB Wi / 16)
  int64_t ysn, addsn;
};

struct CtTap {
  int t, dz, dy, dx;  // weight tap, input offset
};
// tap j of parity class cls: per axis parity 0 takes tap 1 at offset 0; parity 1 takes i = 0 -> tap 2 at
// offset 0, i = 1 -> tap 0 at offset +1; x fastest (tap_of(kind = 2))
constexpr CtTap ct_tap(int cls, int j) {
  const int pz = (cls >> 2) & 1, py = (cls >> 1) & 1, px = cls & 1;
  const int nx = 1 + px, ny = 1 + py;
  const int ix = j % nx, iy = (j / nx) % ny, iz = j / (nx * ny);
  return CtTap{(pz ? (iz ? 0 : 2) : 1) * 9 + (py ? (iy ? 0 : 2) : 1) * 3 + (px ? (ix ? 0 : 2) : 1), pz ? iz : 0,
               py ? iy : 0, px ? ix : 0};
}
constexpr int ct_ntap(int cls) { return (1 + ((cls >> 2) & 1)) * (1 + ((cls >> 1) & 1)) * (1 + (cls & 1)); }
// step s (0 .. 6) of a half: its class, and which pair of the class's taps
constexpr int ct_cls(int half, int s) {
  return half == 0 ? (s < 4 ? 7 : s < 6 ? 3 : 0) : (s < 2 ? 5 : s < 4 ? 6 : s == 4 ? 1 : s == 5 ? 2 : 4);
}
constexpr int ct_pair(int half, int s) { return half == 0 ? (s < 4 ? s : s < 6 ? s - 4 : 0) : (s < 4 ? (s & 1) : 0); }
// the two taps of step s; a class of one tap repeats it (its second tap's weights are zero)
constexpr CtTap ct_step_tap(int half, int s, int hi) {
  const int cls = ct_cls(half, s), e = 2 * ct_pair(half, s) + hi;
  return ct_tap(cls, e < ct_ntap(cls) ? e : ct_ntap(cls) - 1);
}
constexpr bool ct_step_pad(int half, int s, int hi) { return 2 * ct_pair(half, s) + hi >= ct_ntap(ct_cls(half, s)); }

// One tile's seven steps of half HALF: step s + 1's B fragments read ahead of step s's six MFMAs; a class's
// hi + lo written to its partial tile when its last step is done.
template <int HALF>
__device__ __forceinline__ void ct_mma(const tb::bf16x8 (&af)[7][3], const char* rb, int sb0, int sb1, int RPB, int SPL,
                                       int hv, char* pw) {
  using tb::bf16x8;
  bf16x8 bq[2][3];
  auto ldb = [&](int s, bf16x8 (&bf)[3]) {  // read in the order the products take them: parts 1, 2, 0
    const CtTap t0 = ct_step_tap(HALF, s, 0), t1 = ct_step_tap(HALF, s, 1);
    const int c0 = (t0.dz ? sb1 : sb0) + t0.dy * RPB + t0.dx * 32;
    const int c1 = (t1.dz ? sb1 : sb0) + t1.dy * RPB + t1.dx * 32;
    const int o = hv ? c1 : c0;
    bf[1] = *reinterpret_cast<const bf16x8*>(rb + o + SPL);
    bf[2] = *reinterpret_cast<const bf16x8*>(rb + o + 2 * SPL);
    bf[0] = *reinterpret_cast<const bf16x8*>(rb + o);
  };
  tb::f32x4s c = {0.f, 0.f, 0.f, 0.f}, cs = c;  // leading / small products of the class in flight
  ldb(0, bq[0]);
#pragma unroll
  for (int s = 0; s < 7; ++s) {
    if (s + 1 < 7) ldb(s + 1, bq[(s + 1) & 1]);
    tb::mfma_split6(af[s], bq[s & 1], c, cs);
    if (s == 6 || ct_cls(HALF, s + 1) != ct_cls(HALF, s)) {
      c += cs;
      *reinterpret_cast<tb::f32x4s*>(pw + ct_cls(HALF, s) * 1024) = c;
      c = tb::f32x4s{0.f, 0.f, 0.f, 0.f}, cs = c;
    }
  }
  // schedule: step s + 1's three reads, then step s's six MFMAs
  __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);
#pragma unroll
  for (int s = 0; s < 6; ++s) {
    __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 6, 0);
  }
  __builtin_amdgcn_sched_group_barrier(0x008, 6, 0);
}

template <bool ADD>
__global__ __launch_bounds__(512) void k_convT_split(TSArgs a) {
  using tb::bf16x8;
  constexpr int G = 4, NTH = 512;
  extern __shared__ __attribute__((aligned(16))) char ringt[];
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = w & 3, half = w >> 2;
  const int Di = a.Di, Hi = a.Hi, Wi = a.Wi, YB = a.YB, NR = YB + 1;
  const int RPB = (Wi + 1) * 32, GPB = NR * RPB, SPL = G * GPB, SLOT = 3 * SPL;  // bytes: row, group, part, slot
  char* part = ringt + 2 * SLOT;  // [2 buf][4 groups][8 classes][64 lanes] float4
  for (int i = tid; i < 2 * SLOT / 16; i += NTH) reinterpret_cast<uint4*>(ringt)[i] = make_uint4(0, 0, 0, 0);
  int b = (int)blockIdx.x;
  const int zs = b % a.ZS;
  b /= a.ZS;
  const int yb = b % a.nyb, n = b / a.nyb;
  const int y0 = yb * YB;
  const int z0 = zs * a.zlen, z1 = min(Di, z0 + a.zlen);
  // A: lane (m = l & 15, g4 = l >> 4), step s: tap hi = g4 >> 1 of the step's two, channels 16 grp + 8 (g4 & 1) + j
  const int li = lane & 15, g4 = lane >> 4, hi = g4 >> 1;
  bf16x8 af[7][3];
  {
    const float* wl = a.W + ((16 * grp + 8 * (g4 & 1)) * 16 + li) * 27;
#pragma unroll
    for (int s = 0; s < 7; ++s) {
      const int t = half ? (hi ? ct_step_tap(1, s, 1).t : ct_step_tap(1, s, 0).t)
                         : (hi ? ct_step_tap(0, s, 1).t : ct_step_tap(0, s, 0).t);
      const bool pad = hi && (half ? ct_step_pad(1, s, 1) : ct_step_pad(0, s, 1));
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = wl[j * 16 * 27 + t];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = pad ? 0.f : v[j];  // the tap that does not exist: zero weights
      tb::split3(v, af[s][0], af[s][1], af[s][2]);
    }
  }
  const int64_t plane = (int64_t)Hi * Wi, cstride = (int64_t)Di * plane;
  const char* xb = reinterpret_cast<const char*>(a.x + (int64_t)n * 16 * G * cstride);
  // this thread's staging task (channel quad fastest, then row, x quad, group); threads past the last task
  // repeat task tid mod ntask
  const int W4 = Wi >> 2, ntask = 4 * NR * W4 * G;
  const int tk = tid < ntask ? tid : tid % ntask;
  const int cq = tk & 3, rr = (tk >> 2) % NR, r2 = (tk >> 2) / NR, q4 = r2 % W4, sg = r2 / W4;
  const int lof = sg * GPB + rr * RPB + 4 * q4 * 32 + cq * 8;
  const int yi = y0 + rr;
  const bool rowok = yi < Hi;
  // per-lane byte offsets (32 bits: the host keeps a sample below 2 GiB) on wave-uniform bases
  const unsigned chb = (unsigned)(4 * cstride);
  const unsigned gof = rowok ? (unsigned)(16 * sg + 4 * cq) * chb + 4u * (unsigned)(yi * Wi + 4 * q4) : 0u;
  float4 rg[4];
  auto load = [&](int zi) {  // nothing conditional; zeroed by the mask at the store
    const char* src = xb + (int64_t)(zi >= Di ? Di - 1 : zi) * plane * 4;
#pragma unroll
    for (int c = 0; c < 4; ++c) rg[c] = *reinterpret_cast<const float4*>(src + c * chb + gof);
  };
  auto store = [&](int zi) {
    char* d = ringt + (zi & 1) * SLOT + lof;
    const unsigned m = 0u - (unsigned)(rowok && zi < Di);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v[4];
#pragma unroll
      for (int c = 0; c < 4; ++c)
        v[c] = __uint_as_float(__float_as_uint(e == 0 ? rg[c].x : e == 1 ? rg[c].y : e == 2 ? rg[c].z : rg[c].w) & m);
      unsigned p[3][2];
      tb::split3_pk(v[0], v[1], p[0][0], p[1][0], p[2][0]);
      tb::split3_pk(v[2], v[3], p[0][1], p[1][1], p[2][1]);
#pragma unroll
      for (int s = 0; s < 3; ++s) *reinterpret_cast<uint2*>(d + s * SPL + e * 32) = make_uint2(p[s][0], p[s][1]);
    }
  };
  // the sum phase's share of this wave: classes q0, q0 + 1 (px = 0, 1), rows m0 + {0, 1}
  const int pzs = (w >> 1) & 1, pys = w & 1, q0 = pzs * 4 + pys * 2, rh = w >> 2;
  const int m0 = 4 * g4 + 2 * rh;
  const float bm[2] = {a.bias ? a.bias[m0] : 0.f, a.bias ? a.bias[m0 + 1] : 0.f};
  __syncthreads();
  load(z0);
  store(z0);
  load(z0 + 1);
  store(z0 + 1);
  // every start-up load (weights, bias, the first planes) retired here: no vmcnt(0) ahead of a step's MFMAs
  __builtin_amdgcn_s_waitcnt(0x0F70);
  __syncthreads();
  const int npos = YB * Wi, ntile = a.ntile;
  const int64_t oplane = 4 * plane, orow = 2 * Wi, och = 2 * Di * oplane;
  float* yb0 = a.y + (int64_t)n * a.ysn;
  const float* ab0 = ADD ? a.add + (int64_t)n * a.addsn : nullptr;
  const int lb = grp * GPB + 16 * (g4 & 1);  // B lane base: the wave's group, channel half g4 & 1
  int buf = 0;
  // step z: fetch plane z + 2 | per tile: its `add` values fetched, 42 MFMAs, hi + lo per class to the
  // partials, barrier, the tile's sums and stores (they read the buffer the next tile does not write) | barrier
  for (int z = z0; z < z1; ++z) {
    load(z + 2);
    int hv = hi;  // opaque: the per-step B offsets it selects are recomputed, not kept in registers
    asm volatile("" : "+v"(hv));
    const int sb0 = (z & 1) * SLOT, sb1 = ((z + 1) & 1) * SLOT;  // byte offsets of planes z, z + 1
    // the step's last tile (LAST) splits plane z + 2 over plane z's slot right after its barrier (no wave reads
    // that slot any more) and before its own output stores: the wait for the plane's loads then has only
    // stores a tile old behind it, and stands on no skippable path
    auto tile = [&](int t, auto LAST) {
      const int p = 16 * t + li, pc = p < npos ? p : npos - 1;  // past the last position: the last one's values
      const int yy = pc / Wi, xx = pc - yy * Wi;
      const bool ok = p < npos && y0 + yy < Hi;
      // C: column = position li, rows m0, m0 + 1 of classes q0, q0 + 1: one float2 (px = 0, 1) per row
      const int64_t oo = ((int64_t)m0 * (2 * Di) + 2 * z + pzs) * oplane +
                         (int64_t)(2 * min(y0 + yy, Hi - 1) + pys) * orow + 2 * xx;
      float2 av[2];
      if constexpr (ADD) {
#pragma unroll
        for (int r = 0; r < 2; ++r) av[r] = *reinterpret_cast<const float2*>(ab0 + oo + r * och);
      }
      const char* rb = ringt + lb + yy * RPB + xx * 32;
      char* pw = part + (buf * 4 + grp) * 8192 + lane * 16;
      if (half == 0)
        ct_mma<0>(af, rb, sb0, sb1, RPB, SPL, hv, pw);
      else
        ct_mma<1>(af, rb, sb0, sb1, RPB, SPL, hv, pw);
      __syncthreads();
      if constexpr (decltype(LAST)::value) store(z + 2);  // (after the last step a dead slot)
      const char* pr = part + (buf * 32 + q0) * 1024 + lane * 16 + 8 * rh;
      tb::f32x2s v0 = *reinterpret_cast<const tb::f32x2s*>(pr), v1 = *reinterpret_cast<const tb::f32x2s*>(pr + 1024);
#pragma unroll
      for (int gg = 1; gg < G; ++gg) {  // the groups in order
        v0 += *reinterpret_cast<const tb::f32x2s*>(pr + gg * 8192);
        v1 += *reinterpret_cast<const tb::f32x2s*>(pr + gg * 8192 + 1024);
      }
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        float2 o = make_float2(v0[r] + bm[r], v1[r] + bm[r]);
        if constexpr (ADD) o.x += av[r].x, o.y += av[r].y;  // outside the branch: waited for on every path
        if (ok) *reinterpret_cast<float2*>(yb0 + oo + r * och) = o;
      }
      buf ^= 1;
    };
    for (int t = 0; t + 1 < ntile; ++t) tile(t, std::false_type{});
    tile(ntile - 1, std::true_type{});
    __syncthreads();
  }
}
}  // namespace

// ConvTranspose3d(64 -> 16, 3, stride 2, padding 1, output_padding 1) forward:
// x [N][64][Di][Hi][Wi] -> y [N][16][2Di][2Hi][2Wi]; weight [64][16][3][3][3] as the module holds it,
// bias [16] or NULL; Wi % 4 == 0, Wi <= 64.  (csrc/conv_up.hip, k_convT_mfma64)
int tb_convT3d_mfma64_f32(const float* x, const float* W, const float* bias, float* y, int N, int Di, int Hi, int Wi,
                          void* stream) {
  return tb_convT3d_mfma_f32(x, W, bias, y, N, 64, Di, Hi, Wi, stream);
}

// The split kernel's plan for a shape, false where it does not serve it: Cin = 64 (the G = 2 form of Cin = 32 is
// not built), a sample below 2 GiB (32-bit byte offsets), and the most rows per step, up to k_convT_mfma64's 2,
// whose staging tasks fit the block's 512 threads and whose 2-slot ring and 64 KiB of partial tiles fit
// 160 KiB: two rows up to Wi = 40, one up to Wi = 60; Wi = 64 has no plan.  Rows narrower than 32 stay on the
// f32 kernel: with one or two position tiles per step the per-tile barrier and partial exchange are not hidden
// (2 x 64 x 32 x 32 x W, caches flushed, f32 -> split us: W = 8 20.6 -> 31.1, 12 31.5 -> 36.3, 16 32.3 -> 36.5,
// 20 43.6 -> 42.2, 24 44.2 -> 43.0, 32 55.7 -> 48.7, 40 68.7 -> 55.3, 48 79.4 -> 61.7; profiles/r21/README.md).
static bool ct_plan(int Cin, int Di, int Hi, int Wi, TSArgs& s, size_t& lds) {
  if (Cin != 64 || Wi < 32 || (int64_t)Cin * Di * Hi * Wi >= (1LL << 29)) return false;
  for (int YB = std::min(2, Hi); YB >= 1; --YB) {
    lds = (size_t)2 * 3 * 4 * (YB + 1) * (Wi + 1) * 32 + 65536;
    if (4 * 4 * (YB + 1) * (Wi / 4) > 512 || lds > 163840) continue;
    s.Di = Di, s.Hi = Hi, s.Wi = Wi, s.YB = YB;
    s.ntile = (YB * Wi + 15) / 16;
    s.nyb = (Hi + YB - 1) / YB;
    return true;
  }
  return false;
}

// y (samples y_sn floats apart) = convT(x, W) + bias (+ add, samples add_sn floats apart); 0: contiguous
static int convT_call(const float* x, const float* W, const float* bias, const float* add, int64_t add_sn, float* y,
                      int64_t y_sn, int N, int Cin, int Di, int Hi, int Wi, void* stream) {
  if (!x || !W || !y || N < 1 || Di < 1 || Hi < 1 || Wi < 1) return TB_ERR_INVALID_ARG;
  if (Cin != 32 && Cin != 64) return TB_ERR_UNSUPPORTED_SIZE;
  if (Wi % 4 != 0 || Wi > 64 || (reinterpret_cast<uintptr_t>(x) & 15) != 0 || (reinterpret_cast<uintptr_t>(y) & 7) != 0)
    return TB_ERR_UNSUPPORTED_SIZE;
  const int64_t ysz = (int64_t)16 * 8 * Di * Hi * Wi;  // floats of one output sample
  if (y_sn == 0) y_sn = ysz;
  if (add_sn == 0) add_sn = ysz;
  // the float2 stores and `add` loads: 8-byte aligned samples
  if (y_sn < ysz || (y_sn & 1) != 0 || (add && (add_sn < ysz || (add_sn & 1) != 0 || (reinterpret_cast<uintptr_t>(add) & 7) != 0)))
    return TB_ERR_UNSUPPORTED_SIZE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  // k_convT_split where its plan exists; k_convT_mfma64 otherwise
  {
    TSArgs s{};
    size_t slds = 0;
    if (ct_plan(Cin, Di, Hi, Wi, s, slds)) {
      s.x = x, s.W = W, s.bias = bias, s.add = add, s.y = y, s.ysn = y_sn, s.addsn = add_sn;
      s.zlen = tb::zseg(Di, N * s.nyb, 1, 1);  // 8 waves at 2 per SIMD: one block per CU
      s.ZS = (Di + s.zlen - 1) / s.zlen;
      return tb::launch_lds(add ? k_convT_split<true> : k_convT_split<false>, dim3((unsigned)(N * s.nyb * s.ZS)),
                            dim3(512), slds, st, s);
    }
  }
  // two input rows per step; one where the two-row ring does not fit (Cin = 64 past Wi = 52; of those only
  // Wi = 64 comes here, the narrower ones have a split plan, so only that form is built)
  T64Args a{};
  a.x = x, a.W = W, a.bias = bias, a.add = add, a.y = y, a.Di = Di, a.Hi = Hi, a.Wi = Wi;
  a.ysn = y_sn, a.addsn = add_sn;
  a.PX = Wi + 4;
  int YB = 2;
  size_t lds = 0;
  for (; YB >= 1; --YB) {
    a.RX = (YB + 1) * a.PX;
    while ((a.RX & 31) != 16) ++a.RX;
    lds = (size_t)4 * (2 * Cin * a.RX + 2 * 4 * 8 * 256);
    if (lds <= 163840) break;
  }
  if (YB < 1) return TB_ERR_UNSUPPORTED_SIZE;
  a.nyb = (Hi + YB - 1) / YB;
  a.zlen = tb::zseg(Di, N * a.nyb, 1, 1);
  a.ZS = (Di + a.zlen - 1) / a.zlen;
  const int nl = (Cin * (YB + 1) * (Wi / 4) + 255) / 256;
  void (*kern)(T64Args) = nullptr;
  if (YB == 1) {
    if (Cin == 64 && nl == 8) kern = k_convT_mfma64<4, 1, 8>;
  } else {
    switch (nl) {
#define TB_NL(k) \
  case k: kern = Cin == 64 ? k_convT_mfma64<4, 2, k> : k_convT_mfma64<2, 2, k>; break;
      TB_NL(1) TB_NL(2) TB_NL(3) TB_NL(4) TB_NL(5) TB_NL(6) TB_NL(7) TB_NL(8) TB_NL(9) TB_NL(10) TB_NL(11) TB_NL(12)
#undef TB_NL
      default: break;
    }
  }
  if (!kern) return TB_ERR_UNSUPPORTED_SIZE;
  return tb::launch_lds(kern, dim3((unsigned)(N * a.nyb * a.ZS)), dim3(256), lds, st, a);
}

// ConvTranspose3d(Cin -> 16, 3, s2, p1, op1) forward for Cin = 32 or 64 (also the input gradient of
// Conv3d(16 -> Cin, s2, p1) with that layer's weight); as tb_convT3d_mfma64_f32 otherwise.
int tb_convT3d_mfma_f32(const float* x, const float* W, const float* bias, float* y, int N, int Cin, int Di, int Hi,
                        int Wi, void* stream) {
  return convT_call(x, W, bias, nullptr, 0, y, 0, N, Cin, Di, Hi, Wi, stream);
}

// ... with `add` (or NULL) summed into the store, and y and add each a channel slice of a wider tensor where
// their sample strides y_sn / add_sn (floats; 0: contiguous) say so: a stacked stride-2 unit's input gradient
// plus the skip concatenation's share, written straight into the upstream unit's output-gradient buffer.
int tb_convT3d_mfma_add_f32(const float* x, const float* W, const float* bias, const float* add, int64_t add_sn,
                            float* y, int64_t y_sn, int N, int Cin, int Di, int Hi, int Wi, void* stream) {
  return convT_call(x, W, bias, add, add_sn, y, y_sn, N, Cin, Di, Hi, Wi, stream);
}

// ------------------------------------------------- stride-1 3x3x3 conv, C -> C channels (C = 32, 64), on MFMA
// The k_conv3d_fwd16 product with the input channels split over the block's waves: wave w holds the A
// fragments (108 registers) of channel group g = w % G (16 channels) for output tile m = w / G of the
// block's 4 / G; it accumulates NC position tiles at once (NC independent chains; positions = the
// flattened (row, column) of the block's YB rows, so rows need not be a multiple of 16) and the G
// groups' partial tiles meet in LDS, where the waves sum them and store.  A 3-slot plane ring as in
// k_conv3d_fwd16.  The input gradient of the same layer is this kernel with W'[c][m][t] = W[m][c][26 - t].
// Serves the U-Net's 32- and 64-channel units (60 x 60 x 40 and 30 x 30 x 20 at C3).
namespace {
struct S1Args {
  const float* x;     // [N][C][D][H][W]
  const float* W;     // [C m][C c][27]
  const float* bias;  // [C] or null
  const float* add;   // summed into y (y's layout), or null
  float* y;
  int D, H, Wd, YB;
  int ZS, zlen, nyb, MG;  // z segments, row blocks, output-tile groups
  int PX, RX;             // row pitch (data at column x + 4), channel pitch (16 mod 32)
  int flip;               // 1: W is the layer's weight and the call its input gradient (W[c][m][26 - t])
  int64_t addsn;          // floats between samples of `add` (0: contiguous)
};

template <int G, int NC, int NL, int NTH, bool ADD = false>  // NTH 512: two waves per role, alternate tiles
__global__ __launch_bounds__(NTH) void k_conv3d_mfma_s1(S1Args a) {  // (NWG phases); `add` summed into the store
  constexpr int CIN = 16 * G, MTB = 4 / G, NWG = NTH / 256;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = w % G, mt = (w / G) % MTB, h = w / 4;
  const int D = a.D, H = a.H, Wd = a.Wd, YB = a.YB, PX = a.PX, RX = a.RX, SS = CIN * RX;
  const int NR = YB + 2;
  float* ring = smem;            // [3][CIN][NR rows][PX]
  float* part = smem + 3 * SS;   // [NTH / 64 waves][NC][16 m][16 pos]
  float* bsm = part + (NTH / 64) * NC * 256;  // the block's bias values [MTB * 16] (no global load in the loop)
  for (int i = tid; i < 3 * SS; i += NTH) ring[i] = 0.f;
  int b = (int)blockIdx.x;
  const int zs = b % a.ZS;
  b /= a.ZS;
  const int mg = b % a.MG;
  b /= a.MG;
  const int yb = b % a.nyb, n = b / a.nyb;
  const int COUT = 16 * MTB * a.MG;
  const int y0 = yb * YB;
  const int z0 = zs * a.zlen, z1 = min(D, z0 + a.zlen);
  const int li = lane & 15, ks = lane >> 4;
  const int m0 = (mg * MTB + mt) * 16;
  if (tid < MTB * 16) bsm[tid] = a.bias ? a.bias[mg * MTB * 16 + tid] : 0.f;
  float af[108];
#pragma unroll
  for (int kk = 0; kk < 108; ++kk) {
    const int c = 16 * g + 4 * (kk & 3) + ks, t = kk >> 2;
    af[kk] = a.flip ? a.W[(c * CIN + m0 + li) * 27 + 26 - t] : a.W[((m0 + li) * CIN + c) * 27 + t];
  }
  const int64_t plane = (int64_t)H * Wd, cstride = (int64_t)D * plane;
  const float* xb = a.x + (int64_t)n * CIN * cstride;
  const int W4 = Wd >> 2, per_c = NR * W4, total = CIN * per_c;
  int gof[NL], lof[NL], gch[NL];
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    const int i = tid + NTH * j;
    const int c = i / per_c, r2 = i - c * per_c, r = r2 / W4, q = r2 - r * W4;
    const int yi = y0 - 1 + r;
    lof[j] = i < total ? c * RX + r * PX + 4 + 4 * q : 0;  // past the block: zeros over pad columns 0..3
    gof[j] = (i < total && yi >= 0 && yi < H) ? yi * Wd + 4 * q : -1;
    gch[j] = i < total ? c : 0;
  }
  float4 rg[NL];
  auto load = [&](int zi) {
    const bool in = zi >= 0 && zi < D;
    const float* src = xb + (int64_t)(in ? zi : 0) * plane;
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const bool ok = in && gof[j] >= 0;  // zeroed at the store (a select here waits for the load)
      rg[j] = *reinterpret_cast<const float4*>(src + gch[j] * cstride + (ok ? gof[j] : 0));
    }
  };
  auto store = [&](int zi) {  // every lane stores (see k_conv3d_fwd16: no path skips the loads' wait)
    float* d = ring + ((zi + 3) % 3) * SS;
    const bool in = zi >= 0 && zi < D;
#pragma unroll
    for (int j = 0; j < NL; ++j)
      *reinterpret_cast<float4*>(d + lof[j]) = (in && gof[j] >= 0) ? rg[j] : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  __syncthreads();
  load(z0 - 1);
  store(z0 - 1);
  load(z0);
  store(z0);
  load(z0 + 1);
  store(z0 + 1);
  __builtin_amdgcn_s_waitcnt(0x0F70);  // start-up loads retired (as in k_conv3d_fwd16)
  __syncthreads();
  // the host sizes YB so that a step's positions fit the block's NWG x NC chains: one tile round per step
  const int npos = YB * Wd;
  float* ybase = a.y + (int64_t)n * COUT * cstride;
  const float* abase = ADD ? a.add + (int64_t)n * (a.addsn ? a.addsn : COUT * cstride) : nullptr;
  constexpr int NK = (MTB * NWG * NC + NTH / 64 - 1) / (NTH / 64);  // sum-phase combos per wave
  int bl[NC];  // chain c of this wave: position tile NWG c + h
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int p = 16 * (NWG * c + h) + li, pc = p < npos ? p : npos - 1;
    const int yy = pc / Wd, xx = pc - yy * Wd;
    bl[c] = (16 * g + ks) * RX + yy * PX + xx + 3;
  }
  // step z: fetch plane z + 2 | MFMAs over planes z - 1 .. z + 1 into the group partials | barrier | plane
  // z + 2 over plane z - 1's slot, the partials summed and stored | barrier
  for (int z = z0; z < z1; ++z) {
    if (z + 1 < z1) load(z + 2);
    // ADD: the step's `add` values fetched now, summed in the store phase (as in k_conv3d_fwd16)
    float av[NK][4];
    if constexpr (ADD) {
#pragma unroll
      for (int kk = 0; kk < NK; ++kk) {
        const int k = w + kk * (NTH / 64);
        if (k >= MTB * NWG * NC) break;
        const int mq = k / (NWG * NC), r2 = k - mq * (NWG * NC), hq = r2 / NC, c = r2 - hq * NC;
        const int p = 16 * (NWG * c + hq) + li, pc = p < npos ? p : npos - 1;
        const int yy = pc / Wd, xx = pc - yy * Wd, yr = min(y0 + yy, H - 1);
        const int mb = (mg * MTB + mq) * 16;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          av[kk][r] = abase[(int64_t)(mb + 4 * ks + r) * cstride + (int64_t)z * plane + (int64_t)yr * Wd + xx];
      }
    }
    const float* sp[3] = {ring + ((z + 2) % 3) * SS, ring + (z % 3) * SS, ring + ((z + 1) % 3) * SS};
    f32x4 acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    // (B reads a k-step ahead with per-step scheduling barriers measured no change, 209 / 120 us)
#pragma unroll
    for (int tz = 0; tz < 3; ++tz)
#pragma unroll
      for (int ty = 0; ty < 3; ++ty)
#pragma unroll
        for (int tx = 0; tx < 3; ++tx) {
          const int t = tz * 9 + ty * 3 + tx;
          const float* s = sp[tz] + ty * PX + tx;
#pragma unroll
          for (int cq = 0; cq < 4; ++cq)
#pragma unroll
            for (int c = 0; c < NC; ++c)
              acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[4 * t + cq], s[bl[c] + 4 * cq * RX], acc[c], 0, 0, 0);
        }
    float* pw = part + w * NC * 256;
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) pw[c * 256 + (4 * ks + r) * 16 + li] = acc[c][r];
    __syncthreads();
    store(z + 2);  // unconditionally (after the last step a dead slot)
    // (output tile mt', phase h', chain c) combos over the waves: the G groups' partials summed + bias
    // (k, kk): sum-phase combo k = w + kk * waves; kk indexes the prefetched add values (ADD only: the
    // unrolled form keeps them in registers; the plain form keeps the runtime loop and its register count)
    auto combo = [&](int k, int kk) {
      const int mq = k / (NWG * NC), r2 = k - mq * (NWG * NC), hq = r2 / NC, c = r2 - hq * NC;
      const int p = 16 * (NWG * c + hq) + li;
      const int yy = p / Wd, xx = p - yy * Wd;
      const bool ok = p < npos && y0 + yy < H;
      const int mb = (mg * MTB + mq) * 16;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = 4 * ks + r;
        float v = bsm[mq * 16 + m];
#pragma unroll
        for (int gg = 0; gg < G; ++gg) v += part[((hq * 4 + mq * G + gg) * NC + c) * 256 + m * 16 + li];
        const int64_t o = (int64_t)(mb + m) * cstride + (int64_t)z * plane + (int64_t)(y0 + yy) * Wd + xx;
        if (ok) ybase[o] = ADD ? v + av[kk][r] : v;
      }
    };
    if constexpr (ADD) {
#pragma unroll
      for (int kk = 0; kk < NK; ++kk) {
        const int k = w + kk * (NTH / 64);
        if (k >= MTB * NWG * NC) break;
        combo(k, kk);
      }
    } else {
      for (int k = w; k < MTB * NWG * NC; k += NTH / 64) combo(k, 0);
    }
    __syncthreads();
  }
}
}  // namespace

// ------------------------------------------------- the same conv in split precision on the bf16 matrix cores
// k_conv3d_mfma_s1's product on v_mfma_f32_16x16x32_bf16 (split_bf16.h), staged as k_conv16_split stages:
// k = (tap, channel), one 32-k step = two taps x the 16 channels of one channel group, tap 27 with zero
// weights.  8 waves; wave w holds the A fragments of (output tile mt, channel group grp) = (w / G % MTB,
// w % G) for the kernel's life (14 steps x 3 parts, 168 registers, split once at start-up; flip reads
// W[c][m][26 - t]) and takes the position tiles h, h + NWG, .. of a step (h = w / (G MTB), NWG = 8 / (G
// MTB) waves per role), one at a time with step q + 1's B fragments read ahead of step q's six MFMAs.
// Positions are the flattened (row, column) of the block's YB rows.  LDS: a 3-slot plane ring of bf16 part
// images [slot][part][group][row 0..YB + 1][position 0..W + 4][16 ch] (position = x + 1, 32 B each, W + 5
// positions: a row pitch of 8 dwords mod 32 as in k_conv16_split, one ds_read_b128 per part), then the
// partial tiles [tile][role][lane] as the accumulator's own float4 (one ds_write_b128 / ds_read_b128 per
// lane, no bank shared), then the block's bias values.  A staging task (group, x quad, row, channel quad)
// loads four float4 a step ahead and splits them at the LDS store, rows and planes outside the volume
// masked to zero there.  Step z: fetch plane z + 2 | per tile 84 MFMAs, hi + lo to the partials | barrier |
// plane z + 2 over plane z - 1's slot; per (tile, output tile) the G partials summed in group order, then
// the bias, then `add`, and stored | barrier.  No atomics: the order is fixed.
namespace {
struct XSArgs {
  const float* x;     // [N][C][D][H][W]
  const float* W;     // [C m][C c][27]
  const float* bias;  // [C] or null
  const float* add;   // summed into y (y's layout), or null
  float* y;
  int D, H, Wd, YB;
  int ZS, zlen, nyb, MG;  // z segments, row blocks, output-tile groups
  int ntile;              // position tiles per step: ceil(YB W / 16)
  int flip;               // 1: the input gradient, A = W[c][m][26 - t]
  int64_t addsn;          // floats between samples of `add` (0: contiguous)
};

inline size_t xs_slot(int G, int YB, int W) { return (size_t)3 * G * (YB + 2) * (W + 5) * 32; }  // bytes per plane slot

template <int G, int MTB, bool ADD>
__global__ __launch_bounds__(512) void k_conv_mfma_split(XSArgs a) {
  using tb::bf16x8;
  constexpr int CIN = 16 * G, NTH = 512, NWV = NTH / 64, NROLE = G * MTB, NWG = NWV / NROLE;
  static_assert(NROLE * NWG == NWV, "every wave has a role");
  extern __shared__ __attribute__((aligned(16))) char ringx[];
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = w % G, mt = (w / G) % MTB, h = w / NROLE;
  const int D = a.D, H = a.H, Wd = a.Wd, YB = a.YB, NR = YB + 2;
  const int RPB = (Wd + 5) * 32, GPB = NR * RPB, SPL = G * GPB, SLOT = 3 * SPL;  // bytes: row, group, part, slot
  char* part = ringx + 3 * SLOT;                                                 // [ntile][NROLE][64] float4
  float* bsm = reinterpret_cast<float*>(part + a.ntile * NROLE * 1024);          // [MTB * 16]
  for (int i = tid; i < 3 * SLOT / 16; i += NTH) reinterpret_cast<uint4*>(ringx)[i] = make_uint4(0, 0, 0, 0);
  int b = (int)blockIdx.x;
  const int zs = b % a.ZS;
  b /= a.ZS;
  const int mg = b % a.MG;
  b /= a.MG;
  const int yb = b % a.nyb, n = b / a.nyb;
  const int COUT = 16 * MTB * a.MG;
  const int y0 = yb * YB;
  const int z0 = zs * a.zlen, z1 = min(D, z0 + a.zlen);
  if (tid < MTB * 16) bsm[tid] = a.bias ? a.bias[mg * MTB * 16 + tid] : 0.f;
  // A: lane (m = l & 15, g4 = l >> 4), step q: tap 2 q + (g4 >> 1), channels 16 grp + 8 (g4 & 1) + j
  const int li = lane & 15, g4 = lane >> 4, hi = g4 >> 1;
  const int m0 = (mg * MTB + mt) * 16;
  bf16x8 af[14][3];
  {
    const int wsm = a.flip ? 27 : CIN * 27, wsc = a.flip ? CIN * 27 : 27;  // W[m][c][t], flipped W[c][m][26 - t]
    const float* wl = a.W + (m0 + li) * wsm + (16 * grp + 8 * (g4 & 1)) * wsc;
#pragma unroll
    for (int q = 0; q < 14; ++q) {
      const int t = 2 * q + hi, tc = t < 27 ? t : 26;
      const float* wq = wl + (a.flip ? 26 - tc : tc);
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = wq[j * wsc];
      if (q == 13) {  // tap 27 does not exist: zero weights (the B operand there is tap 26's, finite)
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = hi ? 0.f : v[j];
      }
      tb::split3(v, af[q][0], af[q][1], af[q][2]);
    }
  }
  const int64_t plane = (int64_t)H * Wd, cstride = (int64_t)D * plane;
  const char* xb = reinterpret_cast<const char*>(a.x + (int64_t)n * CIN * cstride);
  // this thread's staging task (channel quad fastest, then row, x quad, group); threads past the last task
  // load the sample's first floats and write zeros over the spare positions W + 1 .. W + 4 of row 0
  const int W4 = Wd >> 2;
  const int cq = tid & 3, rr = (tid >> 2) % NR, r2 = (tid >> 2) / NR, q4 = r2 % W4, sg = r2 / W4;
  const bool act = sg < G;
  const int lof = act ? sg * GPB + rr * RPB + (4 * q4 + 1) * 32 + cq * 8 : (Wd + 1) * 32;
  const int yi = y0 - 1 + rr;
  const bool rowok = act && yi >= 0 && yi < H;
  // per-lane byte offsets (32 bits: the host keeps a sample below 2 GiB) on wave-uniform bases
  const unsigned chb = (unsigned)(4 * cstride);
  const unsigned gof = rowok ? (unsigned)(16 * sg + 4 * cq) * chb + 4u * (unsigned)(yi * Wd + 4 * q4) : 0u;
  float4 rg[4];
  auto load = [&](int zi) {  // nothing conditional; zeroed by the mask at the store
    const char* src = xb + (int64_t)(zi < 0 ? 0 : zi >= D ? D - 1 : zi) * plane * 4;
#pragma unroll
    for (int c = 0; c < 4; ++c) rg[c] = *reinterpret_cast<const float4*>(src + c * chb + gof);
  };
  auto store = [&](int zi) {
    char* d = ringx + ((zi + 3) % 3) * SLOT + lof;
    const unsigned m = 0u - (unsigned)(rowok && zi >= 0 && zi < D);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v[4];
#pragma unroll
      for (int c = 0; c < 4; ++c)
        v[c] = __uint_as_float(__float_as_uint(e == 0 ? rg[c].x : e == 1 ? rg[c].y : e == 2 ? rg[c].z : rg[c].w) & m);
      unsigned p[3][2];
      tb::split3_pk(v[0], v[1], p[0][0], p[1][0], p[2][0]);
      tb::split3_pk(v[2], v[3], p[0][1], p[1][1], p[2][1]);
#pragma unroll
      for (int s = 0; s < 3; ++s) *reinterpret_cast<uint2*>(d + s * SPL + e * 32) = make_uint2(p[s][0], p[s][1]);
    }
  };
  __syncthreads();
  load(z0 - 1);
  store(z0 - 1);
  load(z0);
  store(z0);
  load(z0 + 1);
  store(z0 + 1);
  // every start-up load (weights, bias, the first planes) retired here: no vmcnt(0) ahead of a step's MFMAs
  __builtin_amdgcn_s_waitcnt(0x0F70);
  __syncthreads();
  const int npos = YB * Wd, ntile = a.ntile;
  float* ybase = a.y + (int64_t)n * COUT * cstride;
  const float* abase = ADD ? a.add + (int64_t)n * (a.addsn ? a.addsn : COUT * cstride) : nullptr;
  const int lb = grp * GPB + 16 * (g4 & 1);  // B lane base: the wave's group, channel half g4 & 1
  for (int z = z0; z < z1; ++z) {
    load(z + 2);
    int hv = hi;  // opaque: the per-step B offsets it selects are recomputed, not kept in 14 registers
    asm volatile("" : "+v"(hv));
    int sb[3];  // byte offsets of planes z - 1, z, z + 1
#pragma unroll
    for (int tz = 0; tz < 3; ++tz) sb[tz] = ((z + tz + 2) % 3) * SLOT;
    for (int t = h; t < ntile; t += NWG) {
      const int p = 16 * t + li, pc = p < npos ? p : npos - 1;  // past the last position: the last one's values
      const int yy = pc / Wd, xx = pc - yy * Wd;
      const char* rb = ringx + lb + yy * RPB + xx * 32;
      bf16x8 bq[2][3];
      auto ldb = [&](int q, bf16x8 (&bf)[3]) {  // read in the order the products take them: parts 1, 2, 0
        const int t0 = 2 * q, t1 = 2 * q + 1 < 27 ? 2 * q + 1 : 26;
        const int c0 = sb[t0 / 9] + ((t0 / 3) % 3) * RPB + (t0 % 3) * 32;
        const int c1 = sb[t1 / 9] + ((t1 / 3) % 3) * RPB + (t1 % 3) * 32;
        const int o = hv ? c1 : c0;
        bf[1] = *reinterpret_cast<const bf16x8*>(rb + o + SPL);
        bf[2] = *reinterpret_cast<const bf16x8*>(rb + o + 2 * SPL);
        bf[0] = *reinterpret_cast<const bf16x8*>(rb + o);
      };
      tb::f32x4s c = {0.f, 0.f, 0.f, 0.f}, cs = c;  // leading / small products
      ldb(0, bq[0]);
#pragma unroll
      for (int q = 0; q < 14; ++q) {
        if (q + 1 < 14) ldb(q + 1, bq[(q + 1) & 1]);
        tb::mfma_split6(af[q], bq[q & 1], c, cs);
      }
      c += cs;
      // schedule: step q + 1's three reads, then step q's six MFMAs
      __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);
#pragma unroll
      for (int q = 0; q < 13; ++q) {
        __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 6, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x008, 6, 0);
      *reinterpret_cast<tb::f32x4s*>(part + ((t * NROLE + mt * G + grp) * 64 + lane) * 16) = c;
    }
    __syncthreads();
    store(z + 2);  // unconditionally (after the last step a dead slot)
    // (position tile, output tile) combos over the waves: the G groups' partials in group order, the bias, `add`
    for (int k = w; k < ntile * MTB; k += NWV) {
      const int t = k / MTB, mq = k - t * MTB;
      const int p = 16 * t + li, pc = p < npos ? p : npos - 1;
      const int yy = pc / Wd, xx = pc - yy * Wd;
      const bool ok = p < npos && y0 + yy < H;
      const int mb = (mg * MTB + mq) * 16 + 4 * g4;
      // C: column = position li, rows m = 4 g4 + r; 32-bit float offsets on the plane's base
      const unsigned oo = (unsigned)(mb * cstride + (int64_t)min(y0 + yy, H - 1) * Wd + xx);
      float av[4];
      if constexpr (ADD) {
#pragma unroll
        for (int r = 0; r < 4; ++r) av[r] = (abase + (int64_t)z * plane)[oo + (unsigned)r * (unsigned)cstride];
      }
      const char* pr = part + ((t * NROLE + mq * G) * 64 + lane) * 16;
      tb::f32x4s v = *reinterpret_cast<const tb::f32x4s*>(pr);
#pragma unroll
      for (int gg = 1; gg < G; ++gg) v += *reinterpret_cast<const tb::f32x4s*>(pr + gg * 1024);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float o = v[r] + bsm[mq * 16 + 4 * g4 + r];
        if constexpr (ADD) o += av[r];
        if (ok) (ybase + (int64_t)z * plane)[oo + (unsigned)r * (unsigned)cstride] = o;
      }
    }
    __syncthreads();
  }
}
}  // namespace

// Conv3d(C -> C, 3, stride 1, padding 1) forward for C = 32 or 64: x [N][C][D][H][W] -> y, W % 4 == 0,
// W <= 64; weight [C][C][27], bias [C] or NULL.  (csrc/conv_up.hip, k_conv_mfma_split / k_conv3d_mfma_s1)
int tb_conv3d_mfma_f32(const float* x, const float* W, const float* bias, float* y, int N, int C, int D, int H, int Wd,
                       void* stream) {
  return tb_conv3d_mfma_add_f32(x, W, bias, nullptr, y, N, C, D, H, Wd, stream);
}

static int mfma_call(const float* x, const float* W, const float* bias, const float* add, float* y, int N, int C, int D,
                     int H, int Wd, int flip, void* stream, int64_t add_sn = 0);

int tb_conv3d_mfma_add_f32(const float* x, const float* W, const float* bias, const float* add, float* y, int N, int C,
                           int D, int H, int Wd, void* stream) {
  return mfma_call(x, W, bias, add, y, N, C, D, H, Wd, 0, stream);
}

int tb_conv3d_mfma_dgrad_f32(const float* gy, const float* W, const float* add, int64_t add_sn, float* dx, int N, int C,
                             int D, int H, int Wd, void* stream) {
  return mfma_call(gy, W, nullptr, add, dx, N, C, D, H, Wd, 1, stream, add_sn);
}

// The split kernel's plan for a shape, false where it does not serve it: C = 32 puts both output tiles in
// the block (MTB 2, two waves per role), C = 64 one (MTB 1, two waves per role, 4 block groups).  Rows per
// step: the most, up to 4, whose staging tasks fit the block's 512 threads and whose 3-slot ring, partial
// tiles and bias fit 160 KiB.  C = 32 rows narrower than 16 stay on the f32 kernel: at W = 8 the split form
// measured slower without `add` (42.7 against 39.0 us forward at 2 x 32 x 32 x 32 x 8; W = 12 not measured).
static bool xs_plan(int C, int D, int H, int Wd, XSArgs& s, size_t& lds) {
  if ((int64_t)C * D * H * Wd >= (1LL << 29) || (C == 32 && Wd < 16)) return false;
  const int G = C / 16, MTB = G == 2 ? 2 : 1;
  for (int YB = std::min(4, H); YB >= 1; --YB) {
    const int ntile = (YB * Wd + 15) / 16;
    lds = 3 * xs_slot(G, YB, Wd) + (size_t)ntile * G * MTB * 1024 + MTB * 64;
    if (4 * G * (YB + 2) * (Wd / 4) > 512 || lds > 163840) continue;
    s.D = D, s.H = H, s.Wd = Wd, s.YB = YB, s.ntile = ntile;
    s.nyb = (H + YB - 1) / YB;
    s.MG = C / (16 * MTB);
    return true;
  }
  return false;
}

static int mfma_call(const float* x, const float* W, const float* bias, const float* add, float* y, int N, int C, int D,
                     int H, int Wd, int flip, void* stream, int64_t add_sn) {
  if (!x || !W || !y || N < 1 || D < 1 || H < 1 || Wd < 1) return TB_ERR_INVALID_ARG;
  if ((C != 32 && C != 64) || Wd % 4 != 0 || Wd > 64 || (reinterpret_cast<uintptr_t>(x) & 15) != 0)
    return TB_ERR_UNSUPPORTED_SIZE;
  // k_conv_mfma_split where its plan exists (xs_plan: the ring and the partial tiles within the LDS, one
  // staging task per thread, samples below 2 GiB for the 32-bit byte offsets); k_conv3d_mfma_s1 otherwise
  {
    XSArgs s{};
    size_t slds = 0;
    if (xs_plan(C, D, H, Wd, s, slds)) {
      s.x = x, s.W = W, s.bias = bias, s.add = add, s.y = y, s.flip = flip, s.addsn = add_sn;
      s.zlen = tb::zseg(D, N * s.nyb * s.MG, 1, 2);  // 8 waves at 2 per SIMD: one block per CU
      s.ZS = (D + s.zlen - 1) / s.zlen;
      void (*sk)(XSArgs) = C == 32 ? (add ? k_conv_mfma_split<2, 2, true> : k_conv_mfma_split<2, 2, false>)
                                   : (add ? k_conv_mfma_split<4, 1, true> : k_conv_mfma_split<4, 1, false>);
      return tb::launch_lds(sk, dim3((unsigned)(N * s.nyb * s.MG * s.ZS)), dim3(512), slds,
                            reinterpret_cast<hipStream_t>(stream), s);
    }
  }
  // 4 waves with 5 chains each (8 waves, two per role on alternate tiles with 3 chains, measured
  // slower here, 245 vs 211 us at 32 -> 32, unlike k_conv3d_fwd16).  (Persistent step
  // shares as in k_conv3d_fwd16 measured no gain at 32 -> 32, 186 vs 184 us, and the loop they need cost
  // the 64 -> 64 kernel 107 -> 144 us: not used.)
  constexpr int NC = 5;
  const int G = C / 16;
  S1Args a{};
  a.x = x, a.W = W, a.bias = bias, a.add = add, a.y = y, a.D = D, a.H = H, a.Wd = Wd;
  a.flip = flip;
  a.addsn = add_sn;
  a.PX = Wd + 8;
  a.MG = G == 2 ? 1 : 4;  // 32: both output tiles in the block; 64: one tile per block, 4 block groups
  size_t lds = 0;
  // rows per step: the most whose positions fit one round of the block's NWG x NC position tiles
  int YB = std::max(1, 16 * NC / Wd);
  for (; YB >= 1; --YB) {
    a.RX = (YB + 2) * a.PX;
    while ((a.RX & 31) != 16) ++a.RX;
    lds = (size_t)4 * (3 * C * a.RX + 4 * NC * 256 + 64);  // 4 waves
    if (lds <= 163840) break;
  }
  if (YB < 1) return TB_ERR_UNSUPPORTED_SIZE;
  a.YB = YB > H ? H : YB;
  a.nyb = (H + a.YB - 1) / a.YB;
  a.zlen = tb::zseg(D, N * a.nyb * a.MG, 1, 2);
  a.ZS = (D + a.zlen - 1) / a.zlen;
  const int nl = (C * (a.YB + 2) * (Wd / 4) + 255) / 256;
  void (*kern)(S1Args) = nullptr;
#define TB_NL(k)                                                                                      \
  case k:                                                                                             \
    kern = add ? (G == 2 ? k_conv3d_mfma_s1<2, 5, k, 256, true> : k_conv3d_mfma_s1<4, 5, k, 256, true>) \
               : (G == 2 ? k_conv3d_mfma_s1<2, 5, k, 256> : k_conv3d_mfma_s1<4, 5, k, 256>);             \
    break;
  switch (nl) {
    TB_NL(1) TB_NL(2) TB_NL(3) TB_NL(4) TB_NL(5) TB_NL(6) TB_NL(7) TB_NL(8) TB_NL(9) TB_NL(10) TB_NL(11) TB_NL(12)
    default: return TB_ERR_UNSUPPORTED_SIZE;
  }
#undef TB_NL
  return tb::launch_lds(kern, dim3((unsigned)(N * a.nyb * a.MG * a.ZS)), dim3(256), lds,
                        reinterpret_cast<hipStream_t>(stream), a);
}
