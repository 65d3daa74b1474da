// kern_generic.hip -- direct-DFT fallback of the full-spectrum passes, for transform sizes the
// mixed-radix slab passes do not take: an axis length with a prime factor above 31, or a (W, D)
// slab whose half spectrum exceeds the LDS.  The reference's torch.fft.fftn takes any size
// (source_code/filters_and_operators.py:594-632); this path keeps that contract at O(n) work per
// coefficient and axis instead of raising.
//
// The spectrum is the FULL complex one, S[bc][h][w][d] (complex64), in two ping-pong buffers:
//   load x -> S0;  DFT along D, W, H (S0 -> S1 -> S0 -> S1);  op program on S1;  inverse DFT
//   along H, W, D (S1 -> S0 -> S1 -> S0);  y = Re(S0) / (H W D) with the zero D-padding and the
//   per-sample min/max keys.
// The op program is apply_ops (fft_core.h), the same symmetrised form the half-spectrum passes use:
// on a full Hermitian spectrum it keeps the spectrum Hermitian, so Re(IFFT) is the reference's
// `.real` exactly as on the half spectrum.
#include <hip/hip_runtime.h>

#include <cstring>

#include "kernels.h"

namespace tb {

namespace {

constexpr int NT_GEN = 256;

// One DFT along an axis: the volume is viewed as [A][n][Bi] and pencil q = (ao, bi) holds the n
// elements ao*n*Bi + bi + j*Bi.  A workgroup takes PW consecutive pencils: loads them and the
// twiddles into LDS (consecutive bi are adjacent in memory, so a tile load is coalesced; with Bi == 1
// a pencil is one contiguous row), then each output y[k] = sum_j s[j] w^(j k) is one thread's sum.
__global__ __launch_bounds__(NT_GEN) void k_gen_dft(const cf* __restrict__ in, cf* __restrict__ out,
                                                    const cf* __restrict__ tw, int n, int64_t A, int64_t Bi, int PW,
                                                    int inverse) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cf* twl = reinterpret_cast<cf*>(smem);
  cf* s = twl + n;  // [n][PW]
  const int tid = (int)threadIdx.x;
  const int64_t q0 = (int64_t)blockIdx.x * PW, nq = A * Bi;
  const int np = (nq - q0) < PW ? (int)(nq - q0) : PW;
  for (int j = tid; j < n; j += NT_GEN) {
    const cf w = tw[j];
    twl[j] = inverse ? conj(w) : w;  // exp(+-2 pi i j / n)
  }
  const int tot = n * PW;
  for (int idx = tid; idx < tot; idx += NT_GEN) {
    int p, j;
    if (Bi == 1) { p = idx / n; j = idx - p * n; }
    else { j = idx / PW; p = idx - j * PW; }
    cf v = mk(0.f, 0.f);
    if (p < np) {
      const int64_t q = q0 + p, ao = q / Bi, bi = q - ao * Bi;
      v = in[ao * n * Bi + bi + (int64_t)j * Bi];
    }
    s[j * PW + p] = v;
  }
  __syncthreads();
  for (int idx = tid; idx < tot; idx += NT_GEN) {
    int p, k;
    if (Bi == 1) { p = idx / n; k = idx - p * n; }
    else { k = idx / PW; p = idx - k * PW; }
    if (p >= np) continue;
    float ax = 0.f, ay = 0.f;
    int t = 0;  // (j k) mod n
    for (int j = 0; j < n; ++j) {
      const cf a = s[j * PW + p], w = twl[t];
      ax = fmaf(a.x, w.x, fmaf(-a.y, w.y, ax));
      ay = fmaf(a.x, w.y, fmaf(a.y, w.x, ay));
      t += k;
      t = t >= n ? t - n : t;
    }
    const int64_t q = q0 + p, ao = q / Bi, bi = q - ao * Bi;
    out[ao * n * Bi + bi + (int64_t)k * Bi] = mk(ax, ay);
  }
}

struct GenArgs {
  tb_plan_dev pl;
  const float* x;
  int64_t xsbc, xsh, xsw;
  float* y;
  int64_t ysbc, ysh, ysw;
  cf* S;
  int ypad, bc0, C, nbc;
  float scale;
  uint32_t* mm;
  double* out;
  BatchOps ops;
};

// x (any strides, contiguous D) -> S0 = (x, 0)
__global__ __launch_bounds__(NT_GEN) void k_gen_load(GenArgs) {
  const GenArgs& a = kargs<GenArgs>();
  const int H = a.pl.H, W = a.pl.W, D = a.pl.D;
  const int64_t n = (int64_t)H * W * D;
  const int bcl = (int)blockIdx.y, bc = a.bc0 + bcl;
  const float* xb = a.x + (int64_t)bc * a.xsbc;
  cf* Sb = a.S + (int64_t)bcl * n;
  for (int64_t e = (int64_t)blockIdx.x * NT_GEN + threadIdx.x; e < n; e += (int64_t)gridDim.x * NT_GEN) {
    const int64_t hw = e / D, d = e - hw * D, h = hw / W, w = hw - h * W;
    Sb[e] = mk(xb[h * a.xsh + w * a.xsw + d], 0.f);
  }
}

// the sample's op program on every coefficient of the full spectrum (in place)
__global__ __launch_bounds__(NT_GEN) void k_gen_ops(GenArgs) {
  const GenArgs& a = kargs<GenArgs>();
  const int H = a.pl.H, W = a.pl.W, D = a.pl.D;
  const int64_t n = (int64_t)H * W * D;
  const int bcl = (int)blockIdx.y;
  const int s = bcl / a.C, chan = bcl - s * a.C;  // sample within the run (bc0 = first sample * C)
  const tb_sample_ops& so = a.ops.s[s];
  cf* Sb = a.S + (int64_t)bcl * n;
  for (int64_t e = (int64_t)blockIdx.x * NT_GEN + threadIdx.x; e < n; e += (int64_t)gridDim.x * NT_GEN) {
    const int64_t hw = e / D;
    const int kd = (int)(e - hw * D), kh = (int)(hw / W), kw = (int)(hw - (int64_t)kh * W);
    Sb[e] = apply_ops(so, chan, Sb[e], freq_col(kw, kd, W, D), kh, H);
  }
}

// sum of log(|ops(K)| + 1e-10) over the full spectrum (tb_kspace_logabs_sum_f32)
__global__ __launch_bounds__(NT_GEN) void k_gen_logabs(GenArgs) {
  const GenArgs& a = kargs<GenArgs>();
  __shared__ double red[NT_GEN / 64];
  const int H = a.pl.H, W = a.pl.W, D = a.pl.D;
  const int64_t n = (int64_t)H * W * D;
  const int bcl = (int)blockIdx.y, bc = a.bc0 + bcl;
  const int s = bcl / a.C, chan = bcl - s * a.C;
  const tb_sample_ops& so = a.ops.s[s];
  const cf* Sb = a.S + (int64_t)bcl * n;
  double acc = 0.0;
  for (int64_t e = (int64_t)blockIdx.x * NT_GEN + threadIdx.x; e < n; e += (int64_t)gridDim.x * NT_GEN) {
    const int64_t hw = e / D;
    const int kd = (int)(e - hw * D), kh = (int)(hw / W), kw = (int)(hw - (int64_t)kh * W);
    const cf v = apply_ops(so, chan, Sb[e], freq_col(kw, kd, W, D), kh, H);
    acc += (double)logf(f32_sqrt(v.x * v.x + v.y * v.y) + 1e-10f);
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < NT_GEN / 64; ++w) acc += red[w];
    atomicAdd(&a.out[bc], acc);
  }
}

// y = Re(S0) * scale, zero D-padding, per-sample min/max keys (one sample per block)
__global__ __launch_bounds__(NT_GEN) void k_gen_store(GenArgs) {
  const GenArgs& a = kargs<GenArgs>();
  __shared__ float red[2 * NT_GEN / 64];
  const int H = a.pl.H, W = a.pl.W, D = a.pl.D;
  const int len = D + a.ypad;
  const int64_t n = (int64_t)H * W * len;
  const int bcl = (int)blockIdx.y, bc = a.bc0 + bcl;
  const cf* Sb = a.S + (int64_t)bcl * H * W * D;
  float* yb = a.y + (int64_t)bc * a.ysbc;
  float lo = 3.402823466e38f, hi = -3.402823466e38f;
  for (int64_t e = (int64_t)blockIdx.x * NT_GEN + threadIdx.x; e < n; e += (int64_t)gridDim.x * NT_GEN) {
    const int64_t hw = e / len, d = e - hw * len, h = hw / W, w = hw - h * W;
    float v = 0.f;
    if (d < D) {
      v = Sb[hw * D + d].x * a.scale;
      lo = fminf(lo, v);
      hi = fmaxf(hi, v);
    }
    yb[h * a.ysh + w * a.ysw + d] = v;
  }
  if (a.mm) block_minmax_atomic<NT_GEN>(lo, hi, red, a.mm + 2 * (bc / a.C));
}

// Mask gradient on the full spectra X = S, G = Sg ([nbc][H][W][D], natural order): per (mask channel
// slot, coefficient with kd <= D/2) the sum over the launch group's volumes of Re(X conj G), scaled by
// 1 / N, to the centred position of f and, when kd is not self-conjugate (kd = 0, kd = D/2 with D even),
// of -f -- the write-once rule of maskgrad.h: one thread and one write per element of dM, f and -f
// bit-equal.
struct GenMaskGradArgs {
  const cf* S;
  const cf* Sg;
  float* dM;
  int H, W, D, C, nb, Cm, accumulate;
  float scale;
  int cplx;  // dM complex64: conj(X) G / N at f, its conjugate at -f (the TB_OP_CMASK gradient)
};
__global__ __launch_bounds__(NT_GEN) void k_gen_maskgrad(GenMaskGradArgs a) {
  const int H = a.H, W = a.W, D = a.D, Dh = D / 2 + 1;
  const int64_t n = (int64_t)H * W * D, nh = (int64_t)H * W * Dh;
  const int slot = (int)blockIdx.y;
  const int nv = a.Cm == 1 ? a.nb * a.C : a.nb;
  const int Dtop = (D % 2 == 0) ? D / 2 : -1;
  for (int64_t e = (int64_t)blockIdx.x * NT_GEN + threadIdx.x; e < nh; e += (int64_t)gridDim.x * NT_GEN) {
    const int64_t hw = e / Dh;
    const int kd = (int)(e - hw * Dh), kh = (int)(hw / W), kw = (int)(hw - (int64_t)kh * W);
    const int64_t src = hw * D + kd;
    float acc = 0.f, acc2 = 0.f;
    for (int k = 0; k < nv; ++k) {
      const int64_t vol = a.Cm == 1 ? k : (int64_t)k * a.C + slot;
      const cf x = a.S[vol * n + src], g = a.Sg[vol * n + src];
      acc += x.x * g.x + x.y * g.y;
      acc2 += x.x * g.y - x.y * g.x;
    }
    const float v = acc * a.scale;
    if (a.cplx) {
      const float w = acc2 * a.scale;
      cf* p = reinterpret_cast<cf*>(a.dM) + mask_index((int64_t)slot * H, kh, kw, kd, H, W, D);
      *p = a.accumulate ? mk(p->x + v, p->y + w) : mk(v, w);
      if (kd != 0 && kd != Dtop) {
        cf* q = reinterpret_cast<cf*>(a.dM) + mask_index((int64_t)slot * H, negk(kh, H), negk(kw, W), D - kd, H, W, D);
        *q = a.accumulate ? mk(q->x + v, q->y - w) : mk(v, -w);
      }
      continue;
    }
    float* p = a.dM + mask_index((int64_t)slot * H, kh, kw, kd, H, W, D);
    *p = a.accumulate ? *p + v : v;
    if (kd != 0 && kd != Dtop) {
      float* q = a.dM + mask_index((int64_t)slot * H, negk(kh, H), negk(kw, W), D - kd, H, W, D);
      *q = a.accumulate ? *q + v : v;
    }
  }
}

// Centred spectrum K[bc][H][W][D] (spectrum.h) and the full natural-order spectrum S[nbc][H][W][D].
// Export: per coefficient with kd <= D/2, S(f) to the centred position of f and, when kd is not
// self-conjugate, its conjugate to the position of -f: one thread and one write per element of K.
// Import: a shifted gather, S(f) = K[s(f)]; k_gen_store's real part symmetrises.
struct GenSpectrumArgs {
  cf* S;
  cf* K;
  int H, W, D, bc0;
};
__global__ __launch_bounds__(NT_GEN) void k_gen_export(GenSpectrumArgs a) {
  const int H = a.H, W = a.W, D = a.D, Dh = D / 2 + 1;
  const int64_t n = (int64_t)H * W * D, nh = (int64_t)H * W * Dh;
  const int bcl = (int)blockIdx.y;
  const cf* Sb = a.S + (int64_t)bcl * n;
  cf* Kb = a.K + (int64_t)(a.bc0 + bcl) * n;
  for (int64_t e = (int64_t)blockIdx.x * NT_GEN + threadIdx.x; e < nh; e += (int64_t)gridDim.x * NT_GEN) {
    const int64_t hw = e / Dh;
    const int kd = (int)(e - hw * Dh), kh = (int)(hw / W), kw = (int)(hw - (int64_t)kh * W);
    const cf v = Sb[hw * D + kd];
    Kb[mask_index(0, kh, kw, kd, H, W, D)] = v;
    if (kd != 0 && 2 * kd != D) Kb[mask_index(0, negk(kh, H), negk(kw, W), D - kd, H, W, D)] = conj(v);
  }
}
__global__ __launch_bounds__(NT_GEN) void k_gen_import(GenSpectrumArgs a) {
  const int H = a.H, W = a.W, D = a.D;
  const int64_t n = (int64_t)H * W * D;
  const int bcl = (int)blockIdx.y;
  cf* Sb = a.S + (int64_t)bcl * n;
  const cf* Kb = a.K + (int64_t)(a.bc0 + bcl) * n;
  for (int64_t e = (int64_t)blockIdx.x * NT_GEN + threadIdx.x; e < n; e += (int64_t)gridDim.x * NT_GEN) {
    const int64_t hw = e / D;
    const int kd = (int)(e - hw * D), kh = (int)(hw / W), kw = (int)(hw - (int64_t)kh * W);
    Sb[e] = Kb[mask_index(0, kh, kw, kd, H, W, D)];
  }
}

// Amplitude mixing (ampmix.h) on full natural-order spectra [bc][H][W][D] indexed by the absolute bc: the
// closed form of ampmix_unit per coefficient, the mask gathered at s(f) and s(-f).  Every coefficient of the
// full spectrum is written by its own thread (f and -f evaluate the same expression on conjugate inputs),
// k_gen_store's real part takes the rest.
template <bool BWD, bool GY>
__device__ __forceinline__ void gen_ampmix_body(const AmpMixArgs& a) {
  const int H = a.pl.H, W = a.pl.W, D = a.pl.D;
  const int64_t n = (int64_t)H * W * D;
  const int bc = a.bc0 + (int)blockIdx.y;
  const int b = bc / a.C, ch = bc - b * a.C;
  const int ybc = am_partner(a, b) * a.C + ch;
  const float lam = a.lam[b];
  const float* __restrict__ Mb = a.M + (a.Cm == 1 ? 0 : (int64_t)ch * n);
  const cf* Xb = a.Sx + (int64_t)bc * n;
  const cf* Yb = a.Sy + (int64_t)ybc * n;
  cf* Ob = a.So + (int64_t)bc * n;
  for (int64_t e = (int64_t)blockIdx.x * NT_GEN + threadIdx.x; e < n; e += (int64_t)gridDim.x * NT_GEN) {
    const int64_t hw = e / D;
    const int kd = (int)(e - hw * D), kh = (int)(hw / W), kw = (int)(hw - (int64_t)kh * W);
    const float m = lam * mask_factor(Mb[mask_index(0, kh, kw, kd, H, W, D)],
                                      Mb[mask_index(0, negk(kh, H), negk(kw, W), negk(kd, D), H, W, D)]);
    if (BWD) {
      cf gy;
      Ob[e] = am_mix_bwd<GY>(Xb[e], Yb[e], Ob[e], m, gy);
      if (GY) a.Sgy[(int64_t)bc * n + e] = gy;
    } else {
      Ob[e] = am_mix(Xb[e], Yb[e], m);
    }
  }
}
__global__ __launch_bounds__(NT_GEN) void k_gen_ampmix(AmpMixArgs) { gen_ampmix_body<false, false>(kargs<AmpMixArgs>()); }
template <bool GY>
__global__ __launch_bounds__(NT_GEN) void k_gen_ampmix_bwd(AmpMixArgs) { gen_ampmix_body<true, GY>(kargs<AmpMixArgs>()); }

// out[(j, ch)][e] = sum over the samples b with partner j of Sgy[(b, ch)][e], in the order of b
__global__ __launch_bounds__(NT_GEN) void k_ampmix_gysum(const cf* __restrict__ Sgy, cf* __restrict__ out,
                                                         const int* __restrict__ perm, int B, int C, int bc0,
                                                         int64_t vstride) {
  const int bc = bc0 + (int)blockIdx.y;
  const int j = bc / C, ch = bc - j * C;
  for (int64_t e = (int64_t)blockIdx.x * NT_GEN + threadIdx.x; e < vstride; e += (int64_t)gridDim.x * NT_GEN)
    out[(int64_t)bc * vstride + e] = am_gysum(Sgy, perm, B, C, j, ch, vstride, e);
}

unsigned gen_blocks(int64_t n) {
  const int64_t b = (n + NT_GEN * 4 - 1) / (NT_GEN * 4);
  return (unsigned)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

// one axis of every channel-volume of the run: [nbc * before][n][after]
hipError_t gen_axis(const cf* in, cf* out, const cf* tw, int n, int64_t A, int64_t Bi, bool inverse, hipStream_t st) {
  int PW = Bi == 1 ? 4 : 16;
  while (PW > 1 && (size_t)n * (PW + 1) * sizeof(cf) > 65536) PW >>= 1;
  const size_t lds = (size_t)n * (PW + 1) * sizeof(cf);
  if (lds > 163840) return hipErrorInvalidValue;
  hipError_t e = allow_lds(k_gen_dft, lds);
  if (e != hipSuccess) return e;
  const int64_t nq = A * Bi, nb = (nq + PW - 1) / PW;
  if (nb >= (1LL << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_gen_dft, dim3((unsigned)nb), dim3(NT_GEN), lds, st, in, out, tw, n, A, Bi, PW, inverse ? 1 : 0);
  return hipGetLastError();
}

// forward DFT of the run's channel-volumes into S1 (= S0 + nbc H W D)
hipError_t gen_forward(GenArgs& a, hipStream_t st) {
  const int H = a.pl.H, W = a.pl.W, D = a.pl.D;
  const int64_t n = (int64_t)H * W * D;
  cf* S0 = a.S;
  cf* S1 = a.S + (int64_t)a.nbc * n;
  hipLaunchKernelGGL(k_gen_load, dim3(gen_blocks(n), a.nbc), dim3(NT_GEN), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = gen_axis(S0, S1, a.pl.tw[2], D, (int64_t)a.nbc * H * W, 1, false, st);
  if (e == hipSuccess) e = gen_axis(S1, S0, a.pl.tw[1], W, (int64_t)a.nbc * H, D, false, st);
  if (e == hipSuccess) e = gen_axis(S0, S1, a.pl.tw[0], H, a.nbc, (int64_t)W * D, false, st);
  return e;
}

}  // namespace

size_t gen_workspace_bytes(int H, int W, int D, int bc) { return (size_t)2 * bc * H * W * D * sizeof(cf); }

hipError_t launch_gen_filter(const GenLaunch& g, hipStream_t st) {
  GenArgs a;
  std::memset(&a, 0, sizeof(a));
  a.pl = g.pl;
  a.x = g.x;
  a.xsbc = g.xs[0]; a.xsh = g.xs[1]; a.xsw = g.xs[2];
  a.y = g.y;
  a.ysbc = g.ys[0]; a.ysh = g.ys[1]; a.ysw = g.ys[2];
  a.S = g.S;
  a.ypad = g.ypad;
  a.bc0 = g.bc0;
  a.C = g.C;
  a.nbc = g.nbc;
  a.scale = (float)(1.0 / ((double)g.pl.H * (double)g.pl.W * (double)g.pl.D));
  a.mm = g.mm;
  a.ops = *g.ops;
  const int H = a.pl.H, W = a.pl.W, D = a.pl.D;
  const int64_t n = (int64_t)H * W * D;
  cf* S0 = a.S;
  cf* S1 = a.S + (int64_t)a.nbc * n;
  hipError_t e = gen_forward(a, st);
  if (e != hipSuccess) return e;
  a.S = S1;
  hipLaunchKernelGGL(k_gen_ops, dim3(gen_blocks(n), a.nbc), dim3(NT_GEN), 0, st, a);
  e = hipGetLastError();
  if (e == hipSuccess) e = gen_axis(S1, S0, a.pl.tw[0], H, a.nbc, (int64_t)W * D, true, st);
  if (e == hipSuccess) e = gen_axis(S0, S1, a.pl.tw[1], W, (int64_t)a.nbc * H, D, true, st);
  if (e == hipSuccess) e = gen_axis(S1, S0, a.pl.tw[2], D, (int64_t)a.nbc * H * W, 1, true, st);
  if (e != hipSuccess) return e;
  a.S = S0;
  hipLaunchKernelGGL(k_gen_store, dim3(gen_blocks(n), a.nbc), dim3(NT_GEN), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_gen_logabs(const GenLaunch& g, double* out, hipStream_t st) {
  GenArgs a;
  std::memset(&a, 0, sizeof(a));
  a.pl = g.pl;
  a.x = g.x;
  a.xsbc = g.xs[0]; a.xsh = g.xs[1]; a.xsw = g.xs[2];
  a.S = g.S;
  a.bc0 = g.bc0;
  a.C = g.C;
  a.nbc = g.nbc;
  a.out = out;
  a.ops = *g.ops;
  const int64_t n = (int64_t)a.pl.H * a.pl.W * a.pl.D;
  hipError_t e = gen_forward(a, st);
  if (e != hipSuccess) return e;
  a.S = g.S + (int64_t)a.nbc * n;
  hipLaunchKernelGGL(k_gen_logabs, dim3(gen_blocks(n), a.nbc), dim3(NT_GEN), 0, st, a);
  return hipGetLastError();
}

// buffers b0, b1, b2 of nbc H W D coefficients: x transforms in (b1, b2) and leaves X in b2, g then
// transforms in (b0, b1) and leaves G in b1
size_t gen_maskgrad_workspace_bytes(int H, int W, int D, int bc) { return (size_t)3 * bc * H * W * D * sizeof(cf); }

hipError_t launch_gen_spectrum(const GenLaunch& g, hipStream_t st) {
  GenArgs a;
  std::memset(&a, 0, sizeof(a));
  a.pl = g.pl;
  a.x = g.x;
  a.xsbc = g.xs[0]; a.xsh = g.xs[1]; a.xsw = g.xs[2];
  a.S = g.S;
  a.bc0 = g.bc0;
  a.C = g.C;
  a.nbc = g.nbc;
  return gen_forward(a, st);
}

hipError_t launch_gen_maskgrad(const tb_plan_dev& pl, const cf* X, const cf* G, float* dM, int C, int nb, int Cm,
                               int accumulate, hipStream_t st, int cplx) {
  const int64_t n = (int64_t)pl.H * pl.W * pl.D;
  const GenMaskGradArgs m{X, G, dM, pl.H, pl.W, pl.D, C, nb, Cm, accumulate,
                          (float)(1.0 / ((double)pl.H * (double)pl.W * (double)pl.D)), cplx};
  hipLaunchKernelGGL(k_gen_maskgrad, dim3(gen_blocks(n / 2 + 1), Cm), dim3(NT_GEN), 0, st, m);
  return hipGetLastError();
}

hipError_t launch_gen_export(const GenLaunch& g, cf* K, hipStream_t st) {
  const int64_t n = (int64_t)g.pl.H * g.pl.W * g.pl.D;
  const GenSpectrumArgs m{g.S + (int64_t)g.nbc * n, K, g.pl.H, g.pl.W, g.pl.D, g.bc0};
  hipLaunchKernelGGL(k_gen_export, dim3(gen_blocks(n / 2 + 1), g.nbc), dim3(NT_GEN), 0, st, m);
  return hipGetLastError();
}

hipError_t launch_gen_import(const GenLaunch& g, const cf* K, hipStream_t st) {
  GenArgs a;
  std::memset(&a, 0, sizeof(a));
  a.pl = g.pl;
  a.y = g.y;
  a.ysbc = g.ys[0]; a.ysh = g.ys[1]; a.ysw = g.ys[2];
  a.ypad = g.ypad;
  a.bc0 = g.bc0;
  a.C = g.C;
  a.nbc = g.nbc;
  a.scale = (float)(1.0 / ((double)g.pl.H * (double)g.pl.W * (double)g.pl.D));
  const int H = a.pl.H, W = a.pl.W, D = a.pl.D;
  const int64_t n = (int64_t)H * W * D;
  cf* S0 = g.S;
  cf* S1 = g.S + (int64_t)a.nbc * n;
  const GenSpectrumArgs m{S1, const_cast<cf*>(K), H, W, D, g.bc0};
  hipLaunchKernelGGL(k_gen_import, dim3(gen_blocks(n), a.nbc), dim3(NT_GEN), 0, st, m);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = gen_axis(S1, S0, a.pl.tw[0], H, a.nbc, (int64_t)W * D, true, st);
  if (e == hipSuccess) e = gen_axis(S0, S1, a.pl.tw[1], W, (int64_t)a.nbc * H, D, true, st);
  if (e == hipSuccess) e = gen_axis(S1, S0, a.pl.tw[2], D, (int64_t)a.nbc * H * W, 1, true, st);
  if (e != hipSuccess) return e;
  a.S = S0;
  hipLaunchKernelGGL(k_gen_store, dim3(gen_blocks(n), a.nbc), dim3(NT_GEN), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_gen_spectrum_to(const GenLaunch& g, cf* dst, hipStream_t st) {
  GenArgs a;
  std::memset(&a, 0, sizeof(a));
  a.pl = g.pl;
  a.x = g.x;
  a.xsbc = g.xs[0]; a.xsh = g.xs[1]; a.xsw = g.xs[2];
  a.S = g.S;
  a.bc0 = g.bc0;
  a.C = g.C;
  a.nbc = g.nbc;
  const int H = a.pl.H, W = a.pl.W, D = a.pl.D;
  const int64_t n = (int64_t)H * W * D;
  cf* tmp = g.S;
  cf* out = dst + (int64_t)g.bc0 * n;
  hipLaunchKernelGGL(k_gen_load, dim3(gen_blocks(n), a.nbc), dim3(NT_GEN), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = gen_axis(tmp, out, a.pl.tw[2], D, (int64_t)a.nbc * H * W, 1, false, st);
  if (e == hipSuccess) e = gen_axis(out, tmp, a.pl.tw[1], W, (int64_t)a.nbc * H, D, false, st);
  if (e == hipSuccess) e = gen_axis(tmp, out, a.pl.tw[0], H, a.nbc, (int64_t)W * D, false, st);
  return e;
}

hipError_t launch_gen_ampmix(const AmpMixArgs& a, int nbc, hipStream_t st) {
  const int64_t n = (int64_t)a.pl.H * a.pl.W * a.pl.D;
  hipLaunchKernelGGL(k_gen_ampmix, dim3(gen_blocks(n), nbc), dim3(NT_GEN), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_gen_ampmix_bwd(const AmpMixArgs& a, int nbc, hipStream_t st) {
  const int64_t n = (int64_t)a.pl.H * a.pl.W * a.pl.D;
  if (a.need_gy)
    hipLaunchKernelGGL(k_gen_ampmix_bwd<true>, dim3(gen_blocks(n), nbc), dim3(NT_GEN), 0, st, a);
  else
    hipLaunchKernelGGL(k_gen_ampmix_bwd<false>, dim3(gen_blocks(n), nbc), dim3(NT_GEN), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_gen_inverse(const GenLaunch& g, cf* src, hipStream_t st) {
  GenArgs a;
  std::memset(&a, 0, sizeof(a));
  a.pl = g.pl;
  a.y = g.y;
  a.ysbc = g.ys[0]; a.ysh = g.ys[1]; a.ysw = g.ys[2];
  a.ypad = g.ypad;
  a.bc0 = g.bc0;
  a.C = g.C;
  a.nbc = g.nbc;
  a.scale = (float)(1.0 / ((double)g.pl.H * (double)g.pl.W * (double)g.pl.D));
  const int H = a.pl.H, W = a.pl.W, D = a.pl.D;
  const int64_t n = (int64_t)H * W * D;
  cf* in = src + (int64_t)g.bc0 * n;
  cf* tmp = g.S;
  hipError_t e = gen_axis(in, tmp, a.pl.tw[0], H, a.nbc, (int64_t)W * D, true, st);
  if (e == hipSuccess) e = gen_axis(tmp, in, a.pl.tw[1], W, (int64_t)a.nbc * H, D, true, st);
  if (e == hipSuccess) e = gen_axis(in, tmp, a.pl.tw[2], D, (int64_t)a.nbc * H * W, 1, true, st);
  if (e != hipSuccess) return e;
  a.S = tmp;
  hipLaunchKernelGGL(k_gen_store, dim3(gen_blocks(n), a.nbc), dim3(NT_GEN), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_ampmix_gysum(const cf* Sgy, cf* out, const int* perm, int B, int C, int b0, int nb, int64_t vstride,
                               hipStream_t st) {
  hipLaunchKernelGGL(k_ampmix_gysum, dim3(gen_blocks(vstride), nb * C), dim3(NT_GEN), 0, st, Sgy, out, perm, B, C,
                     b0 * C, vstride);
  return hipGetLastError();
}

}  // namespace tb
