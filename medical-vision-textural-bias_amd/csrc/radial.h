// radial.h -- radial profiles in centred k-space: K bins of width dr over the integer radius
//     r2 = k_h^2 + k_w^2 + k_d^2,   k_a = s_a - floor(n_a / 2) the signed index of the centred layout
// (disk_mask's metric; size-1 axes contribute 0).  u = sqrt((float)r2) * inv_dr with
// inv_dr = (float)(1.0 / dr) formed on the host: one correctly rounded square root and one multiply, so
// numpy float32 and the device agree bit for bit.  r2 is invariant under f -> -f.
//   TB_RADIAL_NEAREST  b = min((int)u, K-1), weight 1
//   TB_RADIAL_LINEAR   b0 = (int)u; b0 >= K-1: weight 1 on K-1; else t = u - (float)b0, 1-t on b0, t on b0+1
// The last bin is clamped in both modes; the weights of an element sum to 1.
//
// radial_unit: the fused reduction.  The tiles, the [H][2T] LDS image, the single DIF along H, the
// register accumulation over the launch group's volumes and the loads in flight are maskgrad_unit's
// (maskgrad.h); instead of storing dM the unit reduces Re(X conj G) -- |X|^2 with SELF -- into its K
// bins.  A stored coefficient counts twice when kd is not self-conjugate (it stands for f and -f, which
// share r2) and once in the self-conjugate columns.  The reduction has a fixed order and no
// floating-point atomics: every thread writes its values, already split by the two weights, with their
// bin back over the tile in LDS; thread k then scans the entries in index order and adds those of bin k
// in float64, skipping the groups of entries that cannot hold its bin (rad_scan).  A unit walks `tpg` consecutive tiles in order and keeps the K float64 sums in LDS
// across them; its partial goes to part[unit][slot][K], which radial_sum adds in unit order.
//
// radial_bin_unit: the same scan for a real centred array A[Cm][H][W][D] (the adjoint of the expansion,
// the shell counts, the reduction of the composed route); radial_expand: M[c][s] = sum_k w_k(s) p[c][k].
#pragma once

#include "fft_core.h"
#include "maskgrad.h"

namespace tb {

struct RadialW {
  int b0;        // first bin; the second is b0 + 1 when w1 != 0
  float w0, w1;  // w0 + w1 = 1
};

// Correctly rounded on the device too: fft_core.h's f32_sqrt compiles to the hardware's 1-ulp v_sqrt_f32
// there, which would move an element across a bin edge (or change t) against the float32 definition.
TB_HD float rad_sqrt(float a) { return __builtin_sqrtf(a); }

// unshifted frequency (kh, kw, kd) -> bins and weights.  K < 2^24.
TB_HD RadialW radial_weights(int kh, int kw, int kd, int H, int W, int D, float inv_dr, int K, int mode) {
#if defined(__clang__)
#pragma clang fp contract(off)  // u is the rounded product: u - b0 must not become fma(sqrt, inv_dr, -b0)
#endif
  const int qh = shifted(kh, H) - H / 2, qw = shifted(kw, W) - W / 2, qd = shifted(kd, D) - D / 2;
  const int64_t r2 = (int64_t)qh * qh + (int64_t)qw * qw + (int64_t)qd * qd;
  const float u = rad_sqrt((float)r2) * inv_dr;
  RadialW r;
  if (!(u < (float)(K - 1))) {  // (int)u >= K-1, also for u past the int range
    r.b0 = K - 1; r.w0 = 1.f; r.w1 = 0.f;
    return r;
  }
  r.b0 = (int)u;
  if (mode == TB_RADIAL_NEAREST) { r.w0 = 1.f; r.w1 = 0.f; return r; }
  const float t = u - (float)r.b0;
  r.w0 = 1.f - t;
  r.w1 = t;
  return r;
}
// element (sh, sw, sd) of the centred layout
TB_HD RadialW radial_weights_centred(int sh, int sw, int sd, int H, int W, int D, float inv_dr, int K, int mode) {
  const int kh = sh - H / 2, kw = sw - W / 2, kd = sd - D / 2;
  return radial_weights(kh < 0 ? kh + H : kh, kw < 0 ? kw + W : kw, kd < 0 ? kd + D : kd, H, W, D, inv_dr, K, mode);
}

// one value split over its bins; b0 < 0: an empty entry
struct RadEnt {
  float v0, v1;
  int b0, pad;
};

TB_HD RadEnt rad_ent(const RadialW& w, float v) {
  RadEnt e;
  e.v0 = v * w.w0;
  e.v1 = v * w.w1;
  e.b0 = w.b0;
  e.pad = 0;
  return e;
}
TB_HD RadEnt rad_empty() {
  RadEnt e;
  e.v0 = 0.f; e.v1 = 0.f; e.b0 = -2; e.pad = 0;
  return e;
}

// bins[k] += the entries of bin k, in index order, for the k this thread owns (k = tid, tid + nthreads, ...).
// The entries are taken in groups of RAD_GRP consecutive ones; rng[j] holds the bins group j touches, and a
// thread skips the groups that cannot hold its bin -- neighbours in a tile row or along D lie at nearly the
// same radius, so it reads a few groups instead of all n entries.  A skipped group has no entry of bin k,
// so the sum and its order are those of the plain scan.  Call after a barrier that follows the entry writes.
constexpr int RAD_GRP = 8;
struct RadRange {
  int lo, hi;
};
template <class Ctx>
TB_HD void rad_scan(Ctx& ctx, const RadEnt* ent, int n, RadRange* rng, double* bins, int K) {
  const int ng = (n + RAD_GRP - 1) / RAD_GRP;
  for (int j = ctx.tid; j < ng; j += ctx.nthreads) {
    RadRange r{0x7fffffff, -1};
    const int e1 = (j + 1) * RAD_GRP < n ? (j + 1) * RAD_GRP : n;
    for (int e = j * RAD_GRP; e < e1; ++e) {
      const int b = ent[e].b0;
      if (b < 0) continue;
      r.lo = b < r.lo ? b : r.lo;
      r.hi = b + 1 > r.hi ? b + 1 : r.hi;
    }
    rng[j] = r;
  }
  ctx.sync();
  for (int k = ctx.tid; k < K; k += ctx.nthreads) {
    double s = bins[k];
    for (int j = 0; j < ng; ++j) {
      const RadRange r = rng[j];
      if (k < r.lo || k > r.hi) continue;
      const int e1 = (j + 1) * RAD_GRP < n ? (j + 1) * RAD_GRP : n;
      for (int e = j * RAD_GRP; e < e1; ++e) {
        const RadEnt q = ent[e];
        if (q.b0 == k) s += (double)q.v0;
        else if (q.b0 + 1 == k) s += (double)q.v1;   // v1 = 0 where there is no second bin
      }
    }
    bins[k] = s;
  }
}

struct RadialArgs {
  tb_plan_dev pl;
  const cf* Sx;   // half spectra after pass A, [bc][H][W][D/2+1], indexed by the absolute bc
  const cf* Sg;   // unused with SELF
  double* part;   // [units][slots][K]
  int bc0, C, nb, Cm;  // launch group, as MaskGradArgs; SELF: slot = volume of the group, bc0 + slot
  int T;          // tile width in columns; H * T <= MG_MAX_TILE
  int tpg;        // tiles per unit
  int K, mode;
  float inv_dr;
};

// LDS of a unit, in cf: the [H][2T] tile image with its tables (the RadEnt entries lie over the tile),
// then the K float64 sums and the group ranges of the scan
TB_HD int radial_lds_cf(int H, int T, int K) {
  return tile_geo(H, 2 * T).total_cf + 1 + K + (H * T + RAD_GRP - 1) / RAD_GRP;
}

#if defined(__HIPCC__)
#define TB_RD_EACH(i) \
  _Pragma("unroll") for (int i = 0; i < (NE > 0 ? NE : (1 << 30)) && (NE > 0 || i < ne); ++i)
#else
#define TB_RD_EACH(i) for (int i = 0; i < (NE > 0 ? NE : (1 << 30)) && (NE > 0 || i < ne); ++i)
#endif

// xa, ga: NE (or ne) complex slots per thread (ga unused with SELF); acc: as many floats
template <class Ctx, int RS, int NE, bool PF, bool SELF>
TB_HD void radial_unit(Ctx& ctx, cf* lds, const RadialArgs& a, int slot, int unit, int nslots, int ne, cf* xa, cf* ga,
                       float* acc) {
  const tb_plan_dev& pl = a.pl;
  const int H = pl.H, W = pl.W, D = pl.D, Dh = D / 2 + 1, T = a.T, K = a.K;
  const int LS = SELF ? T : 2 * T;  // row stride of the LDS image
  const int ncols_all = W * Dh;
  const int ntiles = (ncols_all + T - 1) / T;
  const TileGeo tg = tile_geo(H, 2 * T);
  cf* tw = lds + tg.off_tw;
  int* irev = reinterpret_cast<int*>(lds + tg.off_irev);
  double* bins = reinterpret_cast<double*>(lds + ((tg.total_cf + 1) & ~1));
  RadRange* rng = reinterpret_cast<RadRange*>(bins + K);
  RadEnt* ent = reinterpret_cast<RadEnt*>(lds);
  for (int i = ctx.tid; i < H; i += ctx.nthreads) { tw[i] = pl.tw[0][i]; irev[i] = pl.irev_h[i]; }
  for (int k = ctx.tid; k < K; k += ctx.nthreads) bins[k] = 0.0;
  const int64_t vstride = (int64_t)H * ncols_all;
  const int nv = SELF ? 1 : (a.Cm == 1 ? a.nb * a.C : a.nb);
  const MaskGradArgs va{pl, nullptr, nullptr, nullptr, a.bc0, a.C, a.nb, a.Cm, T, 0, 0.f, 0};
  const int Dtop = (D % 2 == 0) ? D / 2 : -1;
  const int t_end = (unit + 1) * a.tpg < ntiles ? (unit + 1) * a.tpg : ntiles;
  for (int tile = unit * a.tpg; tile < t_end; ++tile) {
    const int j0 = tile * T;
    const int nc = (ncols_all - j0) < T ? (ncols_all - j0) : T;
    const MgTile g{ctx.tid, ctx.nthreads, T, nc, H * T, ncols_all, FastDiv::make(T)};
    TB_RD_EACH(i) acc[i] = 0.f;
    if (PF) {
      const int64_t v0 = SELF ? a.bc0 + slot : mg_volume(va, slot, 0);
      mg_load<NE>(g, ne, a.Sx + v0 * vstride + j0, xa);
      if (!SELF) mg_load<NE>(g, ne, a.Sg + v0 * vstride + j0, ga);
    }
    for (int k = 0; k < nv; ++k) {
      if (!PF) {
        const int64_t v = SELF ? a.bc0 + slot : mg_volume(va, slot, k);
        mg_load<NE>(g, ne, a.Sx + v * vstride + j0, xa);
        if (!SELF) mg_load<NE>(g, ne, a.Sg + v * vstride + j0, ga);
      }
      TB_RD_EACH(i) {
        int hh, c;
        if (g.at(i, hh, c)) {
          lds[hh * LS + c] = xa[i];
          if (!SELF) lds[hh * LS + c + nc] = ga[i];
        }
      }
      ctx.sync();
      if (PF && k + 1 < nv) {  // in flight during the transform
        const int64_t v = mg_volume(va, slot, k + 1);
        mg_load<NE>(g, ne, a.Sx + v * vstride + j0, xa);
        if (!SELF) mg_load<NE>(g, ne, a.Sg + v * vstride + j0, ga);
      }
      fft_dif<Ctx, RS>(ctx, lds, tw, pl.ax[0], SELF ? nc : 2 * nc, TileAddr{LS}, true);
      TB_RD_EACH(i) {
        int hh, c;
        if (g.at(i, hh, c)) {
          const cf x = lds[hh * LS + c];
          if (SELF) {
            acc[i] += x.x * x.x + x.y * x.y;
          } else {
            const cf v = lds[hh * LS + c + nc];
            acc[i] += x.x * v.x + x.y * v.y;
          }
        }
      }
      ctx.sync();
    }
    // the tile's values, weighted by their multiplicity and split over their bins, over the tile in LDS
    TB_RD_EACH(i) {
      const int t = ctx.tid + i * ctx.nthreads;
      if (t >= H * T) continue;
      int hp, c;
      RadEnt e = rad_empty();
      if (g.at(i, hp, c)) {
        const int j = j0 + c;
        const int wp = j / Dh, kd = j - wp * Dh;
        const RadialW w = radial_weights(irev[hp], pl.irev_w[wp], kd, H, W, D, a.inv_dr, K, a.mode);
        e = rad_ent(w, (kd != 0 && kd != Dtop) ? 2.f * acc[i] : acc[i]);
      }
      ent[t] = e;
    }
    ctx.sync();
    rad_scan(ctx, ent, H * T, rng, bins, K);
    ctx.sync();
  }
  double* out = a.part + ((int64_t)unit * nslots + slot) * K;
  for (int k = ctx.tid; k < K; k += ctx.nthreads) out[k] = bins[k];
}

#undef TB_RD_EACH

// ------------------------------------------------------------------ dense pair
struct RadialDenseArgs {
  int H, W, D, Cm, K, mode;
  float inv_dr;
  const float* src;  // expand: p[Cm][K];  bin: A[Cm][H][W][D]
  float* M;          // expand: M[Cm][H][W][D]
  double* part;      // bin: [units][Cm][K]
  int chunk, cpu;    // bin: elements per chunk (<= RB_CHUNK), chunks per unit
};

constexpr int RB_CHUNK = 2048;

TB_HD float radial_expand_at(const RadialDenseArgs& a, const float* p, int64_t s) {
  const int sd = (int)(s % a.D);
  const int64_t r = s / a.D;
  const int sw = (int)(r % a.W), sh = (int)(r / a.W);
  const RadialW w = radial_weights_centred(sh, sw, sd, a.H, a.W, a.D, a.inv_dr, a.K, a.mode);
  return w.w1 == 0.f ? p[w.b0] : w.w0 * p[w.b0] + w.w1 * p[w.b0 + 1];
}

// unit `unit` of channel c: chunks [unit cpu, (unit + 1) cpu) of `chunk` consecutive elements each;
// ent: chunk entries, bins: K sums, rng: ceil(chunk / RAD_GRP) group ranges (LDS)
template <class Ctx>
TB_HD void radial_bin_unit(Ctx& ctx, RadEnt* ent, double* bins, RadRange* rng, const RadialDenseArgs& a, int c, int unit) {
  const int64_t N = (int64_t)a.H * a.W * a.D;
  const float* A = a.src + (int64_t)c * N;
  for (int k = ctx.tid; k < a.K; k += ctx.nthreads) bins[k] = 0.0;
  for (int q = 0; q < a.cpu; ++q) {
    const int64_t s0 = ((int64_t)unit * a.cpu + q) * a.chunk;
    if (s0 >= N) break;
    const int n = (N - s0) < a.chunk ? (int)(N - s0) : a.chunk;
    for (int i = ctx.tid; i < n; i += ctx.nthreads) {
      const int64_t s = s0 + i;
      const int sd = (int)(s % a.D);
      const int64_t r = s / a.D;
      const int sw = (int)(r % a.W), sh = (int)(r / a.W);
      ent[i] = rad_ent(radial_weights_centred(sh, sw, sd, a.H, a.W, a.D, a.inv_dr, a.K, a.mode), A[s]);
    }
    ctx.sync();
    rad_scan(ctx, ent, n, rng, bins, a.K);
    ctx.sync();
  }
  double* out = a.part + ((int64_t)unit * a.Cm + c) * a.K;
  for (int k = ctx.tid; k < a.K; k += ctx.nthreads) out[k] = bins[k];
}

// out[j] (j over slots * K) = scale * the partials of j in float64, in a fixed order: the units are cut
// into RSUM_SEG runs of consecutive units, each run is added in unit order, then the runs in run order
struct RadialSumArgs {
  const double* part;  // [units][n]
  float* out;          // [n]
  int units, n;
  double scale;
  int accumulate;      // 1: out += (launch groups after the first)
};
constexpr int RSUM_SEG = 16;
TB_HD double radial_sum_seg(const RadialSumArgs& a, int j, int seg) {
  const int per = (a.units + RSUM_SEG - 1) / RSUM_SEG;
  const int u0 = seg * per, u1 = (u0 + per) < a.units ? (u0 + per) : a.units;
  double s = 0.0;
  for (int u = u0; u < u1; ++u) s += a.part[(int64_t)u * a.n + j];
  return s;
}
TB_HD void radial_sum_store(const RadialSumArgs& a, int j, double s) {
  const float v = (float)(s * a.scale);
  a.out[j] = a.accumulate ? a.out[j] + v : v;
}

}  // namespace tb
