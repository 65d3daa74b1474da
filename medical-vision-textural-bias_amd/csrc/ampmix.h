// ampmix.h -- amplitude mixing in k-space (Fourier domain adaptation, amplitude mix / swap): keep the
// phase of x's spectrum and interpolate its amplitude towards that of a second image y,
//     X = fftshift(fftn(x)),  Y = fftshift(fftn(y[perm]))
//     K = polar((1 - m) |X| + m |Y|, angle(X)),   m = lam[b] M        out = Re(ifftn(ifftshift(K)))
// with a real mask M in the centred layout of TB_OP_MASK and a per-sample strength lam[b] read from
// device memory.  The factor applied to X(f) is data dependent (|Y(f)| / |X(f)|), so no op of the
// program passes expresses it.  The per-unit bodies are here, templated on the context like maskgrad.h
// and spectrum.h, so the host emulator runs the same code as k_kspace_ampmix / k_kspace_ampmix_bwd
// (kern_ampmix.hip).
//
// Closed form on the stored half spectrum.  K is affine in M, so the `.real` symmetrises M exactly as
// for TB_OP_MASK: with m_s(f) = lam[b] (M[s(f)] + M[s(-f)]) / 2 and u = X / |X| (u = 1 where X = 0, what
// angle(0) = 0 gives),
//     X' = (1 - m_s) X + m_s |Y| u
// is Hermitian, and out = ifftn(X').  For an upstream gradient g with G = FFT(g), v = Y / |Y| and
// c = Re(conj(u) G):
//     Gx = (1 - m_s) G + m_s (|Y| / |X|) (G - u c)          gx = Re ifftn(Gx)
//     Gy = m_s c v                                           gy = Re ifftn(Gy), summed over the b with perm[b] = j
// Both are Hermitian again.  At the singularities the unit makes a fixed choice: where |X(f)| = 0 the
// tangential term is dropped (its factor |Y| / |X| is taken as 0), and where |Y(f)| = 0, Gy = 0.
//
// Amplitudes: |X|^2 = re^2 + im^2 in float32, one reciprocal of |X| per coefficient, used for u and for
// |Y| / |X|.  Everything stays finite while |X|^2 and |Y|^2 are below FLT_MAX and above the smallest
// normal float (|X|, |Y| within about 2^-63 .. 2^63); a coefficient whose square underflows to 0 is
// treated as 0.
//
// A unit is (volume bc, tile of T stored half-spectrum columns j = w' (D/2+1) + kd), the unit of pass B.
// After pass A the tiles of S_x[bc] and S_y[partner(bc)] (and, backward, of S_g[bc]) sit side by side in
// LDS as one [H][2 T] ([H][3 T]) tile, so one DIF along H (digit-reversed h') finishes all transforms
// with one set of barriers.  Per coefficient the unit gathers M at s(f) and s(-f) -- the two runs of
// sp_freq (spectrum.h) --, forms X' (Gx, Gy) in place in the x (x and y) columns, runs the DIT over those
// columns only and stores the tile pass C reads.  The forward output may alias S_x (same unit, same
// elements, read before written) unless the partners are taken from S_x itself; backward, Gx goes over
// S_g's storage and Gy, when asked for, to its own buffer.  Every output element is written exactly once,
// no atomics.
//
// perm[b] is read on the device and clamped to [0, B): a value outside is never dereferenced, but the
// caller owes a valid index (the result for such a sample is that of the clamped partner).
#pragma once

#include "fft_core.h"
#include "spectrum.h"

namespace tb {

struct AmpMixArgs {
  tb_plan_dev pl;
  const cf* Sx;      // half spectra after pass A, [bc][H][W][D/2+1], indexed by the absolute bc
  const cf* Sy;      // the partners' spectra (Sx itself when the partners are rows of x)
  cf* So;            // forward: X' (may be Sx when Sy is another buffer); backward: G in, Gx out
  cf* Sgy;           // backward with need_gy: Gy of volume bc (before the sum over equal partners)
  const float* M;    // [Cm][H][W][D], centred layout
  const float* lam;  // [B], device
  const int* perm;   // [B], device, or null: identity
  int C, B, Cm;
  int T;             // tile width in columns
  int bc0;           // first volume of the launch
  int need_gy;
};

constexpr int AM_MAX_TILE = 4096;      // coefficients of the forward's [H][2 T] tile: one 32 KB pass-B tile
constexpr int AM_MAX_TILE_BWD = 6144;  // of the backward's [H][3 T] tile: 48 KB, three workgroups per CU by LDS

// Coefficient t of the [H][T] tile: row t / T, column t % T; columns past the ragged edge are never
// loaded, transformed or stored.  In LDS row hh starts at hh * ld; the x value of column c is at c, the
// partner's nc columns further, the upstream gradient's 2 nc further.
struct AmTile {
  int T, ld, nc, ncols_all;
  FastDiv fT;
  TB_HD bool at(int t, int& hh, int& c) const {
    hh = fT.div(t);
    c = t - hh * T;
    return c < nc;
  }
  TB_HD int off(int hh, int c) const { return hh * ncols_all + c; }  // < H W (D/2+1) < 2^31 (checked by the host)
  TB_HD int slot(int hh, int c) const { return hh * ld + c; }
};

// partner sample of sample b, clamped to [0, B)
TB_HD int am_partner(const AmpMixArgs& a, int b) {
  if (!a.perm) return b;
  const int p = a.perm[b];
  return p < 0 ? 0 : (p >= a.B ? a.B - 1 : p);
}

// u = X / |X| (1 where X = 0) and rx = 1 / |X| (0 where X = 0)
TB_HD cf am_phase(cf x, float& rx) {
  const float a2 = x.x * x.x + x.y * x.y;
  if (!(a2 > 0.f)) {
    rx = 0.f;
    return mk(1.f, 0.f);
  }
  rx = 1.f / f32_sqrt(a2);
  return scl(x, rx);
}
TB_HD float am_abs(cf y) { return f32_sqrt(y.x * y.x + y.y * y.y); }

// X' = (1 - m) X + m |Y| u
TB_HD cf am_mix(cf x, cf y, float m) {
  float rx;
  const cf u = am_phase(x, rx);
  return add(scl(x, 1.f - m), scl(u, m * am_abs(y)));
}

// Gx = (1 - m) G + m (|Y| / |X|) (G - u c),  Gy = m c Y / |Y|,  c = Re(conj(u) G)
template <bool GY>
TB_HD cf am_mix_bwd(cf x, cf y, cf g, float m, cf& gy) {
  float rx;
  const cf u = am_phase(x, rx);
  const float ay = am_abs(y);
  const float c = u.x * g.x + u.y * g.y;
  if (GY) gy = ay > 0.f ? scl(y, m * c / ay) : mk(0.f, 0.f);
  return add(scl(g, 1.f - m), scl(sub(g, scl(u, c)), m * (ay * rx)));
}

template <class Ctx>
TB_HD void am_load(Ctx& ctx, const AmTile& g, int n, const cf* Sb, cf* lds) {
  copy_batched<kCopyUnroll>(
      ctx, n,
      [&](int t) { int hh, c; return g.at(t, hh, c) ? Sb[g.off(hh, c)] : mk(0.f, 0.f); },
      [&](int t, cf v) { int hh, c; if (g.at(t, hh, c)) lds[g.slot(hh, c)] = v; });
}

template <class Ctx>
TB_HD void am_store(Ctx& ctx, const AmTile& g, int n, const cf* lds, cf* Sb) {
  for (int t = ctx.tid; t < n; t += ctx.nthreads) {
    int hh, c;
    if (g.at(t, hh, c)) Sb[g.off(hh, c)] = lds[g.slot(hh, c)];
  }
}

// BWD = false: forward (two tiles); BWD = true: gradients (three tiles), GY: with Gy
template <class Ctx, int RS, bool BWD, bool GY>
TB_HD void ampmix_unit(Ctx& ctx, cf* lds, const AmpMixArgs& a, int bc, int tile) {
  const tb_plan_dev& pl = a.pl;
  const int H = pl.H, W = pl.W, D = pl.D, Dh = D / 2 + 1, T = a.T;
  constexpr int NTILE = BWD ? 3 : 2;
  const int ncols_all = W * Dh;
  const int j0 = tile * T;
  const int nc = (ncols_all - j0) < T ? (ncols_all - j0) : T;
  const TileGeo tg = tile_geo(H, NTILE * T);
  cf* tw = lds + tg.off_tw;
  int* irev = reinterpret_cast<int*>(lds + tg.off_irev);
  sp_tables(ctx, pl, tw, irev);
  const AmTile g{T, NTILE * T, nc, ncols_all, FastDiv::make(T)};
  const int b = bc / a.C, ch = bc - b * a.C;
  const int ybc = am_partner(a, b) * a.C + ch;
  const float lam = a.lam[b];
  const int64_t vstride = (int64_t)H * ncols_all;
  const float* __restrict__ Mb = a.M + (a.Cm == 1 ? 0 : (int64_t)ch * H * W * D);
  const int n = H * T;
  am_load(ctx, g, n, a.Sx + bc * vstride + j0, lds);
  am_load(ctx, g, n, a.Sy + ybc * vstride + j0, lds + nc);
  if (BWD) am_load(ctx, g, n, a.So + bc * vstride + j0, lds + 2 * nc);
  ctx.sync();
  fft_dif<Ctx, RS>(ctx, lds, tw, pl.ax[0], NTILE * nc, TileAddr{NTILE * T}, true);
  // per coefficient: the mask at s(f) and s(-f), then X' (Gx, Gy) in place
  const FastDiv fDh = FastDiv::make(Dh);
  constexpr int U = kCopyUnroll / 2;  // two loads per coefficient
  for (int b0 = ctx.tid; b0 < n; b0 += ctx.nthreads * U) {
    float mf[U], mn[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int t = b0 + u * ctx.nthreads;
      int hp, c;
      if (t < n && g.at(t, hp, c)) {
        const SpFreq q = sp_freq(pl, irev, fDh, Dh, hp, j0 + c);
        mf[u] = Mb[q.f];
        mn[u] = Mb[q.nf];
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int t = b0 + u * ctx.nthreads;
      int hp, c;
      if (t < n && g.at(t, hp, c)) {
        const float m = lam * mask_factor(mf[u], mn[u]);
        const int s = g.slot(hp, c);
        if (BWD) {
          cf gy;
          lds[s] = am_mix_bwd<GY>(lds[s], lds[s + nc], lds[s + 2 * nc], m, gy);
          if (GY) lds[s + nc] = gy;
        } else {
          lds[s] = am_mix(lds[s], lds[s + nc], m);
        }
      }
    }
  }
  ctx.sync();
  fft_dit<Ctx, RS>(ctx, lds, tw, pl.ax[0], (BWD && GY) ? 2 * nc : nc, TileAddr{NTILE * T}, true);
  am_store(ctx, g, n, lds, a.So + bc * vstride + j0);
  if (BWD && GY) am_store(ctx, g, n, lds + nc, a.Sgy + bc * vstride + j0);
}

template <class Ctx, int RS>
TB_HD void ampmix_fwd_unit(Ctx& ctx, cf* lds, const AmpMixArgs& a, int bc, int tile) {
  ampmix_unit<Ctx, RS, false, false>(ctx, lds, a, bc, tile);
}
// need_gy = false skips the v work, the second half of the DIT and the store of Gy
template <class Ctx, int RS, bool GY>
TB_HD void ampmix_bwd_unit(Ctx& ctx, cf* lds, const AmpMixArgs& a, int bc, int tile) {
  ampmix_unit<Ctx, RS, true, GY>(ctx, lds, a, bc, tile);
}

// Sum of the Gy of every sample whose partner is sample j, in the order of b: element e of volume
// (j, ch).  `vstride` elements per volume (half spectra, or full ones on the direct-DFT fallback).
TB_HD cf am_gysum(const cf* Sgy, const int* perm, int B, int C, int j, int ch, int64_t vstride, int64_t e) {
  cf s = mk(0.f, 0.f);
  for (int b = 0; b < B; ++b) {
    const int p = perm[b];
    const int pb = p < 0 ? 0 : (p >= B ? B - 1 : p);
    if (pb == j) s = add(s, Sgy[((int64_t)b * C + ch) * vstride + e]);
  }
  return s;
}

}  // namespace tb
