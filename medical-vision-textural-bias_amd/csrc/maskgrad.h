// maskgrad.h -- gradient of y = Re(IFFT(ifftshift(M . fftshift(FFT x)))) with respect to the real mask M
// (TB_OP_MASK, centred layout), for an upstream gradient g:
//     dL/dM[s(f)] = Re(X(f) conj(G(f))) / N,   X = FFT(x), G = FFT(g), N = H W D,
// summed over the samples (and over the channels when the mask is shared).  The per-unit body is here,
// templated on the context like the pass bodies of fft_core.h, so the host emulator runs the same code
// as k_kspace_maskgrad (kern_maskgrad.hip).
//
// A unit is (mask channel slot, tile of T stored half-spectrum columns j = w' (D/2+1) + kd).  Per
// channel-volume the tile of S_x and the tile of S_g sit side by side in LDS as one [H][2 T] tile, so
// one DIF along H (digit-reversed h') finishes both transforms with one set of barriers; T is half of
// pass B's tile width, which keeps the LDS of one pass-B tile.  The unit accumulates
// x.re g.re + x.im g.im per coefficient in the thread's registers; the next volume's tiles are loaded
// into registers before the current transform.  After the loop every coefficient goes to the
// centred position of f = (irev_h[h'], irev_w[w'], kd) and, when kd is not self-conjugate, of -f.  In a
// self-conjugate column (kd = 0, kd = D/2 with D even) -f is itself a stored coefficient and is
// written by its owner, so every element of dM is written exactly once and no atomics are needed.
//
// The complex mask of TB_OP_CMASK (CX = true, MaskGradArgs::cplx) has the complex gradient
//     dL/dM[s(f)] = conj(X(f)) G(f) / N      (the convention of torch.autograd for a complex leaf),
// whose real part is the value above.  The unit keeps a second accumulator x.re g.im - x.im g.re per
// coefficient, stores a cf at f and its conjugate at -f (dM is then complex64 [Cm][H][W][D]); tiles,
// ownership of the self-conjugate columns and `accumulate` are unchanged.
#pragma once

#include "fft_core.h"

namespace tb {

struct MaskGradArgs {
  tb_plan_dev pl;
  const cf* Sx;  // half spectra after pass A, [bc][H][W][D/2+1], indexed by the absolute bc
  const cf* Sg;
  float* dM;     // [Cm][H][W][D], centred layout
  int bc0, C, nb, Cm;  // launch group: volumes [bc0, bc0 + nb C), bc0 = first sample * C
  int T;               // tile width in columns; H * T <= MG_MAX_TILE
  int accumulate;      // 0: dM = v;  1: dM += v (launch groups after the first)
  float scale;         // 1 / N
  int cplx;            // 1: dM is complex64 (interleaved re, im), the gradient of a TB_OP_CMASK mask
};

constexpr int MG_NE = 8;            // coefficients per thread of k_kspace_maskgrad
constexpr int MG_MAX_TILE = 2048;  // MG_NE * NT_TILE

// Thread-owned coefficients of the [H][T] tile: element i of a thread is t = tid + i * nthreads (row
// t / T, column t % T); columns past the ragged edge are never loaded, transformed or stored.  In LDS
// the x value of (row, c) is at row * 2 T + c and the g value nc columns further.
struct MgTile {
  int tid, nthreads, T, nc, nl, ncols_all;
  FastDiv fT;
  TB_HD bool at(int i, int& hh, int& c) const {
    const int t = tid + i * nthreads;
    hh = fT.div(t);
    c = t - hh * T;
    return t < nl && c < nc;
  }
  TB_HD int off(int hh, int c) const { return hh * ncols_all + c; }  // < H W (D/2+1) < 2^31 (checked by the host)
  TB_HD int slot(int hh, int c) const { return hh * 2 * T + c; }
};

// NE > 0: NE register slots per thread, fully unrolled (device); NE = 0: `ne` slots counted at run time (host)
#if defined(__HIPCC__)
#define TB_MG_EACH(i) \
  _Pragma("unroll") for (int i = 0; i < (NE > 0 ? NE : (1 << 30)) && (NE > 0 || i < ne); ++i)
#else
#define TB_MG_EACH(i) for (int i = 0; i < (NE > 0 ? NE : (1 << 30)) && (NE > 0 || i < ne); ++i)
#endif

template <int NE>
TB_HD void mg_load(const MgTile& g, int ne, const cf* __restrict__ Sb, cf* r) {
  TB_MG_EACH(i) {
    int hh, c;
    if (g.at(i, hh, c)) r[i] = Sb[g.off(hh, c)];
  }
}

template <int NE>
TB_HD void mg_to_lds(const MgTile& g, int ne, cf* lds, const cf* r) {
  TB_MG_EACH(i) {
    int hh, c;
    if (g.at(i, hh, c)) lds[g.slot(hh, c)] = r[i];
  }
}

// volume k of the unit's loop: every volume of the group in index order for a shared mask, else the
// slot's channel of every sample
TB_HD int mg_volume(const MaskGradArgs& a, int slot, int k) { return a.Cm == 1 ? a.bc0 + k : a.bc0 + k * a.C + slot; }

// xa, ga: NE (or ne) complex slots per thread; acc: as many floats.  PF: load the next volume's tiles
// before the transform of the current one.  CX: the complex gradient, with acc2 as many floats again.
template <class Ctx, int RS, int NE, bool PF, bool CX = false>
TB_HD void maskgrad_unit(Ctx& ctx, cf* lds, const MaskGradArgs& a, int slot, int tile, int ne, cf* xa, cf* ga,
                         float* acc, float* acc2 = nullptr) {
  const tb_plan_dev& pl = a.pl;
  const int H = pl.H, W = pl.W, D = pl.D, Dh = D / 2 + 1, T = a.T;
  const int ncols_all = W * Dh;
  const int j0 = tile * T;
  const int nc = (ncols_all - j0) < T ? (ncols_all - j0) : T;
  const TileGeo tg = tile_geo(H, 2 * T);
  cf* tw = lds + tg.off_tw;
  int* irev = reinterpret_cast<int*>(lds + tg.off_irev);
  for (int i = ctx.tid; i < H; i += ctx.nthreads) { tw[i] = pl.tw[0][i]; irev[i] = pl.irev_h[i]; }
  const MgTile g{ctx.tid, ctx.nthreads, T, nc, H * T, ncols_all, FastDiv::make(T)};
  const int64_t vstride = (int64_t)H * ncols_all;
  const int nv = a.Cm == 1 ? a.nb * a.C : a.nb;
  TB_MG_EACH(i) acc[i] = 0.f;
  if (CX) { TB_MG_EACH(i) acc2[i] = 0.f; }
  if (PF) {
    const int64_t v0 = mg_volume(a, slot, 0);
    mg_load<NE>(g, ne, a.Sx + v0 * vstride + j0, xa);
    mg_load<NE>(g, ne, a.Sg + v0 * vstride + j0, ga);
  }
  for (int k = 0; k < nv; ++k) {
    if (!PF) {
      const int64_t v = mg_volume(a, slot, k);
      mg_load<NE>(g, ne, a.Sx + v * vstride + j0, xa);
      mg_load<NE>(g, ne, a.Sg + v * vstride + j0, ga);
    }
    mg_to_lds<NE>(g, ne, lds, xa);
    mg_to_lds<NE>(g, ne, lds + nc, ga);
    ctx.sync();
    if (PF && k + 1 < nv) {  // in flight during the transform
      const int64_t v = mg_volume(a, slot, k + 1);
      mg_load<NE>(g, ne, a.Sx + v * vstride + j0, xa);
      mg_load<NE>(g, ne, a.Sg + v * vstride + j0, ga);
    }
    fft_dif<Ctx, RS>(ctx, lds, tw, pl.ax[0], 2 * nc, TileAddr{2 * T}, true);
    TB_MG_EACH(i) {
      int hh, c;
      if (g.at(i, hh, c)) {
        const cf x = lds[g.slot(hh, c)], v = lds[g.slot(hh, c) + nc];
        acc[i] += x.x * v.x + x.y * v.y;
        if (CX) acc2[i] += x.x * v.y - x.y * v.x;
      }
    }
    ctx.sync();
  }
  // write-once store to the centred positions of f and, off the self-conjugate columns, of -f
  const int64_t ch = (int64_t)slot * H;
  const int Dtop = (D % 2 == 0) ? D / 2 : -1;
  TB_MG_EACH(i) {
    int hp, c;
    if (!g.at(i, hp, c)) continue;
    const int j = j0 + c;
    const int wp = j / Dh, kd = j - wp * Dh;
    const int kh = irev[hp], kw = pl.irev_w[wp];
    const float v = acc[i] * a.scale;
    if (CX) {
      const float w = acc2[i] * a.scale;
      cf* p = reinterpret_cast<cf*>(a.dM) + mask_index(ch, kh, kw, kd, H, W, D);
      *p = a.accumulate ? mk(p->x + v, p->y + w) : mk(v, w);
      if (kd != 0 && kd != Dtop) {
        cf* q = reinterpret_cast<cf*>(a.dM) + mask_index(ch, negk(kh, H), negk(kw, W), D - kd, H, W, D);
        *q = a.accumulate ? mk(q->x + v, q->y - w) : mk(v, -w);
      }
      continue;
    }
    float* p = a.dM + mask_index(ch, kh, kw, kd, H, W, D);
    *p = a.accumulate ? *p + v : v;
    if (kd != 0 && kd != Dtop) {
      float* q = a.dM + mask_index(ch, negk(kh, H), negk(kw, W), D - kd, H, W, D);
      *q = a.accumulate ? *q + v : v;
    }
  }
}

#undef TB_MG_EACH

}  // namespace tb
