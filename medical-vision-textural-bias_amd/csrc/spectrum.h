// spectrum.h -- the centred complex spectrum itself, out of and into the library:
//     export  K = fftshift(fftn(x))                 K complex64 [bc][H][W][D], the layout of TB_OP_MASK
//     import  y = Re(ifftn(ifftshift(K)))           for any complex K (it need not be Hermitian)
// (Fourier.shift_fourier / inv_shift_fourier, source_code/filters_and_operators.py:594-632).  The
// per-unit bodies are here, templated on the context like maskgrad.h, so the host emulator runs the
// same code as k_kspace_export / k_kspace_import (kern_spectrum.hip).
//
// A unit is (volume bc, tile of T stored half-spectrum columns j = w' (D/2+1) + kd), the unit of pass B.
//
// Export, after pass A: the [H][T] tile of S goes to LDS, one DIF along H finishes the transform
// (digit-reversed h'), and the coefficient of slot h' goes to the centred position of
// f = (irev_h[h'], irev_w[w'], kd) and, when kd is not self-conjugate, its conjugate to the position of
// -f.  In a self-conjugate column (kd = 0, kd = D/2 with D even) -f is itself a stored coefficient and
// is written by its owner, so every element of K is written exactly once: no atomics, no zeroing, f and
// -f bit-equal up to the sign of the imaginary part.  Along a tile row the columns of one w' are
// consecutive kd: a contiguous run of K at f, a reversed contiguous run at -f.
//
// Import, before pass C: per slot the unit gathers K(f) and K(-f) (the same two runs), forms the
// symmetrised K_s(f) = (K(f) + conj(K(-f))) / 2 -- Re(ifftn(K)) = ifftn(K_s), and K_s is Hermitian, so
// the half spectrum holds all of it --, runs one DIT along H and writes the tile to S[bc][h][w'][kd].
// Self-conjugate columns need no special case: both owners evaluate the same expression.
#pragma once

#include "fft_core.h"

namespace tb {

struct SpectrumArgs {
  tb_plan_dev pl;
  cf* S;    // half spectrum [bc][H][W][D/2+1], indexed by the absolute bc (export reads, import writes)
  cf* K;    // centred full spectrum [bc][H][W][D], indexed by the absolute bc (export writes, import reads)
  int bc0;  // first volume of the launch
  int T;    // tile width in columns; H * T <= SP_MAX_TILE
};

constexpr int SP_MAX_TILE = 4096;  // coefficients of one tile: a 32 KB pass-B tile of LDS

// Coefficient t of the [H][T] tile: row t / T, column t % T; columns past the ragged edge are never
// loaded, transformed or stored.
struct SpTile {
  int T, nc, ncols_all;
  FastDiv fT;
  TB_HD bool at(int t, int& hh, int& c) const {
    hh = fT.div(t);
    c = t - hh * T;
    return c < nc;
  }
  TB_HD int off(int hh, int c) const { return hh * ncols_all + c; }  // < H W (D/2+1) < 2^31 (checked by the host)
  TB_HD int slot(int hh, int c) const { return hh * T + c; }
};

// centred element offsets of the coefficient (slot h', column j0 + c) and of its mirror, within a volume
struct SpFreq {
  int64_t f, nf;
  bool self;  // kd = 0, or kd = D/2 with D even: -f is a stored coefficient with its own owner
};
TB_HD SpFreq sp_freq(const tb_plan_dev& pl, const int* irev, const FastDiv& fDh, int Dh, int hp, int j) {
  const int H = pl.H, W = pl.W, D = pl.D;
  const int wp = fDh.div(j), kd = j - wp * Dh;
  const int kh = irev[hp], kw = pl.irev_w[wp];
  SpFreq r;
  r.f = mask_index(0, kh, kw, kd, H, W, D);
  r.nf = mask_index(0, negk(kh, H), negk(kw, W), negk(kd, D), H, W, D);
  r.self = kd == 0 || 2 * kd == D;
  return r;
}

template <class Ctx>
TB_HD void sp_tables(Ctx& ctx, const tb_plan_dev& pl, cf* tw, int* irev) {
  for (int i = ctx.tid; i < pl.H; i += ctx.nthreads) { tw[i] = pl.tw[0][i]; irev[i] = pl.irev_h[i]; }
}

template <class Ctx, int RS>
TB_HD void export_unit(Ctx& ctx, cf* lds, const SpectrumArgs& a, int bc, int tile) {
  const tb_plan_dev& pl = a.pl;
  const int H = pl.H, W = pl.W, D = pl.D, Dh = D / 2 + 1, T = a.T;
  const int ncols_all = W * Dh;
  const int j0 = tile * T;
  const int nc = (ncols_all - j0) < T ? (ncols_all - j0) : T;
  const TileGeo tg = tile_geo(H, T);
  cf* tw = lds + tg.off_tw;
  int* irev = reinterpret_cast<int*>(lds + tg.off_irev);
  sp_tables(ctx, pl, tw, irev);
  const SpTile g{T, nc, ncols_all, FastDiv::make(T)};
  const cf* __restrict__ Sb = a.S + (int64_t)bc * H * ncols_all + j0;
  copy_batched<kCopyUnroll>(
      ctx, H * T,
      [&](int t) { int hh, c; return g.at(t, hh, c) ? Sb[g.off(hh, c)] : mk(0.f, 0.f); },
      [&](int t, cf v) { int hh, c; if (g.at(t, hh, c)) lds[g.slot(hh, c)] = v; });
  ctx.sync();
  fft_dif<Ctx, RS>(ctx, lds, tw, pl.ax[0], nc, TileAddr{T}, true);
  // write-once store to the centred positions of f and, off the self-conjugate columns, of -f
  cf* __restrict__ Kb = a.K + (int64_t)bc * H * W * D;
  const FastDiv fDh = FastDiv::make(Dh);
  for (int t = ctx.tid; t < H * T; t += ctx.nthreads) {
    int hp, c;
    if (!g.at(t, hp, c)) continue;
    const SpFreq q = sp_freq(pl, irev, fDh, Dh, hp, j0 + c);
    const cf v = lds[g.slot(hp, c)];
    Kb[q.f] = v;
    if (!q.self) Kb[q.nf] = conj(v);
  }
}

template <class Ctx, int RS>
TB_HD void import_unit(Ctx& ctx, cf* lds, const SpectrumArgs& a, int bc, int tile) {
  const tb_plan_dev& pl = a.pl;
  const int H = pl.H, W = pl.W, D = pl.D, Dh = D / 2 + 1, T = a.T;
  const int ncols_all = W * Dh;
  const int j0 = tile * T;
  const int nc = (ncols_all - j0) < T ? (ncols_all - j0) : T;
  const TileGeo tg = tile_geo(H, T);
  cf* tw = lds + tg.off_tw;
  int* irev = reinterpret_cast<int*>(lds + tg.off_irev);
  sp_tables(ctx, pl, tw, irev);
  ctx.sync();  // the gather reads irev
  const SpTile g{T, nc, ncols_all, FastDiv::make(T)};
  const cf* __restrict__ Kb = a.K + (int64_t)bc * H * W * D;
  const FastDiv fDh = FastDiv::make(Dh);
  constexpr int U = kCopyUnroll / 2;  // two loads per coefficient
  for (int b0 = ctx.tid; b0 < H * T; b0 += ctx.nthreads * U) {
    cf vf[U], vn[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int t = b0 + u * ctx.nthreads;
      int hp, c;
      if (t < H * T && g.at(t, hp, c)) {
        const SpFreq q = sp_freq(pl, irev, fDh, Dh, hp, j0 + c);
        vf[u] = Kb[q.f];
        vn[u] = Kb[q.nf];
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int t = b0 + u * ctx.nthreads;
      int hp, c;
      if (t < H * T && g.at(t, hp, c)) lds[g.slot(hp, c)] = scl(add(vf[u], conj(vn[u])), 0.5f);
    }
  }
  ctx.sync();
  fft_dit<Ctx, RS>(ctx, lds, tw, pl.ax[0], nc, TileAddr{T}, true);
  cf* __restrict__ Sb = a.S + (int64_t)bc * H * ncols_all + j0;
  for (int t = ctx.tid; t < H * T; t += ctx.nthreads) {
    int hh, c;
    if (g.at(t, hh, c)) Sb[g.off(hh, c)] = lds[g.slot(hh, c)];
  }
}

}  // namespace tb
