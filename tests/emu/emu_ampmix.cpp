// Host emulator of the amplitude-mixing passes -- TEST INFRASTRUCTURE ONLY.
//
// Compiles medical-vision-textural-bias_amd/csrc/{fft_core,spectrum,ampmix,plan_host}.h with the host clang++
// and runs the per-unit bodies of k_kspace_ampmix / k_kspace_ampmix_bwd (ampmix.h: ampmix_fwd_unit,
// ampmix_bwd_unit, am_gysum) one workgroup at a time with a single "thread" and a no-op barrier, around the
// run-time planned passes A and C (pass_a_body, pass_c_body) -- the launch sequences of tb_kspace_ampmix_f32 /
// tb_kspace_ampmix_bwd_f32: every forward pass before the first per-coefficient launch, launch groups, the
// aliasing of X' with S_x and of Gx with S_g included.  Each phase of a body consists of independent work
// items, so the result equals the device schedule's.  Never loaded by the product package.
#include <cstring>
#include <vector>

#include "ampmix.h"
#include "fft_core.h"
#include "plan_host.h"
#include "spectrum.h"

using namespace tb;

namespace {
struct HostCtx {
  int tid = 0, nthreads = 1;
  void sync() {}
};

int make_plan(int H, int W, int D, PlanTables& pt, tb_plan_dev& pl) {
  const int rc = build_tables(H, W, D, pt);
  if (rc) return rc;
  pl.H = H; pl.W = W; pl.D = D; pl.pad = 0;
  for (int a = 0; a < 3; ++a) { pl.ax[a] = pt.ax[a]; pl.tw[a] = pt.tw[a].data(); }
  pl.rev_d = pt.rev_d.data();
  pl.irev_h = pt.irev_h.data();
  pl.irev_w = pt.irev_w.data();
  return TB_OK;
}

struct Emu {
  tb_plan_dev pl;
  int H, W, D, B, C, T, ncols, ntiles;
  std::vector<cf> lds;
  HostCtx ctx;
  void forward_all(const float* x, const int64_t* xs, cf* S) {
    for (int b0 = 0; b0 < B; b0 += TB_MAX_BATCH) {
      const int nb = (B - b0) < TB_MAX_BATCH ? (B - b0) : TB_MAX_BATCH;
      for (int bc = b0 * C; bc < (b0 + nb) * C; ++bc)
        for (int h = 0; h < H; ++h) pass_a_body<HostCtx, 1>(ctx, lds.data(), pl, x, xs[0], xs[1], xs[2], S, bc, h);
    }
  }
  void inverse(const cf* S, float* y, const int64_t* ys, int pad, int b0, int nb) {
    const float scale = (float)(1.0 / ((double)H * (double)W * (double)D));
    for (int bc = b0 * C; bc < (b0 + nb) * C; ++bc)
      for (int h = 0; h < H; ++h) {
        float lo, hi;
        pass_c_body<HostCtx, 1>(ctx, lds.data(), pl, S, y, ys[0], ys[1], ys[2], pad, bc, h, scale, &lo, &hi);
      }
  }
};

int setup(Emu& e, PlanTables& pt, int H, int W, int D, int B, int C, int T, int ntile) {
  const int rc = make_plan(H, W, D, pt, e.pl);
  if (rc) return rc;
  e.H = H; e.W = W; e.D = D; e.B = B; e.C = C; e.T = T;
  e.ncols = W * (D / 2 + 1);
  e.ntiles = (e.ncols + T - 1) / T;
  const SlabGeo sg = slab_geo(W, D);
  const TileGeo tg = tile_geo(H, ntile * T);
  e.lds.assign((size_t)(sg.total_cf > tg.total_cf ? sg.total_cf : tg.total_cf) + 16, mk(0.f, 0.f));
  return TB_OK;
}
}  // namespace

extern "C" {

// same contracts as tb_kspace_ampmix_f32 / tb_kspace_ampmix_bwd_f32 with host pointers and no workspace;
// T = columns per unit
int tbemu_kspace_ampmix_f32(int H, int W, int D, const float* x, const int64_t* xs, const float* y,
                            const int64_t* ys_in, const int* perm, const float* M, int Cm, const float* lam, float* out,
                            const int64_t* outs, int out_pad, int B, int C, int T) {
  if (!x || !xs || (y && !ys_in) || !M || !lam || !out || !outs || out_pad < 0 || B < 1 || C < 1 || T < 1 ||
      (Cm != 1 && Cm != C))
    return TB_ERR_INVALID_ARG;
  Emu e;
  PlanTables pt;
  const int rc = setup(e, pt, H, W, D, B, C, T, 2);
  if (rc) return rc;
  const size_t nv = (size_t)B * C * H * e.ncols;
  std::vector<cf> Sx(nv), S2(nv);
  e.forward_all(x, xs, Sx.data());
  if (y) e.forward_all(y, ys_in, S2.data());
  const cf* Sy = y ? S2.data() : Sx.data();
  cf* So = y ? Sx.data() : S2.data();
  for (int b0 = 0; b0 < B; b0 += TB_MAX_BATCH) {
    const int nb = (B - b0) < TB_MAX_BATCH ? (B - b0) : TB_MAX_BATCH;
    const AmpMixArgs a{e.pl, Sx.data(), Sy, So, nullptr, M, lam, perm, C, B, Cm, T, b0 * C, 0};
    for (int bc = b0 * C; bc < (b0 + nb) * C; ++bc)
      for (int t = 0; t < e.ntiles; ++t) ampmix_fwd_unit<HostCtx, 1>(e.ctx, e.lds.data(), a, bc, t);
    e.inverse(So, out, outs, out_pad, b0, nb);
  }
  return TB_OK;
}

int tbemu_kspace_ampmix_bwd_f32(int H, int W, int D, const float* x, const int64_t* xs, const float* y,
                                const int64_t* ys_in, const int* perm, const float* M, int Cm, const float* lam,
                                const float* g, const int64_t* gs, float* gx, const int64_t* gxs, float* gy,
                                const int64_t* gys, int B, int C, int T) {
  if (!x || !xs || (y && !ys_in) || !M || !lam || !g || !gs || !gx || !gxs || (gy && !gys) || B < 1 || C < 1 ||
      T < 1 || (Cm != 1 && Cm != C))
    return TB_ERR_INVALID_ARG;
  Emu e;
  PlanTables pt;
  const int rc = setup(e, pt, H, W, D, B, C, T, 3);
  if (rc) return rc;
  const int64_t vs = (int64_t)H * e.ncols;
  const size_t nv = (size_t)B * C * vs;
  std::vector<cf> Sx(nv), S2(y ? nv : 0), Sg(nv), Sgy(gy ? nv : 0), Sgys(gy && perm ? nv : 0);
  e.forward_all(x, xs, Sx.data());
  if (y) e.forward_all(y, ys_in, S2.data());
  e.forward_all(g, gs, Sg.data());
  const cf* Sy = y ? S2.data() : Sx.data();
  for (int b0 = 0; b0 < B; b0 += TB_MAX_BATCH) {
    const int nb = (B - b0) < TB_MAX_BATCH ? (B - b0) : TB_MAX_BATCH;
    const AmpMixArgs a{e.pl, Sx.data(), Sy, Sg.data(), gy ? Sgy.data() : nullptr, M, lam, perm, C, B, Cm, T, b0 * C,
                       gy ? 1 : 0};
    for (int bc = b0 * C; bc < (b0 + nb) * C; ++bc)
      for (int t = 0; t < e.ntiles; ++t) {
        if (gy)
          ampmix_bwd_unit<HostCtx, 1, true>(e.ctx, e.lds.data(), a, bc, t);
        else
          ampmix_bwd_unit<HostCtx, 1, false>(e.ctx, e.lds.data(), a, bc, t);
      }
    e.inverse(Sg.data(), gx, gxs, 0, b0, nb);
  }
  if (!gy) return TB_OK;
  for (int b0 = 0; b0 < B; b0 += TB_MAX_BATCH) {
    const int nb = (B - b0) < TB_MAX_BATCH ? (B - b0) : TB_MAX_BATCH;
    if (perm)
      for (int bc = b0 * C; bc < (b0 + nb) * C; ++bc)
        for (int64_t i = 0; i < vs; ++i) Sgys[(size_t)bc * vs + i] = am_gysum(Sgy.data(), perm, B, C, bc / C, bc % C, vs, i);
    e.inverse(perm ? Sgys.data() : Sgy.data(), gy, gys, 0, b0, nb);
  }
  return TB_OK;
}
}
