// Host emulator of the complex mask-gradient pass -- TEST INFRASTRUCTURE ONLY.
//
// emu_mask_grad.cpp for the complex form of maskgrad_unit (maskgrad.h, CX = true: the code
// k_kspace_cmaskgrad runs): the run-time planned pass A (pass_a_body) on the image and on the upstream
// gradient, then the per-unit body one workgroup at a time with a single "thread" and a no-op barrier --
// the launch sequence of tb_kspace_cmask_grad_f32, launch groups included.  Never loaded by the product
// package.
#include <cstring>
#include <vector>

#include "fft_core.h"
#include "maskgrad.h"
#include "plan_host.h"

using namespace tb;

namespace {
struct HostCtx {
  int tid = 0, nthreads = 1;
  void sync() {}
};
}  // namespace

extern "C" {

// same contract as tb_kspace_cmask_grad_f32 with host pointers and no workspace; T = columns per unit
int tbemu_kspace_cmask_grad_f32(int H, int W, int D, const float* x, const int64_t* xs, const float* g,
                                const int64_t* gs, void* dM, int Cm, int B, int C, int T) {
  if (!x || !xs || !g || !gs || !dM || B < 1 || C < 1 || (Cm != 1 && Cm != C) || T < 1) return TB_ERR_INVALID_ARG;
  PlanTables pt;
  tb_plan_dev pl;
  int rc = build_tables(H, W, D, pt);
  if (rc) return rc;
  pl.H = H; pl.W = W; pl.D = D; pl.pad = 0;
  for (int a = 0; a < 3; ++a) { pl.ax[a] = pt.ax[a]; pl.tw[a] = pt.tw[a].data(); }
  pl.rev_d = pt.rev_d.data();
  pl.irev_h = pt.irev_h.data();
  pl.irev_w = pt.irev_w.data();
  const int Dh = D / 2 + 1, ncols = W * Dh, ntiles = (ncols + T - 1) / T;
  const SlabGeo sg = slab_geo(W, D);
  const TileGeo tg = tile_geo(H, 2 * T);
  std::vector<cf> lds((size_t)(sg.total_cf > tg.total_cf ? sg.total_cf : tg.total_cf) + 16);
  std::vector<cf> Sx((size_t)B * C * H * ncols), Sg(Sx.size());
  const int ne = H * T;  // one thread owns the whole tile
  std::vector<cf> xa(ne), ga(ne);
  std::vector<float> acc(ne), acc2(ne);
  HostCtx ctx;
  for (int b0 = 0; b0 < B; b0 += TB_MAX_BATCH) {
    const int nb = (B - b0) < TB_MAX_BATCH ? (B - b0) : TB_MAX_BATCH;
    for (int bc = b0 * C; bc < (b0 + nb) * C; ++bc)
      for (int h = 0; h < H; ++h) {
        pass_a_body<HostCtx, 1>(ctx, lds.data(), pl, x, xs[0], xs[1], xs[2], Sx.data(), bc, h);
        pass_a_body<HostCtx, 1>(ctx, lds.data(), pl, g, gs[0], gs[1], gs[2], Sg.data(), bc, h);
      }
    const MaskGradArgs a{pl, Sx.data(), Sg.data(), static_cast<float*>(dM), b0 * C, C, nb, Cm, T, b0 > 0 ? 1 : 0,
                         (float)(1.0 / ((double)H * (double)W * (double)D)), 1};
    for (int slot = 0; slot < Cm; ++slot)
      for (int t = 0; t < ntiles; ++t)
        maskgrad_unit<HostCtx, 1, 0, true, true>(ctx, lds.data(), a, slot, t, ne, xa.data(), ga.data(), acc.data(),
                                                 acc2.data());
  }
  return TB_OK;
}
}
