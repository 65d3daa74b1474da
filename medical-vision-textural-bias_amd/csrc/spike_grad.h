// spike_grad.h -- the per-(volume-channel, spike) arithmetic of the trainable spike layer, in float64.
//
// Reference: spike_layer / Spikes_UNet (source_code/stylization_layers.py:143-174) set |K(f)| = exp(I) at one
// k-space location with the phase kept (KSpaceSpikeNoise._set_spike, filters_and_operators.py:966-983) and
// update I by finite differences (350_stylized_layers/spikes11_layer_domain_GD.py:260-275).  On the closed-form
// route (point.h) the layer is  y = x + Re(sum_j Delta_j e^{i theta_j}) / N,  Delta_j = A_j u_j - K_j,
// A_j = exp(I_j), K_j = sum_n x[n] e^{-i theta_j(n)}, u_j = K_j / |K_j| (1 where K_j = 0, as spike_target), so
// for a real upstream gradient g with G_j = sum_n g[n] e^{-i theta_j(n)} and p + i q = conj(u_j) G_j:
//   dL/dI_j = sum_bc A_j p / N
//   gx      = g + Re(sum_j Gamma_j e^{i theta_j}) / N,  Gamma_j = u_j (-p + i q (A_j / m - 1)),  m = |K_j|
// (setting the modulus removes the radial part of the coefficient's gradient and scales the tangential part
// by A / m); Gamma_j = -G_j where m = 0, the phase being taken as constant there.  Shared by the kernels
// (kern_point.hip: k_spike_delta, k_spike_gamma, k_spike_dI_sum) and the host emulator of the CPU tests.
#pragma once

#include "fft_core.h"

namespace tb {

// (K, A) -> Delta / N
TB_HD void spike_delta(double kr, double ki, double A, double invN, double& dr, double& di) {
  const double m = sqrt(kr * kr + ki * ki);
  const double tr = m > 0.0 ? A * kr / m : A;
  const double ti = m > 0.0 ? A * ki / m : 0.0;
  dr = (tr - kr) * invN;
  di = (ti - ki) * invN;
}

// (K, G, A) -> Gamma / N and this volume-channel's share A p / N of dL/dI
TB_HD void spike_gamma(double kr, double ki, double gr, double gi, double A, double invN, double& cr, double& ci,
                       double& share) {
  const double m = sqrt(kr * kr + ki * ki);
  if (m > 0.0) {
    const double ur = kr / m, ui = ki / m;
    const double p = ur * gr + ui * gi, q = ur * gi - ui * gr;  // conj(u) G
    const double t = q * (A / m - 1.0);
    cr = (-ur * p - ui * t) * invN;
    ci = (ur * t - ui * p) * invN;
    share = A * p * invN;
  } else {
    cr = -gr * invN;
    ci = -gi * invN;
    share = A * gr * invN;
  }
}

// dI[j] = sum over the launch group's volume-channels, in index order; launch groups after the first add to
// their own element (accumulate), as radial_sum_store does
struct SpikeSumArgs {
  const double* share;  // [nbc][S]
  float* dI;            // [S]
  int nbc, S, accumulate;
};
TB_HD double spike_dI_sum(const SpikeSumArgs& a, int j) {
  double s = 0.0;
  for (int b = 0; b < a.nbc; ++b) s += a.share[(int64_t)b * a.S + j];
  return s;
}
TB_HD void spike_dI_store(const SpikeSumArgs& a, int j, double s) {
  const float v = (float)s;
  a.dI[j] = a.accumulate ? a.dI[j] + v : v;
}

}  // namespace tb
