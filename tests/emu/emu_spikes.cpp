// Host emulator of the trainable spike layer's arithmetic -- TEST INFRASTRUCTURE ONLY.
//
// Compiles medical-vision-textural-bias_amd/csrc/spike_grad.h with the host clang++ and runs the functions the
// kernels call (k_spike_delta: spike_delta; k_spike_gamma: spike_gamma; k_spike_dI_sum: spike_dI_sum /
// spike_dI_store, one call per launch group as tb_kspace_spikes_bwd_f32 makes them).  Never loaded by the
// product package.
#include <cmath>
#include <vector>

#include "spike_grad.h"

using namespace tb;

extern "C" {

// n independent (K, A) -> Delta / N
int tbemu_spike_delta(int n, const double* K, const double* A, double invN, double* out) {
  if (n < 1 || !K || !A || !out) return TB_ERR_INVALID_ARG;
  for (int i = 0; i < n; ++i) spike_delta(K[2 * i], K[2 * i + 1], A[i], invN, out[2 * i], out[2 * i + 1]);
  return TB_OK;
}

// n independent (K, G, A) -> Gamma / N and the dI share A p / N
int tbemu_spike_gamma(int n, const double* K, const double* G, const double* A, double invN, double* gam,
                      double* share) {
  if (n < 1 || !K || !G || !A || !gam || !share) return TB_ERR_INVALID_ARG;
  for (int i = 0; i < n; ++i)
    spike_gamma(K[2 * i], K[2 * i + 1], G[2 * i], G[2 * i + 1], A[i], invN, gam[2 * i], gam[2 * i + 1], share[i]);
  return TB_OK;
}

// share[B*C][S] -> dI[S]: launch groups of TB_MAX_BATCH samples, each with its own contiguous share buffer (as the
// workspace holds it); the first group writes, the later ones add to their own elements
int tbemu_spike_dI(const double* share, int B, int C, int S, float* dI) {
  if (!share || !dI || B < 1 || C < 1 || S < 1 || S > TB_MAX_OPS) return TB_ERR_INVALID_ARG;
  for (int b0 = 0; b0 < B; b0 += TB_MAX_BATCH) {
    const int nb = (B - b0) < TB_MAX_BATCH ? (B - b0) : TB_MAX_BATCH;
    const std::vector<double> grp(share + (size_t)b0 * C * S, share + (size_t)(b0 + nb) * C * S);
    const SpikeSumArgs sa{grp.data(), dI, nb * C, S, b0 > 0 ? 1 : 0};
    for (int j = 0; j < S; ++j) spike_dI_store(sa, j, spike_dI_sum(sa, j));
  }
  return TB_OK;
}
}
