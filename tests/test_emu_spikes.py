"""The arithmetic of the trainable spike layer on the host: spike_delta and spike_gamma of csrc/spike_grad.h (the
functions k_spike_delta and k_spike_gamma call per volume-channel and spike) against the numpy formulas of
tests/_spikes_ref.py, and the ordered dI sum (spike_dI_sum / spike_dI_store, what k_spike_dI_sum runs) over the
launch groups of tb_kspace_spikes_bwd_f32.

Bars: both sides are float64 and differ only in the order of a handful of operations, so 1e-13 of the result's
scale -- |Delta| <= A + m, |Gamma| <= |G| max(1, A / m), |share| <= A |G| -- times 1 / N.  The dI sum is compared
bit for bit with the same order of additions in numpy (float64 within a launch group, the group's float32 added
to the element by the later groups) and to float32 rounding with the float64 total.
"""
import numpy as np
import pytest

import _emu_spikes as E
import _spikes_ref as R

TOL = 1e-13
INV_N = 1.0 / (24 * 20 * 15)


def _cases():
    rng = np.random.default_rng(17)
    K = rng.standard_normal(16) + 1j * rng.standard_normal(16)
    G = rng.standard_normal(16) + 1j * rng.standard_normal(16)
    A = np.exp(rng.uniform(-2.0, 12.0, 16))
    # m = 0; a self-conjugate f (K and G real, both signs of K); A / m = 1e-6 and 1e+6
    K[0] = 0.0
    K[1], G[1] = 3.5, -0.25
    K[2], G[2] = -3.5, 0.75
    K[3], A[3] = (0.6 - 0.8j) * 2.0e6, 2.0
    K[4], A[4] = (0.6 + 0.8j) * 2.0e-6, 2.0
    K[5], A[5] = (0.6 + 0.8j) * 1e-100, 1.0   # a tiny modulus still divides (m * m does not underflow)
    return K, G, A


def test_spike_delta_matches_the_formula():
    K, _, A = _cases()
    d = E.spike_delta(K, A, INV_N)
    assert not np.isnan(d.view(np.float64)).any()
    ref = R.spike_delta(K, A) * INV_N
    err = np.abs(d - ref) / ((A + np.abs(K)) * INV_N)
    print("largest error / scale %.2e" % err.max())
    assert err.max() <= TOL
    assert d[0] == A[0] * INV_N                     # m = 0: u = 1
    assert d[1].imag == 0.0 and d[2].imag == 0.0    # a real coefficient stays real
    assert d[2].real < 0.0                          # u = -1: the target is -A


def test_spike_gamma_matches_the_formula():
    K, G, A = _cases()
    gam, share = E.spike_gamma(K, G, A, INV_N)
    assert not np.isnan(gam.view(np.float64)).any() and not np.isnan(share).any()
    rg, rs = R.spike_gamma(K, G, A)
    m = np.abs(K)
    amp = np.where(m > 0, np.maximum(1.0, A / np.where(m > 0, m, 1.0)), 1.0)
    eg = np.abs(gam - rg * INV_N) / (np.abs(G) * amp * INV_N)
    es = np.abs(share - rs * INV_N) / (A * np.abs(G) * INV_N)
    print("largest error / scale: Gamma %.2e share %.2e" % (eg.max(), es.max()))
    assert eg.max() <= TOL and es.max() <= TOL
    assert gam[0] == -G[0] * INV_N and share[0] == A[0] * G[0].real * INV_N    # m = 0: the phase is constant
    # self-conjugate f: q = 0, so Gamma = -u p = -G whatever A / m is, and it is real
    assert gam[1] == -G[1] * INV_N and gam[2] == -G[2] * INV_N
    assert share[1] == A[1] * G[1].real * INV_N and share[2] == -A[2] * G[2].real * INV_N


def test_gamma_is_the_adjoint_of_the_delta_differential():
    # Re(conj(G) dDelta) = Re(conj(Gamma) dK) for the differential of Delta(K) along any dK: the image
    # gradient's coefficient is the adjoint of the forward's, checked by a central difference in float64
    rng = np.random.default_rng(3)
    K = rng.standard_normal(8) + 1j * rng.standard_normal(8)
    G = rng.standard_normal(8) + 1j * rng.standard_normal(8)
    dK = rng.standard_normal(8) + 1j * rng.standard_normal(8)
    A = np.exp(rng.uniform(0.0, 3.0, 8))
    h = 1e-6
    dD = (E.spike_delta(K + h * dK, A, 1.0) - E.spike_delta(K - h * dK, A, 1.0)) / (2 * h)
    gam, _ = E.spike_gamma(K, G, A, 1.0)
    lhs, rhs = (np.conj(G) * dD).real, (np.conj(gam) * dK).real
    assert np.abs(lhs - rhs).max() <= 1e-8 * np.abs(rhs).max()


@pytest.mark.parametrize("B,C,S", [(9, 1, 3), (3, 2, 1), (17, 2, 6)], ids=["two_groups", "one_group", "three_groups"])
def test_dI_sum_is_ordered_and_adds_over_launch_groups(B, C, S):
    rng = np.random.default_rng(B)
    share = rng.standard_normal((B * C, S)) * np.exp(rng.uniform(0.0, 10.0, (B * C, S)))
    dI = E.spike_dI(share, B, C)          # pre-filled with NaN
    assert not np.isnan(dI).any()
    ref = None
    for b0 in range(0, B, 8):
        s = np.zeros(S)
        for r in share[b0 * C:min(b0 + 8, B) * C]:
            s = s + r                     # volume-channel order, float64
        ref = s.astype(np.float32) if ref is None else ref + s.astype(np.float32)
    assert ref.dtype == np.float32 and np.array_equal(dI, ref)
    groups = (B + 7) // 8
    assert np.all(np.abs(dI - share.sum(0)) <= groups * 2.0 ** -23 * np.abs(share).sum(0))
    assert np.array_equal(dI, E.spike_dI(share, B, C))
