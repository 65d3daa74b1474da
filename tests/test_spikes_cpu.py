"""The closed formulas of the trainable spike layer (tests/_spikes_ref.py closed_form, what csrc/spike_grad.h and
the kernels implement) against torch.autograd of the reference's own expression in float64, and the two exact
identities that rest on no FFT reference:
  y(I + ln 2) - y(I) = dy/dI = Re(A u e^{i theta}) / N
  the coefficient the layer set, c_j = FFT(y)(f_j) at a self-conjugate f_j and 2 FFT(y)(f_j) - FFT(x)(f_j)
  elsewhere, has |c_j| = A_j and the phase of FFT(x)(f_j)
(the reference writes K(f_j) alone and takes ``.real``, which halves the change of a coefficient whose conjugate
partner it left untouched: FFT(y)(f_j) = (A_j u + K_j) / 2 there, so |FFT(y)(f_j)| = A_j holds only at DC / Nyquist).
Bar: 1e-9 of the largest reference value -- the reference adds 1e-10 to every modulus, which the closed form does
not, and float64 rounding is five orders below that.
"""
import numpy as np
import pytest

import _spikes_ref as R

TOL = 1e-9
SHAPES = [(2, 3, 8, 6, 5), (1, 2, 6, 4, 4)]


def _locs(spatial):
    generic = tuple(min(n - 1, n // 2 + 1 + a) for a, n in enumerate(spatial))
    kd0 = (1, spatial[1] - 1, spatial[2] // 2)   # kd = 0 plane, not self-conjugate
    return {"generic": [generic], "dc": [R.centre(spatial)], "nyquist": [R.nyquist(spatial)], "kd0": [kd0],
            "all": [generic, R.centre(spatial), R.nyquist(spatial), kd0]}


def _data(shape, S, seed=5):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape), rng.standard_normal(shape), rng.uniform(2.0, 6.0, S)


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("which", ["generic", "dc", "nyquist", "kd0", "all"])
@pytest.mark.parametrize("shape", SHAPES, ids=["8x6x5", "6x4x4"])
def test_closed_form_matches_autograd_of_the_reference_expression(shape, which):
    locs = _locs(shape[2:])[which]
    x, g, I = _data(shape, len(locs))
    y, gx, dI = R.reference_grads(x, g, I, locs, 3)
    c = R.closed_form(x, g, I, locs, 3)
    e = (_rel(c["y"], y), _rel(c["gx"], gx), np.abs(c["dI"] - dI).max() / np.abs(dI).max())
    print("y %.2e gx %.2e dI %.2e" % e)
    assert max(e) <= TOL


@pytest.mark.parametrize("shape", SHAPES, ids=["8x6x5", "6x4x4"])
def test_doubling_the_intensity_adds_the_intensity_derivative(shape):
    locs = _locs(shape[2:])["all"]
    x, g, I = _data(shape, len(locs))
    a, b = R.closed_form(x, g, I, locs, 3), R.closed_form(x, g, I + np.log(2.0), locs, 3)
    # sum_n g (y(I + ln 2) - y(I)) = sum_j dI_j: the derivative itself, not a finite-difference estimate
    assert abs((g * (b["y"] - a["y"])).sum() - a["dI"].sum()) <= 1e-12 * a["dI_scale"].sum()
    # and per spike against the plane wave
    N = float(np.prod(shape[2:]))
    d = np.zeros(shape)
    for j, loc in enumerate(locs):
        K = a["K"][..., j]
        u = K / np.abs(K)
        d += (np.exp(I[j]) * u[..., None, None, None] * R.plane(loc, shape[2:])).real / N
    assert _rel(b["y"] - a["y"], d) <= 1e-12


@pytest.mark.parametrize("which", ["closed_form", "reference"])
@pytest.mark.parametrize("shape", SHAPES, ids=["8x6x5", "6x4x4"])
def test_output_spectrum_has_the_set_modulus_and_the_input_phase(shape, which):
    # on the closed form to float64 rounding, and on the reference's own expression to its 1e-10 offset
    locs = _locs(shape[2:])["all"]
    x, g, I = _data(shape, len(locs))
    y = R.closed_form(x, g, I, locs, 3)["y"] if which == "closed_form" else R.reference_grads(x, g, I, locs, 3)[0]
    tol = 1e-12 if which == "closed_form" else TOL
    ax = (-3, -2, -1)
    ky, kx = np.fft.fftshift(np.fft.fftn(y, axes=ax), axes=ax), np.fft.fftshift(np.fft.fftn(x, axes=ax), axes=ax)
    touched = np.zeros(shape[2:], bool)
    for j, loc in enumerate(locs):
        vy, vx = R.set_coefficient(ky, kx, loc, shape[2:]), kx[(Ellipsis,) + tuple(loc)]
        assert np.abs(np.abs(vy) / np.exp(I[j]) - 1.0).max() <= tol
        assert np.abs(vy / np.abs(vy) - vx / np.abs(vx)).max() <= 100 * tol
        touched[tuple(loc)] = True
        touched[tuple((2 * (n // 2) - s) % n for s, n in zip(loc, shape[2:]))] = True   # the conjugate bin
    assert np.abs((ky - kx)[..., ~touched]).max() <= 1e-9 * np.abs(kx).max()


def test_zero_coefficient_takes_unit_phase_and_constant_phase_gradient():
    # m = 0: u = 1 as spike_target, Gamma = -G
    K, G, A = np.array([0.0 + 0.0j]), np.array([0.3 - 0.7j]), 5.0
    assert R.spike_delta(K, A)[0] == 5.0
    gam, ap = R.spike_gamma(K, G, A)
    assert gam[0] == -G[0] and ap[0] == A * G[0].real
