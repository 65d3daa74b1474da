"""Gradient of the TB_OP_CMASK round trip with respect to the complex mask, on the host emulator of the
per-unit body (maskgrad.h maskgrad_unit with CX = true, the code k_kspace_cmaskgrad runs).

Reference, float64, written here: dM[s(f)] = sum conj(X(f)) G(f) / N with X = FFT(x), G = FFT(g),
N = H W D, summed over the samples and, for a shared mask, the channels; and torch.autograd through the
torch.fft expression of y = Re(IFFT(ifftshift(M . fftshift(FFT x)))) for a complex leaf M, which must agree
with the formula.  Bar (DESIGN (c)): max|dM - ref| / max|ref| <= 1e-5.
"""
import numpy as np
import pytest
import torch

import _emu_cmask_grad as E
import _emu_mask_grad as ER

TOL = 1e-5

# (image shape [B, C, *spatial], transformed axes, columns per unit): those of test_emu_mask_grad.py
CASES = [
    ((2, 3, 12, 10, 9), 3, 7),      # odd D, ragged last tile
    ((1, 2, 9, 8, 6), 3, 8),        # even D: both self-conjugate columns
    ((1, 2, 16, 12), 2, 4),         # 2-D: (H, 1, D)
    ((1, 1, 20, 48, 35), 3, 8),     # prime radix set (5, 7)
    ((9, 1, 12, 10, 9), 3, 5),      # more than TB_MAX_BATCH samples: the second launch group adds
]
IDS = ["odd_d", "even_d", "2d", "prime_radix", "two_groups"]


def crelerr(a, b) -> float:
    """max|a - b| / max|b| over complex values."""
    a, b = np.asarray(a, np.complex128), np.asarray(b, np.complex128)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30))


def ref_cmask_grad(x, g, n_dims, per_channel):
    ax = tuple(range(-n_dims, 0))
    X = np.fft.fftn(np.asarray(x, np.float64), axes=ax)
    G = np.fft.fftn(np.asarray(g, np.float64), axes=ax)
    v = np.fft.fftshift(np.conj(X) * G, axes=ax) / np.prod(x.shape[-n_dims:])
    return v.sum(axis=0) if per_channel else v.sum(axis=(0, 1))


def autograd_cmask_grad(x, g, M, n_dims):
    ax = tuple(range(-n_dims, 0))
    Mt = torch.from_numpy(np.asarray(M, np.complex128)).requires_grad_(True)
    k = torch.fft.fftshift(torch.fft.fftn(torch.from_numpy(np.asarray(x, np.float64)), dim=ax), dim=ax)
    y = torch.fft.ifftn(torch.fft.ifftshift(k * Mt, dim=ax), dim=ax).real
    y.backward(torch.from_numpy(np.asarray(g, np.float64)))
    return Mt.grad.numpy()


def _data(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)


def mirror_defect(dm, n_dims):
    """Elements that are not the exact conjugate of their mirror dM(-f) (flip and roll by one in the
    unshifted layout), over the columns kd whose mirror is not a stored coefficient of its own: there f and
    -f are the two stores of one value, equal bit for bit up to the imaginary sign.  (kd = 0, and kd = D/2
    for even D, hold f and -f as two independently computed values.)"""
    ax = tuple(range(-n_dims, 0))
    u = np.fft.ifftshift(dm, axes=ax)
    m = np.roll(np.flip(u, axis=ax), 1, axis=ax)
    D = dm.shape[-1]
    kd = [k for k in range(1, D) if 2 * k != D]
    a, b = u[..., kd], m[..., kd]
    return int(np.count_nonzero((a.real != b.real) | (a.imag != -b.imag)))


def test_formula_is_the_autograd_of_the_fft_expression():
    x, g = _data((2, 3, 6, 5, 4), 50)
    rng = np.random.default_rng(51)
    for per_channel in (False, True):
        sh = ((3,) if per_channel else ()) + (6, 5, 4)
        M = rng.uniform(0.0, 1.5, sh) * np.exp(1j * rng.uniform(-np.pi, np.pi, sh))
        ref = ref_cmask_grad(x, g, 3, per_channel)
        assert crelerr(autograd_cmask_grad(x, g, M, 3), ref) <= 1e-12
        # Hermitian: dM(-f) = conj(dM(f)), real at the self-conjugate f (DC here)
        u = np.fft.ifftshift(ref, axes=(-3, -2, -1))
        assert crelerr(np.roll(np.flip(u, axis=(-3, -2, -1)), 1, axis=(-3, -2, -1)), np.conj(u)) <= 1e-12
        assert np.max(np.abs(u[..., 0, 0, 0].imag)) <= 1e-12 * np.max(np.abs(u))


@pytest.mark.parametrize("per_channel", [False, True], ids=["shared", "per_channel"])
@pytest.mark.parametrize("shape,n_dims,T", CASES, ids=IDS)
def test_unit_body_matches_float64_and_writes_once(shape, n_dims, T, per_channel):
    x, g = _data(shape, 52)
    per_channel = per_channel and shape[1] > 1   # one channel: mask_channels = 1, the shared form
    cm = shape[1] if per_channel else 1
    dm = E.kspace_cmask_grad(x, g, n_dims, cm, T=T)               # pre-filled with NaN + i NaN
    assert dm.shape == ((shape[1],) if per_channel else ()) + tuple(shape[2:]) and dm.dtype == np.complex64
    assert not np.isnan(dm.real).any() and not np.isnan(dm.imag).any()    # every element written, both halves
    ref = ref_cmask_grad(x, g, n_dims, per_channel)
    assert np.max(np.abs(ref.imag)) > 0.1 * np.max(np.abs(ref))   # the imaginary part is not small
    e = crelerr(dm, ref)          # none written twice: the second group's adds would double it
    print(f"emulator vs float64 {e:.3e}")
    assert e <= TOL
    assert mirror_defect(dm, n_dims) == 0
    assert np.array_equal(dm, E.kspace_cmask_grad(x, g, n_dims, cm, T=T))
    # the real part is the real-mask gradient, the same accumulator
    assert np.array_equal(dm.real, ER.kspace_mask_grad(x, g, n_dims, cm, T=T))


def test_second_launch_group_accumulates():
    """Nine samples are two launch groups (8 + 1): the sum equals the two groups run on their own."""
    x, g = _data((9, 1, 12, 10, 9), 53)
    both = E.kspace_cmask_grad(x, g, 3, 1, T=5)
    first = E.kspace_cmask_grad(x[:8], g[:8], 3, 1, T=5)
    last = E.kspace_cmask_grad(x[8:], g[8:], 3, 1, T=5)
    assert np.array_equal(both, first + last)
    assert crelerr(last, ref_cmask_grad(x[8:], g[8:], 3, False)) <= TOL


def test_tile_width_does_not_change_the_result():
    x, g = _data((2, 3, 12, 10, 9), 54)
    a = E.kspace_cmask_grad(x, g, 3, 1, T=3)
    assert np.array_equal(a, E.kspace_cmask_grad(x, g, 3, 1, T=16))
