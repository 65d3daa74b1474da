"""The centred complex spectrum out of and into the library (shift_fourier / inv_shift_fourier), on the
host emulator of the per-unit bodies (spectrum.h export_unit / import_unit, the code k_kspace_export /
k_kspace_import run), plus the host-side pieces: the autograd formulas, the library symbols, the op
schemas, argument validation and the drop-in switch.

Reference, float64, written here with numpy: K = fftshift(fftn(x)), y = Re(ifftn(ifftshift(K))).
Bar (DESIGN (c)): max|a - ref| / max|ref| <= 1e-5.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import _emu_spectrum as E
from _golden import relerr

TOL = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (image shape [B, C, *spatial], transformed axes, columns per unit)
CASES = [
    ((2, 3, 12, 10, 9), 3, 7),      # odd D, ragged last tile (50 columns)
    ((1, 2, 9, 8, 6), 3, 8),        # even D: both self-conjugate columns
    ((1, 2, 16, 12), 2, 4),         # 2-D: (H, 1, D), ragged (7 columns)
    ((1, 1, 20, 48, 35), 3, 16),    # radix set with 5 and 7
    ((1, 2, 128, 8, 6), 3, 32),     # long H, one tile holds every column
    ((9, 1, 12, 10, 9), 3, 5),      # more than TB_MAX_BATCH samples: two launch groups
    ((1, 1, 6, 128, 128), 3, 64),   # the shape of the compiled slab passes, on the run-time bodies
]
IDS = ["odd_d", "even_d", "2d", "radix_5_7", "long_h", "two_groups", "slab_128"]


def ref_export(x, n_dims):
    ax = tuple(range(-n_dims, 0))
    return np.fft.fftshift(np.fft.fftn(np.asarray(x, np.float64), axes=ax), axes=ax)


def ref_import(k, n_dims):
    ax = tuple(range(-n_dims, 0))
    return np.fft.ifftn(np.fft.ifftshift(np.asarray(k, np.complex128), axes=ax), axes=ax).real


def mirror_defect(k, n_dims):
    """Elements that differ from the conjugate of their mirror K(-f) (flip and roll by one in the
    unshifted layout), over the columns kd whose mirror is not a stored coefficient of its own: there f
    and -f are the two stores of one value."""
    ax = tuple(range(-n_dims, 0))
    u = np.fft.ifftshift(k, axes=ax)
    m = np.conj(np.roll(np.flip(u, axis=ax), 1, axis=ax))
    D = k.shape[-1]
    kd = [i for i in range(1, D) if 2 * i != D]
    return int(np.count_nonzero(u[..., kd] != m[..., kd]))


def _image(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def _spectrum(shape, seed):
    rng = np.random.default_rng(seed)   # not Hermitian: the import symmetrises
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


@pytest.mark.parametrize("shape,n_dims,T", CASES, ids=IDS)
def test_export_unit_matches_float64_and_writes_once(shape, n_dims, T):
    x = _image(shape, 50)
    k = E.kspace_export(x, n_dims, T=T)                 # pre-filled with NaN
    assert k.shape == x.shape and k.dtype == np.complex64
    assert not np.isnan(k.real).any() and not np.isnan(k.imag).any()   # every element written
    ref = ref_export(x, n_dims)
    e = float(np.max(np.abs(k - ref)) / np.max(np.abs(ref)))
    print(f"export, emulator vs float64 {e:.3e}")
    assert e <= TOL
    assert mirror_defect(k, n_dims) == 0
    assert np.array_equal(k, E.kspace_export(x, n_dims, T=T))


@pytest.mark.parametrize("pad", [0, 3], ids=["pad0", "pad3"])
@pytest.mark.parametrize("shape,n_dims,T", CASES, ids=IDS)
def test_import_unit_matches_float64(shape, n_dims, T, pad):
    k = _spectrum(shape, 51)
    y = E.kspace_import(k, n_dims, pad=pad, T=T)        # pre-filled with NaN
    D = shape[-1]
    assert y.shape == shape[:-1] + (D + pad,)
    assert not np.isnan(y).any()
    e = relerr(y[..., :D], ref_import(k, n_dims))
    print(f"import, emulator vs float64 {e:.3e}")
    assert e <= TOL
    assert np.all(y[..., D:] == 0.0)


def test_tile_width_does_not_change_the_result():
    x = _image((2, 3, 12, 10, 9), 52)
    assert np.array_equal(E.kspace_export(x, 3, T=3), E.kspace_export(x, 3, T=16))
    k = _spectrum((2, 3, 12, 10, 9), 53)
    assert np.array_equal(E.kspace_import(k, 3, T=3), E.kspace_import(k, 3, T=16))


def test_round_trip_and_adjoint_identity():
    shape = (2, 3, 12, 10, 9)
    x = _image(shape, 54)
    k = _spectrum(shape, 55)
    kx = E.kspace_export(x, 3, T=7)
    assert relerr(E.kspace_import(kx, 3, T=7), x) <= TOL
    # Re<export(x), K> = N <x, import(K)>
    n = 12 * 10 * 9
    lhs = np.vdot(kx.astype(np.complex128), k.astype(np.complex128)).real
    rhs = n * float(np.sum(x.astype(np.float64) * E.kspace_import(k, 3, T=7).astype(np.float64)))
    assert abs(lhs - rhs) <= 1e-5 * np.linalg.norm(kx.astype(np.complex128)) * np.linalg.norm(k.astype(np.complex128))


# ----------------------------------------------------------------- the autograd formulas, float64
def test_autograd_formulas_are_the_autograd_of_the_fft_expressions():
    rng = np.random.default_rng(56)
    shape, ax = (2, 6, 5, 4), (-3, -2, -1)
    n = 6 * 5 * 4

    def fwd(x):
        return torch.fft.fftshift(torch.fft.fftn(x, dim=ax), dim=ax)

    def inv(k):
        return torch.fft.ifftn(torch.fft.ifftshift(k, dim=ax), dim=ax).real

    def rel(a, b):
        return float((a - b).abs().max() / b.abs().max())

    x = torch.from_numpy(rng.standard_normal(shape)).requires_grad_(True)
    gk = torch.from_numpy(rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
    (gx,) = torch.autograd.grad(fwd(x), x, gk)                       # gK in PyTorch's convention
    assert rel(n * inv(gk), gx) <= 1e-12
    k = torch.from_numpy(rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).requires_grad_(True)
    gy = torch.from_numpy(rng.standard_normal(shape))
    (gkk,) = torch.autograd.grad(inv(k), k, gy)
    assert rel(fwd(gy) / n, gkk) <= 1e-12


# ----------------------------------------------------------------- host-side pieces (no device)
def test_library_exports_the_new_symbols():
    so = os.path.join(ROOT, "medical-vision-textural-bias_amd", "libtexbias.so")
    lib = ctypes.CDLL(so)                                           # loads without a GPU
    for name in ("tb_spectrum_workspace_bytes", "tb_kspace_export_f32", "tb_kspace_import_f32"):
        assert hasattr(lib, name), name


def test_ops_exist_with_the_stated_schemas_and_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from texbias import ops  # noqa: F401
    from texbias._lib import TexbiasError
    assert str(torch.ops.texbias.shift_fourier.default._schema) == \
        "texbias::shift_fourier(Tensor x, SymInt n_dims) -> Tensor"
    assert str(torch.ops.texbias.inv_shift_fourier.default._schema) == \
        "texbias::inv_shift_fourier(Tensor k, SymInt n_dims, SymInt pad=0) -> Tensor"
    with FakeTensorMode():
        x = torch.empty((2, 3, 6, 5, 4))
        k = torch.ops.texbias.shift_fourier(x, 3)
        assert k.shape == x.shape and k.dtype == torch.complex64
        y = torch.ops.texbias.inv_shift_fourier(k, 3, 2)
        assert y.shape == (2, 3, 6, 5, 6) and y.dtype == torch.float32
    with pytest.raises(TexbiasError, match="HIP"):
        torch.ops.texbias.shift_fourier(torch.zeros((2, 3, 6, 5, 4)), 3)
    with pytest.raises(TexbiasError, match="HIP"):
        torch.ops.texbias.inv_shift_fourier(torch.zeros((2, 3, 6, 5, 4), dtype=torch.complex64), 3, 0)


def test_runtime_validation():
    from texbias import runtime as rt
    from texbias._lib import TexbiasError
    x = torch.zeros((2, 3, 6, 5, 4))
    k = torch.zeros((2, 3, 6, 5, 4), dtype=torch.complex64)
    with pytest.raises(ValueError, match="float32"):
        rt.kspace_export(x.double(), 3)
    with pytest.raises(ValueError, match="float32"):
        rt.kspace_export(k, 3)
    with pytest.raises(ValueError, match="complex64"):
        rt.kspace_import(x, 3)
    with pytest.raises(ValueError, match="complex64"):
        rt.kspace_import(k.to(torch.complex128), 3)
    with pytest.raises(ValueError, match="transformed axes"):
        rt.kspace_export(x, 6)
    with pytest.raises(ValueError, match="transformed axes"):
        rt.kspace_import(k, 0)
    with pytest.raises(ValueError, match="torch tensor"):
        rt.kspace_export(x.numpy(), 3)
    with pytest.raises(TexbiasError, match="HIP"):
        rt.kspace_export(x, 3)
    with pytest.raises(TexbiasError, match="HIP"):
        rt.kspace_import(k, 3)


def test_dropin_switch_is_off_by_default_and_leaves_cpu_tensors_on_torch_fft():
    import texbias
    import filters_and_operators as fo
    import stylization_layers as sl
    import utils2
    sp = texbias.spectrum
    assert sp.__all__ == ["shift_fourier", "inv_shift_fourier", "set_dropin", "dropin_enabled"]
    if "TEXBIAS_FOURIER" not in os.environ:
        assert sp.dropin_enabled() is False
    x = torch.from_numpy(_image((2, 6, 5, 4), 57))
    ax = (-3, -2, -1)
    ref_k = torch.fft.fftshift(torch.fft.fftn(x, dim=ax), dim=ax)
    ref_y = torch.fft.ifftn(torch.fft.ifftshift(ref_k, dim=ax), dim=ax).real
    prev = sp.set_dropin(True)
    try:
        assert sp.dropin_enabled() is True
        for cls in (fo.Fourier, sl.Fourier, utils2.FourierTransform):   # CPU tensors: torch.fft either way
            assert torch.equal(cls.shift_fourier(x, 3), ref_k)
            assert torch.equal(cls.inv_shift_fourier(ref_k, 3), ref_y)
        assert not sp.takes(x, torch.float32)
    finally:
        sp.set_dropin(prev)
    assert sp.dropin_enabled() is prev
    for cls in (fo.Fourier, sl.Fourier, utils2.FourierTransform):
        assert torch.equal(cls.shift_fourier(x, 3), ref_k)
        assert torch.equal(cls.inv_shift_fourier(ref_k, 3), ref_y)
