"""Gradient of the TB_OP_MASK round trip with respect to the mask, on the host emulator of the per-unit
body (maskgrad.h maskgrad_unit, the code k_kspace_maskgrad runs), and the host-side validation of the
runtime functions, the custom ops and the LearnedKSpaceMask module.

Reference, float64, written here: dM[s(f)] = sum Re(X(f) conj(G(f))) / N with X = FFT(x), G = FFT(g),
N = H W D, summed over the samples and, for a shared mask, the channels; and torch.autograd through the
torch.fft expression of y = Re(IFFT(ifftshift(M . fftshift(FFT x)))), which must agree with the formula.
Bar (DESIGN (c)): max|dM - ref| / max|ref| <= 1e-5.
"""
import numpy as np
import pytest
import torch

import _emu_mask_grad as E
from _golden import relerr

TOL = 1e-5

# (image shape [B, C, *spatial], transformed axes, columns per unit)
CASES = [
    ((2, 3, 12, 10, 9), 3, 7),      # odd D, ragged last tile
    ((1, 2, 9, 8, 6), 3, 8),        # even D: both self-conjugate columns
    ((1, 2, 16, 12), 2, 4),         # 2-D: (H, 1, D)
    ((1, 1, 20, 48, 35), 3, 8),     # prime radix set (5, 7)
    ((9, 1, 12, 10, 9), 3, 5),      # more than TB_MAX_BATCH samples: the second launch group adds
]
IDS = ["odd_d", "even_d", "2d", "prime_radix", "two_groups"]


def ref_mask_grad(x, g, n_dims, per_channel):
    ax = tuple(range(-n_dims, 0))
    X = np.fft.fftn(np.asarray(x, np.float64), axes=ax)
    G = np.fft.fftn(np.asarray(g, np.float64), axes=ax)
    v = np.fft.fftshift((X * np.conj(G)).real, axes=ax) / np.prod(x.shape[-n_dims:])
    return v.sum(axis=0) if per_channel else v.sum(axis=(0, 1))


def autograd_mask_grad(x, g, M, n_dims):
    ax = tuple(range(-n_dims, 0))
    Mt = torch.from_numpy(np.asarray(M, np.float64)).requires_grad_(True)
    k = torch.fft.fftshift(torch.fft.fftn(torch.from_numpy(np.asarray(x, np.float64)), dim=ax), dim=ax)
    y = torch.fft.ifftn(torch.fft.ifftshift(k * Mt, dim=ax), dim=ax).real
    y.backward(torch.from_numpy(np.asarray(g, np.float64)))
    return Mt.grad.numpy()


def _data(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)


def mirror_defect(dm, n_dims):
    """Elements that differ from their mirror dM(-f) (flip and roll by one in the unshifted layout), over
    the columns kd whose mirror is not a stored coefficient of its own: there f and -f are the two stores
    of one value.  (kd = 0, and kd = D/2 for even D, hold f and -f as two independently computed values.)"""
    ax = tuple(range(-n_dims, 0))
    u = np.fft.ifftshift(dm, axes=ax)
    m = np.roll(np.flip(u, axis=ax), 1, axis=ax)
    D = dm.shape[-1]
    kd = [k for k in range(1, D) if 2 * k != D]
    return int(np.count_nonzero(u[..., kd] != m[..., kd]))


def test_formula_is_the_autograd_of_the_fft_expression():
    x, g = _data((2, 3, 6, 5, 4), 40)
    rng = np.random.default_rng(41)
    for per_channel in (False, True):
        M = rng.uniform(0.0, 1.5, ((3,) if per_channel else ()) + (6, 5, 4))
        ref = ref_mask_grad(x, g, 3, per_channel)
        assert relerr(autograd_mask_grad(x, g, M, 3), ref) <= 1e-12


@pytest.mark.parametrize("per_channel", [False, True], ids=["shared", "per_channel"])
@pytest.mark.parametrize("shape,n_dims,T", CASES, ids=IDS)
def test_unit_body_matches_float64_and_writes_once(shape, n_dims, T, per_channel):
    x, g = _data(shape, 42)
    per_channel = per_channel and shape[1] > 1   # one channel: mask_channels = 1, the shared form
    dm = E.kspace_mask_grad(x, g, n_dims, shape[1] if per_channel else 1, T=T)   # pre-filled with NaN
    assert dm.shape == ((shape[1],) if per_channel else ()) + tuple(shape[2:])
    assert not np.isnan(dm).any()                                  # every element written
    e = relerr(dm, ref_mask_grad(x, g, n_dims, per_channel))       # none twice: the second group's adds would double it
    print(f"emulator vs float64 {e:.3e}")
    assert e <= TOL
    assert mirror_defect(dm, n_dims) == 0
    assert np.array_equal(dm, E.kspace_mask_grad(x, g, n_dims, shape[1] if per_channel else 1, T=T))


def test_tile_width_does_not_change_the_result():
    x, g = _data((2, 3, 12, 10, 9), 43)
    a = E.kspace_mask_grad(x, g, 3, 1, T=3)
    assert np.array_equal(a, E.kspace_mask_grad(x, g, 3, 1, T=16))


# ----------------------------------------------------------------- host-side validation (no device)
def test_runtime_mask_grad_validation():
    from texbias import runtime as rt
    from texbias._lib import TexbiasError
    x = torch.zeros((2, 3, 6, 5, 4))
    with pytest.raises(ValueError, match="does not match"):
        rt.kspace_mask_grad(x, torch.zeros((2, 3, 6, 5, 5)), 3, 1)
    with pytest.raises(ValueError, match="float32"):
        rt.kspace_mask_grad(x, x.double(), 3, 1)
    with pytest.raises(ValueError, match="float32"):
        rt.kspace_mask_grad(x.half(), x.half(), 3, 1)
    with pytest.raises(ValueError, match="mask channels"):
        rt.kspace_mask_grad(x, x, 3, 2)
    with pytest.raises(ValueError, match="do not divide"):
        rt.kspace_mask_grad(x, x, 3, 1, channels=4)
    with pytest.raises(ValueError, match="transformed axes"):
        rt.kspace_mask_grad(x, x, 6, 1)
    with pytest.raises(ValueError, match="torch tensors"):
        rt.kspace_mask_grad(x.numpy(), x, 3, 1)
    with pytest.raises(TexbiasError, match="HIP"):
        rt.kspace_mask_grad(x, x, 3, 1)
    with pytest.raises(TexbiasError, match="HIP"):
        rt.kspace_mask_grad(x, x, 3, 3)


def test_learnable_mask_passes_the_geometry_check_only_on_the_new_path():
    from texbias import runtime as rt
    from texbias._lib import TexbiasError
    x = torch.zeros((2, 3, 6, 5, 4))
    M = torch.ones((6, 5, 4), requires_grad=True)
    with pytest.raises(ValueError, match="requires_grad"):
        rt.mask_geometry(x, M, 3)
    with pytest.raises(ValueError, match="requires_grad"):
        rt.kspace_mask(x, M, 3)
    assert rt.mask_geometry(x, M, 3, learnable=True) == (1, 3)
    assert rt.mask_geometry(x, torch.ones((3, 6, 5, 4), requires_grad=True), 3, learnable=True) == (3, 3)
    with pytest.raises(ValueError, match="neither"):
        rt.kspace_mask_learn(x, torch.ones((6, 5, 5), requires_grad=True), 3)
    with pytest.raises(ValueError, match="float32"):
        rt.kspace_mask_learn(x, torch.ones((6, 5, 4), dtype=torch.float64, requires_grad=True), 3)
    with pytest.raises(ValueError, match="contiguous"):
        rt.kspace_mask_learn(x, torch.ones((6, 5, 8))[..., ::2], 3)
    with pytest.raises(TexbiasError, match="HIP"):
        rt.kspace_mask_learn(x, M, 3)


def test_ops_are_registered_with_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from texbias import ops  # noqa: F401
    from texbias._lib import TexbiasError
    with FakeTensorMode():
        x = torch.empty((2, 3, 6, 5, 4))
        assert torch.ops.texbias.kspace_mask_grad(x, x, 3, 3, 1).shape == (6, 5, 4)
        assert torch.ops.texbias.kspace_mask_grad(x, x, 3, 3, 3).shape == (3, 6, 5, 4)
        assert torch.ops.texbias.kspace_mask_learn(x, torch.empty((6, 5, 4)), 3, 3, 2).shape == (2, 3, 6, 5, 6)
    x = torch.zeros((2, 3, 6, 5, 4))
    with pytest.raises(TexbiasError, match="HIP"):
        torch.ops.texbias.kspace_mask_grad(x, x, 3, 3, 1)
    with pytest.raises(TexbiasError, match="HIP"):
        torch.ops.texbias.kspace_mask_learn(x, torch.ones((6, 5, 4), requires_grad=True), 3, 3, 0)


def test_module_validation_and_state():
    from texbias.masks import KSpaceMask, LearnedKSpaceMask
    from texbias._lib import TexbiasError
    import texbias.masks as masks
    assert "LearnedKSpaceMask" in masks.__all__
    with pytest.raises(ValueError, match="complex"):
        LearnedKSpaceMask(np.ones((6, 5, 4), np.complex64))
    with pytest.raises(ValueError, match="neither spatial"):
        LearnedKSpaceMask(np.ones((5, 4)), n_dims=3)
    init = np.random.default_rng(44).uniform(0.0, 1.0, (3, 6, 5, 4))      # float64 in, float32 parameter
    layer = LearnedKSpaceMask(init)
    assert [n for n, _ in layer.named_parameters()] == ["mask"]
    assert layer.mask.dtype == torch.float32 and layer.mask.is_contiguous() and layer.mask.requires_grad
    assert np.array_equal(layer.mask.detach().numpy(), init.astype(np.float32))
    with pytest.raises(ValueError, match="batch"):
        layer(torch.zeros((3, 6, 5, 4)))
    with pytest.raises(ValueError, match="float32"):
        layer(torch.zeros((2, 3, 6, 5, 4), dtype=torch.float64))
    with pytest.raises(ValueError, match="neither"):
        layer(torch.zeros((2, 3, 6, 5, 5)))
    with pytest.raises(ValueError, match="neither"):
        layer(torch.zeros((2, 2, 6, 5, 4)))
    with pytest.raises(TexbiasError, match="HIP"):
        layer(torch.zeros((2, 3, 6, 5, 4)))
    # as_transform shares the parameter's storage: an optimizer step shows through
    t = layer.as_transform()
    assert isinstance(t, KSpaceMask) and not t.mask.requires_grad
    with torch.no_grad():
        layer.mask.add_(1.0)
    assert t.mask.data_ptr() == layer.mask.data_ptr() and torch.equal(t.mask, layer.mask.detach())
    other = LearnedKSpaceMask(np.zeros((3, 6, 5, 4)))
    other.load_state_dict(layer.state_dict())
    assert torch.equal(other.mask, layer.mask)
