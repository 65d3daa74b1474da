"""Radial k-space profiles, the semantics on the host (numpy / torch only; no device, no emulator).

Restated here (tests/_radial_ref.py holds the code): element s of the centred layout has signed index
k_a = s_a - floor(n_a / 2), r2 = sum k_a^2, u = f32_sqrt((float)r2) * (float)(1 / dr); nearest: bin
min((int)u, K-1); linear: b0 = (int)u, weight 1 on K-1 when b0 >= K-1, else 1-t on b0 and t on b0+1 with
t = u - (float)b0.  expand M[s] = sum_k w_k(s) p[k]; bin q[k] = sum_s w_k(s) A[s]; power P[k] =
sum_f w_k(f) |X(f)|^2 / N; profile gradient dp = bin(Re(X conj G) / N).
"""
import numpy as np
import pytest
import torch

import _radial_ref as R
from _golden import relerr

SHAPES = [(12, 10, 9), (9, 8, 6), (16, 12), (20, 48, 35)]
PARAMS = [(8, 1.0), (3, 2.5), (11, 1.0), (20, 1.5), (40, 0.25)]


@pytest.mark.parametrize("mode", [R.NEAREST, R.LINEAR], ids=["nearest", "linear"])
@pytest.mark.parametrize("spatial", SHAPES, ids=str)
def test_weights_sum_to_one_and_are_even(spatial, mode):
    for K, dr in PARAMS:
        b0, w0, w1 = R.weights(spatial, K, dr, mode)
        assert b0.min() >= 0 and b0.max() <= K - 1
        assert np.all(w1[b0 == K - 1] == 0)                       # no second bin past the clamp
        assert np.array_equal(w0 + w1, np.ones(spatial, np.float32))
        assert np.all(w0 >= 0) and np.all(w1 >= 0)
        # f -> -f: flip and roll by one in the unshifted layout
        ax = tuple(range(len(spatial)))
        for a in (b0, w0, w1):
            u = np.fft.ifftshift(a, axes=ax)
            assert np.array_equal(u, np.roll(np.flip(u, axis=ax), 1, axis=ax))


def test_bin_formula_on_known_elements():
    # (12, 10, 9): centre (6, 5, 4); element (6, 5, 4) has r = 0, (9, 5, 0) has r2 = 9 + 16 = 25
    b0, w0, w1 = R.weights((12, 10, 9), 8, 1.0, R.LINEAR)
    assert b0[6, 5, 4] == 0 and w0[6, 5, 4] == 1 and w1[6, 5, 4] == 0
    assert b0[9, 5, 0] == 5 and w0[9, 5, 0] == 1 and w1[9, 5, 0] == 0
    u = np.float32(np.sqrt(np.float32(2)))                         # (7, 6, 4): r2 = 2
    assert b0[7, 6, 4] == 1 and w1[7, 6, 4] == np.float32(u - np.float32(1))
    assert b0[0, 0, 0] == 7 and w0[0, 0, 0] == 1                   # r2 = 77: past (K-1) dr, clamped
    b0, w0, w1 = R.weights((12, 10, 9), 3, 2.5, R.NEAREST)
    assert b0[9, 5, 0] == 2 and b0[8, 5, 4] == int(np.float32(2) * np.float32(1 / 2.5))


@pytest.mark.parametrize("mode", [R.NEAREST, R.LINEAR], ids=["nearest", "linear"])
def test_bin_is_the_adjoint_of_expand(mode):
    rng = np.random.default_rng(31)
    for spatial, (K, dr) in zip(SHAPES, PARAMS):
        p = rng.standard_normal((3, K))
        A = rng.standard_normal((3,) + spatial)
        lhs = np.sum(R.expand(p, spatial, dr, mode) * A)
        rhs = np.sum(p * R.bin_(A, len(spatial), K, dr, mode))
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)


@pytest.mark.parametrize("spatial", [(12, 10, 9), (9, 8, 6)], ids=str)
@pytest.mark.parametrize("r", [1, 4, 7])
def test_disk_profile_is_the_oracle_disk(spatial, r):
    from oracle.filters_oracle import disk_mask
    from texbias.radial import RadialFilter, max_bin
    f = RadialFilter.disk(r, spatial)
    assert f.dr == 1.0 and f.mode == R.NEAREST and f.profile.shape == (max_bin(spatial) + 1,)
    m = R.expand(f.profile.numpy(), spatial, f.dr, f.mode).astype(np.float32)
    assert np.array_equal(m, disk_mask(spatial, r, 3, False))


def test_max_bin_leaves_nothing_clamped():
    from texbias.radial import max_bin
    for spatial in SHAPES:
        for dr in (1.0, 1.5, 0.25):
            K = max_bin(spatial, dr) + 1
            b0, _, _ = R.weights(spatial, K + 3, dr, R.NEAREST)
            assert b0.max() == K - 1


@pytest.mark.parametrize("mode", [R.NEAREST, R.LINEAR], ids=["nearest", "linear"])
def test_parseval(mode):
    rng = np.random.default_rng(31)
    x = rng.standard_normal((2, 3, 12, 10, 9)).astype(np.float32)
    P = R.power(x, 3, 8, 1.0, mode)
    assert relerr(P.sum(-1), (x.astype(np.float64) ** 2).sum(axis=(2, 3, 4))) <= 1e-12


def _torch_weights(spatial, K, dr, mode):
    b0, w0, w1 = R.weights(spatial, K, dr, mode)
    return (torch.from_numpy(b0), torch.from_numpy(np.minimum(b0 + 1, K - 1)),
            torch.from_numpy(w0.astype(np.float64)), torch.from_numpy(w1.astype(np.float64)))


@pytest.mark.parametrize("mode", [R.NEAREST, R.LINEAR], ids=["nearest", "linear"])
@pytest.mark.parametrize("per_channel", [False, True], ids=["shared", "per_channel"])
def test_profile_gradient_is_the_autograd_of_the_fft_expression(mode, per_channel):
    rng = np.random.default_rng(31)
    spatial, K, dr = (6, 5, 4), 5, 1.0
    x = rng.standard_normal((2, 3) + spatial)
    g = rng.standard_normal((2, 3) + spatial)
    b0, b1, w0, w1 = _torch_weights(spatial, K, dr, mode)
    p = torch.from_numpy(rng.uniform(0.0, 1.5, (3, K) if per_channel else (K,))).requires_grad_(True)
    M = w0 * p[..., b0] + w1 * p[..., b1]
    ax = (-3, -2, -1)
    k = torch.fft.fftshift(torch.fft.fftn(torch.from_numpy(x), dim=ax), dim=ax)
    y = torch.fft.ifftn(torch.fft.ifftshift(k * M, dim=ax), dim=ax).real
    y.backward(torch.from_numpy(g))
    assert relerr(p.grad.numpy(), R.grad(x, g, 3, per_channel, K, dr, mode)) <= 1e-12
    assert relerr(M.detach().numpy(), R.expand(p.detach().numpy(), spatial, dr, mode)) <= 1e-15


@pytest.mark.parametrize("mode", [R.NEAREST, R.LINEAR], ids=["nearest", "linear"])
def test_power_gradient_is_twice_the_filter_with_the_expanded_upstream(mode):
    # gx = 2 Re(IFFT(expand(gP) FFT x)) per volume: the formula texbias::radial_power's backward runs
    rng = np.random.default_rng(31)
    spatial, K, dr = (6, 5, 4), 5, 1.0
    x = torch.from_numpy(rng.standard_normal((2, 3) + spatial)).requires_grad_(True)
    gP = rng.standard_normal((2, 3, K))
    b0, b1, w0, w1 = _torch_weights(spatial, K, dr, mode)
    ax = (-3, -2, -1)
    k2 = torch.fft.fftshift(torch.fft.fftn(x, dim=ax), dim=ax).abs() ** 2 / float(np.prod(spatial))
    P = torch.zeros((2, 3, K), dtype=torch.float64)
    P = P.index_add(2, b0.reshape(-1), (k2 * w0).reshape(2, 3, -1)).index_add(2, b1.reshape(-1), (k2 * w1).reshape(2, 3, -1))
    assert relerr(P.detach().numpy(), R.power(x.detach().numpy(), 3, K, dr, mode)) <= 1e-12
    P.backward(torch.from_numpy(gP))
    M = R.expand(gP, spatial, dr, mode)
    X = np.fft.fftshift(np.fft.fftn(x.detach().numpy(), axes=ax), axes=ax)
    ref = 2.0 * np.fft.ifftn(np.fft.ifftshift(X * M, axes=ax), axes=ax).real
    assert relerr(x.grad.numpy(), ref) <= 1e-12


# ----------------------------------------------------------------- host-side validation (no device)
def test_runtime_validation_and_product_path_errors():
    from texbias import runtime as rt
    from texbias._lib import TexbiasError
    x = torch.zeros((2, 3, 6, 5, 4))
    for bad in (dict(bins=0), dict(bins=rt.RADIAL_MAX_BINS + 1), dict(dr=0.0), dict(dr=float("nan")),
                dict(dr=float("inf")), dict(mode=2), dict(mode="cubic")):
        kw = dict(bins=4, dr=1.0, mode=1)
        kw.update(bad)
        with pytest.raises(ValueError):
            rt.radial_power(x, 3, **kw)
        with pytest.raises(ValueError):
            rt.radial_grad(x, x, 3, 1, **kw)
    with pytest.raises(ValueError, match="does not match"):
        rt.radial_grad(x, torch.zeros((2, 3, 6, 5, 5)), 3, 1, 4)
    with pytest.raises(ValueError, match="channels"):
        rt.radial_grad(x, x, 3, 2, 4)
    with pytest.raises(ValueError, match="profile"):
        rt.radial_mask(torch.zeros((2, 3, 4)), (6, 5, 4))
    with pytest.raises(TexbiasError, match="HIP"):
        rt.radial_power(x, 3, 4)
    with pytest.raises(TexbiasError, match="HIP"):
        rt.radial_grad(x, x, 3, 1, 4)
    with pytest.raises(TexbiasError, match="HIP"):
        rt.radial_mask(torch.zeros(4), (6, 5, 4))
    with pytest.raises(TexbiasError, match="HIP"):
        rt.radial_bin(torch.zeros((6, 5, 4)), 3, 4)


def test_ops_are_registered_with_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from texbias import ops  # noqa: F401
    from texbias._lib import TexbiasError
    with FakeTensorMode():
        x = torch.empty((2, 3, 6, 5, 4))
        assert torch.ops.texbias.radial_power(x, 3, 7, 1.0, 0).shape == (2, 3, 7)
        assert torch.ops.texbias.radial_grad(x, x, 3, 3, 1, 7, 1.0, 1).shape == (7,)
        assert torch.ops.texbias.radial_grad(x, x, 3, 3, 3, 7, 1.0, 1).shape == (3, 7)
        assert torch.ops.texbias.radial_mask(torch.empty(7), [6, 5, 4], 1.0, 1).shape == (6, 5, 4)
        assert torch.ops.texbias.radial_mask(torch.empty((3, 7)), [6, 5, 4], 1.0, 1).shape == (3, 6, 5, 4)
        assert torch.ops.texbias.radial_bin(torch.empty((3, 6, 5, 4)), 3, 7, 1.0, 1).shape == (3, 7)
        y, m = torch.ops.texbias.radial_filter(x, torch.empty((3, 7)), 3, 3, 1.0, 1, 2)
        assert y.shape == (2, 3, 6, 5, 6) and m.shape == (3, 6, 5, 4)
    with pytest.raises(TexbiasError, match="HIP"):
        torch.ops.texbias.radial_power(torch.zeros((2, 3, 6, 5, 4)), 3, 7, 1.0, 0)


def test_module_and_transform_validation_and_state():
    import texbias
    from texbias.radial import LearnedRadialFilter, RadialFilter, RadialFilterd, radial_power_spectrum
    from texbias._lib import TexbiasError
    assert texbias.radial.RadialFilter is RadialFilter
    with pytest.raises(ValueError, match="profile"):
        RadialFilter(np.ones((2, 3, 4)))
    with pytest.raises(ValueError, match="mode"):
        RadialFilter(np.ones(4), mode="cubic")
    with pytest.raises(ValueError, match="dr"):
        LearnedRadialFilter(np.ones(4), dr=-1.0)
    with pytest.raises(ValueError, match="radius"):
        RadialFilter.disk(2.5, (6, 5, 4))
    layer = LearnedRadialFilter(np.linspace(1.0, 0.0, 6).reshape(1, 6).repeat(3, 0), dr=1.5)
    assert [n for n, _ in layer.named_parameters()] == ["profile"]
    assert layer.profile.dtype == torch.float32 and layer.profile.shape == (3, 6) and layer.mode == 1
    with pytest.raises(ValueError, match="batch"):
        layer(torch.zeros((3, 6, 5, 4)))
    with pytest.raises(ValueError, match="float32"):
        layer(torch.zeros((2, 3, 6, 5, 4), dtype=torch.float64))
    with pytest.raises(ValueError, match="channels"):
        layer(torch.zeros((2, 2, 6, 5, 4)))
    with pytest.raises(TexbiasError, match="HIP"):
        layer(torch.zeros((2, 3, 6, 5, 4)))
    t = layer.as_transform()
    assert isinstance(t, RadialFilter) and t.dr == 1.5 and t.mode == 1 and not t.profile.requires_grad
    with torch.no_grad():
        layer.profile.add_(1.0)
    assert t.profile.data_ptr() == layer.profile.data_ptr() and t.profile._version == layer.profile._version
    other = LearnedRadialFilter(np.zeros((3, 6)))
    other.load_state_dict(layer.state_dict())
    assert torch.equal(other.profile, layer.profile)
    assert isinstance(RadialFilterd(["image"], np.ones(4)).transform, RadialFilter)
    with pytest.raises(TexbiasError, match="HIP"):
        radial_power_spectrum(torch.zeros((2, 3, 6, 5, 4)))
    from texbias.pipeline import FusedChain
    FusedChain([RadialFilter(np.ones(4))])                          # a fusable transform
