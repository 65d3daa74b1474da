"""The radial reductions on the host emulator of the per-unit body (radial.h radial_unit, the code k_radial_grad
and k_radial_power run, both SELF values) and of the ordered sum, after the run-time planned pass A, launch
groups included; and the dense pair (radial_expand_at, radial_bin_unit).

Semantics (restated in tests/_radial_ref.py): k_a = s_a - floor(n_a / 2), r2 = sum k_a^2,
u = f32_sqrt((float)r2) * (float)(1 / dr); nearest: bin min((int)u, K-1); linear: 1-t on b0 = (int)u and t on
b0+1, weight 1 on K-1 when b0 >= K-1.  power P[k] = sum_f w_k(f) |X(f)|^2 / N; gradient dp[k] =
sum_f w_k(f) Re(X(f) conj(G(f))) / N.  Bars (DESIGN (c)): max|out - ref| / max|ref| <= 1e-5 against float64,
<= 2e-6 between routes.
"""
import numpy as np
import pytest

import _emu_mask_grad as EM
import _emu_radial as E
import _radial_ref as R
from _golden import relerr

TOL, TOL_ROUTE = 1e-5, 2e-6

# (image shape [B, C, *spatial], transformed axes, K, dr, columns per tile)
CASES = [
    ((2, 3, 12, 10, 9), 3, 8, 1.0, 7),       # odd D, ragged last tile
    ((1, 2, 9, 8, 6), 3, 3, 2.5, 8),         # even D; most of the volume lands in the clamped bin
    ((1, 2, 16, 12), 2, 11, 1.0, 4),         # 2-D: (H, 1, D), two channels
    ((1, 1, 20, 48, 35), 3, 20, 1.5, 8),     # prime radix set (5, 7)
    ((9, 1, 12, 10, 9), 3, 8, 1.0, 5),       # more than TB_MAX_BATCH samples: the second launch group adds
]
IDS = ["odd_d", "clamped", "2d", "prime_radix", "two_groups"]
MODES = [R.NEAREST, R.LINEAR]


def _data(shape, seed=31):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)


@pytest.mark.parametrize("mode", MODES, ids=["nearest", "linear"])
@pytest.mark.parametrize("per_channel", [False, True], ids=["shared", "per_channel"])
@pytest.mark.parametrize("shape,n_dims,K,dr,T", CASES, ids=IDS)
def test_gradient_unit_matches_float64_and_the_binned_mask_gradient(shape, n_dims, K, dr, T, per_channel, mode):
    x, g = _data(shape)
    per_channel = per_channel and shape[1] > 1
    cp = shape[1] if per_channel else 1
    dp = E.radial_grad(x, g, n_dims, cp, K, dr, mode, T=T)            # pre-filled with NaN
    assert dp.shape == ((cp, K) if per_channel else (K,))
    assert not np.isnan(dp).any()
    ref = R.grad(x, g, n_dims, per_channel, K, dr, mode)
    e = relerr(dp, ref)
    dm = EM.kspace_mask_grad(x, g, n_dims, cp, T=T)                   # the composed route's dense dM
    e2 = relerr(dp, R.bin_(dm, n_dims, K, dr, mode))
    print(f"emulator vs float64 {e:.3e}, vs bin(mask gradient) {e2:.3e}")
    assert e <= TOL
    assert e2 <= TOL_ROUTE
    assert np.array_equal(dp, E.radial_grad(x, g, n_dims, cp, K, dr, mode, T=T))


@pytest.mark.parametrize("mode", MODES, ids=["nearest", "linear"])
@pytest.mark.parametrize("shape,n_dims,K,dr,T", CASES, ids=IDS)
def test_power_unit_matches_float64_and_parseval(shape, n_dims, K, dr, T, mode):
    x, _ = _data(shape)
    P = E.radial_power(x, n_dims, K, dr, mode, T=T)
    assert P.shape == shape[:2] + (K,) and not np.isnan(P).any()
    e = relerr(P, R.power(x, n_dims, K, dr, mode))
    ep = relerr(P.astype(np.float64).sum(-1), (x.astype(np.float64) ** 2).sum(axis=tuple(range(2, x.ndim))))
    print(f"emulator vs float64 {e:.3e}, parseval {ep:.3e}")
    assert e <= TOL and ep <= TOL
    assert np.array_equal(P, E.radial_power(x, n_dims, K, dr, mode, T=T))
    # the power spectrum is the gradient with g = x, one volume at a time
    v = x[:1, :1]
    assert relerr(E.radial_grad(v, v, n_dims, 1, K, dr, mode, T=T), P[0, 0]) <= TOL_ROUTE


@pytest.mark.parametrize("mode", MODES, ids=["nearest", "linear"])
def test_tile_width_and_tiles_per_unit_agree(mode):
    x, g = _data((2, 3, 12, 10, 9))
    a = E.radial_grad(x, g, 3, 1, 8, 1.0, mode, T=3, tpg=1)
    assert relerr(E.radial_grad(x, g, 3, 1, 8, 1.0, mode, T=16, tpg=2), a) <= TOL_ROUTE
    assert relerr(E.radial_grad(x, g, 3, 1, 8, 1.0, mode, T=3, tpg=5), a) <= TOL_ROUTE
    p = E.radial_power(x, 3, 8, 1.0, mode, T=3, tpg=1)
    assert relerr(E.radial_power(x, 3, 8, 1.0, mode, T=16, tpg=3), p) <= TOL_ROUTE


@pytest.mark.parametrize("mode", MODES, ids=["nearest", "linear"])
@pytest.mark.parametrize("spatial,K,dr", [((12, 10, 9), 8, 1.0), ((9, 8, 6), 3, 2.5), ((16, 12), 11, 1.0),
                                          ((6, 128, 128), 400, 0.25)], ids=str)
def test_dense_pair(spatial, K, dr, mode):
    rng = np.random.default_rng(31)
    p = rng.standard_normal((2, K)).astype(np.float32)
    M = E.radial_mask(p, spatial, dr, mode)
    assert not np.isnan(M).any() and relerr(M, R.expand(p, spatial, dr, mode)) <= TOL
    # the float32 weights themselves, bit for bit: profiles that are 1 on the even / odd bins expand to w0 or w1
    b0, w0, w1 = R.weights(spatial, K, dr, mode)
    pe = np.stack([np.arange(K) % 2 == 0, np.arange(K) % 2 == 1]).astype(np.float32)
    We = E.radial_mask(pe, spatial, dr, mode)
    assert np.array_equal(We[0], np.where(b0 % 2 == 0, w0, w1)) and np.array_equal(We[1], np.where(b0 % 2 == 0, w1, w0))
    if mode == R.NEAREST:                                             # a pure gather: bit for bit
        assert np.array_equal(M, R.expand(p, spatial, dr, mode).astype(np.float32))
    assert np.array_equal(E.radial_mask(p[0], spatial, dr, mode), M[0])
    A = rng.standard_normal((2,) + spatial).astype(np.float32)
    n = len(spatial)
    q = E.radial_bin(A, n, K, dr, mode)
    assert not np.isnan(q).any() and relerr(q, R.bin_(A, n, K, dr, mode)) <= TOL
    assert relerr(E.radial_bin(A, n, K, dr, mode, chunk=100, cpu=3), q) <= TOL_ROUTE
    cnt = E.radial_bin(np.ones(spatial, np.float32), n, K, dr, mode)
    assert relerr(cnt, R.bin_(np.ones(spatial), n, K, dr, mode)) <= 1e-6
    assert abs(float(cnt.astype(np.float64).sum()) - np.prod(spatial)) <= 1e-6 * np.prod(spatial)


@pytest.mark.parametrize("r", [1, 4, 7])
@pytest.mark.parametrize("spatial", [(12, 10, 9), (9, 8, 6)], ids=str)
def test_disk_profile_expands_to_the_oracle_disk(spatial, r):
    from oracle.filters_oracle import disk_mask
    from texbias.radial import RadialFilter
    f = RadialFilter.disk(r, spatial)
    assert np.array_equal(E.radial_mask(f.profile.numpy(), spatial, f.dr, f.mode), disk_mask(spatial, r, 3, False))
