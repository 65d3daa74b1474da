"""Radial k-space profiles on the GPU: the fused shell reductions (k_radial_grad, k_radial_power, k_radial_sum),
the composed route (the mask gradient into the workspace, then k_radial_bin), the dense pair, the custom ops
(autograd, opcheck, torch.compile, HIP-graph capture), the transforms and the C ABI's argument checks.

Semantics (restated in tests/_radial_ref.py): k_a = s_a - floor(n_a / 2), r2 = sum k_a^2,
u = f32_sqrt((float)r2) * (float)(1 / dr); nearest: bin min((int)u, K-1); linear: 1-t on b0 = (int)u and t on
b0+1, weight 1 on K-1 when b0 >= K-1.  expand M[s] = sum_k w_k(s) p[k]; bin q[k] = sum_s w_k(s) A[s];
power P[k] = sum_f w_k(f) |X(f)|^2 / N; gradient dp[k] = sum_f w_k(f) Re(X(f) conj(G(f))) / N.
Bars (DESIGN (c)): max|out - ref| / max|ref| <= 1e-5 against float64, <= 2e-6 between routes, equality
where stated.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _radial_ref as R
from _golden import relerr
from oracle import filters_oracle as O

pytestmark = pytest.mark.gpu

TOL, TOL_ROUTE = 1e-5, 2e-6
MODES = [R.NEAREST, R.LINEAR]
MODE_IDS = ["nearest", "linear"]


@pytest.fixture(scope="module")
def rt(gpu):
    from texbias import ops  # noqa: F401  (registers torch.ops.texbias.*)
    from texbias import runtime
    return runtime


def _data(shape, seed=31):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)


def ref_mask(x, M, n_dims):
    ax = tuple(range(-n_dims, 0))
    k = np.fft.fftshift(np.fft.fftn(np.asarray(x, np.float64), axes=ax), axes=ax)
    return np.fft.ifftn(np.fft.ifftshift(k * np.asarray(M, np.float64), axes=ax), axes=ax).real


# (shape, transformed axes, K, dr, kernel of pass slot 0 on the fused route or None, direct-DFT fallback)
SHAPES = [
    ((2, 3, 12, 10, 9), 3, 8, 1.0, "k_slab_fwd", False),
    ((1, 2, 9, 8, 6), 3, 3, 2.5, None, False),                 # most of the volume in the clamped bin
    ((1, 2, 16, 12), 2, 11, 1.0, None, False),                 # 2-D
    ((1, 1, 20, 48, 35), 3, 20, 1.5, None, False),             # prime radix set
    ((9, 1, 12, 10, 9), 3, 8, 1.0, None, False),               # two launch groups
    ((1, 2, 37, 8, 6), 3, 8, 1.0, None, True),                 # direct-DFT fallback: always composed
    ((1, 1, 6, 128, 128), 3, 96, 1.0, "k_slab_fwd_ct16", False),   # compiled slab forward
    ((1, 1, 6, 128, 128), 3, 400, 0.25, "k_slab_fwd_ct16", False),  # more bins than threads in a workgroup
]
IDS = ["odd_d", "clamped", "2d", "prime_radix", "two_groups", "fallback", "ct_slab", "many_bins"]


def _timed(rt, fn):
    rt.set_pass_timing(True)
    try:
        out = fn()
        names = rt.pass_stats()[3]
    finally:
        rt.set_pass_timing(False)
    return out, names


def _check_names(names, slot0, generic, fused, kern):
    if generic:
        assert names[1] == "k_gen_maskgrad" and names[2] == "k_radial_bin", names
    elif fused:
        assert names[1] == kern and names[2] == "k_radial_sum", names
        assert slot0 is None or names[0] == slot0, names
    else:
        assert names[1] == "k_kspace_maskgrad" and names[2] == "k_radial_bin", names


def _grad_checked(rt, x, g, n_dims, cp, K, dr, mode, slot0, generic):
    """The profile gradient on both routes into NaN-filled buffers; returns the fused result."""
    xd, gd = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
    out = torch.full((K,) if cp == 1 else (cp, K), float("nan"), device="cuda")
    dp, names = _timed(rt, lambda: rt.radial_grad(xd, gd, n_dims, cp, K, dr, mode, out=out))
    assert dp.data_ptr() == out.data_ptr()
    _check_names(names, slot0, generic, True, "k_radial_grad")
    assert not torch.isnan(dp).any().item()
    assert torch.equal(rt.radial_grad(xd, gd, n_dims, cp, K, dr, mode), dp)      # fixed order: bit-reproducible
    try:
        rt.set_radial_fused(False)
        out2 = torch.full_like(out, float("nan"))
        dc, names = _timed(rt, lambda: rt.radial_grad(xd, gd, n_dims, cp, K, dr, mode, out=out2))
    finally:
        rt.set_radial_fused(True)
    _check_names(names, slot0, generic, False, None)
    assert not torch.isnan(dc).any().item()
    d = relerr(dp.cpu().numpy(), dc.cpu().numpy())
    print(f"fused vs composed {d:.3e}")
    assert d <= TOL_ROUTE
    return dp.cpu().numpy()


def _power_checked(rt, x, n_dims, K, dr, mode, slot0, generic):
    xd = torch.from_numpy(x).cuda()
    out = torch.full(x.shape[:2] + (K,), float("nan"), device="cuda")
    P, names = _timed(rt, lambda: rt.radial_power(xd, n_dims, K, dr, mode, out=out))
    assert P.data_ptr() == out.data_ptr()
    _check_names(names, slot0, generic, True, "k_radial_power")
    assert not torch.isnan(P).any().item()
    assert torch.equal(rt.radial_power(xd, n_dims, K, dr, mode), P)
    try:
        rt.set_radial_fused(False)
        out2 = torch.full_like(out, float("nan"))
        Pc, names = _timed(rt, lambda: rt.radial_power(xd, n_dims, K, dr, mode, out=out2))
    finally:
        rt.set_radial_fused(True)
    _check_names(names, slot0, generic, False, None)
    assert not torch.isnan(Pc).any().item()
    d = relerr(P.cpu().numpy(), Pc.cpu().numpy())
    print(f"fused vs composed {d:.3e}")
    assert d <= TOL_ROUTE
    return P.cpu().numpy()


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape,n_dims,K,dr,slot0,generic", SHAPES, ids=IDS)
def test_gradient_matches_float64_and_the_composed_route(rt, shape, n_dims, K, dr, slot0, generic, mode):
    x, g = _data(shape)
    for per_channel in ((False, True) if shape[1] > 1 else (False,)):
        cp = shape[1] if per_channel else 1
        dp = _grad_checked(rt, x, g, n_dims, cp, K, dr, mode, slot0, generic)
        e = relerr(dp, R.grad(x, g, n_dims, per_channel, K, dr, mode))
        print(f"{shape} profile gradient vs float64 {e:.3e}")
        assert e <= TOL
    # the profile gradient is the binned mask gradient
    xd, gd = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
    dm = rt.kspace_mask_grad(xd, gd, n_dims, 1)
    q = rt.radial_bin(dm, n_dims, K, dr, mode)
    assert relerr(rt.radial_grad(xd, gd, n_dims, 1, K, dr, mode).cpu().numpy(), q.cpu().numpy()) <= TOL_ROUTE


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape,n_dims,K,dr,slot0,generic", SHAPES, ids=IDS)
def test_power_matches_float64_parseval_and_the_composed_route(rt, shape, n_dims, K, dr, slot0, generic, mode):
    x, _ = _data(shape)
    P = _power_checked(rt, x, n_dims, K, dr, mode, slot0, generic)
    e = relerr(P, R.power(x, n_dims, K, dr, mode))
    ep = relerr(P.astype(np.float64).sum(-1), (x.astype(np.float64) ** 2).sum(axis=tuple(range(2, x.ndim))))
    print(f"{shape} power vs float64 {e:.3e}, parseval {ep:.3e}")
    assert e <= TOL and ep <= TOL


def test_workload_slab(rt):
    """1 x 1 x 240 x 240 x 155, the workload's slab, K = 188: the run-time planned k_slab_fwd (as the mask
    gradient's workload test) and the fused reductions at their production tile."""
    shape, K = (1, 1, 240, 240, 155), 188
    x, g = _data(shape, 32)
    dp = _grad_checked(rt, x, g, 3, 1, K, 1.0, R.LINEAR, "k_slab_fwd", False)
    e = relerr(dp, R.grad(x, g, 3, False, K, 1.0, R.LINEAR))
    P = _power_checked(rt, x, 3, K, 1.0, R.NEAREST, "k_slab_fwd", False)
    e2 = relerr(P, R.power(x, 3, K, 1.0, R.NEAREST))
    ep = relerr(P.astype(np.float64).sum(-1), (x.astype(np.float64) ** 2).sum(axis=(2, 3, 4)))
    print(f"240 x 240 x 155 gradient vs float64 {e:.3e}, power {e2:.3e}, parseval {ep:.3e}")
    assert e <= TOL and e2 <= TOL and ep <= TOL


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_strided_views_are_read_in_place(rt, mode):
    shape = (2, 3, 12, 10, 9)
    x, g = _data(shape, 35)
    xb = torch.full(shape[:-1] + (14,), 7.0, device="cuda")
    gb = torch.full(shape[:-1] + (12,), -3.0, device="cuda")
    xb[..., :9].copy_(torch.from_numpy(x))
    gb[..., :9].copy_(torch.from_numpy(g))
    xd, gd = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
    assert torch.equal(rt.radial_grad(xb[..., :9], gb[..., :9], 3, 3, 8, 1.0, mode), rt.radial_grad(xd, gd, 3, 3, 8, 1.0, mode))
    assert torch.equal(rt.radial_power(xb[..., :9], 3, 8, 1.0, mode), rt.radial_power(xd, 3, 8, 1.0, mode))


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("spatial,K,dr", [((12, 10, 9), 8, 1.0), ((9, 8, 6), 3, 2.5), ((16, 12), 11, 1.0),
                                          ((6, 128, 128), 400, 0.25), ((40, 33, 30), 30, 1.0)], ids=str)
def test_dense_pair(rt, spatial, K, dr, mode):
    rng = np.random.default_rng(31)
    n = len(spatial)
    p = rng.standard_normal((2, K)).astype(np.float32)
    A = rng.standard_normal((2,) + spatial).astype(np.float32)
    pd, Ad = torch.from_numpy(p).cuda(), torch.from_numpy(A).cuda()
    M = rt.radial_mask(pd, spatial, dr, mode, out=torch.full((2,) + spatial, float("nan"), device="cuda"))
    Mh = M.cpu().numpy()
    assert not np.isnan(Mh).any() and relerr(Mh, R.expand(p, spatial, dr, mode)) <= TOL
    # the float32 weights themselves, bit for bit: profiles that are 1 on the even / odd bins expand to w0 or w1
    b0, w0, w1 = R.weights(spatial, K, dr, mode)
    pe = np.stack([np.arange(K) % 2 == 0, np.arange(K) % 2 == 1]).astype(np.float32)
    We = rt.radial_mask(torch.from_numpy(pe).cuda(), spatial, dr, mode).cpu().numpy()
    assert np.array_equal(We[0], np.where(b0 % 2 == 0, w0, w1)) and np.array_equal(We[1], np.where(b0 % 2 == 0, w1, w0))
    if mode == R.NEAREST:                                             # a pure gather: bit for bit
        assert np.array_equal(Mh, R.expand(p, spatial, dr, mode).astype(np.float32))
    assert torch.equal(rt.radial_mask(pd[0].contiguous(), spatial, dr, mode), M[0])
    q = rt.radial_bin(Ad, n, K, dr, mode, out=torch.full((2, K), float("nan"), device="cuda"))
    qh = q.cpu().numpy()
    assert not np.isnan(qh).any() and relerr(qh, R.bin_(A, n, K, dr, mode)) <= TOL
    assert torch.equal(rt.radial_bin(Ad, n, K, dr, mode), q)
    # <expand(p), A> = <p, bin(A)>
    lhs = (M.double() * Ad.double()).sum().item()
    rhs = (pd.double() * q.double()).sum().item()
    assert abs(lhs - rhs) <= 1e-5 * M.double().norm().item() * Ad.double().norm().item()
    cnt = rt.radial_bin(torch.ones(spatial, device="cuda"), n, K, dr, mode).cpu().numpy()
    assert relerr(cnt, R.bin_(np.ones(spatial), n, K, dr, mode)) <= 1e-6


# ------------------------------------------------------------------------------------------------ filter
@pytest.mark.parametrize("r", [1, 4, 7])
@pytest.mark.parametrize("spatial", [(12, 10, 9), (9, 8, 6)], ids=str)
def test_disk_profile_is_the_disk(rt, spatial, r):
    from texbias import kprog as K
    from texbias.radial import RadialFilter
    f = RadialFilter.disk(r, spatial)
    M = f.mask_on(spatial, torch.device("cuda", 0))
    assert torch.equal(M, rt.disk_mask_tensor(spatial, r, 3, False, torch.device("cuda", 0)))
    x, _ = _data((2,) + spatial, 33)
    y = f(torch.from_numpy(x).cuda())
    yd = rt.kspace_filter(torch.from_numpy(x).cuda().reshape((1, 2) + spatial), 3, [[K.disk_op(r, False)]], 2)[0]
    assert relerr(y.cpu().numpy(), yd.cpu().numpy()) <= TOL_ROUTE
    assert relerr(y.cpu().numpy(), O.fourier_disk(x, r)) <= TOL


def test_fused_chain_with_a_low_pass_stays_on_the_band_route(rt):
    import filters_and_operators as F
    from texbias.pipeline import FusedChain
    from texbias.radial import RadialFilter, RadialFilterd
    shape, sp = (2, 4, 48, 40, 36), (48, 40, 36)
    x, _ = _data(shape, 23)
    xd = torch.from_numpy(x).cuda()
    p = np.random.default_rng(24).uniform(0.0, 1.5, (4, 20)).astype(np.float32)
    disk = F.RandFourierDiskMaskd(keys="image", r=9.0, inside_off=False, prob=1.0)
    chain = FusedChain([disk, RadialFilterd("image", p, dr=1.5, mode="linear")])
    plans = chain.plan(2, sp, channels=4)
    assert [s[0] for s in plans[0]] == ["k"] and [op.kind for op in plans[0][0][1]] == [1, 7]
    y, names = _timed(rt, lambda: chain(xd, plans=plans))
    assert names[0] == "k_band_fwd", names
    ref = ref_mask(ref_mask(x, O.disk_mask(sp, 9.0, 3, False), 3), R.expand(p, sp, 1.5, R.LINEAR), 3)
    e = relerr(y.cpu().numpy(), ref)
    print(f"low-pass + radial filter vs float64 {e:.3e}")
    assert e <= TOL
    # the array transform on one [C, *spatial] image, CPU in -> CPU out; a shared profile
    t = RadialFilter(p[0], dr=1.5)
    y1 = t(torch.from_numpy(x[0]))
    assert y1.device.type == "cpu" and relerr(y1.numpy(), ref_mask(x[0], R.expand(p[0], sp, 1.5, R.LINEAR), 3)) <= TOL


# ---------------------------------------------------------------------------------------------- autograd
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("per_channel", [False, True], ids=["shared", "per_channel"])
@pytest.mark.parametrize("pad", [0, 3])
def test_filter_forward_and_autograd(rt, pad, per_channel, mode):
    shape, sp, K, dr = (2, 3, 12, 10, 9), (12, 10, 9), 8, 1.0
    x, _ = _data(shape, 36)
    rng = np.random.default_rng(37)
    p = rng.uniform(0.0, 1.5, (3, K) if per_channel else (K,)).astype(np.float32)
    e_dir = rng.standard_normal(p.shape).astype(np.float32)
    xd = torch.from_numpy(x).cuda().requires_grad_(True)
    pd = torch.from_numpy(p).cuda().requires_grad_(True)
    y, M = torch.ops.texbias.radial_filter(xd, pd, 3, 3, dr, mode, pad)
    assert y.shape[-1] == 9 + pad and not M.requires_grad
    assert torch.equal(M, rt.radial_mask(pd.detach(), sp, dr, mode))
    assert torch.equal(y, torch.ops.texbias.kspace_mask(xd.detach(), M, 3, 3, pad))     # the existing TB_OP_MASK routes
    assert relerr(y[..., :9].detach().cpu().numpy(), ref_mask(x, R.expand(p, sp, dr, mode)[None], 3)) <= TOL
    gy = torch.randn(y.shape, device="cuda")
    gx, gp = torch.autograd.grad(y, (xd, pd), gy)
    g = gy[..., :9]
    assert gp.shape == pd.shape
    assert torch.equal(gx, torch.ops.texbias.kspace_mask(g, M, 3, 3, 0))
    assert torch.equal(gp, rt.radial_grad(xd.detach(), g, 3, 3 if per_channel else 1, K, dr, mode))
    assert relerr(gp.cpu().numpy(), R.grad(x, g.cpu().numpy(), 3, per_channel, K, dr, mode)) <= TOL
    # y is linear in p: sum dp . e == sum g . radial_filter(x, e), no finite differences needed
    ye = torch.ops.texbias.radial_filter(xd.detach(), torch.from_numpy(e_dir).cuda(), 3, 3, dr, mode, 0)[0]
    lhs = (gp.double() * torch.from_numpy(e_dir).cuda().double()).sum().item()
    rhs = (g.double() * ye.double()).sum().item()
    bound = 1e-5 * g.double().norm().item() * ye.double().norm().item()
    print(f"linearity defect {abs(lhs - rhs):.3e}, bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound
    # <g, A x> = <A g, x>
    lhs = (g.double() * y[..., :9].detach().double()).sum().item()
    rhs = (gx.double() * xd.detach().double()).sum().item()
    assert abs(lhs - rhs) <= 1e-5 * g.double().norm().item() * y.detach().double().norm().item()
    # one side at a time: the same values
    y2 = torch.ops.texbias.radial_filter(xd.detach(), pd, 3, 3, dr, mode, pad)[0]
    assert torch.equal(torch.autograd.grad(y2, pd, gy)[0], gp)
    y3 = torch.ops.texbias.radial_filter(xd, pd.detach(), 3, 3, dr, mode, pad)[0]
    assert torch.equal(torch.autograd.grad(y3, xd, gy)[0], gx)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_power_autograd(rt, mode):
    shape, sp, K, dr = (2, 3, 12, 10, 9), (12, 10, 9), 8, 1.0
    x, _ = _data(shape, 38)
    gP = np.random.default_rng(39).standard_normal((2, 3, K)).astype(np.float32)
    xd = torch.from_numpy(x).cuda().requires_grad_(True)
    P = torch.ops.texbias.radial_power(xd, 3, K, dr, mode)
    assert torch.equal(P, rt.radial_power(xd.detach(), 3, K, dr, mode))
    gx, = torch.autograd.grad(P, xd, torch.from_numpy(gP).cuda())
    ref = 2.0 * ref_mask(x, R.expand(gP, sp, dr, mode), 3)
    e = relerr(gx.cpu().numpy(), ref)
    print(f"power spectrum image gradient vs float64 {e:.3e}")
    assert e <= TOL
    # a loss on the radial spectrum through the public function
    from texbias.radial import radial_power_spectrum, shell_counts
    xd2 = torch.from_numpy(x).cuda().requires_grad_(True)
    Pm = radial_power_spectrum(xd2, 3, mode=mode, mean=True)
    kb = Pm.shape[-1]
    cnt = shell_counts(sp, kb, 1.0, mode, xd2.device)
    assert kb == 9 and relerr(cnt.cpu().numpy(), R.bin_(np.ones(sp), 3, kb, 1.0, mode)) <= 1e-6
    assert relerr(Pm.detach().cpu().numpy(), R.power(x, 3, kb, 1.0, mode) / R.bin_(np.ones(sp), 3, kb, 1.0, mode)) <= TOL
    Pm.sum().backward()
    assert torch.isfinite(xd2.grad).all().item() and xd2.grad.abs().max().item() > 0


def test_module_gradient_step_and_pruned_launches(rt):
    from texbias.radial import LearnedRadialFilter
    shape, K = (2, 3, 12, 10, 9), 8
    x, g = _data(shape, 40)
    xd, gd = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
    layer = LearnedRadialFilter(np.linspace(1.0, 0.2, K), dr=1.0, mode="linear").cuda()
    opt = torch.optim.Adam(layer.parameters(), lr=0.05)
    before = layer.profile.detach().clone()
    y = layer(xd)
    # only the profile requires grad: the forward passes of x and g, the fused reduction, no inverse pass
    rt.set_pass_timing(True)
    try:
        y.backward(gd)
        _, cnt, _, names = rt.pass_stats()
    finally:
        rt.set_pass_timing(False)
    assert names[1] == "k_radial_grad" and names[2] == "k_radial_sum" and cnt[0] == 1 and cnt[1] == 1 and cnt[2] == 1
    assert torch.equal(layer.profile.grad, rt.radial_grad(xd, gd, 3, 1, K, 1.0, 1))
    opt.step()
    assert not torch.equal(layer.profile.detach(), before)
    # only the image requires grad: the filter's passes alone
    xr = xd.clone().requires_grad_(True)
    layer.profile.requires_grad_(False)
    y = layer(xr)
    rt.set_pass_timing(True)
    try:
        y.backward(gd)
        names = rt.pass_stats()[3]
    finally:
        rt.set_pass_timing(False)
    assert names[1] not in ("k_radial_grad", "k_kspace_maskgrad") and names[2] != "k_radial_sum", names
    layer.profile.requires_grad_(True)
    # texbias.optim.Adam steps it too; the transform follows the parameter
    from texbias.optim import Adam
    from texbias.pipeline import FusedChain
    opt2 = Adam(layer.parameters(), lr=0.05)
    mid = layer.profile.detach().clone()
    opt2.zero_grad()
    layer(xd).backward(gd)
    opt2.step()
    assert not torch.equal(layer.profile.detach(), mid)
    chain = FusedChain([layer.as_transform()])
    with torch.no_grad():
        y = layer(xd)
    assert torch.equal(chain(xd, plans=chain.plan(2, shape[2:], channels=3)), y)
    with torch.no_grad():
        layer.profile.mul_(0.5)
        y2 = layer(xd)
    assert torch.equal(chain(xd, plans=chain.plan(2, shape[2:], channels=3)), y2) and not torch.equal(y2, y)


def test_opcheck(rt):
    shape, K = (2, 3, 12, 10, 9), 8
    x, g = _data(shape, 41)
    xd, gd = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
    utils = ("test_schema", "test_faketensor", "test_autograd_registration")
    rng = np.random.default_rng(42)
    torch.library.opcheck(torch.ops.texbias.radial_power.default, (xd, 3, K, 1.0, 0), test_utils=utils)
    torch.library.opcheck(torch.ops.texbias.radial_power.default, (xd.clone().requires_grad_(True), 3, K, 1.5, 1),
                          test_utils=utils)
    torch.library.opcheck(torch.ops.texbias.radial_bin.default, (xd[0], 3, K, 1.0, 1), test_utils=utils)
    for cp in (1, 3):
        p = torch.from_numpy(rng.uniform(0.0, 1.5, (K,) if cp == 1 else (cp, K)).astype(np.float32)).cuda()
        torch.library.opcheck(torch.ops.texbias.radial_grad.default, (xd, gd, 3, 3, cp, K, 1.0, 1), test_utils=utils)
        torch.library.opcheck(torch.ops.texbias.radial_mask.default, (p, [12, 10, 9], 1.0, 1), test_utils=utils)
        torch.library.opcheck(torch.ops.texbias.radial_filter.default, (xd, p, 3, 3, 1.0, 1, 2), test_utils=utils)
        torch.library.opcheck(torch.ops.texbias.radial_filter.default,
                              (xd.clone().requires_grad_(True), p.clone().requires_grad_(True), 3, 3, 1.0, 0, 2),
                              test_utils=utils)


def test_compile_fullgraph_with_backward(rt):
    from texbias.radial import LearnedRadialFilter
    shape, K = (2, 3, 12, 10, 9), 8
    x, _ = _data(shape, 43)
    init = np.random.default_rng(44).uniform(0.0, 1.5, (3, K)).astype(np.float32)

    def run(compiled):
        layer = LearnedRadialFilter(init, dr=1.0, mode="linear").cuda()
        fn = torch.compile(layer, fullgraph=True, backend="aot_eager") if compiled else layer
        xd = torch.from_numpy(x).cuda().requires_grad_(True)
        y = fn(xd, 2) * 2.0 + 1.0
        w = torch.linspace(-1.0, 1.0, y.numel(), device="cuda").reshape(y.shape)
        (y * w).sum().backward()
        return y.detach(), xd.grad, layer.profile.grad

    ref = run(False)
    torch._dynamo.reset()
    got = run(True)
    for a, b in zip(got, ref):
        torch.testing.assert_close(a, b, rtol=0, atol=0)
    gy = 2.0 * np.linspace(-1.0, 1.0, ref[0].numel()).reshape(ref[0].shape)[..., :9]
    assert relerr(ref[2].cpu().numpy(), R.grad(x, gy, 3, True, K, 1.0, R.LINEAR)) <= TOL


def test_graph_capture_forward_and_backward(rt):
    shape, sp, K = (2, 3, 12, 10, 9), (12, 10, 9), 8
    x1, g = _data(shape, 45)
    x2, _ = _data(shape, 46)
    p = np.random.default_rng(47).uniform(0.0, 1.5, (K,)).astype(np.float32)
    xd = torch.from_numpy(x1).cuda().requires_grad_(True)
    pd = torch.from_numpy(p).cuda().requires_grad_(True)
    gd = torch.from_numpy(g).cuda()

    def step():
        y = torch.ops.texbias.radial_filter(xd, pd, 3, 3, 1.0, 1, 0)[0]
        P = torch.ops.texbias.radial_power(y, 3, K, 1.0, 0)
        gx, gp = torch.autograd.grad(y, (xd, pd), gd)
        return y, P, gx, gp

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):   # warm up: plans and workspaces
        step()
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        outs = step()
    for x in (x1, x2):
        with torch.no_grad():
            xd.copy_(torch.from_numpy(x))
        gr.replay()
        torch.cuda.synchronize()
        eager = step()
        torch.cuda.synchronize()
        for a, b in zip(outs, eager):
            assert torch.equal(a.detach(), b.detach())               # replay is bit-equal to eager
    assert relerr(outs[3].cpu().numpy(), R.grad(x2, g, 3, False, K, 1.0, R.LINEAR)) <= TOL
    assert relerr(outs[3].cpu().numpy(), R.grad(x1, g, 3, False, K, 1.0, R.LINEAR)) > 1e-2


# ------------------------------------------------------------------------------------------------- C ABI
BAD = ["null_out", "null_x", "k0", "k_big", "dr0", "dr_neg", "dr_nan", "dr_inf", "mode", "cp", "b", "short_ws", "null_ws"]


@pytest.mark.parametrize("bad", BAD)
def test_c_abi_argument_checks(rt, bad):
    """The documented codes before any launch: NaN-filled outputs stay NaN."""
    from texbias._abi import TB_ERR_INVALID_ARG, TB_ERR_WORKSPACE, TB_OK
    from texbias._lib import lib
    B, Cc, H, W, D, K = 1, 2, 12, 10, 9, 8
    x = torch.randn((B, Cc, H, W, D), device="cuda")
    g = torch.randn_like(x)
    dp = torch.full((Cc, K), float("nan"), device="cuda")
    P = torch.full((B * Cc, K), float("nan"), device="cuda")
    M = torch.full((Cc, H, W, D), float("nan"), device="cuda")
    q = torch.full((Cc, K), float("nan"), device="cuda")
    prof = torch.ones((Cc, K), device="cuda")
    A = torch.ones((Cc, H, W, D), device="cuda")
    plan = rt.plan_for(x.device, H, W, D)
    need = int(lib().tb_radial_workspace_bytes(plan.handle, B * Cc, K, 1))
    assert need >= 2 * B * Cc * H * W * (D // 2 + 1) * 8
    assert int(lib().tb_radial_workspace_bytes(plan.handle, B * Cc, 0, 1)) == 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    st = (C.c_int64 * 3)(H * W * D, W * D, D)
    stream = torch.cuda.current_stream().cuda_stream
    a = dict(x=x.data_ptr(), out=True, K=K, dr=1.0, mode=1, cp=Cc, B=B, ws=ws.data_ptr(), n=need)
    want = TB_ERR_INVALID_ARG
    if bad == "null_out":
        a["out"] = False
    elif bad == "null_x":
        a["x"] = None
    elif bad == "k0":
        a["K"] = 0
    elif bad == "k_big":
        a["K"] = rt.RADIAL_MAX_BINS + 1
    elif bad == "dr0":
        a["dr"] = 0.0
    elif bad == "dr_neg":
        a["dr"] = -1.0
    elif bad == "dr_nan":
        a["dr"] = float("nan")
    elif bad == "dr_inf":
        a["dr"] = float("inf")
    elif bad == "mode":
        a["mode"] = 2
    elif bad == "cp":
        a["cp"] = 3
    elif bad == "b":
        a["B"] = 0
    elif bad == "short_ws":
        a["n"], want = 64, TB_ERR_WORKSPACE
    else:
        a["ws"], want = None, TB_ERR_WORKSPACE

    def o(t):
        return t.data_ptr() if a["out"] else None

    L = lib()
    rcs = {
        "grad": L.tb_kspace_radial_grad_f32(plan.handle, a["x"], st, g.data_ptr(), st, o(dp), a["cp"], a["K"], a["dr"],
                                            a["mode"], a["ws"], a["n"], a["B"], Cc, stream),
        "power": L.tb_kspace_radial_power_f32(plan.handle, a["x"], st, o(P), a["K"], a["dr"], a["mode"], a["ws"], a["n"],
                                              a["B"], Cc, stream),
        "mask": L.tb_radial_mask_f32(plan.handle, prof.data_ptr() if a["x"] else None, Cc if bad != "cp" else 0, a["K"],
                                     a["dr"], a["mode"], o(M), stream),
        "bin": L.tb_radial_bin_f32(plan.handle, A.data_ptr() if a["x"] else None, Cc if bad != "cp" else 0, a["K"], a["dr"],
                                   a["mode"], o(q), a["ws"], a["n"], stream),
    }
    torch.cuda.synchronize()
    if bad == "cp":
        del rcs["power"]                        # no profile channels there
    if bad == "b":
        del rcs["mask"], rcs["bin"]             # no batch there
    if want == TB_ERR_WORKSPACE:
        del rcs["mask"]                         # no workspace there
    for name, rc in rcs.items():
        assert rc == want, (name, rc)
    outs = {"grad": dp, "power": P, "mask": M, "bin": q}
    for name in rcs:
        assert torch.isnan(outs[name]).all().item(), name
    if bad == "short_ws":                       # the queried size is enough
        assert L.tb_kspace_radial_grad_f32(plan.handle, x.data_ptr(), st, g.data_ptr(), st, dp.data_ptr(), Cc, K, 1.0, 1,
                                           ws.data_ptr(), need, B, Cc, stream) == TB_OK
        torch.cuda.synchronize()
        assert not torch.isnan(dp).any().item()
