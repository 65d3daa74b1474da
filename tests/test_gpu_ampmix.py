"""Amplitude mixing in k-space on the GPU (tb_kspace_ampmix_f32 / tb_kspace_ampmix_bwd_f32, torch.ops.texbias.amp_mix):
every route (run-time planned and compiled slab passes around k_kspace_ampmix, the direct-DFT fallback, two
launch groups with partners that cross them), the special cases, the analytic gradients, the value range, the
custom ops (opcheck, torch.compile, HIP-graph replay after lam and perm were rewritten) and the C ABI's
argument checks.

Reference: tests/_ampmix_ref.py, float64 (torch.fft and its autograd).  Bar (DESIGN (c)):
max|a - ref| / max|ref| <= 1e-5; route against route 2e-6 of max|out|; equality where stated.

Gradients.  A coefficient with tiny |X| makes gx ill-conditioned in any float32 implementation (the factor
|Y| / |X| multiplies the rounding of G - u c), so the 1e-5 bar is held on inputs that keep the amplitudes away
from 0 while the phases still vary over the whole circle (_ampmix_ref.spiked: randn + 6 sqrt(N) delta).  On
plain randn the bar is max(1e-5, 4 x the error of the float32 torch.fft composition of the reference on the
same inputs against float64), computed here on the CPU; the factor 4 covers a different but equally valid
rounding order.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _ampmix_ref as R
from _golden import relerr

pytestmark = pytest.mark.gpu

TOL = 1e-5

# (image shape [B, C, *spatial], transformed axes, kernels of pass slots 0 / 1 / 2 of the forward; None: not named)
SHAPES = [
    ((2, 3, 12, 10, 9), 3, ("k_slab_fwd", "k_kspace_ampmix", "k_slab_inv")),   # odd D, ragged tile
    ((1, 2, 9, 8, 6), 3, None),                                                # even D: both self-conjugate columns
    ((2, 1, 16, 12), 2, None),                                                 # 2-D
    ((1, 1, 20, 48, 35), 3, None),                                             # radices 5 and 7
    ((1, 2, 128, 8, 6), 3, None),                                              # long H
    ((9, 1, 12, 10, 9), 3, None),                                              # two launch groups
    ((1, 2, 37, 8, 6), 3, ("k_gen_dft", "k_gen_ampmix", "k_gen_dft")),         # direct-DFT fallback
    ((1, 1, 6, 128, 128), 3, ("k_slab_fwd_ct16", "k_kspace_ampmix", "k_slab_inv_ct")),   # compiled slab passes
]
IDS = [str(s[0]) for s in SHAPES]


@pytest.fixture(scope="module")
def rt(gpu):
    from texbias import ops  # noqa: F401  (registers torch.ops.texbias.*)
    from texbias import runtime
    return runtime


def _timed(rt, fn):
    rt.set_pass_timing(True)
    try:
        out = fn()
        _, cnt, _, names = rt.pass_stats()
    finally:
        rt.set_pass_timing(False)
    return out, cnt, names


def _randn(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def _lam(B, seed):
    return np.random.default_rng(seed).uniform(size=B).astype(np.float32)


def _mask(shape, n_dims, kind, seed=0):
    from texbias.amplitude import lowfreq_box
    sp = tuple(shape[len(shape) - n_dims:])
    if kind == "box":
        return lowfreq_box(sp, 0.25).numpy()
    rng = np.random.default_rng(seed)            # uniform random, not symmetric; "random_c": one per channel
    return rng.uniform(size=((shape[1],) + sp) if kind == "random_c" else sp).astype(np.float32)


def _cyclic(B):
    return ((np.arange(B) + 1) % B).astype(np.int32)     # sample B-1 takes sample 0: across the launch groups


def _repeated(B):
    p = ((np.arange(B) - 2) % B).astype(np.int32)        # samples 0 and 1 share the partner B-1
    p[:2] = B - 1
    return p


def _dev(*arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _groups(B):
    return (B + 7) // 8


# ----------------------------------------------------------------- forward
@pytest.mark.parametrize("kind", ["box", "random", "random_c"])
@pytest.mark.parametrize("shape,n_dims,names", SHAPES, ids=IDS)
def test_forward_matches_float64(rt, shape, n_dims, names, kind):
    B, D, pad = shape[0], shape[-1], 3
    x, y = _randn(shape, 90), _randn(shape, 91)
    M, lam, perm = _mask(shape, n_dims, kind, 92), _lam(B, 93), _cyclic(B)
    xd, yd, Md, lamd, permd = _dev(x, y, M, lam, perm)
    out = torch.full(shape[:-1] + (D + pad,), float("nan"), device="cuda")
    o, cnt, got = _timed(rt, lambda: rt.kspace_ampmix(xd, yd, Md, lamd, permd, n_dims, pad=pad, out=out))
    assert o.data_ptr() == out.data_ptr()
    assert cnt[:3] == [2 * _groups(B), _groups(B), _groups(B)]       # x and y forward, per-coefficient, inverse
    if names is not None:
        assert tuple(got[:3]) == names, got
    on = out.cpu().numpy()
    assert not np.isnan(on).any()                                    # every element written
    assert np.all(on[..., D:] == 0.0)                                # the pad columns are exactly zero
    e = relerr(on[..., :D], R.reference_np(x, y, M, lam, perm, n_dims))
    print(f"{shape} {kind} forward vs float64 {e:.3e}")
    assert e <= TOL
    assert torch.equal(rt.kspace_ampmix(xd, yd, Md, lamd, permd, n_dims, pad=pad), out)   # bit-reproducible
    if names is not None and names[0] == "k_slab_fwd_ct16":
        # the compiled slab passes against the run-time planned ones
        rt.set_compiled_plans(False)
        try:
            o2, _, got2 = _timed(rt, lambda: rt.kspace_ampmix(xd, yd, Md, lamd, permd, n_dims, pad=pad))
        finally:
            rt.set_compiled_plans(True)
        assert tuple(got2[:3]) == ("k_slab_fwd", "k_kspace_ampmix", "k_slab_inv"), got2
        d = (o2 - out).abs().max().item() / out.abs().max().item()
        print(f"{shape} compiled against run-time planned slab passes {d:.3e}")
        assert d <= 2e-6


def test_lam_zero_is_the_round_trip(rt):
    shape = (2, 3, 12, 10, 9)
    x, y = _randn(shape, 94), _randn(shape, 95)
    xd, yd, Md, lamd = _dev(x, y, _mask(shape, 3, "random"), np.zeros(2, np.float32))
    out = rt.kspace_ampmix(xd, yd, Md, lamd, None, 3)
    e = relerr(out.cpu().numpy(), x)
    print(f"lam = 0 against x {e:.3e}")
    assert e <= 2e-6


def test_full_swap_has_the_partners_amplitude_and_the_images_phase(rt):
    """lam = 1, M = 1: the exported spectrum of the output has |Y| and the unit phasors of X, per coefficient
    (1e-5 of |Y(f)|; phasors 1e-5 apart).  Per-coefficient bars need amplitudes away from 0 -- the rounding of a
    float32 transform is a fraction of the largest coefficient, not of each one -- so the inputs are the spiked
    ones of the gradient tests."""
    shape = (2, 3, 12, 10, 9)
    x, y = R.spiked(shape, 3, 96, 1), R.spiked(shape, 3, 97, 2)
    xd, yd, Md, lamd = _dev(x, y, np.ones(shape[2:], np.float32), np.ones(2, np.float32))
    K = rt.kspace_export(rt.kspace_ampmix(xd, yd, Md, lamd, None, 3), 3).cpu().numpy().astype(np.complex128)
    ax = (-3, -2, -1)
    X = np.fft.fftshift(np.fft.fftn(x.astype(np.float64), axes=ax), axes=ax)
    Y = np.fft.fftshift(np.fft.fftn(y.astype(np.float64), axes=ax), axes=ax)
    ea = float(np.max(np.abs(np.abs(K) - np.abs(Y)) / np.abs(Y)))
    ep = float(np.max(np.abs(K / np.abs(K) - X / np.abs(X))))
    print(f"full swap: amplitude {ea:.3e}, phasor {ep:.3e}")
    assert ea <= TOL and ep <= TOL


def test_zero_image_takes_phase_zero(rt):
    shape = (2, 3, 12, 10, 9)
    y = _randn(shape, 98)
    M, lam = _mask(shape, 3, "random_c", 99), _lam(2, 100)
    z = np.zeros(shape, np.float32)
    zd, yd, Md, lamd = _dev(z, y, M, lam)
    out = rt.kspace_ampmix(zd, yd, Md, lamd, None, 3).cpu().numpy()
    ref, _ = R.closed_form(z, y, M, lam, None, 3)                   # Re ifftn(m_s |Y|)
    assert np.isfinite(out).all() and relerr(out, ref) <= TOL
    gx, gy = rt.kspace_ampmix_grad(zd, zd, Md, lamd, None, yd, 3)    # |X| = |Y| = 0 everywhere: no NaN
    assert torch.isfinite(gx).all().item() and torch.all(gy == 0).item()


@pytest.mark.parametrize("shape", [(2, 3, 12, 10, 9), (9, 1, 12, 10, 9)], ids=str)
def test_partners_from_x_equal_the_explicit_call_with_one_forward_pass_less(rt, shape):
    B = shape[0]
    x = _randn(shape, 101)
    M, lam, perm = _mask(shape, 3, "random"), _lam(B, 102), _cyclic(B)
    xd, Md, lamd, permd = _dev(x, M, lam, perm)
    ydx = xd[torch.from_numpy(perm).long().cuda()].contiguous()
    a, cnt_a, _ = _timed(rt, lambda: rt.kspace_ampmix(xd, xd, Md, lamd, permd, 3))
    b, cnt_b, _ = _timed(rt, lambda: rt.kspace_ampmix(xd, ydx, Md, lamd, None, 3))
    assert torch.equal(a, b)
    g = _groups(B)
    assert cnt_a[:3] == [g, g, g] and cnt_b[:3] == [2 * g, g, g]
    assert relerr(a.cpu().numpy(), R.reference_np(x, x, M, lam, perm, 3)) <= TOL


def test_strided_inputs_and_clamped_partner(rt):
    shape = (2, 3, 12, 10, 9)
    x, y = _randn(shape, 103), _randn(shape, 104)
    M, lam = _mask(shape, 3, "random"), _lam(2, 105)
    xd, yd, Md, lamd = _dev(x, y, M, lam)
    xb = torch.full(shape[:-1] + (14,), 7.0, device="cuda")
    xb[..., :9].copy_(xd)
    ref = rt.kspace_ampmix(xd, yd, Md, lamd, None, 3)
    assert torch.equal(rt.kspace_ampmix(xb[..., :9], yd, Md, lamd, None, 3), ref)     # read in place
    bad, good = _dev(np.array([7, -3], np.int32), np.array([1, 0], np.int32))
    assert torch.equal(rt.kspace_ampmix(xd, yd, Md, lamd, bad, 3), rt.kspace_ampmix(xd, yd, Md, lamd, good, 3))


# ----------------------------------------------------------------- gradients
def _op_grads(x, y, M, lam, perm, g, n_dims, pad=2, same=False):
    """(out, gx, gy) through torch.ops.texbias.amp_mix and autograd; the upstream gradient is g on the image
    columns and anything on the pad columns."""
    xd, yd, Md, lamd, permd, gd = _dev(x, y, M, lam, perm, g)
    xd.requires_grad_(True)
    yd = xd if same else yd.requires_grad_(True)
    out = torch.ops.texbias.amp_mix(xd, yd, Md, lamd, permd, n_dims, x.shape[1], pad)
    go = torch.full(out.shape, 3.0, device="cuda")
    go[..., : x.shape[-1]] = gd
    if same:
        (gx,) = torch.autograd.grad(out, xd, go)
        return out.detach(), gx, None
    gx, gy = torch.autograd.grad(out, (xd, yd), go)
    return out.detach(), gx, gy


@pytest.mark.parametrize("shape,n_dims,names", SHAPES, ids=IDS)
def test_gradients_match_float64_autograd(rt, shape, n_dims, names):
    B = shape[0]
    x, y, g = R.spiked(shape, n_dims, 106, 1), R.spiked(shape, n_dims, 107, 2), _randn(shape, 108)
    M, lam, perm = _mask(shape, n_dims, "random_c", 109), _lam(B, 110), _cyclic(B)
    (out, gx, gy), cnt, got = _timed(rt, lambda: _op_grads(x, y, M, lam, perm, g, n_dims))
    gen = names is not None and names[1] == "k_gen_ampmix"
    assert got[1] == ("k_gen_ampmix_bwd" if gen else "k_kspace_ampmix_bwd"), got
    assert got[3] == "k_ampmix_gysum" and cnt[3] == _groups(B)
    rout, rgx, rgy = R.reference_grads(x, y, M, lam, g, perm, n_dims)
    eo = relerr(out[..., : shape[-1]].cpu().numpy(), rout)
    ex, ey = relerr(gx.cpu().numpy(), rgx), relerr(gy.cpu().numpy(), rgy)
    print(f"{shape} spiked inputs: out {eo:.3e} gx {ex:.3e} gy {ey:.3e}")
    assert eo <= TOL and ex <= TOL and ey <= TOL


@pytest.mark.parametrize("shape,n_dims,names", SHAPES, ids=IDS)
def test_gradients_on_plain_randn(rt, shape, n_dims, names):
    B = shape[0]
    x, y, g = _randn(shape, 111), _randn(shape, 112), _randn(shape, 113)
    M, lam, perm = _mask(shape, n_dims, "random", 114), _lam(B, 115), _cyclic(B)
    _, gx, gy = _op_grads(x, y, M, lam, perm, g, n_dims)
    _, rgx, rgy = R.reference_grads(x, y, M, lam, g, perm, n_dims)
    _, cgx, cgy = R.composed_f32(x, y, M, lam, g, perm, n_dims)
    bx, by = max(TOL, 4 * relerr(cgx, rgx)), max(TOL, 4 * relerr(cgy, rgy))
    ex, ey = relerr(gx.cpu().numpy(), rgx), relerr(gy.cpu().numpy(), rgy)
    print(f"{shape} randn: gx {ex:.3e} (bar {bx:.3e}, float32 torch.fft {relerr(cgx, rgx):.3e}) "
          f"gy {ey:.3e} (bar {by:.3e}, float32 torch.fft {relerr(cgy, rgy):.3e})")
    assert ex <= bx and ey <= by


@pytest.mark.parametrize("shape", [(2, 3, 12, 10, 9), (9, 1, 12, 10, 9)], ids=str)
def test_repeated_partner_sums_in_a_fixed_order(rt, shape):
    B = shape[0]
    x, y, g = R.spiked(shape, 3, 116, 1), R.spiked(shape, 3, 117, 2), _randn(shape, 118)
    M, lam, perm = _mask(shape, 3, "random"), _lam(B, 119), _repeated(B)
    xd, yd, Md, lamd, permd, gd = _dev(x, y, M, lam, perm, g)
    gx, gy = rt.kspace_ampmix_grad(xd, yd, Md, lamd, permd, gd, 3)
    _, rgx, rgy = R.reference_grads(x, y, M, lam, g, perm, 3)
    assert relerr(gx.cpu().numpy(), rgx) <= TOL and relerr(gy.cpu().numpy(), rgy) <= TOL
    unused = sorted(set(range(B)) - set(perm.tolist()))
    assert unused and torch.all(gy[unused] == 0).item()              # nobody's partner: an exact zero
    gx2, gy2 = rt.kspace_ampmix_grad(xd, yd, Md, lamd, permd, gd, 3)
    assert torch.equal(gx, gx2) and torch.equal(gy, gy2)             # no atomics: bit-reproducible


def test_batch_internal_mix_sums_both_contributions(rt):
    shape = (2, 3, 12, 10, 9)
    x, g = R.spiked(shape, 3, 120, 1), _randn(shape, 121)
    M, lam, perm = _mask(shape, 3, "random"), _lam(2, 122), _cyclic(2)
    _, gx, _ = _op_grads(x, x, M, lam, perm, g, 3, same=True)
    _, rgx, rgy = R.reference_grads(x, x.copy(), M, lam, g, perm, 3)
    assert relerr(gx.cpu().numpy(), rgx + rgy) <= TOL


def test_no_partner_gradient_unless_asked(rt):
    shape = (2, 3, 12, 10, 9)
    x, y, g = R.spiked(shape, 3, 123, 1), R.spiked(shape, 3, 124, 2), _randn(shape, 125)
    M, lam, perm = _mask(shape, 3, "random"), _lam(2, 126), _cyclic(2)
    xd, yd, Md, lamd, permd, gd = _dev(x, y, M, lam, perm, g)
    spec = 2 * 3 * 12 * 10 * (9 // 2 + 1) * 8                         # one set of half spectra
    assert rt.ampmix_workspace_bytes(xd, 3, False, False) == 2 * spec
    assert rt.ampmix_workspace_bytes(xd, 3, True, False) == 3 * spec  # no Gy buffer, no buffer of its sum
    assert rt.ampmix_workspace_bytes(xd, 3, True, True) == 5 * spec
    xd.requires_grad_(True)
    out = torch.ops.texbias.amp_mix(xd, yd, Md, lamd, permd, 3, 3, 0)
    (gx,), cnt, got = _timed(rt, lambda: torch.autograd.grad(out, xd, gd))
    assert cnt == [3, 1, 1, 0] and got[1] == "k_kspace_ampmix_bwd"     # x, y, g forward; Gx inverse only
    both, cnt2, _ = _timed(rt, lambda: rt.kspace_ampmix_grad(xd.detach(), yd, Md, lamd, permd, gd, 3))
    assert cnt2 == [3, 1, 2, 1]
    # the same gx either way, to rounding: the two kernels are separate instantiations of the unit
    assert relerr(gx.cpu().numpy(), both[0].cpu().numpy()) <= 2e-6
    gx3, none = rt.kspace_ampmix_grad(xd.detach(), yd, Md, lamd, permd, gd, 3, need_gy=False)
    assert none is None and torch.equal(gx3, gx)
    with pytest.raises(ValueError, match="no gradient"):
        torch.ops.texbias.amp_mix(xd, yd, Md.clone().requires_grad_(True), lamd, permd, 3, 3, 0)


# ----------------------------------------------------------------- value range
@pytest.mark.parametrize("ex", [-40, 40])
def test_value_range(rt, ex):
    shape = (2, 3, 12, 10, 9)
    s = np.float32(2.0 ** ex)
    x, y, g = R.spiked(shape, 3, 127, 1) * s, R.spiked(shape, 3, 128, 2) * s, _randn(shape, 129)
    M, lam, perm = _mask(shape, 3, "random_c", 130), _lam(2, 131), _cyclic(2)
    out, gx, gy = _op_grads(x, y, M, lam, perm, g, 3, pad=0)
    rout, rgx, rgy = R.reference_grads(x, y, M, lam, g, perm, 3)
    e = (relerr(out.cpu().numpy(), rout), relerr(gx.cpu().numpy(), rgx), relerr(gy.cpu().numpy(), rgy))
    print("scale 2^%d: out %.3e gx %.3e gy %.3e" % ((ex,) + e))
    assert max(e) <= TOL


# ----------------------------------------------------------------- the front end
def test_transforms(rt):
    import texbias
    A = texbias.amplitude
    shape = (4, 2, 12, 10, 9)
    x, y = _randn(shape, 132), _randn(shape, 133)
    xd, yd = _dev(x, y)
    box = A.lowfreq_box(shape[2:], 0.25)
    out = A.AmplitudeMix(0.25, lam=0.7)(xd, yd)
    ref = R.reference_np(x, y, box.numpy(), np.full(4, 0.7, np.float32), None, 3)
    assert relerr(out.cpu().numpy(), ref) <= TOL
    t = A.RandAmplitudeMix(box, lam_range=(0.3, 1.0), prob=0.5)
    t.set_random_state(seed=7)
    out, cnt, _ = _timed(rt, lambda: t(xd))
    assert cnt[:3] == [1, 1, 1]                                       # one launch sequence with y = x
    assert (t.lam == 0).any() and (t.lam != 0).any()
    ref = R.reference_np(x, x, box.numpy(), t.lam, t.perm, 3)
    on = out.cpu().numpy()
    assert relerr(on, ref) <= TOL
    off = np.flatnonzero(t.lam == 0)
    assert relerr(on[off], x[off]) <= 2e-6                            # undrawn: the round trip of the input


# ----------------------------------------------------------------- plumbing
def test_opcheck(rt):
    shape = (2, 3, 12, 10, 9)
    x, y, g = R.spiked(shape, 3, 134, 1), R.spiked(shape, 3, 135, 2), _randn(shape, 136)
    xd, yd, Md, lamd, permd, gd = _dev(x, y, _mask(shape, 3, "random"), _lam(2, 137), _cyclic(2), g)
    utils = ("test_schema", "test_faketensor", "test_autograd_registration")
    op = torch.ops.texbias.amp_mix.default
    torch.library.opcheck(op, (xd, yd, Md, lamd, permd, 3, 3, 2), test_utils=utils)
    torch.library.opcheck(op, (xd.clone().requires_grad_(True), yd.clone().requires_grad_(True), Md, lamd, None, 3, 3),
                          test_utils=utils)
    opg = torch.ops.texbias.amp_mix_grad.default
    torch.library.opcheck(opg, (xd, yd, Md, lamd, permd, gd, 3, 3, True), test_utils=utils)
    torch.library.opcheck(opg, (xd, yd, Md, lamd, None, gd, 3, 3, False), test_utils=utils)


def test_compile_fullgraph_with_backward(rt):
    shape = (2, 3, 12, 10, 9)
    x, y = R.spiked(shape, 3, 138, 1), R.spiked(shape, 3, 139, 2)
    _, _, Md, lamd, permd = _dev(None, None, _mask(shape, 3, "random_c", 140), _lam(2, 141), _cyclic(2))

    def f(a, b):
        return torch.ops.texbias.amp_mix(a, b, Md, lamd, permd, 3, 3, 2) * 2.0 + 1.0

    def run(fn):
        xd, yd = _dev(x, y)
        xd.requires_grad_(True)
        yd.requires_grad_(True)
        o = fn(xd, yd)
        w = torch.linspace(-1.0, 1.0, o.numel(), device="cuda").reshape(o.shape)
        (o * w).sum().backward()
        return o.detach(), xd.grad, yd.grad

    ref = run(f)
    torch._dynamo.reset()
    got = run(torch.compile(f, fullgraph=True, backend="aot_eager"))
    for a, b in zip(got, ref):
        torch.testing.assert_close(a, b, rtol=0, atol=0)


def test_graph_replay_reads_the_rewritten_lam_and_perm(rt):
    shape = (3, 2, 12, 10, 9)
    x = _randn(shape, 142)
    M = _mask(shape, 3, "random", 143)
    lam1, perm1 = _lam(3, 144), np.array([1, 2, 0], np.int32)
    lam2, perm2 = _lam(3, 145), np.array([2, 2, 1], np.int32)
    xd, Md, lamd, permd = _dev(x, M, lam1, perm1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):   # warm up: plan and workspace
        rt.kspace_ampmix(xd, xd, Md, lamd, permd, 3)
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        out = rt.kspace_ampmix(xd, xd, Md, lamd, permd, 3)
    for lam, perm in ((lam1, perm1), (lam2, perm2)):
        lamd.copy_(torch.from_numpy(lam))          # in place: the graph holds the addresses
        permd.copy_(torch.from_numpy(perm))
        gr.replay()
        torch.cuda.synchronize()
        assert relerr(out.cpu().numpy(), R.reference_np(x, x, M, lam, perm, 3)) <= TOL
    assert relerr(out.cpu().numpy(), R.reference_np(x, x, M, lam1, perm1, 3)) > 1e-2


# ----------------------------------------------------------------- C ABI
FWD_BAD = ["null_x", "null_ys", "null_m", "null_lam", "null_out", "b", "c", "cm", "pad", "short_ws", "null_ws"]


@pytest.mark.parametrize("bad", FWD_BAD)
def test_c_abi_forward_argument_checks(rt, bad):
    """The documented codes before any launch: a pre-filled output keeps its contents."""
    from texbias._abi import TB_ERR_INVALID_ARG, TB_ERR_WORKSPACE, TB_OK
    from texbias._lib import lib
    B, Cc, H, W, D = 2, 3, 12, 10, 9
    x, y = _randn((B, Cc, H, W, D), 146), _randn((B, Cc, H, W, D), 147)
    M, lam = _mask((B, Cc, H, W, D), 3, "random"), _lam(B, 148)
    xd, yd, Md, lamd = _dev(x, y, M, lam)
    out = torch.full((B, Cc, H, W, D), 7.0, device="cuda")
    plan = rt.plan_for(xd.device, H, W, D)
    need = int(lib().tb_ampmix_workspace_bytes(plan.handle, B * Cc, 0, 0))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    st = (C.c_int64 * 3)(H * W * D, W * D, D)
    stream = torch.cuda.current_stream().cuda_stream
    a = dict(x=xd.data_ptr(), ys=st, m=Md.data_ptr(), cm=1, lam=lamd.data_ptr(), out=out.data_ptr(), pad=0,
             ws=ws.data_ptr(), n=need, B=B, C=Cc)
    want = TB_ERR_INVALID_ARG
    if bad == "null_x":
        a["x"] = None
    elif bad == "null_ys":
        a["ys"] = None                     # y given without its strides
    elif bad == "null_m":
        a["m"] = None
    elif bad == "null_lam":
        a["lam"] = None
    elif bad == "null_out":
        a["out"] = None
    elif bad == "b":
        a["B"] = 0
    elif bad == "c":
        a["C"] = 0
    elif bad == "cm":
        a["cm"] = 2
    elif bad == "pad":
        a["pad"] = -1
    elif bad == "short_ws":
        a["n"], want = need - 1, TB_ERR_WORKSPACE
    else:
        a["ws"], want = None, TB_ERR_WORKSPACE

    def call(a):
        return lib().tb_kspace_ampmix_f32(plan.handle, a["x"], st, yd.data_ptr(), a["ys"], None, a["m"], a["cm"],
                                          a["lam"], a["out"], st, a["pad"], a["ws"], a["n"], a["B"], a["C"], stream)

    assert call(a) == want
    torch.cuda.synchronize()
    assert torch.all(out == 7.0).item()
    if bad == "short_ws":   # the exact size is enough; y and perm may be null
        assert call(dict(a, n=need)) == TB_OK
        torch.cuda.synchronize()
        assert relerr(out.cpu().numpy(), R.reference_np(x, y, M, lam, None, 3)) <= TOL


@pytest.mark.parametrize("bad", ["null_g", "null_gx", "null_gys", "cm", "short_ws_gy", "null_ws"])
def test_c_abi_backward_argument_checks(rt, bad):
    from texbias._abi import TB_ERR_INVALID_ARG, TB_ERR_WORKSPACE, TB_OK
    from texbias._lib import lib
    B, Cc, H, W, D = 2, 3, 12, 10, 9
    shape = (B, Cc, H, W, D)
    x, y, g = R.spiked(shape, 3, 149, 1), R.spiked(shape, 3, 150, 2), _randn(shape, 151)
    M, lam = _mask(shape, 3, "random"), _lam(B, 152)
    xd, yd, Md, lamd, gd = _dev(x, y, M, lam, g)
    gx = torch.full(shape, 7.0, device="cuda")
    gy = torch.full(shape, 7.0, device="cuda")
    plan = rt.plan_for(xd.device, H, W, D)
    need_gy = int(lib().tb_ampmix_workspace_bytes(plan.handle, B * Cc, 1, 1))
    need_gx = int(lib().tb_ampmix_workspace_bytes(plan.handle, B * Cc, 1, 0))
    assert need_gx < need_gy
    ws = torch.empty(need_gy, dtype=torch.uint8, device="cuda")
    st = (C.c_int64 * 3)(H * W * D, W * D, D)
    stream = torch.cuda.current_stream().cuda_stream
    a = dict(g=gd.data_ptr(), gx=gx.data_ptr(), gys=st, cm=1, ws=ws.data_ptr(), n=need_gy)
    want = TB_ERR_INVALID_ARG
    if bad == "null_g":
        a["g"] = None
    elif bad == "null_gx":
        a["gx"] = None
    elif bad == "null_gys":
        a["gys"] = None                    # gy given without its strides
    elif bad == "cm":
        a["cm"] = 2
    elif bad == "short_ws_gy":
        a["n"], want = need_gx, TB_ERR_WORKSPACE   # enough without gy, short with it
    else:
        a["ws"], want = None, TB_ERR_WORKSPACE

    def call(a, with_gy=True):
        return lib().tb_kspace_ampmix_bwd_f32(plan.handle, xd.data_ptr(), st, yd.data_ptr(), st, None, Md.data_ptr(),
                                              a["cm"], lamd.data_ptr(), a["g"], st, a["gx"], st,
                                              gy.data_ptr() if with_gy else None, a["gys"], a["ws"], a["n"], B, Cc,
                                              stream)

    assert call(a) == want
    torch.cuda.synchronize()
    assert torch.all(gx == 7.0).item() and torch.all(gy == 7.0).item()
    if bad == "short_ws_gy":
        assert call(a, with_gy=False) == TB_OK          # without gy that workspace is enough, and gy stays
        torch.cuda.synchronize()
        _, rgx, _ = R.reference_grads(x, y, M, lam, g, None, 3)
        assert relerr(gx.cpu().numpy(), rgx) <= TOL and torch.all(gy == 7.0).item()
