"""Learnable complex k-space masks on the GPU: the mask gradient of the TB_OP_CMASK round trip on every
route (run-time planned and compiled forward passes, the per-tile k_kspace_cmaskgrad, the direct-DFT
fallback, two launch groups), the write-once store, the custom ops (autograd, opcheck, torch.compile,
HIP-graph capture), the LearnedComplexKSpaceMask module and the optimizers.

Reference, float64, written here: dM[s(f)] = sum conj(X(f)) G(f) / N, X = FFT(x), G = FFT(g), N = H W D,
summed over the samples and, for a shared mask, the channels (tests/test_emu_cmask_grad.py checks this
formula against torch.autograd of the torch.fft expression).
Bar (DESIGN (c)): max|dM - ref| / max|ref| <= 1e-5; equality where stated.
"""
import numpy as np
import pytest
import torch

from _golden import relerr

pytestmark = pytest.mark.gpu

TOL = 1e-5


def crelerr(a, b) -> float:
    a, b = np.asarray(a, np.complex128), np.asarray(b, np.complex128)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30))


def ref_cmask(x, M, n_dims):
    ax = tuple(range(-n_dims, 0))
    k = np.fft.fftshift(np.fft.fftn(np.asarray(x, np.float64), axes=ax), axes=ax)
    return np.fft.ifftn(np.fft.ifftshift(k * np.asarray(M, np.complex128), axes=ax), axes=ax).real


def ref_cmask_grad(x, g, n_dims, per_channel, channels=None):
    """x, g: [*lead, *spatial]; the leading axes are (samples, channels) with `channels` last."""
    ax = tuple(range(-n_dims, 0))
    sp = x.shape[-n_dims:]
    channels = channels if channels is not None else (x.shape[-n_dims - 1] if x.ndim > n_dims else 1)
    X = np.fft.fftn(np.asarray(x, np.float64), axes=ax)
    G = np.fft.fftn(np.asarray(g, np.float64), axes=ax)
    v = np.fft.fftshift(np.conj(X) * G, axes=ax).reshape((-1, channels) + tuple(sp)) / np.prod(sp)
    return v.sum(axis=0) if per_channel else v.sum(axis=(0, 1))


def mirror_defect(dm, n_dims):
    """Elements that are not the exact conjugate of their mirror dM(-f) over the columns kd whose mirror is
    not a stored coefficient of its own (kd != 0, and kd != D/2 for even D): one value, two stores."""
    ax = tuple(range(-n_dims, 0))
    u = np.fft.ifftshift(dm, axes=ax)
    m = np.roll(np.flip(u, axis=ax), 1, axis=ax)
    D = dm.shape[-1]
    kd = [k for k in range(1, D) if 2 * k != D]
    a, b = u[..., kd], m[..., kd]
    return int(np.count_nonzero((a.real != b.real) | (a.imag != -b.imag)))


@pytest.fixture(scope="module")
def rt(gpu):
    from texbias import ops  # noqa: F401  (registers torch.ops.texbias.*)
    from texbias import runtime
    return runtime


def _data(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)


def _mask(shape, n_dims, per_channel, seed):
    msh = ((shape[-n_dims - 1],) if per_channel else ()) + tuple(shape[-n_dims:])
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.0, 1.5, msh) * np.exp(1j * rng.uniform(-np.pi, np.pi, msh))).astype(np.complex64)


# (shape, transformed axes, channels, expected kernel names of pass slots 0 / 1 or None): test_gpu_mask_grad.py's
SHAPES = [
    ((2, 3, 12, 10, 9), 3, 3, ("k_slab_fwd", "k_kspace_cmaskgrad")),         # odd D, ragged tiles
    ((1, 2, 9, 8, 6), 3, 2, None),                                           # even D, both self-conjugate columns
    ((2, 16, 12), 2, 2, None),                                               # 2-D, [C, H, D]
    ((1, 1, 20, 48, 35), 3, 1, None),                                        # prime radix set
    ((1, 2, 128, 8, 6), 3, 2, None),
    ((1, 2, 37, 8, 6), 3, 2, (None, "k_gen_maskgrad")),                      # direct-DFT fallback
    ((9, 1, 12, 10, 9), 3, 1, None),                                         # two launch groups
    ((1, 1, 6, 128, 128), 3, 1, ("k_slab_fwd_ct16", "k_kspace_cmaskgrad")),  # compiled slab forward
]
CASES = [(s, n, c, names, pc) for (s, n, c, names) in SHAPES for pc in ((False, True) if c > 1 else (False,))]


def _run_checked(rt, x, g, n_dims, channels, per_channel, names):
    """The gradient into a NaN-filled buffer, with every property that needs no second reference."""
    xd, gd = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
    cm = channels if per_channel else 1
    sp = tuple(x.shape[-n_dims:])
    nan = float("nan")
    out = torch.full(sp if cm == 1 else (cm,) + sp, complex(nan, nan), dtype=torch.complex64, device="cuda")
    rt.set_pass_timing(True)
    try:
        dm = rt.kspace_cmask_grad(xd, gd, n_dims, cm, channels=channels, out=out)
        got = rt.pass_stats()[3]
    finally:
        rt.set_pass_timing(False)
    assert dm.data_ptr() == out.data_ptr()
    if names is not None:
        for slot, name in enumerate(names):
            assert name is None or got[slot] == name, got
    d = dm.cpu().numpy()
    assert not np.isnan(d.real).any() and not np.isnan(d.imag).any()   # every element written, both halves
    assert mirror_defect(d, n_dims) == 0                               # f and -f: one value, two stores
    again = rt.kspace_cmask_grad(xd, gd, n_dims, cm, channels=channels)
    assert torch.equal(again, dm)                                      # no atomics: bit-reproducible
    # the real part is the real-mask gradient (another kernel instantiation: the bar between routes)
    real = rt.kspace_mask_grad(xd, gd, n_dims, cm, channels=channels).cpu().numpy()
    assert relerr(d.real, real) <= 2e-6
    return d


@pytest.mark.parametrize("shape,n_dims,channels,names,per_channel", CASES,
                         ids=[f"{s}-{'per_channel' if pc else 'shared'}" for (s, _, _, _, pc) in CASES])
def test_grad_matches_float64_and_is_written_once(rt, shape, n_dims, channels, names, per_channel):
    x, g = _data(shape, 71)
    d = _run_checked(rt, x, g, n_dims, channels, per_channel, names)
    e = crelerr(d, ref_cmask_grad(x, g, n_dims, per_channel, channels))
    print(f"{shape} complex mask gradient vs float64 {e:.3e}")
    assert e <= TOL


@pytest.mark.parametrize("per_channel", [False, True], ids=["shared", "per_channel"])
def test_linearity_identity(rt, per_channel):
    """y is real-linear in M: Re sum conj(dM) . E == sum g . kspace_cmask(x, E) for any complex E."""
    shape = (2, 3, 12, 10, 9)
    x, g = _data(shape, 72)
    E = _mask(shape, 3, per_channel, 73)
    xd, gd, Ed = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda(), torch.from_numpy(E).cuda()
    dm = rt.kspace_cmask_grad(xd, gd, 3, 3 if per_channel else 1)
    yE = rt.kspace_cmask(xd, Ed, 3)
    lhs = (dm.to(torch.complex128).conj() * Ed.to(torch.complex128)).sum().real.item()
    rhs = (gd.double() * yE.double()).sum().item()
    bound = 1e-5 * gd.double().norm().item() * yE.double().norm().item()
    print(f"linearity defect {abs(lhs - rhs):.3e}, bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound


def test_strided_views_are_read_in_place(rt):
    shape = (2, 3, 12, 10, 9)
    x, g = _data(shape, 74)
    xb = torch.full(shape[:-1] + (14,), 7.0, device="cuda")
    gb = torch.full(shape[:-1] + (12,), -3.0, device="cuda")
    xb[..., :9].copy_(torch.from_numpy(x))
    gb[..., :9].copy_(torch.from_numpy(g))
    dm = rt.kspace_cmask_grad(xb[..., :9], gb[..., :9], 3, 3)
    assert torch.equal(dm, rt.kspace_cmask_grad(torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda(), 3, 3))
    assert crelerr(dm.cpu().numpy(), ref_cmask_grad(x, g, 3, True)) <= TOL


@pytest.mark.parametrize("per_channel", [False, True], ids=["shared", "per_channel"])
@pytest.mark.parametrize("pad", [0, 3])
def test_learn_forward_and_autograd(rt, pad, per_channel):
    shape = (2, 3, 12, 10, 9)
    x, _ = _data(shape, 75)
    M = _mask(shape, 3, per_channel, 76)
    xd = torch.from_numpy(x).cuda().requires_grad_(True)
    Md = torch.from_numpy(M).cuda().requires_grad_(True)
    y = torch.ops.texbias.kspace_cmask_learn(xd, Md, 3, 3, pad)
    assert y.shape[-1] == 9 + pad
    assert torch.equal(y, torch.ops.texbias.kspace_cmask(xd.detach(), Md.detach(), 3, 3, pad, False))   # the same pass
    gy = torch.randn(y.shape, device="cuda")
    gx, gm = torch.autograd.grad(y, (xd, Md), gy)
    assert torch.equal(gx, torch.ops.texbias.kspace_cmask(gy[..., :9], Md.detach(), 3, 3, 0, True))
    gh = gy[..., :9].cpu().numpy()
    assert relerr(gx.cpu().numpy(), ref_cmask(gh, np.conj(M), 3)) <= TOL
    assert gm.shape == Md.shape and gm.dtype == torch.complex64
    e = crelerr(gm.cpu().numpy(), ref_cmask_grad(x, gh, 3, per_channel))
    print(f"complex mask gradient through autograd vs float64 {e:.3e}")
    assert e <= TOL
    # only the mask requires grad: no image gradient is computed, the mask gradient is the same
    y2 = torch.ops.texbias.kspace_cmask_learn(xd.detach(), Md, 3, 3, pad)
    gm2, = torch.autograd.grad(y2, Md, gy)
    assert torch.equal(gm2, gm)
    # only the image requires grad
    y3 = torch.ops.texbias.kspace_cmask_learn(xd, Md.detach(), 3, 3, pad)
    gx3, = torch.autograd.grad(y3, xd, gy)
    assert torch.equal(gx3, gx)


def test_only_the_asked_gradients_are_launched(rt):
    """With only the mask requiring grad the backward runs the mask-gradient passes and no inverse pass."""
    shape = (2, 3, 12, 10, 9)
    x, _ = _data(shape, 77)
    xd = torch.from_numpy(x).cuda()
    Md = torch.from_numpy(_mask(shape, 3, False, 78)).cuda().requires_grad_(True)
    y = torch.ops.texbias.kspace_cmask_learn(xd, Md, 3, 3, 0)
    gy = torch.randn_like(y)
    rt.set_pass_timing(True)
    try:
        torch.autograd.grad(y, Md, gy)
        _, cnt, _, names = rt.pass_stats()
    finally:
        rt.set_pass_timing(False)
    assert names[1] == "k_kspace_cmaskgrad" and cnt[0] == 1 and cnt[1] == 1 and cnt[2] == 0


def test_opcheck(rt):
    shape = (2, 3, 12, 10, 9)
    x, g = _data(shape, 79)
    xd, gd = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
    utils = ("test_schema", "test_faketensor", "test_autograd_registration")
    for cm in (1, 3):
        torch.library.opcheck(torch.ops.texbias.kspace_cmask_grad.default, (xd, gd, 3, 3, cm), test_utils=utils)
    for per_channel in (False, True):
        Md = torch.from_numpy(_mask(shape, 3, per_channel, 80)).cuda()
        torch.library.opcheck(torch.ops.texbias.kspace_cmask_learn.default, (xd, Md, 3, 3, 2), test_utils=utils)
        torch.library.opcheck(torch.ops.texbias.kspace_cmask_learn.default,
                              (xd.clone().requires_grad_(True), Md.clone().requires_grad_(True), 3, 3, 2),
                              test_utils=utils)


def test_compile_fullgraph_with_backward(rt):
    shape = (2, 3, 12, 10, 9)
    x, _ = _data(shape, 81)
    M = _mask(shape, 3, True, 82)

    def f(t, m):
        return torch.ops.texbias.kspace_cmask_learn(t, m, 3, 3, 2) * 2.0 + 1.0

    def run(fn):
        xd = torch.from_numpy(x).cuda().requires_grad_(True)
        Md = torch.from_numpy(M).cuda().requires_grad_(True)
        y = fn(xd, Md)
        w = torch.linspace(-1.0, 1.0, y.numel(), device="cuda").reshape(y.shape)
        (y * w).sum().backward()
        return y.detach(), xd.grad, Md.grad

    ref = run(f)
    torch._dynamo.reset()
    got = run(torch.compile(f, fullgraph=True, backend="aot_eager"))
    for a, b in zip(got, ref):
        torch.testing.assert_close(a, b, rtol=0, atol=0)
    w = 2.0 * np.linspace(-1.0, 1.0, ref[0].numel()).reshape(ref[0].shape)[..., :9]
    assert crelerr(ref[2].cpu().numpy(), ref_cmask_grad(x, w, 3, True)) <= TOL


def test_graph_capture_forward_and_backward(rt):
    shape = (2, 3, 12, 10, 9)
    x1, g = _data(shape, 83)
    x2, _ = _data(shape, 84)
    M = _mask(shape, 3, False, 85)
    xd = torch.from_numpy(x1).cuda().requires_grad_(True)
    Md = torch.from_numpy(M).cuda().requires_grad_(True)
    gd = torch.from_numpy(g).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):   # warm up: plan and workspaces
        y = torch.ops.texbias.kspace_cmask_learn(xd, Md, 3, 3, 0)
        torch.autograd.grad(y, (xd, Md), gd)
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        y = torch.ops.texbias.kspace_cmask_learn(xd, Md, 3, 3, 0)
        gx, gm = torch.autograd.grad(y, (xd, Md), gd)
    for x in (x1, x2):
        with torch.no_grad():
            xd.copy_(torch.from_numpy(x))
        gr.replay()
        torch.cuda.synchronize()
        assert relerr(y.detach().cpu().numpy(), ref_cmask(x, M, 3)) <= TOL
        assert relerr(gx.cpu().numpy(), ref_cmask(g, np.conj(M), 3)) <= TOL
        assert crelerr(gm.cpu().numpy(), ref_cmask_grad(x, g, 3, False)) <= TOL
    assert crelerr(gm.cpu().numpy(), ref_cmask_grad(x1, g, 3, False)) > 1e-2


def _phase_ramp(sp, s):
    """exp(-2 pi i f.s / n) in the centred layout: a shift by s voxels (fractions allowed)."""
    ph = np.zeros(sp, np.float64)
    for a, n in enumerate(sp):
        sh = [1] * len(sp)
        sh[a] = n
        ph = ph + ((np.arange(n) - n // 2) * s[a] / n).reshape(sh)
    return np.exp(-2j * np.pi * ph).astype(np.complex64)


def test_module_recovers_a_phase_ramp(rt):
    """A sanity check on signs, conjugates and scaling, not a convergence benchmark: torch.optim.Adam
    (lr 0.05, 40 steps) from ones towards the ramp of a (0.5, -0.3, 0.25)-voxel shift; the same run on
    torch.fft in float32 ends at 0.009 of its start, falling at each of the first ten steps.  A gradient
    with the wrong conjugate makes the loss rise."""
    from texbias.masks import LearnedComplexKSpaceMask
    from texbias.pipeline import FusedChain
    shape = (2, 2, 12, 10, 9)
    x, _ = _data(shape, 70)
    Mt = _phase_ramp(shape[2:], (0.5, -0.3, 0.25))
    xd = torch.from_numpy(x).cuda()
    target = rt.kspace_cmask(xd, torch.from_numpy(Mt).cuda(), 3)
    layer = LearnedComplexKSpaceMask(np.ones(shape[2:], np.complex64)).cuda()
    opt = torch.optim.Adam(layer.parameters(), lr=0.05)
    losses = []
    for _ in range(40):
        opt.zero_grad()
        loss = ((layer(xd) - target) ** 2).sum()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    with torch.no_grad():
        y = layer(xd)
        losses.append(((y - target) ** 2).sum().item())
    print("losses", [f"{v:.4g}" for v in losses])
    assert all(b < a for a, b in zip(losses[:6], losses[1:7]))
    assert losses[-1] < 0.1 * losses[0]
    # the trained mask in a FusedChain for inference: the same fused pass, and it follows later steps
    chain = FusedChain([layer.as_transform()])
    assert torch.equal(chain(xd, plans=chain.plan(2, shape[2:], channels=2)), y)
    with torch.no_grad():
        layer.mask.mul_(0.5j)
        y2 = layer(xd)
    assert torch.equal(chain(xd, plans=chain.plan(2, shape[2:], channels=2)), y2) and not torch.equal(y2, y)


def test_texbias_adam_steps_a_complex_mask_as_torch_does(rt):
    """texbias.optim.Adam hands a complex parameter to torch.optim.Adam's own update (its kernel is float32
    only): one step equals torch's capturable Adam (what texbias.optim.Adam is) bit for bit.  torch's default
    Adam evaluates the same update in another order: each result is the rounding of p - update at |p| < 2,
    where float32 values are 2^-23 apart, so the two differ by at most two such steps plus the difference of
    the updates themselves (size lr, a few float32 roundings: below lr * 1e-5)."""
    from texbias import optim
    from texbias.masks import LearnedComplexKSpaceMask
    shape = (2, 2, 12, 10, 9)
    x, g = _data(shape, 86)
    xd, gd = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
    init = _mask(shape, 3, True, 87)
    lr = 1e-2
    after = []
    for make in (lambda p: optim.Adam(p, lr=lr), lambda p: torch.optim.Adam(p, lr=lr, capturable=True),
                 lambda p: torch.optim.Adam(p, lr=lr)):
        layer = LearnedComplexKSpaceMask(init).cuda()
        opt = make(layer.parameters())
        (layer(xd) * gd).sum().backward()
        opt.step()
        after.append(layer.mask.detach().clone())
    assert not torch.equal(after[0], torch.from_numpy(init).cuda())
    assert torch.equal(after[0], after[1])
    assert after[0].abs().max().item() < 2.0
    torch.testing.assert_close(after[0], after[2], rtol=0, atol=2.0 * 2.0 ** -23 + lr * 1e-5)
