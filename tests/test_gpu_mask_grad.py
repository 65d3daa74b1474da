"""Learnable k-space masks on the GPU: the mask gradient of the TB_OP_MASK round trip on every route
(run-time planned and compiled forward passes, the per-tile k_kspace_maskgrad, the direct-DFT fallback,
two launch groups), the write-once store, the custom ops (autograd, opcheck, torch.compile, HIP-graph
capture), the LearnedKSpaceMask module and the C ABI's argument checks.

Reference, float64, written here: dM[s(f)] = sum Re(X(f) conj(G(f))) / N, X = FFT(x), G = FFT(g),
N = H W D, summed over the samples and, for a shared mask, the channels (tests/test_emu_mask_grad.py
checks this formula against torch.autograd of the torch.fft expression).
Bar (DESIGN (c)): max|dM - ref| / max|ref| <= 1e-5; equality where stated.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from _golden import relerr

pytestmark = pytest.mark.gpu

TOL = 1e-5


def ref_mask(x, M, n_dims):
    ax = tuple(range(-n_dims, 0))
    k = np.fft.fftshift(np.fft.fftn(np.asarray(x, np.float64), axes=ax), axes=ax)
    return np.fft.ifftn(np.fft.ifftshift(k * np.asarray(M, np.float64), axes=ax), axes=ax).real


def ref_mask_grad(x, g, n_dims, per_channel, channels=None):
    """x, g: [*lead, *spatial]; the leading axes are (samples, channels) with `channels` last."""
    ax = tuple(range(-n_dims, 0))
    sp = x.shape[-n_dims:]
    channels = channels if channels is not None else (x.shape[-n_dims - 1] if x.ndim > n_dims else 1)
    X = np.fft.fftn(np.asarray(x, np.float64), axes=ax)
    G = np.fft.fftn(np.asarray(g, np.float64), axes=ax)
    v = np.fft.fftshift((X * np.conj(G)).real, axes=ax).reshape((-1, channels) + tuple(sp)) / np.prod(sp)
    return v.sum(axis=0) if per_channel else v.sum(axis=(0, 1))


def mirror_defect(dm, n_dims):
    """Elements that differ from their mirror dM(-f) (flip and roll by one in the unshifted layout) over
    the columns kd whose mirror is not a stored coefficient of its own (kd != 0, and kd != D/2 for even
    D): there f and -f are the two stores of one value."""
    ax = tuple(range(-n_dims, 0))
    u = np.fft.ifftshift(dm, axes=ax)
    m = np.roll(np.flip(u, axis=ax), 1, axis=ax)
    D = dm.shape[-1]
    kd = [k for k in range(1, D) if 2 * k != D]
    return int(np.count_nonzero(u[..., kd] != m[..., kd]))


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
    return np.random.default_rng(seed).uniform(0.0, 1.5, msh).astype(np.float32)


# (shape, transformed axes, channels, expected kernel names of pass slots 0 / 1 or None)
SHAPES = [
    ((2, 3, 12, 10, 9), 3, 3, ("k_slab_fwd", "k_kspace_maskgrad")),         # odd D, ragged tiles
    ((1, 2, 9, 8, 6), 3, 2, None),                                          # even D, both self-conjugate columns
    ((2, 16, 12), 2, 2, None),                                              # 2-D, [C, H, D]
    ((1, 1, 20, 48, 35), 3, 1, None),                                       # prime radix set
    ((1, 2, 128, 8, 6), 3, 2, None),
    ((1, 2, 37, 8, 6), 3, 2, (None, "k_gen_maskgrad")),                     # direct-DFT fallback
    ((9, 1, 12, 10, 9), 3, 1, None),                                        # two launch groups
    ((1, 1, 6, 128, 128), 3, 1, ("k_slab_fwd_ct16", "k_kspace_maskgrad")),  # compiled slab forward
]
CASES = [(s, n, c, names, pc) for (s, n, c, names) in SHAPES for pc in ((False, True) if c > 1 else (False,))]


def _run_checked(rt, x, g, n_dims, channels, per_channel, names):
    """The gradient into a NaN-filled buffer, with every property that needs no second reference."""
    xd, gd = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
    cm = channels if per_channel else 1
    sp = tuple(x.shape[-n_dims:])
    out = torch.full(sp if cm == 1 else (cm,) + sp, float("nan"), device="cuda")
    rt.set_pass_timing(True)
    try:
        dm = rt.kspace_mask_grad(xd, gd, n_dims, cm, channels=channels, out=out)
        got = rt.pass_stats()[3]
    finally:
        rt.set_pass_timing(False)
    assert dm.data_ptr() == out.data_ptr()
    if names is not None:
        for slot, name in enumerate(names):
            assert name is None or got[slot] == name, got
    d = dm.cpu().numpy()
    assert not np.isnan(d).any()                      # every element written
    assert mirror_defect(d, n_dims) == 0              # f and -f: one value, two stores
    again = rt.kspace_mask_grad(xd, gd, n_dims, cm, channels=channels)
    assert torch.equal(again, dm)                     # no atomics: bit-reproducible
    return d


@pytest.mark.parametrize("shape,n_dims,channels,names,per_channel", CASES,
                         ids=[f"{s}-{'per_channel' if pc else 'shared'}" for (s, _, _, _, pc) in CASES])
def test_grad_matches_float64_and_is_written_once(rt, shape, n_dims, channels, names, per_channel):
    x, g = _data(shape, 31)
    d = _run_checked(rt, x, g, n_dims, channels, per_channel, names)
    e = relerr(d, ref_mask_grad(x, g, n_dims, per_channel, channels))
    print(f"{shape} mask gradient vs float64 {e:.3e}")
    assert e <= TOL


def test_workload_slab(rt):
    """1 x 1 x 240 x 240 x 155, the workload's slab, on the whole-slab forward pass.  The plan has no
    compiled whole-slab kernel for (240, 155) (only half units, which this pass does not use: the split
    spectrum would need a W butterfly), so the forward is the run-time planned k_slab_fwd."""
    x, g = _data((1, 1, 240, 240, 155), 32)
    d = _run_checked(rt, x, g, 3, 1, False, ("k_slab_fwd", "k_kspace_maskgrad"))
    e = relerr(d, ref_mask_grad(x, g, 3, False, 1))
    print(f"240 x 240 x 155 mask gradient vs float64 {e:.3e}")
    assert e <= TOL


@pytest.mark.parametrize("per_channel", [False, True], ids=["shared", "per_channel"])
def test_linearity_identity(rt, per_channel):
    """y is linear in M: sum dM . E == sum g . kspace_mask(x, E) for any E (no reference needed)."""
    shape = (2, 3, 12, 10, 9)
    x, g = _data(shape, 33)
    E = _mask(shape, 3, per_channel, 34) - 0.75
    xd, gd, Ed = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda(), torch.from_numpy(E).cuda()
    dm = rt.kspace_mask_grad(xd, gd, 3, 3 if per_channel else 1)
    yE = rt.kspace_mask(xd, Ed, 3)
    lhs = (dm.double() * Ed.double()).sum().item()
    rhs = (gd.double() * yE.double()).sum().item()
    bound = 1e-5 * gd.double().norm().item() * yE.double().norm().item()
    print(f"linearity defect {abs(lhs - rhs):.3e}, bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound


def test_strided_views_are_read_in_place(rt):
    shape = (2, 3, 12, 10, 9)
    x, g = _data(shape, 35)
    xb = torch.full(shape[:-1] + (14,), 7.0, device="cuda")
    gb = torch.full(shape[:-1] + (12,), -3.0, device="cuda")
    xb[..., :9].copy_(torch.from_numpy(x))
    gb[..., :9].copy_(torch.from_numpy(g))
    dm = rt.kspace_mask_grad(xb[..., :9], gb[..., :9], 3, 3)
    assert torch.equal(dm, rt.kspace_mask_grad(torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda(), 3, 3))
    assert relerr(dm.cpu().numpy(), ref_mask_grad(x, g, 3, True)) <= TOL


@pytest.mark.parametrize("per_channel", [False, True], ids=["shared", "per_channel"])
@pytest.mark.parametrize("pad", [0, 3])
def test_learn_forward_and_autograd(rt, pad, per_channel):
    shape = (2, 3, 12, 10, 9)
    x, _ = _data(shape, 36)
    M = _mask(shape, 3, per_channel, 37)
    xd = torch.from_numpy(x).cuda().requires_grad_(True)
    Md = torch.from_numpy(M).cuda().requires_grad_(True)
    y = torch.ops.texbias.kspace_mask_learn(xd, Md, 3, 3, pad)
    assert y.shape[-1] == 9 + pad
    assert torch.equal(y, torch.ops.texbias.kspace_mask(xd.detach(), Md.detach(), 3, 3, pad))   # the same fused pass
    gy = torch.randn(y.shape, device="cuda")
    gx, gm = torch.autograd.grad(y, (xd, Md), gy)
    assert torch.equal(gx, torch.ops.texbias.kspace_mask(gy[..., :9], Md.detach(), 3, 3, 0))
    ref = ref_mask_grad(x, gy[..., :9].cpu().numpy(), 3, per_channel)
    assert gm.shape == Md.shape
    e = relerr(gm.cpu().numpy(), ref)
    print(f"mask gradient through autograd vs float64 {e:.3e}")
    assert e <= TOL
    # only the mask requires grad: no image gradient is computed, the mask gradient is the same
    y2 = torch.ops.texbias.kspace_mask_learn(xd.detach(), Md, 3, 3, pad)
    gm2, = torch.autograd.grad(y2, Md, gy)
    assert torch.equal(gm2, gm)
    # only the image requires grad
    y3 = torch.ops.texbias.kspace_mask_learn(xd, Md.detach(), 3, 3, pad)
    gx3, = torch.autograd.grad(y3, xd, gy)
    assert torch.equal(gx3, gx)


def test_only_the_asked_gradients_are_launched(rt):
    """With only the mask requiring grad the backward runs the mask-gradient passes and no inverse pass."""
    shape = (2, 3, 12, 10, 9)
    x, _ = _data(shape, 38)
    xd = torch.from_numpy(x).cuda()
    Md = torch.from_numpy(_mask(shape, 3, False, 39)).cuda().requires_grad_(True)
    y = torch.ops.texbias.kspace_mask_learn(xd, Md, 3, 3, 0)
    gy = torch.randn_like(y)
    rt.set_pass_timing(True)
    try:
        torch.autograd.grad(y, Md, gy)
        _, cnt, _, names = rt.pass_stats()
    finally:
        rt.set_pass_timing(False)
    assert names[1] == "k_kspace_maskgrad" and cnt[0] == 1 and cnt[1] == 1 and cnt[2] == 0


def test_opcheck(rt):
    shape = (2, 3, 12, 10, 9)
    x, g = _data(shape, 40)
    xd, gd = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
    utils = ("test_schema", "test_faketensor", "test_autograd_registration")
    for cm in (1, 3):
        torch.library.opcheck(torch.ops.texbias.kspace_mask_grad.default, (xd, gd, 3, 3, cm), test_utils=utils)
    for per_channel in (False, True):
        Md = torch.from_numpy(_mask(shape, 3, per_channel, 41)).cuda()
        torch.library.opcheck(torch.ops.texbias.kspace_mask_learn.default, (xd, Md, 3, 3, 2), test_utils=utils)
        torch.library.opcheck(torch.ops.texbias.kspace_mask_learn.default,
                              (xd.clone().requires_grad_(True), Md.clone().requires_grad_(True), 3, 3, 2),
                              test_utils=utils)


def test_compile_fullgraph_with_backward(rt):
    shape = (2, 3, 12, 10, 9)
    x, _ = _data(shape, 42)
    M = _mask(shape, 3, True, 43)

    def f(t, m):
        return torch.ops.texbias.kspace_mask_learn(t, m, 3, 3, 2) * 2.0 + 1.0

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
    assert relerr(ref[2].cpu().numpy(),
                  ref_mask_grad(x, 2.0 * np.linspace(-1.0, 1.0, ref[0].numel()).reshape(ref[0].shape)[..., :9], 3, True)) <= TOL


def test_graph_capture_forward_and_backward(rt):
    shape = (2, 3, 12, 10, 9)
    x1, g = _data(shape, 44)
    x2, _ = _data(shape, 45)
    M = _mask(shape, 3, False, 46)
    xd = torch.from_numpy(x1).cuda().requires_grad_(True)
    Md = torch.from_numpy(M).cuda().requires_grad_(True)
    gd = torch.from_numpy(g).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):   # warm up: plan and workspaces
        y = torch.ops.texbias.kspace_mask_learn(xd, Md, 3, 3, 0)
        torch.autograd.grad(y, (xd, Md), gd)
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        y = torch.ops.texbias.kspace_mask_learn(xd, Md, 3, 3, 0)
        gx, gm = torch.autograd.grad(y, (xd, Md), gd)
    for x in (x1, x2):
        with torch.no_grad():
            xd.copy_(torch.from_numpy(x))
        gr.replay()
        torch.cuda.synchronize()
        assert relerr(y.detach().cpu().numpy(), ref_mask(x, M, 3)) <= TOL
        assert relerr(gx.cpu().numpy(), ref_mask(g, M, 3)) <= TOL
        assert relerr(gm.cpu().numpy(), ref_mask_grad(x, g, 3, False)) <= TOL
    assert relerr(gm.cpu().numpy(), ref_mask_grad(x1, g, 3, False)) > 1e-2


def test_module_learns_a_target_mask(rt):
    """A sanity check on signs and scaling, not a convergence benchmark: Adam (lr 0.05, 12 steps) from
    ones towards a uniform(0, 1.5) target; the same run on torch.fft in float32 ends at 0.06 of its start,
    falling at every step."""
    from texbias.masks import LearnedKSpaceMask
    from texbias.pipeline import FusedChain
    shape = (2, 2, 12, 10, 9)
    x, _ = _data(shape, 50)
    Mt = _mask(shape, 3, False, 51)
    xd = torch.from_numpy(x).cuda()
    target = rt.kspace_mask(xd, torch.from_numpy(Mt).cuda(), 3)
    layer = LearnedKSpaceMask(np.ones(shape[2:], np.float32)).cuda()
    opt = torch.optim.Adam(layer.parameters(), lr=0.05)
    losses = []
    for _ in range(12):
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
        layer.mask.mul_(0.5)
        y2 = layer(xd)
    assert torch.equal(chain(xd, plans=chain.plan(2, shape[2:], channels=2)), y2) and not torch.equal(y2, y)
    other = LearnedKSpaceMask(np.zeros(shape[2:], np.float32)).cuda()
    other.load_state_dict(layer.state_dict())
    assert torch.equal(other.mask, layer.mask) and torch.equal(other(xd), y2)


@pytest.mark.parametrize("bad", ["cm", "null_dm", "null_g", "b", "c", "short_ws", "null_ws"])
def test_c_abi_argument_checks(rt, bad):
    """The documented codes before any launch: a pre-filled dM keeps its contents."""
    from texbias._abi import TB_ERR_INVALID_ARG, TB_ERR_WORKSPACE, TB_OK
    from texbias._lib import lib
    B, Cc, H, W, D = 1, 2, 12, 10, 9
    x = torch.randn((B, Cc, H, W, D), device="cuda")
    g = torch.randn_like(x)
    dm = torch.full((Cc, H, W, D), 7.0, device="cuda")
    plan = rt.plan_for(x.device, H, W, D)
    need = int(lib().tb_mask_grad_workspace_bytes(plan.handle, B * Cc))
    assert need == 2 * B * Cc * H * W * (D // 2 + 1) * 8        # two half spectra
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    st = (C.c_int64 * 3)(H * W * D, W * D, D)
    stream = torch.cuda.current_stream().cuda_stream
    args = dict(g=g.data_ptr(), dm=dm.data_ptr(), cm=Cc, ws=ws.data_ptr(), n=need, B=B, C=Cc)
    want = TB_ERR_INVALID_ARG
    if bad == "cm":
        args["cm"] = 3
    elif bad == "null_dm":
        args["dm"] = None
    elif bad == "null_g":
        args["g"] = None
    elif bad == "b":
        args["B"] = 0
    elif bad == "c":
        args["C"], args["cm"] = 0, 1
    elif bad == "short_ws":
        args["n"], want = need - 1, TB_ERR_WORKSPACE
    else:
        args["ws"], want = None, TB_ERR_WORKSPACE

    def call(a):
        return lib().tb_kspace_mask_grad_f32(plan.handle, x.data_ptr(), st, a["g"], st, a["dm"], a["cm"], a["ws"],
                                             a["n"], a["B"], a["C"], stream)

    assert call(args) == want
    torch.cuda.synchronize()
    assert torch.all(dm == 7.0).item()
    if bad == "short_ws":   # the exact size is enough
        assert call(dict(args, n=need)) == TB_OK
        torch.cuda.synchronize()
        assert relerr(dm.cpu().numpy(), ref_mask_grad(x.cpu().numpy(), g.cpu().numpy(), 3, True)) <= TOL
