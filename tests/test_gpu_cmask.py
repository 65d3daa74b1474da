"""Complex user-supplied k-space masks (TB_OP_CMASK) on the GPU: every route a mask program can take
(run-time planned pass B, compiled tile plans, the half-unit split spectrum, the band passes, the
direct-DFT fallback), the custom op (autograd through the conjugate flag, opcheck, torch.compile, HIP-graph
capture), the transforms inside a FusedChain, and the C ABI's argument checks.

Reference: y = Re(IFFT(ifftshift(M . fftshift(FFT x)))) in numpy float64 with a complex M, written here.
Bars (DESIGN (c)): max|y - ref| / max|ref| <= 1e-5 against float64, <= 2e-6 between routes.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from _golden import relerr
from oracle import filters_oracle as O
from texbias import kprog as K

pytestmark = pytest.mark.gpu

TOL = 1e-5


def ref_cmask(x, M, n_dims):
    ax = tuple(range(-n_dims, 0))
    k = np.fft.fftshift(np.fft.fftn(np.asarray(x, np.float64), axes=ax), axes=ax)
    return np.fft.ifftn(np.fft.ifftshift(k * np.asarray(M, np.complex128), axes=ax), axes=ax).real


def ref_wrap(x, alpha, n_dims):
    W = np.ones(x.shape[-n_dims:], np.float64)
    for a in range(n_dims):
        sl = [slice(None)] * n_dims
        sl[a] = slice(1, None, 2)
        W[tuple(sl)] *= np.float64(np.float32(alpha))
    return ref_cmask(x, W, n_dims)


@pytest.fixture(scope="module")
def rt(gpu):
    from texbias import runtime
    return runtime


def draw_mask(rng, shape):
    return (rng.uniform(0.0, 1.5, shape) * np.exp(1j * rng.uniform(-np.pi, np.pi, shape))).astype(np.complex64)


def _data(shape, n_dims, per_channel, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape).astype(np.float32)
    msh = ((shape[-n_dims - 1],) if per_channel else ()) + tuple(shape[-n_dims:])
    return x, draw_mask(rng, msh)


# those of test_gpu_mask.py
SHAPES = [
    ((2, 3, 12, 10, 9), 3),      # odd D, run-time planned pass B
    ((1, 2, 9, 8, 6), 3),        # even D: kd = 0 and Nyquist columns
    ((2, 16, 12), 2),            # 2-D, [C, H, D]
    ((1, 1, 20, 48, 35), 3),     # radix-5/7 D, prime radix set
    ((1, 1, 128, 4, 6), 3),      # compiled tile plan H = 128, one tile (ops_bfly)
    ((1, 2, 128, 8, 6), 3),      # compiled tile plan H = 128, paired persistent kernel
    ((1, 2, 37, 8, 6), 3),       # prime 37: the direct-DFT fallback
]


@pytest.mark.parametrize("per_channel", [False, True], ids=["shared", "per_channel"])
@pytest.mark.parametrize("shape,n_dims", SHAPES, ids=[str(s[0]) for s in SHAPES])
def test_cmask_matches_float64(rt, shape, n_dims, per_channel):
    x, M = _data(shape, n_dims, per_channel, 61)
    y = rt.kspace_cmask(torch.from_numpy(x).cuda(), torch.from_numpy(M).cuda(), n_dims)
    assert y.shape == x.shape
    yh = y.cpu().numpy()
    assert relerr(yh, x) > 1e-2
    e = relerr(yh, ref_cmask(x, M, n_dims))
    print(f"vs float64 {e:.3e}")
    assert e <= TOL


def test_half_unit_volume_with_padding(rt):
    """1 x 1 x 240 x 240 x 155, pad 5: the half-unit passes and the split-spectrum pass B."""
    x, M = _data((1, 1, 240, 240, 155), 3, False, 62)
    rt.set_pass_timing(True)
    try:
        y = rt.kspace_cmask(torch.from_numpy(x).cuda(), torch.from_numpy(M).cuda(), 3, pad=5)
        names = rt.pass_stats()[3]
    finally:
        rt.set_pass_timing(False)
    assert names[1] == "k_kspace_half"
    yh = y.cpu().numpy()
    assert yh.shape[-1] == 160 and np.all(yh[..., 155:] == 0.0)
    e = relerr(yh[..., :155], ref_cmask(x, M, 3))
    print(f"vs float64 {e:.3e}")
    assert e <= TOL


def test_cmask_inside_band_program(rt):
    """[disk 9.0, cmask, wrap 0.5]: the band passes agree with the full-spectrum ones and with float64."""
    shape, sp = (2, 4, 48, 40, 36), (48, 40, 36)
    x, M = _data(shape, 3, True, 63)
    xd, Md = torch.from_numpy(x).cuda(), torch.from_numpy(M).cuda()
    prog = [K.disk_op(9.0, False), K.cmask_op(Md.data_ptr(), 4, K.geometry(sp).hwd), K.wrap_op(0.5)]
    rt.set_pass_timing(True)
    try:
        yb = rt.kspace_filter(xd, 3, [prog, prog], 4)
        names = rt.pass_stats()[3]
    finally:
        rt.set_pass_timing(False)
    assert names[0] == "k_band_fwd"
    try:
        rt.set_band_plans(False)
        yf = rt.kspace_filter(xd, 3, [prog, prog], 4)
    finally:
        rt.set_band_plans(True)
    d = (yb - yf).abs().max().item() / yf.abs().max().item()
    disk = O.disk_mask(sp, 9.0, 3, False)
    ref = ref_wrap(ref_cmask(ref_cmask(x, disk, 3), M, 3), 0.5, 3)
    e = relerr(yb.cpu().numpy(), ref)
    print(f"band vs full {d:.3e}, band vs float64 {e:.3e}")
    assert d <= 2e-6
    assert e <= TOL
    nodisk = ref_wrap(ref_cmask(x, M, 3), 0.5, 3)
    assert relerr(ref, nodisk) > 1e-2 and relerr(ref, ref_wrap(ref_cmask(x, disk, 3), 0.5, 3)) > 1e-2


@pytest.mark.parametrize("shape", [(2, 2, 12, 10, 9), (1, 2, 37, 8, 6)], ids=["mixed_radix", "fallback"])
def test_logabs_sums_after_cmask(rt, shape):
    """k_kspace_stats / k_gen_logabs apply the program through apply_ops: the complex factor there too."""
    x, M = _data(shape, 3, True, 69)
    sp = shape[2:]
    Md = torch.from_numpy(M).cuda()
    prog = [K.cmask_op(Md.data_ptr(), shape[1], K.geometry(sp).hwd)]
    got = rt.logabs_sums(torch.from_numpy(x).cuda(), 3, [prog] * shape[0], shape[1]).cpu().numpy()
    ax = (-3, -2, -1)
    Mu = np.fft.ifftshift(M.astype(np.complex128), axes=ax)              # unshifted layout
    Mn = np.roll(np.flip(Mu, axis=ax), 1, axis=ax)                        # M(-f)
    k = np.fft.fftn(x.astype(np.float64), axes=ax) * (0.5 * (Mu + np.conj(Mn)))
    ref = np.log(np.abs(k) + 1e-10).sum(axis=ax).reshape(-1)
    assert np.max(np.abs(got - ref) / np.abs(ref)) <= 1e-5


@pytest.mark.parametrize("per_channel", [False, True], ids=["shared", "per_channel"])
@pytest.mark.parametrize("pad", [0, 3])
def test_autograd_is_the_conjugate_mask(rt, pad, per_channel):
    from texbias import ops  # noqa: F401  (registers torch.ops.texbias.*)
    x, M = _data((2, 3, 12, 10, 9), 3, per_channel, 64)
    xd = torch.from_numpy(x).cuda().requires_grad_(True)
    Md = torch.from_numpy(M).cuda()
    y = torch.ops.texbias.kspace_cmask(xd, Md, 3, 3, pad, False)
    assert y.shape[-1] == 9 + pad
    g = torch.randn(y.shape, device="cuda")
    gx, = torch.autograd.grad(y, xd, g)
    gh = g[..., :9].cpu().numpy()
    e = relerr(gx.cpu().numpy(), ref_cmask(gh, np.conj(M), 3))       # the float64 adjoint
    lhs = (g.double() * y.detach().double()).sum().item()              # <g, A x> (pad columns of A x are 0)
    rhs = (gx.double() * xd.detach().double()).sum().item()            # <A* g, x>
    bound = 1e-5 * g.double().norm().item() * y.detach().double().norm().item()
    print(f"adjoint vs float64 {e:.3e}; defect {abs(lhs - rhs):.3e}, bound {bound:.3e}")
    assert e <= TOL
    assert abs(lhs - rhs) <= bound
    assert relerr(gx.cpu().numpy(), ref_cmask(gh, M, 3)) > 1e-2        # not self-adjoint
    # the adjoint of the adjoint is the op
    g2 = torch.from_numpy(gh).cuda().requires_grad_(True)
    z = torch.ops.texbias.kspace_cmask(g2, Md, 3, 3, 0, True)
    assert torch.equal(z.detach(), gx)
    gz, = torch.autograd.grad(z, g2, xd.detach())
    assert torch.equal(gz, torch.ops.texbias.kspace_cmask(xd.detach(), Md, 3, 3, 0, False))
    with pytest.raises(ValueError):
        torch.ops.texbias.kspace_cmask(xd, Md.clone().requires_grad_(True), 3, 3, pad, False)


def test_opcheck_and_compile_fullgraph(rt):
    from texbias import ops  # noqa: F401
    x, M = _data((2, 3, 12, 10, 9), 3, False, 65)
    xd, Md = torch.from_numpy(x).cuda(), torch.from_numpy(M).cuda()
    torch.library.opcheck(torch.ops.texbias.kspace_cmask.default, (xd, Md, 3, 3, 2, False),
                          test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(torch.ops.texbias.kspace_cmask.default, (xd.clone().requires_grad_(True), Md, 3, 3, 2, True),
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))

    def f(t, m):
        return torch.ops.texbias.kspace_cmask(t, m, 3, 3, 2, False) * 2.0 + 1.0

    ref = f(xd, Md)
    torch._dynamo.reset()
    got = torch.compile(f, fullgraph=True, backend="aot_eager")(xd, Md)
    torch.testing.assert_close(got, ref, rtol=0, atol=0)


def test_graph_capture_reads_the_live_mask(rt):
    """A captured launch keeps reading the mask buffer: new values written between replays apply."""
    from texbias import ops  # noqa: F401
    x, M1 = _data((2, 3, 12, 10, 9), 3, False, 66)
    M2 = draw_mask(np.random.default_rng(67), M1.shape)
    xd, Md = torch.from_numpy(x).cuda(), torch.from_numpy(M1).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):   # warm up: plan and workspace
        torch.ops.texbias.kspace_cmask(xd, Md, 3, 3, 0, False)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y = torch.ops.texbias.kspace_cmask(xd, Md, 3, 3, 0, False)
    g.replay()
    torch.cuda.synchronize()
    assert relerr(y.cpu().numpy(), ref_cmask(x, M1, 3)) <= TOL
    Md.copy_(torch.from_numpy(M2))
    g.replay()
    torch.cuda.synchronize()
    assert relerr(y.cpu().numpy(), ref_cmask(x, M2, 3)) <= TOL
    assert relerr(y.cpu().numpy(), ref_cmask(x, M1, 3)) > 1e-2


def test_transforms_and_fused_chain(rt):
    import filters_and_operators as F
    from texbias.masks import ComplexKSpaceMask, ComplexKSpaceMaskd
    from texbias.pipeline import FusedChain
    shape, sp = (2, 2, 24, 20, 18), (24, 20, 18)
    x, M = _data(shape, 3, True, 68)
    xd = torch.from_numpy(x).cuda()
    disk = F.RandFourierDiskMaskd(keys="image", r=5.5, inside_off=False, prob=1.0)
    chain3 = FusedChain([disk, ComplexKSpaceMaskd("image", M), F.SaltAndPepper(0.05)])
    assert [s[0] for s in chain3.plan(2, sp, channels=2)[0]] == ["k", "sap"]
    z = chain3(xd)                                                 # runs next to the disk and salt-and-pepper
    ref = ref_cmask(ref_cmask(x, O.disk_mask(sp, 5.5, 3, False), 3), M, 3)
    zh = z.cpu().numpy()
    assert zh.shape == x.shape
    kept = np.abs(zh - ref) <= TOL * np.abs(ref).max()             # salt-and-pepper changes about 5 % of the voxels
    assert 0.90 <= kept.mean() < 1.0
    chain = FusedChain([disk, ComplexKSpaceMaskd("image", M)])
    plans = chain.plan(2, sp, channels=2)
    assert [s[0] for s in plans[0]] == ["k"] and [op.kind for op in plans[0][0][1]] == [1, 8]
    y = chain(xd, plans=plans)
    assert relerr(y.cpu().numpy(), ref) <= TOL
    # the array and dictionary transforms on one [C, *spatial] image, CPU in -> CPU out
    t = ComplexKSpaceMask(M)
    y1 = t(torch.from_numpy(x[0]))
    assert y1.device.type == "cpu" and relerr(y1.numpy(), ref_cmask(x[0], M, 3)) <= TOL
    d = ComplexKSpaceMaskd("image", M)({"image": xd[1], "label": 3})
    assert d["label"] == 3 and relerr(d["image"].cpu().numpy(), ref_cmask(x[1], M, 3)) <= TOL


@pytest.mark.parametrize("bad", ["null", "w", "d", "channels"])
def test_c_abi_rejects_bad_cmask_ops(rt, bad):
    """TB_ERR_INVALID_ARG before any launch: the output buffer keeps its contents."""
    from texbias._abi import TB_ERR_INVALID_ARG, programs_array
    from texbias._lib import lib
    B, Cc, H, W, D = 1, 2, 12, 10, 9
    x = torch.randn((B, Cc, H, W, D), device="cuda")
    y = torch.full_like(x, 7.0)
    M = torch.ones((H, W, D), dtype=torch.complex64, device="cuda")
    op = K.cmask_op(M.data_ptr(), 1, (H, W, D))
    if bad == "null":
        op.l = 0
    elif bad == "w":
        op.i[1] = W + 1
    elif bad == "d":
        op.i[2] = D - 1
    else:
        op.i[0] = 3
    plan = rt.plan_for(x.device, H, W, D)
    ws = rt.workspace(x.device, plan.workspace_bytes(B * Cc))
    st = (C.c_int64 * 3)(H * W * D, W * D, D)
    progs = programs_array([[K.wrap_op(0.5), op]])
    stream = torch.cuda.current_stream().cuda_stream
    rc = lib().tb_kspace_filter_f32(plan.handle, x.data_ptr(), st, y.data_ptr(), st, 0, ws.data_ptr(), ws.numel(),
                                    B, Cc, C.addressof(progs), None, stream)
    assert rc == TB_ERR_INVALID_ARG
    out = torch.full((B * Cc,), -1.0, dtype=torch.float64, device="cuda")
    rc = lib().tb_kspace_logabs_sum_f32(plan.handle, x.data_ptr(), st, ws.data_ptr(), ws.numel(), B, Cc,
                                        C.addressof(progs), out.data_ptr(), stream)
    assert rc == TB_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert torch.all(y == 7.0).item() and torch.all(out == -1.0).item()
