"""The centred complex spectrum on the GPU: export (shift_fourier) and import (inv_shift_fourier) on every
route (run-time planned and compiled slab passes, the per-tile k_kspace_export / k_kspace_import, the
direct-DFT fallback, two launch groups), the write-once mirror store, the custom ops (autograd, opcheck,
torch.compile, HIP-graph capture), the drop-in switch and the C ABI's argument checks.

Reference, float64, written here with numpy: K = fftshift(fftn(x)), y = Re(ifftn(ifftshift(K))).
Bar (DESIGN (c)): max|a - ref| / max|ref| <= 1e-5; route against route 2e-6 of max|y|; equality where stated.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from _golden import relerr

pytestmark = pytest.mark.gpu

TOL = 1e-5


def ref_export(x, n_dims):
    ax = tuple(range(-n_dims, 0))
    return np.fft.fftshift(np.fft.fftn(np.asarray(x, np.float64), axes=ax), axes=ax)


def ref_import(k, n_dims):
    ax = tuple(range(-n_dims, 0))
    return np.fft.ifftn(np.fft.ifftshift(np.asarray(k, np.complex128), axes=ax), axes=ax).real


def crelerr(a, b):
    a, b = np.asarray(a, np.complex128), np.asarray(b, np.complex128)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30))


def mirror_defect(k, n_dims):
    """Elements that differ from the conjugate of their mirror K(-f) (flip and roll by one in the unshifted
    layout) over the columns kd whose mirror is not a stored coefficient of its own (kd != 0, and
    kd != D/2 for even D): there f and -f are the two stores of one value."""
    ax = tuple(range(-n_dims, 0))
    u = np.fft.ifftshift(k, axes=ax)
    m = np.conj(np.roll(np.flip(u, axis=ax), 1, axis=ax))
    D = k.shape[-1]
    kd = [i for i in range(1, D) if 2 * i != D]
    return int(np.count_nonzero(u[..., kd] != m[..., kd]))


@pytest.fixture(scope="module")
def rt(gpu):
    from texbias import ops  # noqa: F401  (registers torch.ops.texbias.*)
    from texbias import runtime
    return runtime


def _image(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def _spectrum(shape, seed):
    rng = np.random.default_rng(seed)   # not Hermitian
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


# (shape, transformed axes, export kernels of pass slots 0 / 1, import kernels of pass slots 1 / 2; None: not named)
SHAPES = [
    ((2, 3, 12, 10, 9), 3, ("k_slab_fwd", "k_kspace_export"), ("k_kspace_import", "k_slab_inv")),  # odd D, ragged tile
    ((1, 2, 9, 8, 6), 3, None, None),                                      # even D: both self-conjugate columns
    ((2, 16, 12), 2, None, None),                                          # 2-D, [C, H, D]
    ((1, 1, 20, 48, 35), 3, None, None),                                   # radix set with 5 and 7
    ((1, 2, 128, 8, 6), 3, None, None),                                    # long H
    ((1, 2, 37, 8, 6), 3, (None, "k_gen_export"), ("k_gen_import", None)),  # direct-DFT fallback
    ((9, 1, 12, 10, 9), 3, None, None),                                    # two launch groups
    ((1, 1, 6, 128, 128), 3, ("k_slab_fwd_ct16", "k_kspace_export"), ("k_kspace_import", "k_slab_inv_ct")),
]
IDS = [str(s[0]) for s in SHAPES]


def _timed(rt, fn):
    rt.set_pass_timing(True)
    try:
        out = fn()
        _, cnt, _, names = rt.pass_stats()
    finally:
        rt.set_pass_timing(False)
    return out, cnt, names


def _export_checked(rt, x, n_dims, names):
    """The export into a NaN-filled buffer, with every property that needs no second reference."""
    xd = torch.from_numpy(x).cuda()
    out = torch.full(x.shape, complex(float("nan"), float("nan")), dtype=torch.complex64, device="cuda")
    k, cnt, got = _timed(rt, lambda: rt.kspace_export(xd, n_dims, out=out))
    assert k.data_ptr() == out.data_ptr()
    groups = 2 if (n_dims < x.ndim and int(np.prod(x.shape[:-n_dims])) > 8) else 1
    assert cnt[0] == groups and cnt[1] == groups and cnt[2] == 0
    if names is not None:
        for slot, name in enumerate(names):
            assert name is None or got[slot] == name, got
    kn = k.cpu().numpy()
    assert not np.isnan(kn.real).any() and not np.isnan(kn.imag).any()   # every element written
    assert mirror_defect(kn, n_dims) == 0                                # f and -f: one value, two stores
    assert torch.equal(rt.kspace_export(xd, n_dims), k)                  # no atomics: bit-reproducible
    return kn


@pytest.mark.parametrize("shape,n_dims,enames,inames", SHAPES, ids=IDS)
def test_export_matches_float64_and_is_written_once(rt, shape, n_dims, enames, inames):
    x = _image(shape, 60)
    k = _export_checked(rt, x, n_dims, enames)
    e = crelerr(k, ref_export(x, n_dims))
    print(f"{shape} export vs float64 {e:.3e}")
    assert e <= TOL


@pytest.mark.parametrize("pad", [0, 3], ids=["pad0", "pad3"])
@pytest.mark.parametrize("shape,n_dims,enames,inames", SHAPES, ids=IDS)
def test_import_matches_float64(rt, shape, n_dims, enames, inames, pad):
    kn = _spectrum(shape, 61)
    kd = torch.from_numpy(kn).cuda()
    D = shape[-1]
    # out= a strided view of a longer-pitched buffer: the bytes outside the view stay
    base = torch.full(shape[:-1] + (D + pad + 5,), 7.0, device="cuda")
    view = base[..., : D + pad]
    y, cnt, got = _timed(rt, lambda: rt.kspace_import(kd, n_dims, pad=pad, out=view))
    assert y.data_ptr() == base.data_ptr()
    if inames is not None:
        for slot, name in zip((1, 2), inames):
            assert name is None or got[slot] == name, got
        assert cnt[0] == 0 and cnt[1] == 1
    yn = base.cpu().numpy()
    e = relerr(yn[..., :D], ref_import(kn, n_dims))
    print(f"{shape} pad {pad} import vs float64 {e:.3e}")
    assert e <= TOL
    assert np.all(yn[..., D: D + pad] == 0.0)          # the pad columns are exactly zero
    assert np.all(yn[..., D + pad:] == 7.0)            # outside the view: untouched
    y2 = rt.kspace_import(kd, n_dims, pad=pad)         # a fresh contiguous output: the same values
    assert y2.is_contiguous() and torch.equal(y2, view)


def test_workload_slab(rt):
    """1 x 1 x 240 x 240 x 155, the workload's slab, on the run-time planned whole-slab passes (the plan
    has half units only for (240, 155), which these passes do not use)."""
    shape = (1, 1, 240, 240, 155)
    x = _image(shape, 62)
    k = _export_checked(rt, x, 3, ("k_slab_fwd", "k_kspace_export"))
    ref = ref_export(x, 3)
    e = crelerr(k, ref)
    print(f"240 x 240 x 155 export vs float64 {e:.3e}")
    assert e <= TOL
    kn = _spectrum(shape, 63)
    kd = torch.from_numpy(kn).cuda()
    y, cnt, got = _timed(rt, lambda: rt.kspace_import(kd, 3))
    assert got[1] == "k_kspace_import" and got[2] == "k_slab_inv" and cnt[:3] == [0, 1, 1]
    e = relerr(y.cpu().numpy(), ref_import(kn, 3))
    print(f"240 x 240 x 155 import vs float64 {e:.3e}")
    assert e <= TOL


@pytest.mark.parametrize("shape,n_dims,enames,inames", SHAPES, ids=IDS)
def test_round_trip_and_adjoint_identity(rt, shape, n_dims, enames, inames):
    x = _image(shape, 64)
    kn = _spectrum(shape, 65)
    xd, kd = torch.from_numpy(x).cuda(), torch.from_numpy(kn).cuda()
    kx = rt.kspace_export(xd, n_dims)
    e = relerr(rt.kspace_import(kx, n_dims).cpu().numpy(), x)
    print(f"{shape} round trip {e:.3e}")
    assert e <= TOL
    # Re<export(x), K> = N <x, import(K)>: no reference needed
    n = float(np.prod(shape[-n_dims:]))
    yk = rt.kspace_import(kd, n_dims)
    kx128, k128 = kx.to(torch.complex128), kd.to(torch.complex128)
    lhs = torch.sum(kx128.conj() * k128).real.item()
    rhs = n * torch.sum(xd.double() * yk.double()).item()
    bound = 1e-5 * torch.linalg.vector_norm(kx128).item() * torch.linalg.vector_norm(k128).item()
    print(f"{shape} adjoint defect {abs(lhs - rhs):.3e}, bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound


def test_strided_input_is_read_in_place(rt):
    shape = (2, 3, 12, 10, 9)
    x = _image(shape, 66)
    xb = torch.full(shape[:-1] + (14,), 7.0, device="cuda")
    xb[..., :9].copy_(torch.from_numpy(x))
    k = rt.kspace_export(xb[..., :9], 3)
    assert torch.equal(k, rt.kspace_export(torch.from_numpy(x).cuda(), 3))
    assert crelerr(k.cpu().numpy(), ref_export(x, 3)) <= TOL


def test_import_of_a_lazily_conjugated_or_strided_spectrum(rt):
    shape = (2, 3, 12, 10, 9)
    kn = _spectrum(shape, 84)
    kd = torch.from_numpy(kn).cuda()
    kc = kd.conj()                                       # a view with the conjugate bit: same memory
    assert kc.is_conj() and kc.data_ptr() == kd.data_ptr()
    assert relerr(rt.kspace_import(kc, 3).cpu().numpy(), ref_import(np.conj(kn), 3)) <= TOL
    kb = torch.zeros(shape[:-1] + (14,), dtype=torch.complex64, device="cuda")
    kb[..., :9].copy_(kd)
    assert torch.equal(rt.kspace_import(kb[..., :9], 3), rt.kspace_import(kd, 3))


# ----------------------------------------------------------------- autograd
def _ramp(shape, n_dims, shift, dtype):
    """exp(-2 pi i f . shift) in the centred layout: a sub-voxel shift by `shift` voxels per axis."""
    ph = torch.zeros(shape[-n_dims:], dtype=torch.float64)
    for a, s in enumerate(shift):
        n = shape[-n_dims + a]
        f = torch.fft.fftshift(torch.fft.fftfreq(n, dtype=torch.float64))
        ph = ph + (f * s).reshape([-1 if i == a else 1 for i in range(n_dims)])
    ang = -2.0 * np.pi * ph
    return torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1).to(dtype)


def _cmul(K, ramp):
    """K * ramp with torch.view_as_real arithmetic; ramp: [..., 2] real."""
    kr = torch.view_as_real(K)
    re = kr[..., 0] * ramp[..., 0] - kr[..., 1] * ramp[..., 1]
    im = kr[..., 0] * ramp[..., 1] + kr[..., 1] * ramp[..., 0]
    return torch.view_as_complex(torch.stack([re, im], dim=-1))


def test_autograd_of_a_phase_ramp_shift(rt):
    shape, n_dims, pad = (2, 3, 12, 10, 9), 3, 2
    ax = (-3, -2, -1)
    x = _image(shape, 67)
    kn = _spectrum(shape, 68)
    w = np.random.default_rng(69).standard_normal(shape[:-1] + (shape[-1] + pad,)).astype(np.float32)
    shift = (0.3, -1.25, 0.5)

    # ours
    xd = torch.from_numpy(x).cuda().requires_grad_(True)
    kd = torch.from_numpy(kn).cuda().requires_grad_(True)
    r32 = _ramp(shape, n_dims, shift, torch.float32).cuda()
    wd = torch.from_numpy(w).cuda()
    y = torch.ops.texbias.inv_shift_fourier(_cmul(torch.ops.texbias.shift_fourier(xd, n_dims), r32), n_dims, pad)
    (gx,) = torch.autograd.grad((y * wd).sum(), xd)
    yk = torch.ops.texbias.inv_shift_fourier(_cmul(kd, r32), n_dims, pad)
    (gk,) = torch.autograd.grad((yk * wd).sum(), kd)

    # float64 torch.fft autograd
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    k64 = torch.from_numpy(kn).to(torch.complex128).requires_grad_(True)
    r64 = _ramp(shape, n_dims, shift, torch.float64)
    w64 = torch.from_numpy(w).double()[..., : shape[-1]]

    def inv(k):
        return torch.fft.ifftn(torch.fft.ifftshift(k, dim=ax), dim=ax).real

    y64 = inv(_cmul(torch.fft.fftshift(torch.fft.fftn(x64, dim=ax), dim=ax), r64))
    (gx64,) = torch.autograd.grad((y64 * w64).sum(), x64)
    (gk64,) = torch.autograd.grad((inv(_cmul(k64, r64)) * w64).sum(), k64)

    ey = relerr(y[..., : shape[-1]].detach().cpu().numpy(), y64.detach().numpy())
    ex = relerr(gx.cpu().numpy(), gx64.numpy())
    ek = crelerr(gk.cpu().numpy(), gk64.numpy())
    print(f"phase-ramp shift: y {ey:.3e}, gx {ex:.3e}, gK {ek:.3e}")
    assert torch.all(y[..., shape[-1]:] == 0).item()
    assert ey <= TOL and ex <= TOL and ek <= TOL


def test_backward_formulas_bitwise_and_only_when_asked(rt):
    shape, n_dims = (2, 3, 12, 10, 9), 3
    n = float(np.prod(shape[-3:]))
    xd = torch.from_numpy(_image(shape, 70)).cuda().requires_grad_(True)
    gK = torch.from_numpy(_spectrum(shape, 71)).cuda()
    K = torch.ops.texbias.shift_fourier(xd, n_dims)
    (gx,) = torch.autograd.grad(K, xd, gK)
    assert torch.equal(gx, n * torch.ops.texbias.inv_shift_fourier(gK, n_dims, 0))
    kd = torch.from_numpy(_spectrum(shape, 72)).cuda().requires_grad_(True)
    y = torch.ops.texbias.inv_shift_fourier(kd, n_dims, 3)
    gy = torch.randn_like(y)
    (gk,) = torch.autograd.grad(y, kd, gy)
    assert torch.equal(gk, torch.ops.texbias.shift_fourier(gy[..., :9], n_dims) / n)
    # twice differentiable: the gradient of the gradient runs the ops again
    x2 = torch.from_numpy(_image(shape, 73)).cuda().requires_grad_(True)
    (g1,) = torch.autograd.grad(torch.ops.texbias.shift_fourier(x2, n_dims), x2, gK.clone().requires_grad_(True),
                                create_graph=True)
    assert g1.requires_grad
    # no input requires grad: nothing recorded, nothing launched in a backward
    with torch.no_grad():
        assert not torch.ops.texbias.shift_fourier(xd, n_dims).requires_grad


def test_opcheck(rt):
    shape = (2, 3, 12, 10, 9)
    xd = torch.from_numpy(_image(shape, 74)).cuda()
    kd = torch.from_numpy(_spectrum(shape, 75)).cuda()
    utils = ("test_schema", "test_faketensor", "test_autograd_registration")
    torch.library.opcheck(torch.ops.texbias.shift_fourier.default, (xd, 3), test_utils=utils)
    torch.library.opcheck(torch.ops.texbias.shift_fourier.default, (xd.clone().requires_grad_(True), 3), test_utils=utils)
    torch.library.opcheck(torch.ops.texbias.inv_shift_fourier.default, (kd, 3, 2), test_utils=utils)
    torch.library.opcheck(torch.ops.texbias.inv_shift_fourier.default, (kd.clone().requires_grad_(True), 3, 2),
                          test_utils=utils)


def test_compile_fullgraph_with_backward(rt):
    shape = (2, 3, 12, 10, 9)
    x = _image(shape, 76)
    r32 = _ramp(shape, 3, (0.5, 0.25, -0.75), torch.float32).cuda()

    def f(t):
        return torch.ops.texbias.inv_shift_fourier(_cmul(torch.ops.texbias.shift_fourier(t, 3), r32), 3, 2) * 2.0 + 1.0

    def run(fn):
        xd = torch.from_numpy(x).cuda().requires_grad_(True)
        y = fn(xd)
        w = torch.linspace(-1.0, 1.0, y.numel(), device="cuda").reshape(y.shape)
        (y * w).sum().backward()
        return y.detach(), xd.grad

    ref = run(f)
    torch._dynamo.reset()
    got = run(torch.compile(f, fullgraph=True, backend="aot_eager"))
    for a, b in zip(got, ref):
        torch.testing.assert_close(a, b, rtol=0, atol=0)


def test_graph_capture_export_multiply_import(rt):
    shape = (2, 3, 12, 10, 9)
    x1, x2 = _image(shape, 77), _image(shape, 78)
    m = _spectrum(shape[-3:], 79)
    xd = torch.from_numpy(x1).cuda()
    md = torch.from_numpy(m).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):   # warm up: plan and workspace
        rt.kspace_import(rt.kspace_export(xd, 3) * md, 3)
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        y = rt.kspace_import(rt.kspace_export(xd, 3) * md, 3)
    for x in (x1, x2):
        xd.copy_(torch.from_numpy(x))
        gr.replay()
        torch.cuda.synchronize()
        assert relerr(y.cpu().numpy(), ref_import(ref_export(x, 3) * m.astype(np.complex128), 3)) <= TOL
    assert relerr(y.cpu().numpy(), ref_import(ref_export(x1, 3) * m.astype(np.complex128), 3)) > 1e-2


def test_consistent_with_the_fused_mask_op(rt):
    shape = (2, 3, 12, 10, 9)
    xd = torch.from_numpy(_image(shape, 80)).cuda()
    M = torch.from_numpy(np.random.default_rng(81).uniform(0.0, 1.5, shape[-3:]).astype(np.float32)).cuda()
    fused = rt.kspace_mask(xd, M, 3)
    ours = rt.kspace_import(rt.kspace_export(xd, 3) * M, 3)
    d = (ours - fused).abs().max().item() / fused.abs().max().item()
    print(f"export . M -> import against kspace_mask: {d:.3e}")
    assert d <= 2e-6


def test_dropin_switch(rt):
    import filters_and_operators as fo
    import stylization_layers as sl
    import texbias
    import utils2
    sp = texbias.spectrum
    shape = (2, 3, 12, 10, 9)
    x = _image(shape, 82)
    xd = torch.from_numpy(x).cuda()
    ax = (-3, -2, -1)
    fft_k = torch.fft.fftshift(torch.fft.fftn(xd, dim=ax), dim=ax)
    prev = sp.set_dropin(True)
    try:
        for cls in (fo.Fourier, sl.Fourier, utils2.FourierTransform):
            k, cnt, names = _timed(rt, lambda: cls.shift_fourier(xd, 3))
            assert names[1] == "k_kspace_export" and cnt[:3] == [1, 1, 0]
            assert k.dtype == torch.complex64 and crelerr(k.cpu().numpy(), ref_export(x, 3)) <= TOL
            y, cnt, names = _timed(rt, lambda: cls.inv_shift_fourier(k, 3))
            assert names[1] == "k_kspace_import" and cnt[:3] == [0, 1, 1]
            assert y.dtype == torch.float32 and relerr(y.cpu().numpy(), x) <= TOL
        # other dtypes and the complex inverse stay on torch.fft
        _, cnt, _ = _timed(rt, lambda: fo.Fourier.shift_fourier(xd.double(), 3))
        assert cnt[:3] == [0, 0, 0]
        _, cnt, _ = _timed(rt, lambda: fo.Fourier.inv_shift_fourier_complex(fft_k, 3))
        assert cnt[:3] == [0, 0, 0]
        # off, the default: the torch.fft expressions, no pass of ours
        sp.set_dropin(False)
        k, cnt, _ = _timed(rt, lambda: fo.Fourier.shift_fourier(xd, 3))
        assert cnt[:3] == [0, 0, 0] and torch.equal(k, fft_k)
        y, cnt, _ = _timed(rt, lambda: utils2.FourierTransform.inv_shift_fourier(fft_k, 3))
        assert cnt[:3] == [0, 0, 0]
        assert torch.equal(y, torch.fft.ifftn(torch.fft.ifftshift(fft_k, dim=ax), dim=ax).real)
    finally:
        sp.set_dropin(prev)


# ----------------------------------------------------------------- C ABI
@pytest.mark.parametrize("bad", ["null_x", "null_k", "b", "c", "short_ws", "null_ws"])
def test_c_abi_export_argument_checks(rt, bad):
    """The documented codes before any launch: a pre-filled K keeps its contents."""
    from texbias._abi import TB_ERR_INVALID_ARG, TB_ERR_WORKSPACE, TB_OK
    from texbias._lib import lib
    B, Cc, H, W, D = 1, 2, 12, 10, 9
    x = torch.randn((B, Cc, H, W, D), device="cuda")
    k = torch.full((B, Cc, H, W, D), 7.0 + 0j, dtype=torch.complex64, device="cuda")
    plan = rt.plan_for(x.device, H, W, D)
    need = int(lib().tb_spectrum_workspace_bytes(plan.handle, B * Cc))
    assert need == B * Cc * H * W * (D // 2 + 1) * 8        # one half spectrum
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    st = (C.c_int64 * 3)(H * W * D, W * D, D)
    stream = torch.cuda.current_stream().cuda_stream
    args = dict(x=x.data_ptr(), k=k.data_ptr(), ws=ws.data_ptr(), n=need, B=B, C=Cc)
    want = TB_ERR_INVALID_ARG
    if bad == "null_x":
        args["x"] = None
    elif bad == "null_k":
        args["k"] = None
    elif bad == "b":
        args["B"] = 0
    elif bad == "c":
        args["C"] = 0
    elif bad == "short_ws":
        args["n"], want = need - 1, TB_ERR_WORKSPACE
    else:
        args["ws"], want = None, TB_ERR_WORKSPACE

    def call(a):
        return lib().tb_kspace_export_f32(plan.handle, a["x"], st, a["k"], a["ws"], a["n"], a["B"], a["C"], stream)

    assert call(args) == want
    torch.cuda.synchronize()
    assert torch.all(k == 7.0).item()
    if bad == "short_ws":   # the exact size is enough
        assert call(dict(args, n=need)) == TB_OK
        torch.cuda.synchronize()
        assert crelerr(k.cpu().numpy(), ref_export(x.cpu().numpy(), 3)) <= TOL


@pytest.mark.parametrize("bad", ["null_k", "null_y", "b", "c", "pad", "short_ws", "null_ws"])
def test_c_abi_import_argument_checks(rt, bad):
    """The documented codes before any launch: a pre-filled y keeps its contents."""
    from texbias._abi import TB_ERR_INVALID_ARG, TB_ERR_WORKSPACE, TB_OK
    from texbias._lib import lib
    B, Cc, H, W, D = 1, 2, 12, 10, 9
    kn = _spectrum((B, Cc, H, W, D), 83)
    k = torch.from_numpy(kn).cuda()
    y = torch.full((B, Cc, H, W, D), 7.0, device="cuda")
    plan = rt.plan_for(k.device, H, W, D)
    need = int(lib().tb_spectrum_workspace_bytes(plan.handle, B * Cc))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    st = (C.c_int64 * 3)(H * W * D, W * D, D)
    stream = torch.cuda.current_stream().cuda_stream
    args = dict(k=k.data_ptr(), y=y.data_ptr(), pad=0, ws=ws.data_ptr(), n=need, B=B, C=Cc)
    want = TB_ERR_INVALID_ARG
    if bad == "null_k":
        args["k"] = None
    elif bad == "null_y":
        args["y"] = None
    elif bad == "b":
        args["B"] = 0
    elif bad == "c":
        args["C"] = 0
    elif bad == "pad":
        args["pad"] = -1
    elif bad == "short_ws":
        args["n"], want = need - 1, TB_ERR_WORKSPACE
    else:
        args["ws"], want = None, TB_ERR_WORKSPACE

    def call(a):
        return lib().tb_kspace_import_f32(plan.handle, a["k"], a["y"], st, a["pad"], a["ws"], a["n"], a["B"], a["C"],
                                          stream)

    assert call(args) == want
    torch.cuda.synchronize()
    assert torch.all(y == 7.0).item()
    if bad == "short_ws":   # the exact size is enough
        assert call(dict(args, n=need)) == TB_OK
        torch.cuda.synchronize()
        assert relerr(y.cpu().numpy(), ref_import(kn, 3)) <= TOL
