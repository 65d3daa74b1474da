"""Complex user-supplied k-space masks (TB_OP_CMASK) on the host emulator of the pass kernels.

The emulator runs the device's item functions (fft_core.h apply_ops, kspace_ct.h ops_bfly / b_mid_split)
unchanged, so a numpy complex64 array's address in ``op.l`` exercises the op on every route the CPU can
reach: the run-time-planned pass B, the compiled tile plan (H = 128) and the half-unit split spectrum.
Reference: y = Re(IFFT(ifftshift(M . fftshift(FFT x)))) in numpy float64 with a complex M, written here.
Bars (DESIGN (c)): max|y - ref| / max|ref| <= 1e-5 against float64, <= 2e-6 between routes.
"""
import numpy as np
import pytest
import torch

import _emu
from _golden import relerr
from texbias import kprog as K
from texbias._abi import TB_OP_CMASK

TOL = 1e-5
ROUTES = 2e-6

# (image shape [B, C, *spatial], transformed axes, emulator route ct, tile width T): those of test_emu_mask.py
CASES = [
    ((2, 3, 12, 10, 9), 3, 0, 7),     # odd D, several ragged tiles
    ((1, 2, 9, 8, 6), 3, 0, 0),       # even D: the kd = 0 and Nyquist columns
    ((1, 2, 16, 12), 2, 0, 0),        # 2-D: (H, 1, D)
    ((1, 1, 20, 48, 35), 3, 2, 0),    # half units over the split spectrum (b_mid_split)
    ((1, 1, 128, 4, 6), 3, 1, 0),     # compiled tile plan H = 128 (ops_bfly)
]
IDS = ["odd_d", "even_d", "2d", "half", "ct128"]


def draw_mask(rng, shape):
    """M = uniform(0, 1.5) exp(i uniform(-pi, pi)), complex64."""
    return (rng.uniform(0.0, 1.5, shape) * np.exp(1j * rng.uniform(-np.pi, np.pi, shape))).astype(np.complex64)


def ref_cmask(x, M, n_dims):
    """float64: complex M in the layout of fftshift(fftn(x)); broadcasts over the leading axes."""
    ax = tuple(range(-n_dims, 0))
    k = np.fft.fftshift(np.fft.fftn(np.asarray(x, np.float64), axes=ax), axes=ax)
    return np.fft.ifftn(np.fft.ifftshift(k * np.asarray(M, np.complex128), axes=ax), axes=ax).real


def ref_spike(x, idx, log_intensity, n_dims):
    """float64: |k| := exp(log_intensity) at the shifted index (all channels), phase kept, `.real`."""
    ax = tuple(range(-n_dims, 0))
    k = np.fft.fftshift(np.fft.fftn(np.asarray(x, np.float64), axes=ax), axes=ax)
    sel = (Ellipsis,) + tuple(idx)
    k[sel] = np.exp(np.float64(np.float32(log_intensity))) * np.exp(1j * np.angle(k[sel]))
    return np.fft.ifftn(np.fft.ifftshift(k, axes=ax), axes=ax).real


def ref_wrap(x, alpha, n_dims):
    W = np.ones(x.shape[-n_dims:], np.float64)
    for a in range(n_dims):
        sl = [slice(None)] * n_dims
        sl[a] = slice(1, None, 2)
        W[tuple(sl)] *= np.float64(np.float32(alpha))
    return ref_cmask(x, W, n_dims)


def cmask_prog(M, channels, spatial, chan=-1, conj=False):
    """One CMASK op reading the numpy array M (kept alive by the caller) in place."""
    assert M.dtype == np.complex64 and M.flags.c_contiguous
    return [K.cmask_op(M.ctypes.data, channels, K.geometry(spatial).hwd, chan, conj)]


def emu(x, n_dims, progs, ct, T, pad=0):
    y, _ = _emu.kspace_filter(x, n_dims, progs, pad=pad, T=T, ct=ct)
    return y


def test_op_constant_and_builder_layout():
    assert TB_OP_CMASK == 8
    op = K.cmask_op(0x1000, 3, (12, 10, 9), chan=1)
    assert (op.kind, op.chan, op.l, list(op.i), op.reserved) == (8, 1, 0x1000, [3, 10, 9], 0)
    assert list(op.f) == [0.0] * 4
    op = K.cmask_op(0x2000, 1, (12, 10, 9), conj=True)
    assert (op.kind, op.chan, op.l, list(op.i), op.reserved) == (8, -1, 0x2000, [1, 10, 9], 1)
    with pytest.raises(ValueError):
        K.cmask_op(0, 1, (12, 10, 9))
    with pytest.raises(ValueError):
        K.cmask_op(0x1000, 0, (12, 10, 9))


@pytest.mark.parametrize("shape,n_dims,ct,T", CASES, ids=IDS)
def test_shared_mask(shape, n_dims, ct, T):
    rng = np.random.default_rng(21)
    x = rng.standard_normal(shape).astype(np.float32)
    sp = shape[-n_dims:]
    M = draw_mask(rng, sp)
    y = emu(x, n_dims, [cmask_prog(M, 1, sp)] * shape[0], ct, T)
    assert relerr(y, x) > 1e-2   # the op ran: an unknown kind leaves the input untouched
    e = relerr(y, ref_cmask(x, M, n_dims))
    print(f"emulator vs float64 {e:.3e}")
    assert e <= TOL


@pytest.mark.parametrize("shape,n_dims,ct,T", CASES, ids=IDS)
def test_per_channel_mask(shape, n_dims, ct, T):
    rng = np.random.default_rng(22)
    x = rng.standard_normal(shape).astype(np.float32)
    sp, C = shape[-n_dims:], shape[1]
    M = draw_mask(rng, (C,) + sp)
    y = emu(x, n_dims, [cmask_prog(M, C, sp)] * shape[0], ct, T)
    assert relerr(y, x) > 1e-2
    assert relerr(y, ref_cmask(x, M, n_dims)) <= TOL


@pytest.mark.parametrize("shape,n_dims,ct,T", CASES, ids=IDS)
def test_chan_selected_mask(shape, n_dims, ct, T):
    """An op with chan = c filters channel c only; the other channels pass through."""
    rng = np.random.default_rng(23)
    x = rng.standard_normal(shape).astype(np.float32)
    sp, C = shape[-n_dims:], shape[1]
    c = C - 1
    M = draw_mask(rng, sp)
    y = emu(x, n_dims, [cmask_prog(M, 1, sp, chan=c)] * shape[0], ct, T)
    ref = np.asarray(x, np.float64).copy()
    ref[:, c] = ref_cmask(x[:, c], M, n_dims)
    assert relerr(y[:, c], x[:, c]) > 1e-2
    assert relerr(y, ref) <= TOL
    if C > 1:
        assert relerr(y[:, 0], x[:, 0]) <= ROUTES   # identity round trip of an untouched channel


@pytest.mark.parametrize("shape,n_dims,ct,T", CASES, ids=IDS)
def test_mask_with_padding(shape, n_dims, ct, T):
    rng = np.random.default_rng(24)
    x = rng.standard_normal(shape).astype(np.float32)
    sp = shape[-n_dims:]
    M = draw_mask(rng, sp)
    y = emu(x, n_dims, [cmask_prog(M, 1, sp)] * shape[0], ct, T, pad=5)
    D = sp[-1]
    assert y.shape[-1] == D + 5 and np.all(y[..., D:] == 0.0)
    yd = y[..., :D].reshape(x.shape)     # a squeezed size-1 axis comes back in the padded output's shape
    assert relerr(yd, x) > 1e-2
    assert relerr(yd, ref_cmask(x, M, n_dims)) <= TOL


@pytest.mark.parametrize("shape,n_dims,ct,T", CASES, ids=IDS)
def test_purely_imaginary_constant_gives_zero(shape, n_dims, ct, T):
    """M = i everywhere: (M(f) + conj(M(-f))) / 2 = 0 at every coefficient, so y == 0 exactly."""
    x = np.random.default_rng(25).standard_normal(shape).astype(np.float32)
    sp = shape[-n_dims:]
    M = np.full(sp, 1j, np.complex64)
    y = emu(x, n_dims, [cmask_prog(M, 1, sp)] * shape[0], ct, T)
    assert np.all(y == 0.0)


@pytest.mark.parametrize("shape,n_dims,ct,T", CASES, ids=IDS)
def test_integer_phase_ramp_is_a_roll(shape, n_dims, ct, T):
    """M = exp(-2 pi i f.s / n) with an integer shift s is np.roll(x, s): a check with no FFT reference."""
    x = np.random.default_rng(26).standard_normal(shape).astype(np.float32)
    sp = shape[-n_dims:]
    s = (3, -2, 1)[:n_dims]
    ph = np.zeros(sp, np.float64)
    for a, n in enumerate(sp):
        f = np.arange(n) - n // 2                      # the centred layout's frequency at index i
        sh = [1] * n_dims
        sh[a] = n
        ph = ph + (f * s[a] / n).reshape(sh)
    M = np.exp(-2j * np.pi * ph).astype(np.complex64)
    y = emu(x, n_dims, [cmask_prog(M, 1, sp)] * shape[0], ct, T)
    ref = np.roll(x, s, axis=tuple(range(-n_dims, 0)))
    assert relerr(ref, x) > 1e-2
    # an even axis has a Nyquist frequency, where the .real keeps cos(pi s) = +-1: still the exact roll
    assert relerr(y, ref) <= TOL


@pytest.mark.parametrize("shape,n_dims,ct,T", CASES, ids=IDS)
def test_real_valued_complex_mask_agrees_with_the_real_op(shape, n_dims, ct, T):
    rng = np.random.default_rng(27)
    x = rng.standard_normal(shape).astype(np.float32)
    sp = shape[-n_dims:]
    Mr = rng.uniform(0.0, 1.5, sp).astype(np.float32)
    Mc = Mr.astype(np.complex64)
    yc = emu(x, n_dims, [cmask_prog(Mc, 1, sp)] * shape[0], ct, T)
    yr = emu(x, n_dims, [[K.mask_op(Mr.ctypes.data, 1, K.geometry(sp).hwd)]] * shape[0], ct, T)
    assert relerr(yc, yr) <= ROUTES


@pytest.mark.parametrize("per_channel", [False, True], ids=["shared", "per_channel"])
@pytest.mark.parametrize("shape,n_dims,ct,T", CASES, ids=IDS)
def test_conjugate_flag_is_the_adjoint(shape, n_dims, ct, T, per_channel):
    """<g, A x> = <A* g, x> with A* the op with conj = True, and A* = the float64 reference with conj(M)."""
    rng = np.random.default_rng(28)
    x = rng.standard_normal(shape).astype(np.float32)
    g = rng.standard_normal(shape).astype(np.float32)
    sp, C = shape[-n_dims:], shape[1]
    cm = C if per_channel else 1
    M = draw_mask(rng, ((C,) if per_channel else ()) + sp)
    ax = emu(x, n_dims, [cmask_prog(M, cm, sp)] * shape[0], ct, T)
    ag = emu(g, n_dims, [cmask_prog(M, cm, sp, conj=True)] * shape[0], ct, T)
    assert relerr(ag, ref_cmask(g, np.conj(M), n_dims)) <= TOL
    lhs = np.sum(np.asarray(g, np.float64) * ax)
    rhs = np.sum(np.asarray(ag, np.float64) * x)
    scale = np.linalg.norm(g.astype(np.float64)) * np.linalg.norm(ax.astype(np.float64))
    assert abs(lhs - rhs) <= 1e-5 * scale
    assert relerr(ag, ax) > 1e-2      # M is not real: the adjoint is another operator


@pytest.mark.parametrize("shape,n_dims,ct,T", [CASES[0], CASES[3]], ids=["odd_d", "half"])
def test_cmask_spike_wrap_program(shape, n_dims, ct, T):
    rng = np.random.default_rng(29)
    x = rng.standard_normal(shape).astype(np.float32)
    sp = shape[-3:]
    M = draw_mask(rng, sp)
    idx = (sp[0] // 2 + 2, sp[1] // 2 - 3, sp[2] // 2 + 1)
    prog = cmask_prog(M, 1, sp) + [K.spike_op(idx, K.geometry(sp), 6.0), K.wrap_op(0.5)]
    y = emu(x, 3, [prog] * shape[0], ct, T)
    ref = ref_wrap(ref_spike(ref_cmask(x, M, 3), idx, 6.0, 3), 0.5, 3)
    assert relerr(y, ref) <= TOL


# ------------------------------------------------------------------ host validation (no GPU needed)
def test_cmask_geometry_accepts():
    from texbias import runtime as rt
    x = torch.zeros((2, 3, 6, 5, 4))
    c = torch.complex64
    assert rt.cmask_geometry(x, torch.ones((6, 5, 4), dtype=c), 3) == (1, 3)
    assert rt.cmask_geometry(x, torch.ones((3, 6, 5, 4), dtype=c), 3) == (3, 3)
    assert rt.cmask_geometry(x.reshape(6, 6, 5, 4), torch.ones((3, 6, 5, 4), dtype=c), 3, channels=3) == (3, 3)
    assert rt.cmask_geometry(torch.zeros((2, 1, 6, 1, 4)), torch.ones((6, 1, 4), dtype=c), 3) == (1, 1)
    assert rt.cmask_geometry(x, torch.ones((6, 5, 4), dtype=c, requires_grad=True), 3, learnable=True) == (1, 3)


@pytest.mark.parametrize("bad", ["shape", "channels", "float32", "complex128", "contiguity", "device", "grad",
                                 "numpy"])
def test_cmask_geometry_rejects(bad):
    from texbias import runtime as rt
    x = torch.zeros((2, 3, 6, 5, 4))
    c = torch.complex64
    m = {"shape": torch.ones((6, 5, 5), dtype=c),
         "channels": torch.ones((2, 6, 5, 4), dtype=c),
         "float32": torch.ones((6, 5, 4)),
         "complex128": torch.ones((6, 5, 4), dtype=torch.complex128),
         "contiguity": torch.ones((6, 4, 5), dtype=c).transpose(1, 2),
         "device": torch.ones((6, 5, 4), dtype=c, device="meta"),
         "grad": torch.ones((6, 5, 4), dtype=c, requires_grad=True),
         "numpy": np.ones((6, 5, 4), np.complex64)}[bad]
    with pytest.raises(ValueError):
        rt.cmask_geometry(x, m, 3)
    if bad != "numpy":
        with pytest.raises(ValueError):
            rt.kspace_cmask(x, m, 3)


def test_runtime_paths_need_hip_and_learn_takes_requires_grad():
    from texbias import runtime as rt
    x = torch.zeros((2, 3, 6, 5, 4))
    M = torch.ones((6, 5, 4), dtype=torch.complex64)
    Mg = M.clone().requires_grad_(True)
    with pytest.raises(rt.TexbiasError, match="HIP"):
        rt.kspace_cmask(x, M, 3)
    with pytest.raises(ValueError, match="requires_grad"):
        rt.kspace_cmask(x, Mg, 3)
    with pytest.raises(rt.TexbiasError, match="HIP"):
        rt.kspace_cmask_learn(x, Mg, 3)
    with pytest.raises(ValueError, match="complex64"):
        rt.kspace_cmask_learn(x, torch.ones((6, 5, 4), requires_grad=True), 3)
    with pytest.raises(ValueError, match="does not match"):
        rt.kspace_cmask_grad(x, torch.zeros((2, 3, 6, 5, 5)), 3, 1)
    with pytest.raises(ValueError, match="float32"):
        rt.kspace_cmask_grad(x, x.double(), 3, 1)
    with pytest.raises(ValueError, match="mask channels"):
        rt.kspace_cmask_grad(x, x, 3, 2)
    with pytest.raises(rt.TexbiasError, match="HIP"):
        rt.kspace_cmask_grad(x, x, 3, 3)
    # the real-mask entry points still turn a complex mask away
    with pytest.raises(ValueError, match="float32"):
        rt.kspace_mask(x, M, 3)


def test_ops_are_registered_with_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from texbias import ops  # noqa: F401
    from texbias._lib import TexbiasError
    with FakeTensorMode():
        x = torch.empty((2, 3, 6, 5, 4))
        M = torch.empty((6, 5, 4), dtype=torch.complex64)
        assert torch.ops.texbias.kspace_cmask(x, M, 3, 3, 2, False).shape == (2, 3, 6, 5, 6)
        assert torch.ops.texbias.kspace_cmask(x, M, 3, 3, 0, True).dtype == torch.float32
        assert torch.ops.texbias.kspace_cmask_learn(x, M, 3, 3, 2).shape == (2, 3, 6, 5, 6)
        d = torch.ops.texbias.kspace_cmask_grad(x, x, 3, 3, 1)
        assert d.shape == (6, 5, 4) and d.dtype == torch.complex64
        d = torch.ops.texbias.kspace_cmask_grad(x, x, 3, 3, 3)
        assert d.shape == (3, 6, 5, 4) and d.dtype == torch.complex64
    x = torch.zeros((2, 3, 6, 5, 4))
    with pytest.raises(TexbiasError, match="HIP"):
        torch.ops.texbias.kspace_cmask(x, torch.ones((6, 5, 4), dtype=torch.complex64), 3, 3, 0, False)
    with pytest.raises(TexbiasError, match="HIP"):
        torch.ops.texbias.kspace_cmask_grad(x, x, 3, 3, 1)


def test_transform_program_and_chain_stage():
    from texbias import masks, pipeline
    assert {"ComplexKSpaceMask", "ComplexKSpaceMaskd"} <= pipeline.KSPACE
    assert {"ComplexKSpaceMask", "ComplexKSpaceMaskd", "LearnedComplexKSpaceMask"} <= set(masks.__all__)
    t = masks.ComplexKSpaceMask(np.full((6, 5, 4), 1j, np.complex128))
    assert t.mask.dtype == torch.complex64 and t.mask.is_contiguous()
    with pytest.raises(ValueError):
        t.program((6, 5, 5), 2)
    with pytest.raises(ValueError):
        masks.ComplexKSpaceMask(torch.ones((6, 5, 4), dtype=torch.complex64, requires_grad=True))
    d = masks.ComplexKSpaceMaskd(["image"], np.ones((6, 5, 4), np.complex64))
    assert isinstance(d.transform, masks.ComplexKSpaceMask)
    pipeline.FusedChain([d, t])                                  # both names are fusable
    with pytest.raises(ValueError):                                # the real classes keep rejecting complex arrays
        masks.KSpaceMask(np.ones((6, 5, 4), np.complex64))


def test_learned_module_validation_and_state():
    from texbias.masks import ComplexKSpaceMask, LearnedComplexKSpaceMask
    from texbias._lib import TexbiasError
    with pytest.raises(ValueError, match="neither spatial"):
        LearnedComplexKSpaceMask(np.ones((5, 4), np.complex64), n_dims=3)
    rng = np.random.default_rng(30)
    init = draw_mask(rng, (3, 6, 5, 4)).astype(np.complex128)      # complex128 in, complex64 parameter
    layer = LearnedComplexKSpaceMask(init)
    assert [n for n, _ in layer.named_parameters()] == ["mask"]
    assert layer.mask.dtype == torch.complex64 and layer.mask.is_contiguous() and layer.mask.requires_grad
    assert np.array_equal(layer.mask.detach().numpy(), init.astype(np.complex64))
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
    t = layer.as_transform()
    assert isinstance(t, ComplexKSpaceMask) and not t.mask.requires_grad
    with torch.no_grad():
        layer.mask.mul_(1j)
    assert t.mask.data_ptr() == layer.mask.data_ptr() and torch.equal(t.mask, layer.mask.detach())
    other = LearnedComplexKSpaceMask(np.zeros((3, 6, 5, 4)))
    other.load_state_dict(layer.state_dict())
    assert torch.equal(other.mask, layer.mask)


def test_texbias_adam_sends_a_complex_parameter_to_torch():
    """optim.Adam's native kernel is float32 only: a complex parameter is not eligible, so its group takes
    torch.optim.Adam's own step."""
    from texbias import optim
    p = torch.nn.Parameter(torch.ones((4,), dtype=torch.complex64))
    p.grad = torch.ones_like(p)
    assert not optim._eligible(p, {})
