"""User-supplied k-space masks (TB_OP_MASK) on the host emulator of the pass kernels.

The emulator runs the device's item functions (fft_core.h apply_ops, kspace_ct.h ops_bfly / b_mid_split)
unchanged, so a numpy array's address in ``op.l`` exercises the op on every route the CPU can reach:
the run-time-planned pass B, the compiled tile plan (H = 128) and the half-unit split spectrum.
Reference: y = Re(IFFT(ifftshift(M . fftshift(FFT x)))) in numpy float64, written here.
Bars (DESIGN (c)): max|y - ref| / max|ref| <= 1e-5 against float64; equality where stated.
"""
import numpy as np
import pytest
import torch

import _emu
from _golden import relerr
from oracle import filters_oracle as O
from texbias import kprog as K
from texbias._abi import TB_OP_MASK

TOL = 1e-5

# (image shape [B, C, *spatial], transformed axes, emulator route ct, tile width T)
CASES = [
    ((2, 3, 12, 10, 9), 3, 0, 7),     # odd D, several ragged tiles
    ((1, 2, 9, 8, 6), 3, 0, 0),       # even D: the kd = 0 and Nyquist columns
    ((1, 2, 16, 12), 2, 0, 0),        # 2-D: (H, 1, D)
    ((1, 1, 20, 48, 35), 3, 2, 0),    # half units over the split spectrum (b_mid_split)
    ((1, 1, 128, 4, 6), 3, 1, 0),     # compiled tile plan H = 128 (ops_bfly)
]
IDS = ["odd_d", "even_d", "2d", "half", "ct128"]


def ref_mask(x, M, n_dims):
    """float64: M in the layout of fftshift(fftn(x)); broadcasts over the leading axes."""
    ax = tuple(range(-n_dims, 0))
    k = np.fft.fftshift(np.fft.fftn(np.asarray(x, np.float64), axes=ax), axes=ax)
    return np.fft.ifftn(np.fft.ifftshift(k * np.asarray(M, np.float64), axes=ax), axes=ax).real


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
    return ref_mask(x, W, n_dims)


def mask_prog(M, channels, spatial, chan=-1):
    """One MASK op reading the numpy array M (kept alive by the caller) in place."""
    assert M.dtype == np.float32 and M.flags.c_contiguous
    return [K.mask_op(M.ctypes.data, channels, K.geometry(spatial).hwd, chan)]


def emu(x, n_dims, progs, ct, T, pad=0):
    y, _ = _emu.kspace_filter(x, n_dims, progs, pad=pad, T=T, ct=ct)
    return y


def test_op_constant_and_builder():
    assert TB_OP_MASK == 7
    op = K.mask_op(0x1000, 3, (12, 10, 9), chan=1)
    assert (op.kind, op.chan, op.l, list(op.i)) == (7, 1, 0x1000, [3, 10, 9])
    with pytest.raises(ValueError):
        K.mask_op(0, 1, (12, 10, 9))


@pytest.mark.parametrize("shape,n_dims,ct,T", CASES, ids=IDS)
def test_shared_mask(shape, n_dims, ct, T):
    rng = np.random.default_rng(11)
    x = rng.standard_normal(shape).astype(np.float32)
    sp = shape[-n_dims:]
    M = rng.uniform(0.0, 1.5, sp).astype(np.float32)
    y = emu(x, n_dims, [mask_prog(M, 1, sp)] * shape[0], ct, T)
    assert relerr(y, x) > 1e-2   # the op ran: an unknown kind leaves the input untouched
    assert relerr(y, ref_mask(x, M, n_dims)) <= TOL


@pytest.mark.parametrize("shape,n_dims,ct,T", CASES, ids=IDS)
def test_per_channel_mask(shape, n_dims, ct, T):
    rng = np.random.default_rng(12)
    x = rng.standard_normal(shape).astype(np.float32)
    sp, C = shape[-n_dims:], shape[1]
    M = rng.uniform(0.0, 1.5, (C,) + sp).astype(np.float32)
    y = emu(x, n_dims, [mask_prog(M, C, sp)] * shape[0], ct, T)
    assert relerr(y, ref_mask(x, M, n_dims)) <= TOL


@pytest.mark.parametrize("shape,n_dims,ct,T", CASES, ids=IDS)
def test_chan_selected_mask(shape, n_dims, ct, T):
    """An op with chan = c filters channel c only; the other channels pass through."""
    rng = np.random.default_rng(13)
    x = rng.standard_normal(shape).astype(np.float32)
    sp, C = shape[-n_dims:], shape[1]
    c = C - 1
    M = rng.uniform(0.0, 1.5, sp).astype(np.float32)
    y = emu(x, n_dims, [mask_prog(M, 1, sp, chan=c)] * shape[0], ct, T)
    ref = np.asarray(x, np.float64).copy()
    ref[:, c] = ref_mask(x[:, c], M, n_dims)
    assert relerr(y, ref) <= TOL
    if C > 1:
        assert relerr(y[:, 0], x[:, 0]) <= 2e-6   # identity round trip of an untouched channel


def test_mask_with_padding():
    rng = np.random.default_rng(14)
    shape, sp = (1, 2, 12, 10, 9), (12, 10, 9)
    x = rng.standard_normal(shape).astype(np.float32)
    M = rng.uniform(0.0, 1.5, sp).astype(np.float32)
    y = emu(x, 3, [mask_prog(M, 1, sp)], 0, 0, pad=5)
    assert y.shape[-1] == 14 and np.all(y[..., 9:] == 0.0)
    assert relerr(y[..., :9], ref_mask(x, M, 3)) <= TOL


@pytest.mark.parametrize("shape,n_dims,ct,T", [CASES[0], CASES[1], CASES[3], CASES[4]],
                         ids=["odd_d", "even_d", "half", "ct128"])
@pytest.mark.parametrize("inside_off", [False, True])
def test_disk_mask_equals_disk_op(shape, n_dims, ct, T, inside_off):
    """A mask equal to the reference's disk gives the DISK op's output bit for bit (same route)."""
    rng = np.random.default_rng(15)
    x = rng.standard_normal(shape).astype(np.float32)
    sp = shape[-3:]
    M = np.ascontiguousarray(O.disk_mask((1,) + sp, 4.0, 3, inside_off)[0], np.float32)
    assert 0 < M.sum() < M.size
    ym = emu(x, 3, [mask_prog(M, 1, sp)] * shape[0], ct, T)
    yd = emu(x, 3, [[K.disk_op(4.0, inside_off)]] * shape[0], ct, T)
    assert np.array_equal(ym, yd)


@pytest.mark.parametrize("shape,n_dims,ct,T", [CASES[0], CASES[1], CASES[3], CASES[4]],
                         ids=["odd_d", "even_d", "half", "ct128"])
def test_gibbs_mask_equals_gibbs_op(shape, n_dims, ct, T):
    """An off-centre mask (sqrt(d2) <= r about (n-1)/2, not symmetric under f -> -f on even axes)
    gives the GIBBS op's output bit for bit: both symmetrise as (m(f) + m(-f)) / 2."""
    rng = np.random.default_rng(16)
    x = rng.standard_normal(shape).astype(np.float32)
    sp = shape[-3:]
    alpha = 0.7
    M = np.ascontiguousarray(O.gibbs_mask(sp, alpha), np.float32)
    assert 0 < M.sum() < M.size
    ym = emu(x, 3, [mask_prog(M, 1, sp)] * shape[0], ct, T)
    yg = emu(x, 3, [[K.gibbs_op(alpha, sp)]] * shape[0], ct, T)
    assert np.array_equal(ym, yg)


@pytest.mark.parametrize("shape,n_dims,ct,T", [CASES[0], CASES[3]], ids=["odd_d", "half"])
def test_mask_spike_wrap_program(shape, n_dims, ct, T):
    rng = np.random.default_rng(17)
    x = rng.standard_normal(shape).astype(np.float32)
    sp = shape[-3:]
    M = rng.uniform(0.0, 1.5, sp).astype(np.float32)
    idx = (sp[0] // 2 + 2, sp[1] // 2 - 3, sp[2] // 2 + 1)
    prog = mask_prog(M, 1, sp) + [K.spike_op(idx, K.geometry(sp), 6.0), K.wrap_op(0.5)]
    y = emu(x, 3, [prog] * shape[0], ct, T)
    ref = ref_wrap(ref_spike(ref_mask(x, M, 3), idx, 6.0, 3), 0.5, 3)
    assert relerr(y, ref) <= TOL


# ------------------------------------------------------------------ host validation (no GPU needed)
def test_mask_geometry_accepts():
    from texbias import runtime as rt
    x = torch.zeros((2, 3, 6, 5, 4))
    assert rt.mask_geometry(x, torch.ones((6, 5, 4)), 3) == (1, 3)
    assert rt.mask_geometry(x, torch.ones((3, 6, 5, 4)), 3) == (3, 3)
    assert rt.mask_geometry(x.reshape(6, 6, 5, 4), torch.ones((3, 6, 5, 4)), 3, channels=3) == (3, 3)
    assert rt.mask_geometry(torch.zeros((2, 1, 6, 1, 4)), torch.ones((6, 1, 4)), 3) == (1, 1)   # size-1 axis kept


@pytest.mark.parametrize("bad", ["shape", "channels", "dtype", "contiguity", "device", "grad", "numpy"])
def test_mask_geometry_rejects(bad):
    from texbias import runtime as rt
    x = torch.zeros((2, 3, 6, 5, 4))
    m = {"shape": torch.ones((6, 5, 5)),
         "channels": torch.ones((2, 6, 5, 4)),
         "dtype": torch.ones((6, 5, 4), dtype=torch.float64),
         "contiguity": torch.ones((6, 4, 5)).transpose(1, 2),
         "device": torch.ones((6, 5, 4), device="meta"),
         "grad": torch.ones((6, 5, 4), requires_grad=True),
         "numpy": np.ones((6, 5, 4), np.float32)}[bad]
    with pytest.raises(ValueError):
        rt.mask_geometry(x, m, 3)


def test_kspace_mask_needs_hip():
    from texbias import runtime as rt
    with pytest.raises(rt.TexbiasError):
        rt.kspace_mask(torch.zeros((1, 6, 5, 4)), torch.ones((6, 5, 4)), 3)


def test_transform_program_and_chain_stage():
    """KSpaceMask(d).program validates the shape on the host; FusedChain counts them as k-space."""
    from texbias import masks, pipeline
    assert {"KSpaceMask", "KSpaceMaskd"} <= pipeline.KSPACE
    t = masks.KSpaceMask(np.ones((6, 5, 4)))
    assert t.mask.dtype == torch.float32 and t.mask.is_contiguous()
    with pytest.raises(ValueError):
        t.program((6, 5, 5), 2)
    with pytest.raises(ValueError):
        masks.KSpaceMask(np.ones((6, 5, 4), np.complex64))
    with pytest.raises(ValueError):
        masks.KSpaceMask(torch.ones((6, 5, 4), requires_grad=True))
