"""Radix by axis on the device: the table of tests/_fft_plan_cases.py (every radix of the run-time planner
alone, as the first, a middle and the last stage, on each axis) through texbias.runtime, each direction
against float64 numpy, and the consumers of the mixed-radix passes (fused filter, log-|k| sums, both mask
gradients) on the four corners of the host's radix-set dispatch.  The emulator sweep
(tests/test_emu_fft_plans.py) pins the shared arithmetic; what is checked here is the device build of it:
the radix set chosen per plan, the kernel objects of the second radix set, the LDS carve at long prime
axes.  A stage whose radix is not compiled into the launched kernel is skipped without an error, and a
plan may fall to the direct-DFT fallback without one: the first shows against float64, the second in the
kernel names.

Bar (DESIGN (c)): max|a - ref| / max|ref| <= 1e-5 for the export, the import, the filter and the gradients;
the log-|k| sums with the tolerance of tests/test_gpu_generic.py.  Worst measured on an MI355X: export
1.9e-7, import 2.3e-7, filter 7.0e-7, gradients 2.3e-7, sums 5.7e-8 relative.
"""
import numpy as np
import pytest
import torch

import _fft_plan_cases as P
from _golden import relerr
from texbias import kprog as K

pytestmark = pytest.mark.gpu

TOL = 1e-5
NAN = float("nan")


@pytest.fixture(scope="module")
def rt(gpu):
    from texbias import runtime
    return runtime


@pytest.fixture
def full_spectrum(rt):
    """The full-spectrum passes for every program: no band, closed-form spike or separable wrap route."""
    try:
        rt.set_band_plans(False)
        rt.set_point_plans(False)
        rt.set_wrap_plans(False)
        yield
    finally:
        rt.set_band_plans(True)
        rt.set_point_plans(True)
        rt.set_wrap_plans(True)


def _timed(rt, fn):
    rt.set_pass_timing(True)
    try:
        out = fn()
        _, cnt, _, names = rt.pass_stats()
    finally:
        rt.set_pass_timing(False)
    return out, cnt, names


def _lead(case):
    shape, n_dims = case
    return (P.CHANNELS,) + tuple(shape), n_dims


# ----------------------------------------------------------------- the table: export, import, plan
@pytest.mark.parametrize("case", P.ALL_CASES, ids=P.case_id)
def test_plan_radices(rt, case):
    hwd = K.geometry(case[0]).hwd
    plan = rt.plan_for(torch.device("cuda"), *hwd)
    for axis in range(3):
        assert plan.radices(axis) == P.expected_radices(hwd[axis]), (hwd, axis)


@pytest.mark.parametrize("case", P.ALL_CASES, ids=P.case_id)
def test_export_matches_float64(rt, case):
    shape, n_dims = _lead(case)
    x = P.image(shape, 93)
    xd = torch.from_numpy(x).cuda()
    out = torch.full(shape, complex(NAN, NAN), dtype=torch.complex64, device="cuda")
    k, cnt, names = _timed(rt, lambda: rt.kspace_export(xd, n_dims, out=out))
    assert k.data_ptr() == out.data_ptr()
    assert names[0] == "k_slab_fwd" and names[1] == "k_kspace_export", names   # not the direct-DFT fallback
    assert cnt[:3] == [1, 1, 0]
    kn = k.cpu().numpy()
    assert not np.isnan(kn.real).any() and not np.isnan(kn.imag).any()   # every element written
    e = P.crelerr(kn, P.ref_export(x, n_dims))
    print(f"{case[0]} export vs float64 {e:.3e}")
    assert e <= TOL
    assert P.mirror_defect(kn, n_dims) == 0                              # f and -f: one value, two stores
    assert torch.equal(rt.kspace_export(xd, n_dims), k)                  # no atomics: bit-reproducible


@pytest.mark.parametrize("case", P.ALL_CASES, ids=P.case_id)
def test_import_matches_float64(rt, case):
    shape, n_dims = _lead(case)
    pad, D = 3, shape[-1]
    kn = P.spectrum(shape, 94)
    kd = torch.from_numpy(kn).cuda()
    base = torch.full(shape[:-1] + (D + pad + 5,), NAN, device="cuda")   # a longer-pitched buffer
    view = base[..., : D + pad]
    y, cnt, names = _timed(rt, lambda: rt.kspace_import(kd, n_dims, pad=pad, out=view))
    assert y.data_ptr() == base.data_ptr()
    assert names[1] == "k_kspace_import" and names[2] == "k_slab_inv", names   # not the direct-DFT fallback
    assert cnt[:3] == [0, 1, 1]
    yn = base.cpu().numpy()
    assert not np.isnan(yn[..., : D + pad]).any()                        # every element written
    e = relerr(yn[..., :D], P.ref_import(kn, n_dims))
    print(f"{case[0]} import vs float64 {e:.3e}")
    assert e <= TOL
    assert np.all(yn[..., D: D + pad] == 0.0)                            # the pad columns are exactly zero
    assert np.isnan(yn[..., D + pad:]).all()                             # outside the view: untouched


# ----------------------------------------------------------------- the consumers, on the dispatch corners
CORNER_IDS = [f"{c[0]}_{c[1]}-{'x'.join(map(str, s))}" for c, s in P.CORNERS]


def _filter_checked(rt, hwd):
    x = P.image((1, P.CHANNELS) + hwd, 95)
    xd = torch.from_numpy(x).cuda()
    D, pad = hwd[2], 3
    mm = torch.empty((1, 2), dtype=torch.int32, device="cuda")
    out = torch.full((1, P.CHANNELS) + hwd[:2] + (D + pad,), NAN, device="cuda")
    y, cnt, names = _timed(rt, lambda: rt.kspace_filter(xd, 3, [P.filter_program(hwd)], P.CHANNELS, out=out, pad=pad,
                                                        minmax=mm))
    assert names[:3] == ["k_slab_fwd", "k_kspace", "k_slab_inv"], names
    yn = y.cpu().numpy()
    assert not np.isnan(yn).any()
    e = relerr(yn[0, ..., :D], P.filter_reference(x[0], hwd))
    print(f"{hwd} filter vs oracle {e:.3e}")
    assert e <= TOL
    assert np.all(yn[..., D:] == 0.0)
    np.testing.assert_array_equal(rt.keys_to_float(mm)[0], [yn[..., :D].min(), yn[..., :D].max()])


@pytest.mark.parametrize("corner,hwd", P.CORNERS, ids=CORNER_IDS)
def test_corner_filter(rt, full_spectrum, corner, hwd):
    assert P.corner_of(hwd) == corner
    _filter_checked(rt, hwd)


@pytest.mark.parametrize("hwd", P.PRIME_ROWS, ids=lambda s: "x".join(map(str, s)))
def test_prime_row_filter(rt, full_spectrum, hwd):
    """One streamed radix alone on H: forward DFT, the op program called out of line, inverse DFT."""
    _filter_checked(rt, hwd)


@pytest.mark.parametrize("corner,hwd", P.CORNERS, ids=CORNER_IDS)
def test_corner_logabs_sums(rt, corner, hwd):
    x = P.image((P.CHANNELS,) + hwd, 96)
    s = rt.logabs_sums(torch.from_numpy(x).cuda()[None], 3, [[]], P.CHANNELS).cpu().numpy()
    la = np.log(np.abs(np.fft.fftn(x.astype(np.float64), axes=(-3, -2, -1))) + 1e-10)
    ref = la.reshape(P.CHANNELS, -1).sum(axis=1)
    print(f"{hwd} log-|k| sums vs float64: rel {np.max(np.abs(s - ref) / np.abs(ref)):.3e}, "
          f"abs {np.max(np.abs(s - ref)):.3e} (atol {1e-3 * np.sqrt(la[0].size):.3e})")
    assert np.allclose(s, ref, rtol=1e-5, atol=1e-3 * np.sqrt(la[0].size))


def _ref_grads(x, g):
    """[Cm = C][H][W][D] float64: Re(X conj G) / N and conj(X) G / N in the centred layout, summed over
    the samples (one here); the shared mask's is the sum over the channels."""
    ax = (-3, -2, -1)
    X, G = np.fft.fftn(x.astype(np.float64), axes=ax), np.fft.fftn(g.astype(np.float64), axes=ax)
    n = np.prod(x.shape[-3:])
    real = np.fft.fftshift((X * np.conj(G)).real, axes=ax).sum(axis=0) / n
    cplx = np.fft.fftshift(np.conj(X) * G, axes=ax).sum(axis=0) / n
    return real, cplx


@pytest.mark.parametrize("per_channel", [False, True], ids=["shared", "per_channel"])
@pytest.mark.parametrize("corner,hwd", P.CORNERS, ids=CORNER_IDS)
def test_corner_mask_gradients(rt, corner, hwd, per_channel):
    shape = (1, P.CHANNELS) + hwd
    x, g = P.image(shape, 97), P.image(shape, 98)
    xd, gd = torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda()
    cm = P.CHANNELS if per_channel else 1
    msh = hwd if cm == 1 else (cm,) + hwd
    ref_r, ref_c = _ref_grads(x, g)
    if not per_channel:
        ref_r, ref_c = ref_r.sum(axis=0), ref_c.sum(axis=0)

    out = torch.full(msh, NAN, device="cuda")
    dm, _, names = _timed(rt, lambda: rt.kspace_mask_grad(xd, gd, 3, cm, channels=P.CHANNELS, out=out))
    assert names[0] == "k_slab_fwd" and names[1] == "k_kspace_maskgrad", names
    d = dm.cpu().numpy()
    assert not np.isnan(d).any()
    e = relerr(d, ref_r)
    print(f"{hwd} mask gradient vs float64 {e:.3e}")
    assert e <= TOL

    outc = torch.full(msh, complex(NAN, NAN), dtype=torch.complex64, device="cuda")
    dc, _, names = _timed(rt, lambda: rt.kspace_cmask_grad(xd, gd, 3, cm, channels=P.CHANNELS, out=outc))
    assert names[0] == "k_slab_fwd" and names[1] == "k_kspace_cmaskgrad", names
    c = dc.cpu().numpy()
    assert not np.isnan(c.real).any() and not np.isnan(c.imag).any()
    e = P.crelerr(c, ref_c)
    print(f"{hwd} complex mask gradient vs float64 {e:.3e}")
    assert e <= TOL
