"""Radix by axis: every radix of the run-time planner, alone, as the first, a middle and the last stage,
on each of the three axes, on the host emulators of the pass bodies (fft_core.h, spectrum.h) against
float64 numpy.  A round trip cannot see an error the forward and the inverse transform share (a permuted
output slot, a wrong butterfly constant, a twiddle exponent wrong in both directions), so each direction
is checked on its own: the export against fftshift(fftn(x)), the import against Re(ifftn(ifftshift(K))),
and the fused filter (the op program reads each coefficient's position) against the numpy oracle.

Bar (DESIGN (c)): max|a - ref| / max|ref| <= 1e-5.  Worst measured: export 2.2e-7 (H = 961),
import 2.4e-7 (D = 899), filter 1.3e-6 (W = 686).
"""
import ctypes

import numpy as np
import pytest

import _emu
import _emu_spectrum as E
import _fft_plan_cases as P
from _golden import relerr

TOL = 1e-5


def test_table_coverage():
    """Conditions on the table, computed from the restated factorisation."""
    cov = P.coverage()
    assert cov["single"] == set(P.RADIX_PREF) and len(P.RADIX_PREF) == 19
    assert set(P.PRIMES) <= cov["non_last"]
    assert set(P.PRIMES) <= cov["last"]
    assert 3 in cov["stages"] and 4 in cov["stages"]
    assert cov["middle"] & set(P.STREAMED)
    # the filter subset: every streamed prime alone (one-radix pass B), first, last and in the middle
    sub = P.coverage(P.FILTER_LENGTHS)
    assert set(P.STREAMED) <= sub["single"]
    assert sub["non_last"] & set(P.STREAMED) and sub["last"] & set(P.STREAMED) and sub["middle"] & set(P.STREAMED)
    # the consumers' shapes sit on the dispatch corners they are listed under, and all four are there
    assert all(P.corner_of(hwd) == corner for corner, hwd in P.CORNERS)
    assert {c for c, _ in P.CORNERS} == {(a, b) for a in (P.SMALL, P.ALL) for b in (P.SMALL, P.ALL)}
    assert all(P.corner_of(hwd) == (P.SMALL, P.ALL) and P.expected_radices(hwd[0]) == [hwd[0]] for hwd in P.PRIME_ROWS)
    # every case is one the planner takes, each length once
    assert len(set(P.LENGTHS)) == len(P.LENGTHS) == 52
    assert all(P.expected_radices(n) is not None and len(P.expected_radices(n)) <= 8 for n in P.LENGTHS)
    assert P.expected_radices(37) is None and P.expected_radices(2 * 37) is None


def test_restated_factorisation_products():
    for n in list(range(1, 1025)):
        r = P.expected_radices(n)
        if r is not None:
            assert int(np.prod(r, dtype=np.int64)) == n and all(q in P.RADIX_PREF for q in r)


@pytest.mark.parametrize("n", P.LENGTHS)
def test_planner_radices(n):
    buf = (ctypes.c_int * 8)()
    nst = _emu.lib().tbemu_radices(n, buf)
    assert list(buf[:max(nst, 0)]) == P.expected_radices(n)


def _bc(case):
    shape, n_dims = case
    return (1, P.CHANNELS) + tuple(shape), n_dims


@pytest.mark.parametrize("case", P.ALL_CASES, ids=P.case_id)
def test_export_matches_float64(case):
    shape, n_dims = _bc(case)
    x = P.image(shape, 90)
    k = E.kspace_export(x, n_dims)                    # pre-filled with NaN
    assert not np.isnan(k.real).any() and not np.isnan(k.imag).any()   # every element written
    e = P.crelerr(k, P.ref_export(x, n_dims))
    print(f"{case[0]} export, emulator vs float64 {e:.3e}")
    assert e <= TOL
    assert P.mirror_defect(k, n_dims) == 0


@pytest.mark.parametrize("case", P.ALL_CASES, ids=P.case_id)
def test_import_matches_float64(case):
    shape, n_dims = _bc(case)
    k = P.spectrum(shape, 91)
    y = E.kspace_import(k, n_dims)                    # pre-filled with NaN
    assert y.shape == shape and not np.isnan(y).any()
    e = relerr(y, P.ref_import(k, n_dims))
    print(f"{case[0]} import, emulator vs float64 {e:.3e}")
    assert e <= TOL


@pytest.mark.parametrize("hwd", P.FILTER_CASES, ids=lambda s: "x".join(map(str, s)))
def test_fused_filter_matches_oracle(hwd):
    """Pass B's last stage with an op program that reads the position: the inlined call for the small
    radices, the out-of-line one for a streamed prime as the last H radix."""
    x = P.image((P.CHANNELS,) + hwd, 92)
    y, mm = _emu.kspace_filter(x[None], 3, [P.filter_program(hwd)])
    ref = P.filter_reference(x, hwd)
    e = relerr(y[0], ref)
    print(f"{hwd} filter, emulator vs oracle {e:.3e}")
    assert e <= TOL
    np.testing.assert_array_equal(mm[0], [y.min(), y.max()])
