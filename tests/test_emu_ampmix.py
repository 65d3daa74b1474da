"""Amplitude mixing in k-space on the host emulator of the per-unit bodies (ampmix.h ampmix_fwd_unit /
ampmix_bwd_unit / am_gysum, the code k_kspace_ampmix / k_kspace_ampmix_bwd run), in the launch sequences of
tb_kspace_ampmix_f32 / tb_kspace_ampmix_bwd_f32.  Outputs are pre-filled with NaN, so an element no pass
writes shows.

Reference: tests/_ampmix_ref.py, float64 (torch.fft and its autograd).  Bar (DESIGN (c)):
max|a - ref| / max|ref| <= 1e-5.  The gradients run on the inputs that keep the amplitudes away from 0
(_ampmix_ref.spiked): with plain randn a coefficient with tiny |X| makes gx ill-conditioned in any float32
implementation.
"""
import os
import subprocess

import numpy as np
import pytest

import _ampmix_ref as R
import _emu_ampmix as E
from _golden import relerr

TOL = 1e-5
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "medical-vision-textural-bias_amd", "csrc")

# image shape [B, C, *spatial], transformed axes; the shapes of test_gpu_spectrum.py (its 2-D [2, 16, 12] as
# two one-channel samples, so that a partner index has something to choose)
CASES = [
    ((2, 3, 12, 10, 9), 3),     # odd D, ragged tile
    ((1, 2, 9, 8, 6), 3),       # even D: both self-conjugate columns
    ((2, 1, 16, 12), 2),        # 2-D
    ((1, 1, 20, 48, 35), 3),    # radices 5 and 7
    ((1, 2, 128, 8, 6), 3),     # long H
    ((9, 1, 12, 10, 9), 3),     # two launch groups; the partners cross them
]
IDS = ["odd_d", "even_d", "2d", "radix_5_7", "long_h", "two_groups"]
PERMS = ["none", "cyclic", "repeated"]


def make_perm(kind, B):
    if kind == "none":
        return None
    if kind == "cyclic":
        return ((np.arange(B) + 1) % B).astype(np.int32)      # sample B-1 -> 0: across the launch groups
    p = ((np.arange(B) - 2) % B).astype(np.int32)             # samples 0 and 1 share the partner B-1
    p[:2] = B - 1
    return p


def make_mask(shape, n_dims, per_channel, seed):
    sp = shape[len(shape) - n_dims:]
    rng = np.random.default_rng(seed)
    return rng.uniform(size=((shape[1],) + sp) if per_channel else sp).astype(np.float32)


def make_lam(B, seed):
    return np.random.default_rng(seed).uniform(size=B).astype(np.float32)


_ref_cache = {}


def _reference(key, fn):
    if key not in _ref_cache:
        _ref_cache[key] = fn()
    return _ref_cache[key]


@pytest.mark.parametrize("from_x", [False, True], ids=["y_given", "y_from_x"])
@pytest.mark.parametrize("perm_kind", PERMS)
@pytest.mark.parametrize("per_channel", [False, True], ids=["cm1", "cmC"])
@pytest.mark.parametrize("T", [1, 8])
@pytest.mark.parametrize("shape,n_dims", CASES, ids=IDS)
def test_forward_unit_matches_float64(shape, n_dims, T, per_channel, perm_kind, from_x):
    rng = np.random.default_rng(70)
    x = rng.standard_normal(shape).astype(np.float32)
    y = x if from_x else rng.standard_normal(shape).astype(np.float32)
    M = make_mask(shape, n_dims, per_channel, 71)
    lam = make_lam(shape[0], 72)
    perm = make_perm(perm_kind, shape[0])
    pad = 3 if T == 8 else 0
    out = E.ampmix(x, None if from_x else y, M, lam, perm, n_dims, pad=pad, T=T)
    D = shape[-1]
    assert out.shape == shape[:-1] + (D + pad,)
    assert not np.isnan(out).any()                                  # every element written
    assert np.all(out[..., D:] == 0.0)
    ref = _reference(("f", shape, per_channel, perm_kind, from_x),
                     lambda: R.reference_np(x, y, M, lam, perm, n_dims))
    e = relerr(out[..., :D], ref)
    print(f"forward, emulator vs float64 {e:.3e}")
    assert e <= TOL


@pytest.mark.parametrize("from_x", [False, True], ids=["y_given", "y_from_x"])
@pytest.mark.parametrize("perm_kind", PERMS)
@pytest.mark.parametrize("per_channel", [False, True], ids=["cm1", "cmC"])
@pytest.mark.parametrize("T", [1, 8])
@pytest.mark.parametrize("shape,n_dims", CASES, ids=IDS)
def test_backward_unit_matches_float64_autograd(shape, n_dims, T, per_channel, perm_kind, from_x):
    x = R.spiked(shape, n_dims, 73, 1)
    y = x if from_x else R.spiked(shape, n_dims, 74, 2)
    g = np.random.default_rng(75).standard_normal(shape).astype(np.float32)
    M = make_mask(shape, n_dims, per_channel, 76)
    lam = make_lam(shape[0], 77)
    perm = make_perm(perm_kind, shape[0])
    gx, gy = E.ampmix_bwd(x, None if from_x else y, M, lam, g, perm, n_dims, T=T)
    assert not np.isnan(gx).any() and not np.isnan(gy).any()
    _, rgx, rgy = _reference(("b", shape, per_channel, perm_kind, from_x),
                             lambda: R.reference_grads(x, y.copy(), M, lam, g, perm, n_dims))
    ex, ey = relerr(gx, rgx), relerr(gy, rgy)
    print(f"backward, emulator vs float64 autograd: gx {ex:.3e} gy {ey:.3e}")
    assert ex <= TOL and ey <= TOL
    # without gy the same gx (to rounding: a separate instantiation of the unit) and no second output
    gx2, none = E.ampmix_bwd(x, None if from_x else y, M, lam, g, perm, n_dims, T=T, need_gy=False)
    assert none is None and relerr(gx2, gx) <= 2e-6


def test_tile_width_and_partner_source_do_not_change_the_result():
    shape = (2, 3, 12, 10, 9)
    rng = np.random.default_rng(78)
    x = rng.standard_normal(shape).astype(np.float32)
    M, lam, perm = make_mask(shape, 3, True, 79), make_lam(2, 80), make_perm("cyclic", 2)
    a = E.ampmix(x, None, M, lam, perm, 3, T=3)
    assert np.array_equal(a, E.ampmix(x, None, M, lam, perm, 3, T=16))
    assert np.array_equal(a, E.ampmix(x, x[perm], M, lam, None, 3, T=5))    # the explicit y = x[perm]


def test_special_cases():
    shape = (2, 3, 12, 10, 9)
    rng = np.random.default_rng(81)
    x = rng.standard_normal(shape).astype(np.float32)
    y = rng.standard_normal(shape).astype(np.float32)
    M = make_mask(shape, 3, False, 82)
    # lam = 0: the FFT round trip of x
    out = E.ampmix(x, y, M, np.zeros(2, np.float32), None, 3)
    assert relerr(out, x) <= 2e-6
    # x = 0: u = 1, Re ifftn(m_s |Y|); and no NaN from the zero amplitudes, forward or backward
    lam = make_lam(2, 83)
    z = np.zeros(shape, np.float32)
    out = E.ampmix(z, y, M, lam, None, 3)
    assert relerr(out, R.closed_form(z, y, M, lam, None, 3)[0]) <= TOL
    gx, gy = E.ampmix_bwd(z, z, M, lam, y, None, 3)
    assert np.isfinite(gx).all() and np.all(gy == 0.0)
    # a partner index outside [0, B) is clamped, never dereferenced
    bad = np.array([7, -3], np.int32)
    assert np.array_equal(E.ampmix(x, y, M, lam, bad, 3), E.ampmix(x, y, M, lam, np.array([1, 0], np.int32), 3))


@pytest.mark.parametrize("ex", [-40, 40])
def test_value_range(ex):
    shape = (2, 3, 12, 10, 9)
    s = np.float32(2.0 ** ex)
    x, y = R.spiked(shape, 3, 84, 1) * s, R.spiked(shape, 3, 85, 2) * s
    g = np.random.default_rng(86).standard_normal(shape).astype(np.float32)
    M, lam = make_mask(shape, 3, True, 87), make_lam(2, 88)
    perm = make_perm("cyclic", 2)
    out = E.ampmix(x, y, M, lam, perm, 3)
    gx, gy = E.ampmix_bwd(x, y, M, lam, g, perm, 3)
    rout, rgx, rgy = R.reference_grads(x, y, M, lam, g, perm, 3)
    assert relerr(out, rout) <= TOL and relerr(gx, rgx) <= TOL and relerr(gy, rgy) <= TOL


def test_emulator_entry_points_under_asan_ubsan():
    """tests/emu/emu_ampmix_asan_main.cpp: the emulator's entry points over three launch groups, one
    executable built with -fsanitize=address,undefined and run as a plain child process."""
    src = [os.path.join(HERE, "emu", "emu_ampmix_asan_main.cpp"), os.path.join(HERE, "emu", "emu_ampmix.cpp")] + \
          [os.path.join(CSRC, h) for h in ("fft_core.h", "spectrum.h", "ampmix.h", "plan_host.h")]
    exe = os.path.join(HERE, "emu", "_build", "emu_ampmix_asan")
    newest = max(os.path.getmtime(p) for p in src)
    if not os.path.exists(exe) or os.path.getmtime(exe) < newest:
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        tmp = exe + f".{os.getpid()}.tmp"
        cxx = os.environ.get("TB_EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")
        subprocess.check_call([cxx, "-O0", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "include"), "-I", CSRC, src[0], "-o", tmp])
        os.replace(tmp, exe)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "emu ampmix sanitizer run ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
