"""Amplitude mixing in k-space, the parts that need no device: the closed form the kernels evaluate
(csrc/ampmix.h, restated with numpy in tests/_ampmix_ref.py) against the float64 ``torch.fft`` definition and
its ``torch.autograd``, the low-frequency box, the draws of ``RandAmplitudeMix``, the op schemas and fake
kernels, the library symbols and the host-side argument checks.

Bar of the float64 identities: 1e-12 of max|ref| (they hold to a few 1e-15).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import _ampmix_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = 1e-12

CASES = [
    ((2, 3, 12, 10, 9), 3),
    ((1, 2, 9, 8, 6), 3),
    ((2, 1, 16, 12), 2),
    ((1, 1, 20, 48, 35), 3),
    ((1, 2, 128, 8, 6), 3),
    ((9, 1, 12, 10, 9), 3),
    ((1, 2, 37, 8, 6), 3),
]
IDS = ["odd_d", "even_d", "2d", "radix_5_7", "long_h", "two_groups", "prime_h"]


def rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


@pytest.mark.parametrize("perm_kind", ["none", "cyclic", "repeated"])
@pytest.mark.parametrize("per_channel", [False, True], ids=["cm1", "cmC"])
@pytest.mark.parametrize("shape,n_dims", CASES, ids=IDS)
def test_closed_form_is_the_definition_and_its_autograd(shape, n_dims, per_channel, perm_kind):
    rng = np.random.default_rng(60)
    B, C = shape[:2]
    sp = shape[2:]
    x, y, g = rng.standard_normal(shape), rng.standard_normal(shape), rng.standard_normal(shape)
    M = rng.uniform(size=((C,) + sp) if per_channel else sp)       # not symmetric: the .real symmetrises
    lam = rng.uniform(size=B)
    perm = None
    if perm_kind == "cyclic":
        perm = (np.arange(B) + 1) % B
    elif perm_kind == "repeated":
        perm = (np.arange(B) - 2) % B
        perm[:2] = B - 1
    out, gx, gy = R.reference_grads(x, y, M, lam, g, perm, n_dims)
    cf, imag = R.closed_form(x, y, M, lam, perm, n_dims)
    cgx, cgy = R.closed_form_grads(x, y, M, lam, g, perm, n_dims)
    e = (rel(cf, out), imag / np.max(np.abs(out)), rel(cgx, gx), rel(cgy, gy))
    print("closed form vs definition: out %.2e  imag %.2e  gx %.2e  gy %.2e" % e)
    assert max(e) <= EXACT


def test_zero_amplitudes_take_the_documented_values():
    # x = 0: angle(0) = 0, so u = 1 and out = Re ifftn(m_s |Y|); the closed form drops the tangential term there
    rng = np.random.default_rng(61)
    shape = (2, 2, 6, 5, 4)
    y, g = rng.standard_normal(shape), rng.standard_normal(shape)
    M, lam = rng.uniform(size=shape[2:]), rng.uniform(size=2)
    z = np.zeros(shape)
    assert rel(R.closed_form(z, y, M, lam)[0], R.reference_np(z, y, M, lam)) <= EXACT
    gx, gy = R.closed_form_grads(z, z, M, lam, g)
    assert np.all(gy == 0.0) and np.isfinite(gx).all()


def test_lowfreq_box_geometry_and_symmetry():
    from texbias.amplitude import lowfreq_box
    for spatial, beta in [((12, 10, 9), 0.25), ((9, 8, 6), 0.25), ((16, 12), 0.1), ((20, 48, 35), 0.01),
                          ((6, 128, 128), 0.25), ((8, 8, 8), 0.9)]:
        m = lowfreq_box(spatial, beta)
        assert m.shape == spatial and m.dtype == torch.float32
        b = max(1, int(np.floor(min(spatial) * beta)))
        ref = np.ones(spatial, np.float32)
        for a, n in enumerate(spatial):
            idx = np.arange(n)
            ins = ((idx >= n // 2 - b) & (idx <= n // 2 + b)).astype(np.float32)
            ref = ref * ins.reshape([-1 if i == a else 1 for i in range(len(spatial))])
        assert np.array_equal(m.numpy(), ref)
        assert m[tuple(n // 2 for n in spatial)] == 1.0                       # DC is inside
        ax = tuple(range(len(spatial)))
        u = np.fft.ifftshift(m.numpy(), axes=ax)
        assert np.array_equal(u, np.roll(np.flip(u, axis=ax), 1, axis=ax))    # M[s(f)] = M[s(-f)]
    with pytest.raises(ValueError):
        lowfreq_box((8, 8), -0.1)
    with pytest.raises(ValueError):
        lowfreq_box((), 0.1)


def test_rand_amplitude_mix_draws():
    from texbias.amplitude import RandAmplitudeMix
    t = RandAmplitudeMix(0.1, lam_range=(0.2, 0.7), prob=0.5)
    t.set_random_state(seed=123)
    draws = []
    for _ in range(20):
        t.randomize(16)
        assert t.perm.dtype == np.int32 and t.lam.dtype == np.float32
        assert sorted(t.perm.tolist()) == list(range(16))                    # a permutation
        on = t.lam != 0
        assert np.all((t.lam[on] >= np.float32(0.2)) & (t.lam[on] <= np.float32(0.7)))
        draws.append((t.perm.copy(), t.lam.copy()))
    frac = np.mean([np.mean(lam != 0) for _, lam in draws])
    assert 0.3 < frac < 0.7                                                  # about prob of them are drawn
    t.set_random_state(seed=123)
    for perm, lam in draws:                                                  # replays from the seed
        t.randomize(torch.empty((16, 1, 4, 4)))
        assert np.array_equal(t.perm, perm) and np.array_equal(t.lam, lam)
    never = RandAmplitudeMix(0.1, prob=0.0)
    never.set_random_state(seed=1)
    never.randomize(5)
    assert np.all(never.lam == 0.0)                                          # undrawn samples: lam = 0
    always = RandAmplitudeMix(0.1, lam_range=(0.5, 0.5), prob=1.0)
    always.set_random_state(seed=1)
    always.randomize(5)
    assert np.all(always.lam == np.float32(0.5))
    with pytest.raises(ValueError):
        RandAmplitudeMix(0.1, lam_range=(1.0, 0.0))


def test_library_exports_the_new_symbols():
    lib = ctypes.CDLL(os.path.join(ROOT, "medical-vision-textural-bias_amd", "libtexbias.so"))   # loads without a GPU
    for name in ("tb_ampmix_workspace_bytes", "tb_kspace_ampmix_f32", "tb_kspace_ampmix_bwd_f32"):
        assert hasattr(lib, name), name


def test_ops_exist_with_the_stated_schemas_and_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from texbias import ops  # noqa: F401
    assert str(torch.ops.texbias.amp_mix.default._schema) == \
        "texbias::amp_mix(Tensor x, Tensor y, Tensor mask, Tensor lam, Tensor? perm, SymInt n_dims, " \
        "SymInt channels, SymInt pad=0) -> Tensor"
    assert str(torch.ops.texbias.amp_mix_grad.default._schema) == \
        "texbias::amp_mix_grad(Tensor x, Tensor y, Tensor mask, Tensor lam, Tensor? perm, Tensor g, SymInt n_dims, " \
        "SymInt channels, bool need_gy) -> (Tensor, Tensor)"
    with FakeTensorMode():
        x = torch.empty((2, 3, 6, 5, 4))
        m = torch.empty((6, 5, 4))
        lam = torch.empty((2,))
        perm = torch.empty((2,), dtype=torch.int32)
        out = torch.ops.texbias.amp_mix(x, x, m, lam, perm, 3, 3, 2)
        assert out.shape == (2, 3, 6, 5, 6) and out.dtype == torch.float32
        out = torch.ops.texbias.amp_mix(x, x, m, lam, None, 3, 3)
        assert out.shape == x.shape
        gx, gy = torch.ops.texbias.amp_mix_grad(x, x, m, lam, perm, x, 3, 3, True)
        assert gx.shape == x.shape and gy.shape == x.shape
        gx, gy = torch.ops.texbias.amp_mix_grad(x, x, m, lam, None, x, 3, 3, False)
        assert gx.shape == x.shape and gy.shape == (0,)


def test_runtime_validation_and_lazy_export():
    import texbias
    from texbias import runtime as rt
    from texbias._lib import TexbiasError
    A = texbias.amplitude
    assert A.__all__ == ["amplitude_mix", "lowfreq_box", "AmplitudeMix", "RandAmplitudeMix"]
    x = torch.zeros((2, 3, 6, 5, 4))
    m = torch.zeros((6, 5, 4))
    lam = torch.zeros((2,))
    perm = torch.zeros((2,), dtype=torch.int32)
    with pytest.raises(ValueError, match="mask shape"):
        rt.kspace_ampmix(x, x, torch.zeros((5, 4)), lam, perm, 3)
    with pytest.raises(ValueError, match="float32"):
        rt.kspace_ampmix(x, x.double(), m, lam, perm, 3)
    with pytest.raises(ValueError, match="does not match"):
        rt.kspace_ampmix(x, x[:1], m, lam, perm, 3)
    with pytest.raises(ValueError, match="lam"):
        rt.kspace_ampmix(x, x, m, torch.zeros((3,)), perm, 3)
    with pytest.raises(ValueError, match="lam"):
        rt.kspace_ampmix(x, x, m, 0.5, perm, 3)
    with pytest.raises(ValueError, match="perm"):
        rt.kspace_ampmix(x, x, m, lam, perm.long(), 3)
    with pytest.raises(ValueError, match="perm"):
        rt.kspace_ampmix(x, x, m, lam, torch.zeros((3,), dtype=torch.int32), 3)
    with pytest.raises(ValueError, match="upstream"):
        rt.kspace_ampmix_grad(x, x, m, lam, perm, x[:1], 3)
    with pytest.raises(TexbiasError, match="HIP"):                 # no CPU fallback
        rt.kspace_ampmix(x, x, m, lam, perm, 3)
    with pytest.raises(TexbiasError, match="HIP"):
        rt.kspace_ampmix_grad(x, x, m, lam, None, x, 3)
    with pytest.raises(TexbiasError, match="HIP"):
        A.amplitude_mix(x, x, m, 0.5)
    with pytest.raises(ValueError, match="mask"):
        A.amplitude_mix(x, x, torch.zeros((4,)), 0.5)
