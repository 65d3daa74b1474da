"""csrc/split_bf16.h restated in numpy: the three-part bf16 split of an f32 value and the six-product 32-k
accumulation step of k_conv16_split, against the f32 MFMA chain it replaces (k = 4 per accumulation step).

Model of one MFMA (either kind): the k products of the step and the accumulator are summed exactly and rounded
to f32 once.  bf16 x bf16 products are exact in f32, f32 x f32 products are taken exactly (float64)."""
import numpy as np
import pytest

K, NDOT = 432, 20000  # 27 taps x 16 channels; dot products


TOP = np.array([0x7F7F7FFF], np.uint32).view(np.float32)[0]  # the largest f32 that rounds to a finite bf16


def rne_bf16(x):
    """f32 -> nearest-even bf16, as an f32 value (v_cvt_pk_bf16_f32 on finite values)"""
    u = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def split3(x):
    x = x.astype(np.float32)
    x0 = rne_bf16(np.clip(x, -TOP, TOP))  # the leading part: never infinite for finite x
    r1 = x - x0  # exact: the 16 significand bits below it
    x1 = rne_bf16(r1)
    r2 = r1 - x1  # exact
    x2 = rne_bf16(r2)
    return x0, x1, x2


def mfma(acc, a, b):
    """acc (f32) + sum_k a b, summed exactly, rounded to f32 once"""
    return (acc.astype(np.float64) + (a.astype(np.float64) * b.astype(np.float64)).sum(-1)).astype(np.float32)


def dot_split(a, b):
    """the kernel's order: per 32-k step a1 b1, a0 b2, a2 b0, a0 b1, a1 b0 into `lo` (smallest first) and
    a0 b0 into `hi`, each an MFMA of its own; hi + lo at the end"""
    pad = (-a.shape[-1]) % 32
    a, b = np.pad(a, ((0, 0), (0, pad))), np.pad(b, ((0, 0), (0, pad)))
    A, B = split3(a), split3(b)
    hi, lo = np.zeros(a.shape[0], np.float32), np.zeros(a.shape[0], np.float32)
    for k in range(0, a.shape[-1], 32):
        s = slice(k, k + 32)
        for i, j in ((1, 1), (0, 2), (2, 0), (0, 1), (1, 0)):
            lo = mfma(lo, A[i][:, s], B[j][:, s])
        hi = mfma(hi, A[0][:, s], B[0][:, s])
    return hi + lo


def dot_f32(a, b):
    acc = np.zeros(a.shape[0], np.float32)
    for k in range(0, a.shape[-1], 4):
        acc = mfma(acc, a[:, k:k + 4], b[:, k:k + 4])
    return acc


def test_parts_sum_exactly():
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(200000) * np.exp(rng.uniform(-60, 60, 200000))).astype(np.float32)
    fmax = np.finfo(np.float32).max
    x = np.concatenate([x, np.float32([0.0, -0.0, 1.0, -1.0, fmax, -fmax, np.nextafter(np.float32(1), np.float32(2)),
                                       2.0 ** -100, 3.0 * 2.0 ** -110, 16777215.0, 1.0 - 2.0 ** -24])])
    x0, x1, x2 = split3(x)
    assert np.all(np.isfinite(x0)) and np.all(np.isfinite(x1)) and np.all(np.isfinite(x2))
    assert np.array_equal(x0.astype(np.float64) + x1.astype(np.float64) + x2.astype(np.float64), x.astype(np.float64))
    for p in (x0, x1, x2):  # each part is a bf16: its low 16 bits are clear
        assert not np.any(p.view(np.uint32) & np.uint32(0xFFFF))
    nz = x != 0
    assert np.all(np.abs(x1[nz]) <= np.abs(x[nz]) * 2.0 ** -7) and np.all(np.abs(x2[nz]) <= np.abs(x[nz]) * 2.0 ** -15)


@pytest.mark.parametrize("scale", [1.0, 30.0, 1e-6, 2.0 ** -100])
def test_six_products_no_worse_than_f32_chain(scale):
    rng = np.random.default_rng(1)
    a = (rng.standard_normal((NDOT, K)) * scale).astype(np.float32)
    b = (rng.uniform(-1, 1, (NDOT, K)) / np.sqrt(K)).astype(np.float32)
    ref = (a.astype(np.float64) * b.astype(np.float64)).sum(-1)
    top = np.abs(ref).max()
    e_split = np.abs(dot_split(a, b).astype(np.float64) - ref).max() / top
    e_f32 = np.abs(dot_f32(a, b).astype(np.float64) - ref).max() / top
    print(f"scale {scale:.3e}: six-product split bf16 {e_split:.2e}, f32 chain {e_f32:.2e} of max|y|")
    assert e_split <= e_f32
