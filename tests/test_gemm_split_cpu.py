"""The split-precision tile of csrc/gemm_core.h (SplitTile) restated in numpy, against the f32 tile (Tile) it
stands beside, at the reduction lengths of the conv GEMMs (K = Cin x taps: 8 x 27, 128 x 9 ... 256 x 27).

SplitTile, as built: a stage is 32 k (K zero-padded to it) and runs as two 16-k steps in k order; in a step
the five small part products a1 b1, a0 b2, a2 b0, a0 b1, a1 b0 go, in that order, into `lo` and a0 b0 into `hi`,
each one v_mfma_f32_32x32x16_bf16 (16 products and the accumulator summed, rounded to f32 once); hi + lo is
taken once at the end, then the bias is added (the kernel's store).  Tile: per stage the sixteen
mfma_f32_32x32x2f32 pair element 8 h + st with element 16 + 8 h + st (h = 0, 1; st = 0 .. 7): one rounding per
2 k; the bias is added at the store as well.

The helpers (split3, mfma) are those of tests/test_split_bf16_cpu.py."""
import numpy as np
import pytest

from test_split_bf16_cpu import mfma, split3

NDOT = 3000


def dot_split_tile(a, b, bias):
    pad = (-a.shape[-1]) % 32
    a, b = np.pad(a, ((0, 0), (0, pad))), np.pad(b, ((0, 0), (0, pad)))
    A, B = split3(a), split3(b)
    hi, lo = np.zeros(a.shape[0], np.float32), np.zeros(a.shape[0], np.float32)
    for k in range(0, a.shape[-1], 16):
        s = slice(k, k + 16)
        for i, j in ((1, 1), (0, 2), (2, 0), (0, 1), (1, 0)):
            lo = mfma(lo, A[i][:, s], B[j][:, s])
        hi = mfma(hi, A[0][:, s], B[0][:, s])
    return (hi + lo) + bias


def dot_f32_tile(a, b, bias):
    pad = (-a.shape[-1]) % 32
    a, b = np.pad(a, ((0, 0), (0, pad))), np.pad(b, ((0, 0), (0, pad)))
    acc = np.zeros(a.shape[0], np.float32)
    for k in range(0, a.shape[-1], 32):
        for h in range(2):
            for st in range(8):
                e = [k + 8 * h + st, k + 16 + 8 * h + st]
                acc = mfma(acc, a[:, e], b[:, e])
    return acc + bias


def operands(cls, K, rng):
    if cls == "positive":  # both operands positive with mean 3: every partial sum grows, no cancellation
        return rng.uniform(2, 4, (NDOT, K)).astype(np.float32), rng.uniform(2, 4, (NDOT, K)).astype(np.float32)
    a = (rng.standard_normal((NDOT, K)) * cls).astype(np.float32)
    b = (rng.uniform(-1, 1, (NDOT, K)) / np.sqrt(K)).astype(np.float32)
    return a, b


@pytest.mark.parametrize("K", [216, 1152, 4512, 6912])
@pytest.mark.parametrize("cls", [1.0, 2.0 ** -100, 2.0 ** 60, "positive"])
def test_split_tile_no_worse_than_f32_tile(K, cls):
    rng = np.random.default_rng(K)
    a, b = operands(cls, K, rng)
    ref = (a.astype(np.float64) * b.astype(np.float64)).sum(-1)
    bias = (rng.standard_normal(NDOT) * np.abs(ref).mean()).astype(np.float32)
    ref = ref + bias
    top = np.abs(ref).max()
    e_split = np.abs(dot_split_tile(a, b, bias).astype(np.float64) - ref).max() / top
    e_f32 = np.abs(dot_f32_tile(a, b, bias).astype(np.float64) - ref).max() / top
    print(f"K {K} class {cls}: split tile {e_split:.2e}, f32 tile {e_f32:.2e} of max|y|, ratio {e_f32 / e_split:.2f}")
    assert e_split <= e_f32
