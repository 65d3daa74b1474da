"""The accumulation order of k_conv_mfma_split (csrc/conv_up.hip) restated in numpy, with the model of
tests/test_split_bf16_cpu.py: per channel group 432 k = 27 taps x 16 channels in 14 six-product steps of 32 k
(tap 27 zero), the group's partial hi + lo rounded to f32; then the G partials summed in group order, then the
bias -- against the f32 MFMA chain restated the same way (108 steps of k = 4 per group, the same final sums)."""
import numpy as np
import pytest
from test_split_bf16_cpu import dot_f32, dot_split

KG, NDOT = 432, 6000  # k per channel group; dot products


def conv_sum(dot, x, w, bias):
    """x, w [NDOT][G][432], bias [NDOT]: ((p_0 + p_1) + .. + p_(G-1)) + bias in f32, p_g the group's dot product"""
    v = dot(x[:, 0], w[:, 0])
    for g in range(1, x.shape[1]):
        v = (v + dot(x[:, g], w[:, g])).astype(np.float32)
    return (v + bias).astype(np.float32)


@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("scale", [1.0, 30.0, 1e-6, 2.0 ** -100])
def test_group_sums_no_worse_than_f32_chain(G, scale):
    rng = np.random.default_rng(1)
    x = (rng.standard_normal((NDOT, G, KG)) * scale).astype(np.float32)
    w = (rng.uniform(-1, 1, (NDOT, G, KG)) / np.sqrt(G * KG)).astype(np.float32)
    bias = (rng.standard_normal(NDOT) * scale).astype(np.float32)
    ref = (x.astype(np.float64) * w.astype(np.float64)).sum((-1, -2)) + bias.astype(np.float64)
    top = np.abs(ref).max()
    e_split = np.abs(conv_sum(dot_split, x, w, bias).astype(np.float64) - ref).max() / top
    e_f32 = np.abs(conv_sum(dot_f32, x, w, bias).astype(np.float64) - ref).max() / top
    print(f"G {G} scale {scale:.3e}: split {e_split:.2e}, f32 chain {e_f32:.2e} of max|y| "
          f"(ratio {e_split / e_f32:.2f})")
    assert e_split <= e_f32
