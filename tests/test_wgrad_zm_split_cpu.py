"""The accumulation order of k_conv3d_wgrad_zm_split (csrc/conv_wgrad.hip) restated in numpy, with the model of
tests/test_split_bf16_cpu.py, at the 32 -> 32 layer of the C3 step (2 x 60 x 60 x 40: z segments of 30 planes, 60
workgroups per tile): a plane's 4 x 40 positions are five 32-position steps, wave phase p of the four takes steps
p and p + 4, so over the segment a wave chains 60 or 30 six-product steps into its hi and lo; hi + lo once; the
phases meet as (p0 + p2) + (p1 + p3); k_wgrad_reduce then sums the workgroups' partial tiles (16 groups of every
16th workgroup, four interleaved sums where the group has them, the groups in order).  Against the f32 kernel
restated the same way: a wave (row yy, half row) chains 5 k-steps of 4 positions per plane, the 8 waves meet as
(w0 + (w2 + (w4 + w6))) + (w1 + (w3 + (w5 + w7))), the same reduction."""
import numpy as np
import pytest
from test_split_bf16_cpu import dot_f32, dot_split

ZLEN, NBLK, ROWS, W, NDOT = 30, 60, 4, 40, 24  # planes per segment, workgroups per tile, rows, row width; dot products


def f32(x):
    return x.astype(np.float32)


def block_split(a, b):
    """a, b [NDOT][ZLEN][ROWS * W]: one workgroup's sum on the split kernel"""
    steps = a.shape[-1] // 32
    s = []
    for p in range(4):
        idx = np.concatenate([np.arange(32 * k, 32 * k + 32) for k in range(p, steps, 4)])
        s.append(dot_split(a[:, :, idx].reshape(a.shape[0], -1), b[:, :, idx].reshape(a.shape[0], -1)))
    return f32(f32(s[0] + s[2]) + f32(s[1] + s[3]))


def block_f32(a, b):
    """the same workgroup on k_conv3d_wgrad_zm: wave = (row yy = wave % 4, half = wave // 4)"""
    w = []
    for wave in range(8):
        yy, half = wave % 4, wave // 4
        idx = np.arange(yy * W + half * (W // 2), yy * W + (half + 1) * (W // 2))
        w.append(dot_f32(a[:, :, idx].reshape(a.shape[0], -1), b[:, :, idx].reshape(a.shape[0], -1)))
    lo = f32(w[0] + f32(w[2] + f32(w[4] + w[6])))
    hi = f32(w[1] + f32(w[3] + f32(w[5] + w[7])))
    return f32(lo + hi)


def reduce_blocks(part):
    """k_wgrad_reduce: part [NBLK][NDOT] -> [NDOT]"""
    nblk = part.shape[0]
    red = []
    for bg in range(16):
        s = [np.zeros(part.shape[1], np.float32) for _ in range(4)]
        b = bg
        while b + 48 < nblk:
            for i in range(4):
                s[i] = f32(s[i] + part[b + 16 * i])
            b += 64
        while b < nblk:
            s[0] = f32(s[0] + part[b])
            b += 16
        red.append(f32(f32(s[0] + s[1]) + f32(s[2] + s[3])))
    v = np.zeros(part.shape[1], np.float32)
    for g in range(16):
        v = f32(v + red[g])
    return v


@pytest.mark.parametrize("scale", [1.0, 30.0, 1e-6, 2.0 ** -100])
def test_segment_and_block_sums_no_worse_than_f32_chain(scale):
    rng = np.random.default_rng(3)
    n = ROWS * W
    a = (rng.standard_normal((NBLK, NDOT, ZLEN, n)) * scale).astype(np.float32)
    b = (rng.uniform(-1, 1, (NBLK, NDOT, ZLEN, n)) / np.sqrt(NBLK * ZLEN * n)).astype(np.float32)
    ref = (a.astype(np.float64) * b.astype(np.float64)).sum((0, 2, 3))
    top = np.abs(ref).max()
    split = reduce_blocks(np.stack([block_split(a[i], b[i]) for i in range(NBLK)]))
    chain = reduce_blocks(np.stack([block_f32(a[i], b[i]) for i in range(NBLK)]))
    e_split = np.abs(split.astype(np.float64) - ref).max() / top
    e_f32 = np.abs(chain.astype(np.float64) - ref).max() / top
    print(f"scale {scale:.3e}: split {e_split:.2e}, f32 chain {e_f32:.2e} of max|dW| (ratio {e_split / e_f32:.2f})")
    assert e_split <= e_f32
