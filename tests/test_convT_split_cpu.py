"""The step tables and the accumulation order of k_convT_split (csrc/conv_up.hip) restated in numpy, with the
model of tests/test_split_bf16_cpu.py.

ConvTranspose3d(3, stride 2, padding 1, output_padding 1) puts input i and tap t at output 2 i + t - 1 per axis:
tap 1 -> parity 0 of position i (offset 0), tap 2 -> parity 1 of position i (offset 0), tap 0 -> parity 1 of
position i - 1 (the output's position reads its neighbour at offset +1).  The 8 parity classes (pz py px) so own
1, 2, 2, 4, 2, 4, 4, 8 taps.  The kernel pairs a class's taps into 32-k steps (two taps x the 16 channels of one
channel group; class 0's second tap has zero weights): 14 steps per group, 7 on each of a group's two waves
(classes 7, 3, 0 and 5, 6, 1, 2, 4).  Per class and group a (hi, lo) accumulator pair, hi + lo rounded once;
then the four groups in order, then the bias.

Checks: the tables place every tap exactly once, in the class and at the offset the stride-2 geometry (and
tap_of(kind = 2) of csrc/conv_gemm.hip, restated) gives it; a small integer volume run through the tables
equals the layer's definition; the restated order's worst error is no larger than the f32 MFMA chain's
(k_convT_mfma64: per class and group a chain of k = 4 steps, the bias first, then the groups in order)."""
import numpy as np
import pytest
from test_split_bf16_cpu import dot_f32, dot_split

G, NDOT = 4, 4000


def tap_of2(cls, j):
    """tap_of(kind = 2, cls, j) of csrc/conv_gemm.hip: (dz, dy, dx, weight index)"""
    pz, py, px = (cls >> 2) & 1, (cls >> 1) & 1, cls & 1
    nx, ny = 1 + px, 1 + py
    ix, iy, iz = j % nx, (j // nx) % ny, j // (nx * ny)
    tz, ty, tx = ((0 if iz else 2) if pz else 1), ((0 if iy else 2) if py else 1), ((0 if ix else 2) if px else 1)
    return (iz if pz else 0, iy if py else 0, ix if px else 0, tz * 9 + ty * 3 + tx)


def ntap(cls):
    return (1 + ((cls >> 2) & 1)) * (1 + ((cls >> 1) & 1)) * (1 + (cls & 1))


HALVES = ((7, 7, 7, 7, 3, 3, 0), (5, 5, 6, 6, 1, 2, 4))  # ct_cls(half, s)
PAIRS = ((0, 1, 2, 3, 0, 1, 0), (0, 1, 0, 1, 0, 0, 0))   # ct_pair(half, s)


def steps():
    """(class, [(tap of lane half 0), (tap of lane half 1) or None]) of the 14 steps"""
    out = []
    for h in range(2):
        for cls, pr in zip(HALVES[h], PAIRS[h]):
            taps = [tap_of2(cls, 2 * pr + hi) if 2 * pr + hi < ntap(cls) else None for hi in range(2)]
            out.append((cls, taps))
    return out


def test_every_tap_once_at_its_offset():
    seen = {}
    per_cls = {c: 0 for c in range(8)}
    for cls, taps in steps():
        per_cls[cls] += 1
        assert taps[0] is not None
        for t in taps:
            if t is None:
                assert cls == 0  # only the single-tap class is padded
                continue
            dz, dy, dx, wi = t
            assert wi not in seen
            seen[wi] = (cls, dz, dy, dx)
    assert sorted(seen) == list(range(27))
    assert [per_cls[c] for c in range(8)] == [1, 1, 1, 2, 1, 2, 2, 4] and sum(per_cls.values()) == 14
    for wi, (cls, dz, dy, dx) in seen.items():
        for t, par, d in ((wi // 9, (cls >> 2) & 1, dz), ((wi // 3) % 3, (cls >> 1) & 1, dy), (wi % 3, cls & 1, dx)):
            assert (par, d) == {1: (0, 0), 2: (1, 0), 0: (1, 1)}[t]  # output 2 i + t - 1


def test_tables_compute_the_layer():
    """Integer data on a 3 x 2 x 3 volume, 2 channels -> 2: the classes' tap lists reproduce the definition
    y[m][2 i + t - 1] += W[c][m][t] x[c][i] exactly."""
    rng = np.random.default_rng(3)
    D, H, W, C, M = 3, 2, 3, 2, 2
    x = rng.integers(-4, 5, (C, D, H, W)).astype(np.float64)
    w = rng.integers(-2, 3, (C, M, 27)).astype(np.float64)
    ref = np.zeros((M, 2 * D, 2 * H, 2 * W))
    for z in range(D):
        for y in range(H):
            for xx in range(W):
                for t in range(27):
                    oz, oy, ox = 2 * z + t // 9 - 1, 2 * y + (t // 3) % 3 - 1, 2 * xx + t % 3 - 1
                    if 0 <= oz < 2 * D and 0 <= oy < 2 * H and 0 <= ox < 2 * W:
                        ref[:, oz, oy, ox] += w[:, :, t].T @ x[:, z, y, xx]
    xp = np.pad(x, ((0, 0), (0, 1), (0, 1), (0, 1)))  # the zero neighbours at + 1
    out = np.zeros_like(ref)
    for cls, taps in steps():
        pz, py, px = (cls >> 2) & 1, (cls >> 1) & 1, cls & 1
        for t in taps:
            if t is None:
                continue
            dz, dy, dx, wi = t
            out[:, pz::2, py::2, px::2] += np.einsum("cm,czyx->mzyx", w[:, :, wi],
                                                     xp[:, dz:dz + D, dy:dy + H, dx:dx + W])
    assert np.array_equal(out, ref)


def class_sum(dot, x, w, bias, bias_first):
    """x, w [NDOT][G][k]: the G group dot products in group order and the bias, in f32"""
    if bias_first:  # k_convT_mfma64: v = bias, += group partials
        v = bias.copy()
        for g in range(G):
            v = (v + dot(x[:, g], w[:, g])).astype(np.float32)
        return v
    v = dot(x[:, 0], w[:, 0])
    for g in range(1, G):
        v = (v + dot(x[:, g], w[:, g])).astype(np.float32)
    return (v + bias).astype(np.float32)


@pytest.mark.parametrize("scale", [1.0, 30.0, 1e-6, 2.0 ** -100])
def test_order_no_worse_than_f32_chain(scale):
    rng = np.random.default_rng(1)
    e_split = e_f32 = top = 0.0
    for cls in range(8):
        k = 16 * ntap(cls)  # per group; dot_split pads class 0's 16 k to the 32-k step with zeros
        x = (rng.standard_normal((NDOT, G, k)) * scale).astype(np.float32)
        w = (rng.uniform(-1, 1, (NDOT, G, k)) / np.sqrt(G * k)).astype(np.float32)
        bias = (rng.standard_normal(NDOT) * scale).astype(np.float32)
        ref = (x.astype(np.float64) * w.astype(np.float64)).sum((-1, -2)) + bias.astype(np.float64)
        top = max(top, np.abs(ref).max())
        e_split = max(e_split, np.abs(class_sum(dot_split, x, w, bias, False).astype(np.float64) - ref).max())
        e_f32 = max(e_f32, np.abs(class_sum(dot_f32, x, w, bias, True).astype(np.float64) - ref).max())
    print(f"scale {scale:.3e}: split {e_split / top:.2e}, f32 chain {e_f32 / top:.2e} of max|y| "
          f"(ratio {e_split / e_f32:.2f})")
    assert e_split <= e_f32
