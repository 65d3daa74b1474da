"""Numpy restatement of the radial-profile semantics (include/texbias.h, csrc/radial.h) -- test infrastructure.

Element s of the centred layout has signed index k_a = s_a - floor(n_a / 2); r2 = sum k_a^2 (exact integer);
u = f32_sqrt((float)r2) * inv_dr with inv_dr = (float)(1.0 / dr): one correctly rounded float32 square root and
one float32 multiply, so numpy and the device agree bit for bit.  Modes over K bins:
  nearest (0)  b = min((int)u, K-1), weight 1
  linear  (1)  b0 = (int)u; b0 >= K-1: weight 1 on K-1; else t = u - (float)b0, 1-t on b0 and t on b0+1
Everything downstream of the float32 weights is float64.
"""
import numpy as np

NEAREST, LINEAR = 0, 1


def weights(spatial, K, dr, mode):
    """(b0 int64, w0 float32, w1 float32) over the centred layout ``spatial``; the second bin is b0 + 1."""
    spatial = tuple(int(n) for n in spatial)
    r2 = np.zeros(spatial, np.int64)
    for a, n in enumerate(spatial):
        k = (np.arange(n, dtype=np.int64) - n // 2) ** 2
        r2 = r2 + k.reshape([-1 if i == a else 1 for i in range(len(spatial))])
    u = np.sqrt(r2.astype(np.float32)) * np.float32(1.0 / float(dr))
    assert u.dtype == np.float32
    clamp = ~(u < np.float32(K - 1))
    b0 = np.where(clamp, K - 1, np.where(clamp, 0, u).astype(np.int64))
    if mode == NEAREST:
        return b0, np.ones(spatial, np.float32), np.zeros(spatial, np.float32)
    t = (u - b0.astype(np.float32)).astype(np.float32)
    w1 = np.where(clamp, np.float32(0), t).astype(np.float32)
    w0 = np.where(clamp, np.float32(1), np.float32(1) - t).astype(np.float32)
    return b0, w0, w1


def expand(p, spatial, dr, mode):
    """p [K] or [C, K] -> float64 mask ``spatial`` or (C,) + spatial."""
    p = np.asarray(p, np.float64)
    K = p.shape[-1]
    b0, w0, w1 = weights(spatial, K, dr, mode)
    b1 = np.minimum(b0 + 1, K - 1)
    return w0.astype(np.float64) * p[..., b0] + w1.astype(np.float64) * p[..., b1]


def bin_(A, n_dims, K, dr, mode):
    """A [*lead, *spatial] -> float64 [*lead, K]: the adjoint of ``expand``."""
    A = np.asarray(A, np.float64)
    spatial = A.shape[A.ndim - n_dims:]
    b0, w0, w1 = weights(spatial, K, dr, mode)
    b1 = np.minimum(b0 + 1, K - 1).ravel()
    b0, w0, w1 = b0.ravel(), w0.ravel().astype(np.float64), w1.ravel().astype(np.float64)
    flat = A.reshape((-1, b0.size))
    out = np.stack([np.bincount(b0, w0 * v, K) + np.bincount(b1, w1 * v, K) for v in flat])
    return out.reshape(A.shape[: A.ndim - n_dims] + (K,))


def power(x, n_dims, K, dr, mode):
    """Float64 shell power spectrum [*lead, K] of x [*lead, *spatial]."""
    ax = tuple(range(-n_dims, 0))
    X = np.fft.fftn(np.asarray(x, np.float64), axes=ax)
    v = np.fft.fftshift(X.real ** 2 + X.imag ** 2, axes=ax) / np.prod(x.shape[-n_dims:])
    return bin_(v, n_dims, K, dr, mode)


def mask_grad(x, g, n_dims, per_channel):
    """Float64 dM of tests/test_emu_mask_grad.py: x, g [B, C, *spatial]."""
    ax = tuple(range(-n_dims, 0))
    X = np.fft.fftn(np.asarray(x, np.float64), axes=ax)
    G = np.fft.fftn(np.asarray(g, np.float64), axes=ax)
    v = np.fft.fftshift((X * np.conj(G)).real, axes=ax) / np.prod(x.shape[-n_dims:])
    return v.sum(axis=0) if per_channel else v.sum(axis=(0, 1))


def grad(x, g, n_dims, per_channel, K, dr, mode):
    """Float64 profile gradient [K] or [C, K]."""
    return bin_(mask_grad(x, g, n_dims, per_channel), n_dims, K, dr, mode)
