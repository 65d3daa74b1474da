"""Float64 references of amplitude mixing in k-space (test infrastructure).

``reference``: the definition, composed from ``torch.fft`` (differentiable, so ``torch.autograd`` gives the
reference gradients):

    X = fftshift(fftn(x)),  Y = fftshift(fftn(y[perm]))
    K = polar((1 - m) |X| + m |Y|, angle(X)),  m = lam[b] M
    out = ifftn(ifftshift(K)).real

``closed_form`` / ``closed_form_grads``: what the kernels evaluate (csrc/ampmix.h), written with numpy on the
full unshifted spectrum: the symmetrised mask, X' = (1 - m_s) X + m_s |Y| u, and the analytic gradients.
``composed_f32``: the same composition as ``reference`` in float32, the yardstick for what float32 can hold.
"""
from __future__ import annotations

import numpy as np
import torch


def _axes(n_dims):
    return tuple(range(-n_dims, 0))


def _mask_b(mask, lam, x, n_dims):
    """m[b, c, *spatial] = lam[b] * M, M of shape spatial or (C,) + spatial."""
    lam = lam.reshape((-1,) + (1,) * (x.dim() - 1))
    m = mask if mask.dim() == n_dims else mask.unsqueeze(0)
    return lam * m


def reference(x, y, mask, lam, perm=None, n_dims=3, dtype=torch.float64):
    """x, y: [B, C, *spatial] torch tensors (y may be x); mask: spatial or (C,) + spatial; lam: [B];
    perm: [B] integer partner indices or None.  Computed in ``dtype``."""
    ax = _axes(n_dims)
    cd = torch.complex128 if dtype == torch.float64 else torch.complex64
    x = x.to(dtype)
    y = y.to(dtype)
    yp = y if perm is None else y[torch.as_tensor(np.asarray(perm), dtype=torch.long)]
    m = _mask_b(mask.to(dtype), lam.to(dtype), x, n_dims)
    X = torch.fft.fftshift(torch.fft.fftn(x, dim=ax), dim=ax)
    Y = torch.fft.fftshift(torch.fft.fftn(yp, dim=ax), dim=ax)
    K = torch.polar((1 - m) * X.abs() + m * Y.abs(), torch.angle(X)).to(cd)
    return torch.fft.ifftn(torch.fft.ifftshift(K, dim=ax), dim=ax).real


def reference_np(x, y, mask, lam, perm=None, n_dims=3):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    return reference(t(x), t(y), t(mask), t(lam), perm, n_dims).numpy()


def reference_grads(x, y, mask, lam, g, perm=None, n_dims=3, dtype=torch.float64):
    """(out, gx, gy) of ``reference`` by torch.autograd for the upstream gradient g; x and y are separate
    leaves (pass clones for batch-internal mixing and add the two gradients)."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)  # noqa: E731
    xt = t(x).requires_grad_(True)
    yt = t(y).requires_grad_(True)
    out = reference(xt, yt, t(mask), t(lam), perm, n_dims, dtype)
    gx, gy = torch.autograd.grad(out, (xt, yt), t(g))
    return out.detach().numpy(), gx.numpy(), gy.numpy()


def composed_f32(x, y, mask, lam, g=None, perm=None, n_dims=3):
    """The float32 ``torch.fft`` composition of the reference: out, or (out, gx, gy) with g."""
    if g is None:
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))  # noqa: E731
        return reference(t(x), t(y), t(mask), t(lam), perm, n_dims, torch.float32).numpy()
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    return reference_grads(f(x), f(y), f(mask), f(lam), f(g), perm, n_dims, torch.float32)


def _sym_mask(mask, lam, shape, n_dims):
    """m_s on the unshifted full spectrum, [B, C, *spatial]: lam[b] (M[s(f)] + M[s(-f)]) / 2."""
    ax = _axes(n_dims)
    M = np.asarray(mask, np.float64)
    if M.ndim == n_dims:
        M = M[None]
    Mu = np.fft.ifftshift(M, axes=ax)                              # M at the unshifted f
    Mn = np.roll(np.flip(Mu, axis=ax), 1, axis=ax)                 # M at -f
    ms = 0.5 * (Mu + Mn)
    lam = np.asarray(lam, np.float64).reshape((-1,) + (1,) * (len(shape) - 1))
    return lam * ms[None]


def closed_form(x, y, mask, lam, perm=None, n_dims=3):
    ax = _axes(n_dims)
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    yp = y if perm is None else y[np.asarray(perm)]
    X, Y = np.fft.fftn(x, axes=ax), np.fft.fftn(yp, axes=ax)
    ms = _sym_mask(mask, lam, x.shape, n_dims)
    aX = np.abs(X)
    u = np.where(aX > 0, X / np.where(aX > 0, aX, 1.0), 1.0)
    Xp = (1 - ms) * X + ms * np.abs(Y) * u
    out = np.fft.ifftn(Xp, axes=ax)
    return out.real, float(np.max(np.abs(out.imag)))


def closed_form_grads(x, y, mask, lam, g, perm=None, n_dims=3):
    """(gx, gy) by the closed form; gy summed over equal partners in the order of b."""
    ax = _axes(n_dims)
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    p = np.arange(x.shape[0]) if perm is None else np.asarray(perm)
    X, Y, G = np.fft.fftn(x, axes=ax), np.fft.fftn(y[p], axes=ax), np.fft.fftn(np.asarray(g, np.float64), axes=ax)
    ms = _sym_mask(mask, lam, x.shape, n_dims)
    aX, aY = np.abs(X), np.abs(Y)
    u = np.where(aX > 0, X / np.where(aX > 0, aX, 1.0), 1.0)
    v = np.where(aY > 0, Y / np.where(aY > 0, aY, 1.0), 0.0)
    ratio = np.where(aX > 0, aY / np.where(aX > 0, aX, 1.0), 0.0)
    c = (np.conj(u) * G).real
    Gx = (1 - ms) * G + ms * ratio * (G - u * c)
    Gy = ms * c * v
    gx = np.fft.ifftn(Gx, axes=ax).real
    gyb = np.fft.ifftn(Gy, axes=ax).real
    gy = np.zeros_like(y)
    for b in range(x.shape[0]):
        gy[p[b]] += gyb[b]
    return gx, gy


def spiked(shape, n_dims, seed, where):
    """randn + 6 sqrt(N) delta(p), p_a = n_a // 3 (where = 1) or (2 n_a) // 3 (where = 2): amplitudes kept
    away from 0 while the phases vary over the whole circle."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(shape)
    sp = shape[len(shape) - n_dims:]
    idx = tuple((where * n) // 3 for n in sp)
    a[(Ellipsis,) + idx] += 6.0 * np.sqrt(float(np.prod(sp)))
    return a.astype(np.float32)
