"""Float64 restatement of the trainable spike layer (include/texbias.h, csrc/spike_grad.h) -- test infrastructure.

``reference``: the reference's own expression (KSpaceSpikeNoise._set_spike, filters_and_operators.py:966-983, as
spike_layer.forward applies it, stylization_layers.py:143-151) with ``torch.fft`` in float64 and a float64 leaf I:
log(|k| + 1e-10) / angle / exp with the spike written into the log-amplitude of the centred spectrum, then
``.real`` of the inverse; ``torch.autograd`` gives its gradients.

``closed_form``: the formulas the kernels implement, in numpy float64.  With f_j the unshifted frequency of spike
j, theta_j(n) = 2 pi sum_a f_a n_a / N_a, K_j = sum_n x[n] e^{-i theta_j(n)} per volume-channel, A_j = exp(I_j),
m = |K_j|, u = K_j / m (1 where m = 0):
  y  = x + Re(sum_j (A_j u - K_j) e^{i theta_j}) / N
  G_j = sum_n g[n] e^{-i theta_j(n)},  p + i q = conj(u) G_j
  dI_j = sum_{b,c} A_j p / N
  gx = g + Re(sum_j Gamma_j e^{i theta_j}) / N,  Gamma_j = u (-p + i q (A_j / m - 1))   (-G_j where m = 0)
"""
import numpy as np
import torch


def unshift(loc, spatial):
    return tuple((int(s) - n // 2) % n for s, n in zip(loc, spatial))


def reference(x, I, locs, n_dims):
    """x float64 [*lead, *spatial] and I float64 [S] (torch, either may require grad) -> y."""
    dims = tuple(range(-n_dims, 0))
    k = torch.fft.fftshift(torch.fft.fftn(x, dim=dims), dim=dims)
    log_abs = torch.log(torch.abs(k) + 1e-10)
    phase = torch.angle(k)
    log_abs = log_abs.clone()
    for j, loc in enumerate(locs):
        log_abs[(Ellipsis,) + tuple(int(v) for v in loc)] = I[j]
    k2 = torch.exp(log_abs) * torch.exp(1j * phase)
    return torch.fft.ifftn(torch.fft.ifftshift(k2, dim=dims), dim=dims).real


def reference_grads(x, g, I, locs, n_dims):
    """(y, gx, dI) of ``reference`` for the upstream gradient g, numpy float64 in and out."""
    xt = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    It = torch.tensor(np.asarray(I, np.float64), requires_grad=True)
    y = reference(xt, It, locs, n_dims)
    gx, dI = torch.autograd.grad(y, (xt, It), torch.tensor(np.asarray(g, np.float64)))
    return y.detach().numpy(), gx.numpy(), dI.numpy()


def plane(loc, spatial):
    """e^{i theta(n)} over ``spatial`` for the centred location ``loc``."""
    th = np.zeros(spatial, np.float64)
    for a, (f, n) in enumerate(zip(unshift(loc, spatial), spatial)):
        ax = (f * np.arange(n, dtype=np.int64)) % n  # exact phase index
        th = th + (2.0 * np.pi * ax / n).reshape([-1 if i == a else 1 for i in range(len(spatial))])
    return np.exp(1j * th)


def spike_delta(K, A):
    """Delta = A u - K (numpy, elementwise)."""
    m = np.abs(K)
    u = np.where(m > 0, K / np.where(m > 0, m, 1.0), 1.0)
    return A * u - K


def spike_gamma(K, G, A):
    """(Gamma, A p): the image-gradient coefficient and the dI share (numpy, elementwise)."""
    m = np.abs(K)
    ms = np.where(m > 0, m, 1.0)
    u = np.where(m > 0, K / ms, 1.0)
    c = np.conj(u) * G
    p, q = c.real, c.imag
    gam = np.where(m > 0, u * (-p + 1j * q * (A / ms - 1.0)), -G)
    return gam, A * p


def closed_form(x, g, I, locs, n_dims):
    """numpy float64: dict with y, gx, dI, K, G [*lead, S] and dI_scale[j] = sum_{b,c} A_j |G_j| / N."""
    x, g, I = np.asarray(x, np.float64), np.asarray(g, np.float64), np.asarray(I, np.float64)
    spatial = x.shape[x.ndim - n_dims:]
    axes = tuple(range(x.ndim - n_dims, x.ndim))
    N = float(np.prod(spatial))
    y, gx = x.copy(), g.copy()
    Ks, Gs, dI, scale = [], [], [], []
    for j, loc in enumerate(locs):
        e = plane(loc, spatial)
        A = np.exp(I[j])
        K = (x * np.conj(e)).sum(axes)
        G = (g * np.conj(e)).sum(axes)
        sh = (...,) + (None,) * n_dims
        y += (spike_delta(K, A)[sh] * e).real / N
        gam, ap = spike_gamma(K, G, A)
        gx += (gam[sh] * e).real / N
        dI.append(ap.sum() / N)
        scale.append((A * np.abs(G)).sum() / N)
        Ks.append(K)
        Gs.append(G)
    return {"y": y, "gx": gx, "dI": np.array(dI), "K": np.stack(Ks, -1), "G": np.stack(Gs, -1),
            "dI_scale": np.array(scale)}


def centre(spatial):
    """The centred index of DC."""
    return tuple(n // 2 for n in spatial)


def nyquist(spatial):
    """The centred index of the Nyquist frequency on every even axis (DC on the odd ones): self-conjugate."""
    return tuple(0 if n % 2 == 0 else n // 2 for n in spatial)


def self_conjugate(loc, spatial):
    """The centred location's frequency is its own conjugate (DC, or Nyquist, on every axis)."""
    f = unshift(loc, spatial)
    return all((n - k) % n == k for k, n in zip(f, spatial))


def set_coefficient(ky, kx, loc, spatial):
    """The coefficient the layer set at ``loc``, from the centred spectra of y and x: ``.real`` halves the change
    of a coefficient whose conjugate partner was left alone, FFT(y)(f) = (A u + K) / 2, so c = 2 ky - kx there; at a
    self-conjugate f it is ky itself.  |c| = A and c has the phase of kx."""
    idx = (Ellipsis,) + tuple(int(v) for v in loc)
    return ky[idx] if self_conjugate(loc, spatial) else 2.0 * ky[idx] - kx[idx]
