"""Amplitude mixing in k-space on the native passes (Fourier domain adaptation, amplitude mix / swap).

The standard Fourier tool against a network leaning on scanner texture keeps an image's *phase* (anatomy,
shape) and replaces or interpolates its *amplitude* (contrast, texture) with that of a second image, usually
only in a low-frequency box:

    X = fftshift(fftn(x)),  Y = fftshift(fftn(y))
    out = ifftn(ifftshift(polar((1 - m) |X| + m |Y|, angle(X)))).real,    m = lam * mask

Composed from ``Fourier.shift_fourier`` / ``inv_shift_fourier`` (filters_and_operators.py:594-632) with ``abs``,
``angle`` and ``polar`` it writes two full complex spectra and sweeps them several times; here it is one fused
sequence -- forward passes, one per-coefficient pass, one inverse pass -- that stores no spectrum outside the
workspace (``torch.ops.texbias.amp_mix``, csrc/ampmix.h), with analytic gradients with respect to both images.
``lam`` and the mask are constants: no gradient with respect to either.

  ``amplitude_mix(x, y, mask, lam, perm=None)``  the functional form on [B, C, *spatial] float32 HIP tensors
  ``lowfreq_box(spatial, beta)``                 the usual low-frequency box mask, symmetric about DC
  ``AmplitudeMix(mask_or_beta, lam)``            deterministic, for a pair of images or batches
  ``RandAmplitudeMix(mask_or_beta, lam_range, prob)``  a batch stage: every drawn sample is mixed with another
                                                 sample of the same batch, one launch sequence with y = x
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .transform_base import Randomizable, Transform


def _ops():
    from . import ops  # noqa: F401 - registers torch.ops.texbias.*
    return torch.ops.texbias


def lowfreq_box(spatial: Sequence[int], beta: float, device=None) -> torch.Tensor:
    """Float32 mask of shape ``spatial`` in the centred layout: 1 on [n_a // 2 - b, n_a // 2 + b] along every
    axis (clipped to the axis), 0 elsewhere, with b = max(1, floor(min(spatial) * beta)) -- the low-frequency
    box of the domain-adaptation recipes.  The box is centred on DC (index n_a // 2), so it is symmetric under
    f -> -f (the Nyquist index of an even axis is its own mirror)."""
    spatial = tuple(int(n) for n in spatial)
    if not spatial or min(spatial) < 1:
        raise ValueError(f"lowfreq_box: spatial must be positive sizes, got {spatial}")
    beta = float(beta)
    if not (beta >= 0.0) or not math.isfinite(beta):
        raise ValueError(f"lowfreq_box: beta must be a finite number >= 0, got {beta}")
    b = max(1, int(math.floor(min(spatial) * beta)))
    m = torch.ones(spatial, dtype=torch.float32)
    for a, n in enumerate(spatial):
        idx = torch.arange(n)
        inside = ((idx >= n // 2 - b) & (idx <= n // 2 + b)).to(torch.float32)
        m = m * inside.reshape([-1 if i == a else 1 for i in range(len(spatial))])
    return m if device is None else m.to(device)


def amplitude_mix(x: torch.Tensor, y: torch.Tensor, mask: torch.Tensor, lam: Union[float, torch.Tensor],
                  perm: Optional[torch.Tensor] = None, pad: int = 0) -> torch.Tensor:
    """Mix the amplitude of ``y[perm]`` into ``x`` ([B, C, *spatial], float32, HIP; the transformed axes are the
    mask's).  ``mask``: float32, ``spatial`` or ``(C,) + spatial``, centred layout, on x's device.  ``lam``: a
    number (uploaded once as a [B] tensor) or a float32 [B] tensor on x's device, one strength per sample.
    ``perm``: int32 [B] on x's device or None (sample b with y[b]); indices must lie in [0, B) -- the kernel
    clamps others.  ``y`` may be ``x`` itself: batch-internal mixing from one set of forward passes.
    Differentiable with respect to ``x`` and ``y``."""
    if not isinstance(x, torch.Tensor) or not isinstance(mask, torch.Tensor):
        raise ValueError("amplitude_mix: image and mask must be torch tensors")
    if x.dim() < 3:
        raise ValueError(f"amplitude_mix: [B, C, *spatial] expected, got {tuple(x.shape)}")
    C = x.shape[1]
    n_dims = x.dim() - 2
    if mask.dim() not in (n_dims, n_dims + 1):
        raise ValueError(f"amplitude_mix: mask {tuple(mask.shape)} for an image {tuple(x.shape)}")
    if not isinstance(lam, torch.Tensor):
        lam = torch.full((x.shape[0],), float(lam), dtype=torch.float32, device=x.device)
    return _ops().amp_mix(x, y, mask, lam, perm, n_dims, C, pad)


def _resolve_mask(mask_or_beta, x: torch.Tensor, cache: dict) -> torch.Tensor:
    if isinstance(mask_or_beta, torch.Tensor):
        return mask_or_beta if mask_or_beta.device == x.device else mask_or_beta.to(x.device)
    key = (tuple(x.shape[2:]), x.device)
    if key not in cache:
        cache.clear()
        cache[key] = lowfreq_box(x.shape[2:], float(mask_or_beta), x.device)
    return cache[key]


class AmplitudeMix(Transform):
    """Deterministic amplitude mixing of a pair: ``AmplitudeMix(mask_or_beta, lam)(x, y)`` gives x's phase with
    the amplitude (1 - lam M) |X| + lam M |Y|.  ``mask_or_beta``: a float32 mask in the centred layout, or the
    ``beta`` of ``lowfreq_box`` (built once per image size).  x, y: [B, C, *spatial] float32 HIP tensors."""

    def __init__(self, mask_or_beta: Union[float, torch.Tensor], lam: float = 1.0):
        self.mask_or_beta = mask_or_beta
        self.lam = float(lam)
        self._cache: dict = {}

    def __call__(self, x: torch.Tensor, y: torch.Tensor, perm: Optional[torch.Tensor] = None) -> torch.Tensor:
        return amplitude_mix(x, y, _resolve_mask(self.mask_or_beta, x, self._cache), self.lam, perm)


class RandAmplitudeMix(Randomizable, Transform):
    """Batch stage: every sample of ``x`` [B, C, *spatial] is, with probability ``prob``, mixed with another
    sample of the same batch at a strength drawn uniformly from ``lam_range``.  ``randomize`` draws, from the
    transform's own ``RandomState`` (``set_random_state``), a permutation of the batch, one uniform per sample
    for the decision and one for the strength; undrawn samples get lam = 0.  The two device tensors (lam,
    perm) are uploaded once per call, and one launch sequence runs with y = x.

    A sample with lam = 0 is the FFT round trip of its input (within 2e-6 of it), not a bit copy."""

    def __init__(self, mask_or_beta: Union[float, torch.Tensor], lam_range: Tuple[float, float] = (0.0, 1.0),
                 prob: float = 0.5):
        lo, hi = float(lam_range[0]), float(lam_range[1])
        if not (lo <= hi):
            raise ValueError(f"RandAmplitudeMix: lam_range must be (low, high) with low <= high, got {lam_range}")
        self.mask_or_beta = mask_or_beta
        self.lam_range = (lo, hi)
        self.prob = min(max(float(prob), 0.0), 1.0)
        self.lam: Optional[np.ndarray] = None
        self.perm: Optional[np.ndarray] = None
        self._cache: dict = {}

    def randomize(self, data) -> None:
        B = int(data) if isinstance(data, (int, np.integer)) else int(data.shape[0])
        self.perm = self.R.permutation(B).astype(np.int32)
        drawn = self.R.rand(B) < self.prob
        lam = self.R.uniform(self.lam_range[0], self.lam_range[1], size=B)
        self.lam = np.where(drawn, lam, 0.0).astype(np.float32)

    def __call__(self, x: torch.Tensor, randomize: bool = True) -> torch.Tensor:
        if randomize:
            self.randomize(x)
        if self.lam is None or self.perm is None or len(self.lam) != x.shape[0]:
            raise ValueError("RandAmplitudeMix: randomize() has not drawn for this batch size")
        lam = torch.from_numpy(self.lam).to(x.device)
        perm = torch.from_numpy(self.perm).to(x.device)
        return amplitude_mix(x, x, _resolve_mask(self.mask_or_beta, x, self._cache), lam, perm)


__all__ = ["amplitude_mix", "lowfreq_box", "AmplitudeMix", "RandAmplitudeMix"]
