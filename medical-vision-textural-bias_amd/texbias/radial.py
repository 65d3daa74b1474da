"""Radial k-space profiles: the shell power spectrum and a trainable radial filter.

Everything this package filters with is a function of radius in centred k-space (``disk_mask``, the Gibbs
truncation, ``GibbsNoiseLayer``: 0/1 steps in |f|), and the reference's research question -- textural bias --
is about how image energy is distributed over |f|.  This module has the radial operations themselves:

* ``radial_power_spectrum``: the radially binned power spectrum, the texture diagnostic the reference's
  notebooks look at by eye (``show_slice_and_fourier``), in one forward pass and one fused shell reduction
  with no spectrum stored; differentiable with respect to the image, so a loss on it trains;
* ``RadialFilter`` / ``RadialFilterd``: a k-space mask M(f) = p(|f|) given by a profile of K values, as a
  transform that composes with the built-in filters in a ``pipeline.FusedChain``; ``RadialFilter.disk`` is the
  reference's disk as a profile;
* ``LearnedRadialFilter``: the trainable form, a few hundred parameters with an analytic gradient (the
  reference updates its Gibbs layer's alpha by finite differences, ``Gibbs_GD``, because a hard step has no
  gradient).

Bins: ``bins`` shells of width ``dr`` over r = sqrt(k_h^2 + k_w^2 + k_d^2), k the signed index of the centred
layout (centre floor(n / 2), ``disk_mask``'s metric); ``mode`` "nearest" puts an element in bin int(r / dr),
"linear" splits it between the two nearest bin positions; the last bin is clamped (``include/texbias.h``).
"""
from __future__ import annotations

from typing import Dict, Hashable, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from . import kprog as K
from . import ops as _ops  # noqa: F401 - registers torch.ops.texbias.*
from . import runtime as rt
from .transform_base import MapTransform, Transform


def max_bin(spatial: Sequence[int], dr: float = 1.0) -> int:
    """int(u) of the farthest element of the centred layout, in the kernels' float32 arithmetic: with
    ``max_bin + 1`` bins nothing is clamped."""
    r2 = sum((int(n) // 2) ** 2 for n in spatial if int(n) > 1)
    return int(np.sqrt(np.float32(r2)) * np.float32(1.0 / float(dr)))


_counts: Dict[Tuple, torch.Tensor] = {}


def shell_counts(spatial: Sequence[int], bins: int, dr: float, mode, device: torch.device) -> torch.Tensor:
    """Summed weights of every bin, ``radial_bin(ones)`` (float32 [bins]); cached per (geometry, bins, dr, mode)."""
    bins, dr, mode = rt.radial_params("shell_counts", bins, dr, mode)
    spatial = tuple(int(s) for s in spatial)
    key = (device.type, device.index, K.geometry(spatial).hwd, bins, dr, mode)
    c = _counts.get(key)
    if c is None:
        c = torch.ops.texbias.radial_bin(torch.ones(spatial, dtype=torch.float32, device=device), len(spatial), bins, dr,
                                         mode)
        _counts[key] = c
    return c


def radial_power_spectrum(x: torch.Tensor, n_dims: int = 3, bins: Optional[int] = None, dr: float = 1.0,
                          mode="nearest", mean: bool = False) -> torch.Tensor:
    """P[..., k] = sum over shell k of |FFT(x)|^2 / N for every volume of ``x`` [*lead, *spatial] (float32, on a
    HIP device): float32 [*lead, bins], with P.sum(-1) = (x**2).sum(spatial) (Parseval).  ``bins`` = None takes
    ``max_bin + 1`` bins, so nothing is clamped; ``mean``: divide by the shell counts (the mean power per
    coefficient of a shell; empty shells give 0).  Differentiable with respect to ``x``."""
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"radial_power_spectrum: a torch tensor is expected, got {type(x).__name__}")
    n_dims = int(n_dims)
    if n_dims < 1 or x.dim() < n_dims:
        raise ValueError(f"radial_power_spectrum: {n_dims} transformed axes on a {x.dim()}-d tensor")
    spatial = tuple(x.shape[x.dim() - n_dims:])
    if bins is None:
        bins = max_bin(spatial, dr) + 1
    bins, dr, mode = rt.radial_params("radial_power_spectrum", bins, dr, mode)
    P = torch.ops.texbias.radial_power(x, n_dims, bins, dr, mode)
    if mean:
        c = shell_counts(spatial, bins, dr, mode, x.device)
        P = torch.where(c > 0, P / c.clamp_min(torch.finfo(torch.float32).tiny), torch.zeros_like(P))
    return P


class RadialFilter(Transform):
    """y = Re(IFFT(ifftshift(M * fftshift(FFT(img))))) with M(f) = profile(|f|) for an image [C, *spatial]:
    ``profile`` [K] (shared by every channel) or [C, K], bins of width ``dr``.  The profile is expanded to the
    centred mask on the device when a program is built (again when the profile has been written to); the
    transform keeps the mask alive."""

    def __init__(self, profile, dr: float = 1.0, mode="linear") -> None:
        p = torch.as_tensor(profile)
        if p.is_complex() or p.dim() not in (1, 2):
            raise ValueError(f"RadialFilter: a real profile [K] or [C, K] is expected, got {tuple(p.shape)}")
        if p.requires_grad:
            raise ValueError("RadialFilter: a profile with requires_grad is not supported (LearnedRadialFilter)")
        _, self.dr, self.mode = rt.radial_params("RadialFilter", p.shape[-1], dr, mode)
        self.profile = p.to(torch.float32).contiguous()
        self._masks: Dict[Tuple, Tuple[torch.Tensor, int]] = {}

    @staticmethod
    def disk(r: int, spatial: Sequence[int]) -> "RadialFilter":
        """The reference's disk (``disk_mask`` with an integer radius: r2 < r^2) as a radial filter:
        p[b] = 1 for b < r, dr = 1, nearest."""
        if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or r < 0:
            raise ValueError(f"RadialFilter.disk: an integer radius >= 0 is expected, got {r!r}")
        k = max_bin(spatial) + 1
        if k > rt.RADIAL_MAX_BINS:
            raise ValueError(f"RadialFilter.disk: {k} bins for {tuple(spatial)} (at most {rt.RADIAL_MAX_BINS})")
        p = np.zeros(k, np.float32)
        p[: int(r)] = 1.0
        return RadialFilter(p, dr=1.0, mode="nearest")

    def mask_on(self, spatial: Sequence[int], device: Optional[torch.device] = None) -> torch.Tensor:
        """The expanded float32 mask for ``spatial`` on ``device`` (default: the profile's or the current HIP device)."""
        spatial = tuple(int(s) for s in spatial)
        if device is None and self.profile.device.type == "cuda":
            device = self.profile.device
        if device is None:
            if torch.utils.data.get_worker_info() is not None:
                raise rt.TexbiasError("RadialFilter cannot run inside a (forked) DataLoader worker: apply it to the "
                                      "collated batch (texbias.pipeline.FusedChain)")
            if not torch.cuda.is_available():
                raise rt.TexbiasError("RadialFilter needs a HIP device (there is no CPU implementation)")
            device = torch.device("cuda", torch.cuda.current_device())
        key = (device, spatial)
        hit = self._masks.get(key)
        if hit is not None and hit[1] == self.profile._version:
            return hit[0]
        p = self.profile if self.profile.device == device else self.profile.to(device)
        m = rt.radial_mask(p, spatial, self.dr, self.mode, out=hit[0] if hit is not None else None)
        self._masks[key] = (m, self.profile._version)
        return m

    def program(self, spatial: Sequence[int], channels: int, device: Optional[torch.device] = None) -> List:
        """The op program for images [channels, *spatial]: one TB_OP_MASK over the expanded mask."""
        if self.profile.dim() == 2 and int(self.profile.shape[0]) != int(channels):
            raise ValueError(f"RadialFilter: a profile for {int(self.profile.shape[0])} channels on {int(channels)}")
        m = self.mask_on(spatial, device)
        cm = 1 if self.profile.dim() == 1 else int(channels)
        return [K.mask_op(m.data_ptr(), cm, K.geometry(tuple(int(s) for s in spatial)).hwd)]

    def __call__(self, img):
        x = torch.Tensor(img) if isinstance(img, np.ndarray) else img
        if x.dim() < 2:
            raise ValueError("RadialFilter expects an image [C, *spatial]")
        if self.profile.dim() == 2 and int(self.profile.shape[0]) != int(x.shape[0]):
            raise ValueError(f"RadialFilter: a profile for {int(self.profile.shape[0])} channels on {int(x.shape[0])}")
        m = self.mask_on(tuple(x.shape[1:]), x.device if x.device.type == "cuda" else None)
        xd = x.to(device=m.device, dtype=torch.float32)
        y = torch.ops.texbias.kspace_mask(xd, m, xd.dim() - 1, xd.shape[0], 0)
        return y if x.device == m.device else y.to(x.device)


class RadialFilterd(MapTransform):
    """Dictionary version of :class:`RadialFilter`."""

    def __init__(self, keys, profile, dr: float = 1.0, mode="linear", allow_missing_keys: bool = False) -> None:
        MapTransform.__init__(self, keys, allow_missing_keys)
        self.transform = RadialFilter(profile, dr, mode)

    def program(self, spatial: Sequence[int], channels: int, device: Optional[torch.device] = None) -> List:
        return self.transform.program(spatial, channels, device)

    def __call__(self, data: Mapping[Hashable, torch.Tensor]):
        d = dict(data)
        for key in self.key_iterator(d):
            d[key] = self.transform(d[key])
        return d


class LearnedRadialFilter(torch.nn.Module):
    """A trainable radial k-space filter: y = Re(IFFT(ifftshift(M * fftshift(FFT(x))))) with M(f) =
    profile(|f|) for a batch ``x`` [B, C, *spatial], with autograd with respect to ``x`` and to ``profile``
    (``torch.ops.texbias.radial_filter``).  ``init``: [K] (shared by every channel) or [C, K]; held as the
    float32 ``nn.Parameter`` ``profile``.  Trains with ``texbias.optim.Adam`` or any ``torch.optim`` optimizer."""

    def __init__(self, init, n_dims: int = 3, dr: float = 1.0, mode="linear") -> None:
        super().__init__()
        p = torch.as_tensor(init)
        if p.is_complex() or p.dim() not in (1, 2):
            raise ValueError(f"LearnedRadialFilter: a real profile [K] or [C, K] is expected, got {tuple(p.shape)}")
        n_dims = int(n_dims)
        if n_dims < 1:
            raise ValueError(f"LearnedRadialFilter: {n_dims} transformed axes")
        _, self.dr, self.mode = rt.radial_params("LearnedRadialFilter", p.shape[-1], dr, mode)
        self.n_dims = n_dims
        self.profile = torch.nn.Parameter(p.detach().to(torch.float32).contiguous().clone())

    def forward(self, x: torch.Tensor, pad: int = 0) -> torch.Tensor:
        if not isinstance(x, torch.Tensor) or x.dim() != self.n_dims + 2:
            raise ValueError(f"LearnedRadialFilter expects a batch [B, C, *spatial] with {self.n_dims} spatial axes")
        if x.dtype != torch.float32:
            raise ValueError(f"LearnedRadialFilter: float32 images expected, got {x.dtype}")
        channels = int(x.shape[1])
        if self.profile.dim() == 2 and int(self.profile.shape[0]) != channels:
            raise ValueError(f"LearnedRadialFilter: a profile for {int(self.profile.shape[0])} channels on {channels}")
        if x.device.type != "cuda":
            raise rt.TexbiasError("LearnedRadialFilter needs a HIP device (there is no CPU implementation)")
        return torch.ops.texbias.radial_filter(x, self.profile, self.n_dims, channels, self.dr, self.mode, pad)[0]

    def as_transform(self) -> RadialFilter:
        """A :class:`RadialFilter` over ``self.profile.detach()``, e.g. for a ``pipeline.FusedChain`` at
        inference.  It shares the parameter's storage: after an optimizer step the next program expands the
        new profile; after moving the module to another device, take a new one."""
        return RadialFilter(self.profile.detach(), self.dr, self.mode)


__all__ = ["radial_power_spectrum", "shell_counts", "max_bin", "RadialFilter", "RadialFilterd", "LearnedRadialFilter"]
