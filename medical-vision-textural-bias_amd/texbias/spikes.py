"""The trainable spike layer: k-space spikes with device-resident log-intensities and closed-form gradients.

The reference's ``spike_layer`` (``stylization_layers.py:143-151``) sets |K(f)| = exp(intensity) at one random
k-space location shared by the batch and keeps the phase; its drivers train the log-intensity by finite
differences (``350_stylized_layers/spikes11_layer_domain_GD.py:260-275``): two more forwards of filter and U-Net
per step, each with its own random location.  ``LearnedSpikeLayer`` is the same filter on the closed-form route
(``csrc/point.h``) with

* the log-intensities as a float32 ``nn.Parameter`` that the kernels read on the device: no ``.item()``, no host
  sync, so the layer sits in a captured graph with a live intensity;
* the gradient with respect to the log-intensities (one read of the upstream gradient) and to the image (one more
  read and write) in closed form (``csrc/spike_grad.h``, ``torch.ops.texbias.kspace_spikes``).

Locations stay on the host: two spikes at equal or conjugate frequencies cannot be told apart without reading
them, and the layer draws them from its own ``numpy`` random state as the reference's transforms do.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import kprog as K
from . import ops as _ops  # noqa: F401 - registers torch.ops.texbias.*
from . import runtime as rt
from ._abi import TB_MAX_OPS

_DRAWS = 1000  # redraws of one spike before the volume is declared too small for n_spikes


class LearnedSpikeLayer(torch.nn.Module):
    """y = x with |FFT(x)(f_j)| := exp(log_intensity[j]) at ``n_spikes`` k-space locations shared by every channel
    of every sample of a batch ``x`` [B, C, *spatial] (float32, on a HIP device); all axes after the first two are
    transformed, so the reference's [B, 1, H, W, D] call works unchanged.  ``log_intensity``: float32
    ``nn.Parameter`` [n_spikes] (a scalar initialises every spike), with autograd with respect to it and to ``x``.
    Trains with ``texbias.optim.Adam`` or any ``torch.optim`` optimizer."""

    def __init__(self, log_intensity=15.0, n_spikes: int = 1, seed: Optional[int] = None) -> None:
        super().__init__()
        n_spikes = int(n_spikes)
        if not 1 <= n_spikes <= TB_MAX_OPS:
            raise ValueError(f"LearnedSpikeLayer: {n_spikes} spikes (1 to {TB_MAX_OPS} are supported)")
        v = torch.as_tensor(log_intensity, dtype=torch.float32).detach().reshape(-1)
        if v.numel() == 1:
            v = v.repeat(n_spikes)
        if v.numel() != n_spikes:
            raise ValueError(f"LearnedSpikeLayer: {v.numel()} log-intensities for {n_spikes} spikes")
        self.n_spikes = n_spikes
        self.log_intensity = torch.nn.Parameter(v.contiguous().clone())
        self.last_loc: Optional[List[Tuple[int, ...]]] = None
        self.R = np.random.RandomState(seed)

    def set_rand_state(self, seed: Optional[int] = None, state: Optional[np.random.RandomState] = None):
        """Reseed the location draws (MONAI's ``Randomizable.set_random_state`` protocol)."""
        self.R = state if state is not None else np.random.RandomState(seed)
        return self

    def draw(self, spatial: Sequence[int]) -> List[Tuple[int, ...]]:
        """One centred location per spike, ``randint(0, n)`` per spatial axis; a spike at the frequency of an
        earlier one, or at its conjugate, is drawn again."""
        spatial = tuple(int(s) for s in spatial)
        geo = K.geometry(spatial)
        locs: List[Tuple[int, ...]] = []
        freqs: List[Tuple[int, int, int]] = []
        for _ in range(self.n_spikes):
            for _try in range(_DRAWS):
                idx = tuple(int(self.R.randint(0, n)) for n in spatial)
                f = geo.to_hwd(K.unshift(idx, spatial))
                if not any(rt.spikes_touch(f, e, geo.hwd) for e in freqs):
                    break
            else:
                raise ValueError(f"LearnedSpikeLayer: no room for {self.n_spikes} non-touching spikes in {spatial}")
            locs.append(idx)
            freqs.append(f)
        return locs

    def _locations(self, loc, nd: Optional[int]) -> List[Tuple[int, ...]]:
        loc = list(loc)
        if loc and not isinstance(loc[0], (Sequence, np.ndarray)):
            loc = [loc]
        locs = [tuple(int(v) for v in l) for l in loc]
        if len(locs) != self.n_spikes or any(len(l) != (len(locs[0]) if nd is None else nd) for l in locs):
            raise ValueError(f"LearnedSpikeLayer: {self.n_spikes} locations of equal rank are expected, got {locs}")
        return locs

    def forward(self, x: torch.Tensor, loc=None, pad: int = 0) -> torch.Tensor:
        if not isinstance(x, torch.Tensor) or x.dim() < 3:
            raise ValueError("LearnedSpikeLayer expects a batch [B, C, *spatial]")
        if x.dtype != torch.float32:
            raise ValueError(f"LearnedSpikeLayer: float32 images expected, got {x.dtype}")
        spatial = tuple(x.shape[2:])
        locs = self.draw(spatial) if loc is None else self._locations(loc, len(spatial))
        flat = [v for l in locs for v in l]
        rt.spike_locations("LearnedSpikeLayer", flat, spatial)  # argument errors before the device is asked for
        if x.device.type != "cuda":
            raise rt.TexbiasError("LearnedSpikeLayer needs a HIP device (there is no CPU implementation)")
        self.last_loc = locs
        return torch.ops.texbias.kspace_spikes(x, self.log_intensity, flat, len(spatial), int(x.shape[1]), pad)[0]

    def as_transform(self, loc=None):
        """A ``KSpaceSpikeNoise`` at ``loc`` (default: the locations of the last forward) holding the trained
        intensities, for [C, *spatial] images at inference.  The one place that reads the intensities back to the
        host."""
        from filters_and_operators import KSpaceSpikeNoise
        if loc is None:
            if self.last_loc is None:
                raise ValueError("LearnedSpikeLayer.as_transform: no location given and no forward has run")
            locs = self.last_loc
        else:
            locs = self._locations(loc, None)
        vals = [float(v) for v in self.log_intensity.detach().cpu().tolist()]
        return KSpaceSpikeNoise(loc=[tuple(l) for l in locs], k_intensity=vals)


__all__ = ["LearnedSpikeLayer"]
