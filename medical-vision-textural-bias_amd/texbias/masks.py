"""User-supplied k-space masks as transforms (TB_OP_MASK, TB_OP_CMASK).

The reference's notebooks build a mask by hand and multiply it into ``Fourier.shift_fourier(x)``
(filters_and_operators.py:594-632): an annulus, an anisotropic low-pass, a Hann window, Cartesian line
undersampling.  ``KSpaceMask`` / ``KSpaceMaskd`` run such a mask through the same fused
forward-FFT -> op program -> inverse-FFT round trip as the drop-in filters, with no spectrum stored,
and compose with them in a ``pipeline.FusedChain``.  ``LearnedKSpaceMask`` is the trainable form: an
``nn.Module`` whose mask is a parameter with a gradient (``torch.ops.texbias.kspace_mask_learn``).  These
classes are additions of this package; the drop-in modules keep exactly the reference's names.

The mask is real, laid out like ``fftshift(fftn(x))`` over the spatial axes: shape ``spatial`` (shared
by every channel) or ``(C,) + spatial``.  It lives on the device: a numpy array or CPU tensor is copied
there once at first use, a HIP tensor is used in place, so later writes to it take effect.

``ComplexKSpaceMask`` / ``ComplexKSpaceMaskd`` / ``LearnedComplexKSpaceMask`` are the same three for a
complex64 mask (TB_OP_CMASK): a phase ramp (sub-voxel shift, motion), a B0-like phase, a complex
apodisation.  The real-mask classes keep rejecting complex arrays, so a mask never changes meaning
by its dtype alone.
"""
from __future__ import annotations

from typing import Dict, Hashable, List, Mapping, Optional, Sequence

import numpy as np
import torch

from . import kprog as K
from . import ops as _ops  # noqa: F401 - registers torch.ops.texbias.*
from . import runtime as rt
from .transform_base import MapTransform, Transform


class KSpaceMask(Transform):
    """y = Re(IFFT(ifftshift(mask * fftshift(FFT(img))))) for an image [C, *spatial]."""

    def __init__(self, mask) -> None:
        m = torch.as_tensor(mask)
        if m.is_complex():
            raise ValueError("KSpaceMask: complex masks are not supported")
        if m.requires_grad:
            raise ValueError("KSpaceMask: a mask with requires_grad is not supported")
        self.mask = m.to(torch.float32).contiguous()
        self._dev: Dict[torch.device, torch.Tensor] = {}

    def mask_on(self, device: Optional[torch.device] = None) -> torch.Tensor:
        """The float32 contiguous mask on ``device`` (default: the current HIP device)."""
        if self.mask.device.type == "cuda" and (device is None or device == self.mask.device):
            return self.mask
        if device is None:
            if torch.utils.data.get_worker_info() is not None:
                raise rt.TexbiasError(f"{type(self).__name__} cannot run inside a (forked) DataLoader worker: apply "
                                      "it to the collated batch (texbias.pipeline.FusedChain)")
            if not torch.cuda.is_available():
                raise rt.TexbiasError(f"{type(self).__name__} needs a HIP device (there is no CPU implementation)")
            device = torch.device("cuda", torch.cuda.current_device())
        m = self._dev.get(device)
        if m is None:
            m = self.mask.to(device).contiguous()
            self._dev[device] = m
        return m

    def program(self, spatial: Sequence[int], channels: int, device: Optional[torch.device] = None) -> List:
        """The op program for images [channels, *spatial] (as the drop-in filters' ``program``)."""
        spatial = tuple(int(s) for s in spatial)
        if tuple(self.mask.shape) == spatial:
            cm = 1
        elif tuple(self.mask.shape) == (int(channels),) + spatial:
            cm = int(channels)
        else:
            raise ValueError(f"KSpaceMask: mask shape {tuple(self.mask.shape)} is neither {spatial} nor "
                             f"{(int(channels),) + spatial}")
        return [K.mask_op(self.mask_on(device).data_ptr(), cm, K.geometry(spatial).hwd)]

    def __call__(self, img):
        x = torch.Tensor(img) if isinstance(img, np.ndarray) else img
        if x.dim() < 2:
            raise ValueError("KSpaceMask expects an image [C, *spatial]")
        dev = x.device if x.device.type == "cuda" else None
        m = self.mask_on(dev)
        xd = x.to(device=m.device, dtype=torch.float32)
        n_dims = xd.dim() - 1
        y = torch.ops.texbias.kspace_mask(xd, m, n_dims, xd.shape[0], 0)
        return y if x.device == m.device else y.to(x.device)


class KSpaceMaskd(MapTransform):
    """Dictionary version of :class:`KSpaceMask`."""

    def __init__(self, keys, mask, allow_missing_keys: bool = False) -> None:
        MapTransform.__init__(self, keys, allow_missing_keys)
        self.transform = KSpaceMask(mask)

    def program(self, spatial: Sequence[int], channels: int, device: Optional[torch.device] = None) -> List:
        return self.transform.program(spatial, channels, device)

    def __call__(self, data: Mapping[Hashable, torch.Tensor]):
        d = dict(data)
        for key in self.key_iterator(d):
            d[key] = self.transform(d[key])
        return d


class LearnedKSpaceMask(torch.nn.Module):
    """A trainable real k-space mask: y = Re(IFFT(ifftshift(mask * fftshift(FFT(x))))) for a batch
    ``x`` [B, C, *spatial], with autograd with respect to ``x`` and to ``mask`` (every element of the
    centred layout is an independent parameter).  ``init``: array or tensor of shape ``spatial`` (shared
    by every channel) or ``(C,) + spatial``; held as the float32 contiguous ``nn.Parameter`` ``mask``."""

    def __init__(self, init, n_dims: int = 3) -> None:
        super().__init__()
        m = torch.as_tensor(init)
        if m.is_complex():
            raise ValueError("LearnedKSpaceMask: complex masks are not supported")
        n_dims = int(n_dims)
        if n_dims < 1 or m.dim() not in (n_dims, n_dims + 1):
            raise ValueError(f"LearnedKSpaceMask: init of shape {tuple(m.shape)} is neither spatial nor (C,) + spatial "
                             f"for {n_dims} transformed axes")
        self.n_dims = n_dims
        self.mask = torch.nn.Parameter(m.detach().to(torch.float32).contiguous().clone())

    def forward(self, x: torch.Tensor, pad: int = 0) -> torch.Tensor:
        if not isinstance(x, torch.Tensor) or x.dim() != self.n_dims + 2:
            raise ValueError(f"LearnedKSpaceMask expects a batch [B, C, *spatial] with {self.n_dims} spatial axes")
        if x.dtype != torch.float32:
            raise ValueError(f"LearnedKSpaceMask: float32 images expected, got {x.dtype}")
        spatial, channels = tuple(x.shape[2:]), int(x.shape[1])
        if tuple(self.mask.shape) not in (spatial, (channels,) + spatial):
            raise ValueError(f"LearnedKSpaceMask: mask shape {tuple(self.mask.shape)} is neither {spatial} nor "
                             f"{(channels,) + spatial}")
        if x.device.type != "cuda":
            raise rt.TexbiasError("LearnedKSpaceMask needs a HIP device (there is no CPU implementation)")
        return torch.ops.texbias.kspace_mask_learn(x, self.mask, self.n_dims, channels, pad)

    def as_transform(self) -> KSpaceMask:
        """A :class:`KSpaceMask` over ``self.mask.detach()``, e.g. for a ``pipeline.FusedChain`` at
        inference.  It shares the parameter's storage, so later optimizer steps show through; after
        moving the module to another device, take a new one."""
        return KSpaceMask(self.mask.detach())


class ComplexKSpaceMask(KSpaceMask):
    """:class:`KSpaceMask` with a complex mask (held as complex64): y = Re(IFFT(ifftshift(mask *
    fftshift(FFT(img))))) for an image [C, *spatial], in the same fused round trip.  A real array is
    accepted and taken as ``mask + 0j``."""

    def __init__(self, mask) -> None:
        m = torch.as_tensor(mask)
        if m.requires_grad:
            raise ValueError("ComplexKSpaceMask: a mask with requires_grad is not supported")
        self.mask = m.to(torch.complex64).contiguous()
        self._dev: Dict[torch.device, torch.Tensor] = {}

    def program(self, spatial: Sequence[int], channels: int, device: Optional[torch.device] = None) -> List:
        spatial = tuple(int(s) for s in spatial)
        if tuple(self.mask.shape) == spatial:
            cm = 1
        elif tuple(self.mask.shape) == (int(channels),) + spatial:
            cm = int(channels)
        else:
            raise ValueError(f"ComplexKSpaceMask: mask shape {tuple(self.mask.shape)} is neither {spatial} nor "
                             f"{(int(channels),) + spatial}")
        return [K.cmask_op(self.mask_on(device).data_ptr(), cm, K.geometry(spatial).hwd)]

    def __call__(self, img):
        x = torch.Tensor(img) if isinstance(img, np.ndarray) else img
        if x.dim() < 2:
            raise ValueError("ComplexKSpaceMask expects an image [C, *spatial]")
        dev = x.device if x.device.type == "cuda" else None
        m = self.mask_on(dev)
        xd = x.to(device=m.device, dtype=torch.float32)
        y = torch.ops.texbias.kspace_cmask(xd, m, xd.dim() - 1, xd.shape[0], 0, False)
        return y if x.device == m.device else y.to(x.device)


class ComplexKSpaceMaskd(KSpaceMaskd):
    """Dictionary version of :class:`ComplexKSpaceMask`."""

    def __init__(self, keys, mask, allow_missing_keys: bool = False) -> None:
        MapTransform.__init__(self, keys, allow_missing_keys)
        self.transform = ComplexKSpaceMask(mask)


class LearnedComplexKSpaceMask(torch.nn.Module):
    """A trainable complex k-space mask: :class:`LearnedKSpaceMask` with a complex64 ``nn.Parameter``
    ``mask`` (``spatial`` or ``(C,) + spatial``), autograd with respect to ``x`` and to ``mask`` in torch's
    convention for complex leaves (``torch.ops.texbias.kspace_cmask_learn``), so ``torch.optim`` optimizers
    step it as they step any complex parameter."""

    def __init__(self, init, n_dims: int = 3) -> None:
        super().__init__()
        m = torch.as_tensor(init)
        n_dims = int(n_dims)
        if n_dims < 1 or m.dim() not in (n_dims, n_dims + 1):
            raise ValueError(f"LearnedComplexKSpaceMask: init of shape {tuple(m.shape)} is neither spatial nor "
                             f"(C,) + spatial for {n_dims} transformed axes")
        self.n_dims = n_dims
        self.mask = torch.nn.Parameter(m.detach().to(torch.complex64).contiguous().clone())

    def forward(self, x: torch.Tensor, pad: int = 0) -> torch.Tensor:
        if not isinstance(x, torch.Tensor) or x.dim() != self.n_dims + 2:
            raise ValueError(f"LearnedComplexKSpaceMask expects a batch [B, C, *spatial] with {self.n_dims} spatial axes")
        if x.dtype != torch.float32:
            raise ValueError(f"LearnedComplexKSpaceMask: float32 images expected, got {x.dtype}")
        spatial, channels = tuple(x.shape[2:]), int(x.shape[1])
        if tuple(self.mask.shape) not in (spatial, (channels,) + spatial):
            raise ValueError(f"LearnedComplexKSpaceMask: mask shape {tuple(self.mask.shape)} is neither {spatial} nor "
                             f"{(channels,) + spatial}")
        if x.device.type != "cuda":
            raise rt.TexbiasError("LearnedComplexKSpaceMask needs a HIP device (there is no CPU implementation)")
        return torch.ops.texbias.kspace_cmask_learn(x, self.mask, self.n_dims, channels, pad)

    def as_transform(self) -> ComplexKSpaceMask:
        """A :class:`ComplexKSpaceMask` over ``self.mask.detach()`` (shares the parameter's storage), e.g.
        for a ``pipeline.FusedChain`` at inference; after moving the module, take a new one."""
        return ComplexKSpaceMask(self.mask.detach())


__all__ = ["KSpaceMask", "KSpaceMaskd", "LearnedKSpaceMask", "ComplexKSpaceMask", "ComplexKSpaceMaskd",
           "LearnedComplexKSpaceMask"]
