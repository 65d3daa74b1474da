"""The centred complex spectrum on the native passes.

``shift_fourier(x, n_dims)`` is the reference's ``Fourier.shift_fourier``
(filters_and_operators.py:594-612; the same pair at stylization_layers.py:16-52 and as
``FourierTransform`` at 50_reconstruction/reconGan/utils2.py:6-31): ``fftshift(fftn(x, dims), dims)``,
float32 in, complex64 out.  ``inv_shift_fourier(k, n_dims, pad=0)`` is ``Fourier.inv_shift_fourier``
(:614-632): ``ifftn(ifftshift(k, dims), dims).real`` for any complex64 ``k``, float32 out, with optional
zero columns after the last axis.  Both are ``torch.ops.texbias`` custom ops with autograd (each is the
other's adjoint up to N), so a complex edit between them -- a phase ramp, a coil weighting, measured
coefficients written in, a loss on the coefficients -- stays on the library's passes and differentiates.

The drop-in switch (default off) sends the reference-named helpers ``Fourier.shift_fourier`` /
``Fourier.inv_shift_fourier`` (filters_and_operators, stylization_layers) and
``utils2.FourierTransform`` to these ops for CUDA float32 (forward) / complex64 (inverse) tensors;
everything else -- CPU tensors, other dtypes, ``inv_shift_fourier_complex`` -- stays on ``torch.fft``.
``set_dropin(True)`` or ``TEXBIAS_FOURIER=1`` turns it on.
"""
from __future__ import annotations

import os

import torch

from . import ops as _ops  # noqa: F401 - registers torch.ops.texbias.*

_dropin = os.environ.get("TEXBIAS_FOURIER", "0") not in ("", "0")


def shift_fourier(x: torch.Tensor, n_dims: int) -> torch.Tensor:
    """``fftshift(fftn(x, dims), dims)`` over the trailing ``n_dims`` axes of a float32 HIP tensor."""
    return torch.ops.texbias.shift_fourier(x, n_dims)


def inv_shift_fourier(k: torch.Tensor, n_dims: int, pad: int = 0) -> torch.Tensor:
    """``ifftn(ifftshift(k, dims), dims).real`` over the trailing ``n_dims`` axes of a complex64 HIP
    tensor; ``pad`` zero columns are appended to the last axis."""
    return torch.ops.texbias.inv_shift_fourier(k, n_dims, pad)


def set_dropin(enable: bool) -> bool:
    """Route the reference-named Fourier helpers to the native ops (see the module docstring).  Returns
    the previous setting."""
    global _dropin
    prev, _dropin = _dropin, bool(enable)
    return prev


def dropin_enabled() -> bool:
    return _dropin


def takes(t, dtype: torch.dtype) -> bool:
    """True when the switch is on and ``t`` is a CUDA tensor of ``dtype``: the helper runs the native op."""
    return _dropin and isinstance(t, torch.Tensor) and t.device.type == "cuda" and t.dtype == dtype


__all__ = ["shift_fourier", "inv_shift_fourier", "set_dropin", "dropin_enabled"]
