"""PyTorch custom operators over the texbias C ABI (``torch.ops.texbias.*``).

The filters of ``filters_and_operators.py`` / ``stylization_layers.py`` run through these ops, so
they are visible to ``torch.compile`` (fake-tensor / meta propagation via ``register_fake``, no
graph break), to ``torch.cuda.graphs`` capture (stream-ordered launches on the current stream, no
host synchronisation) and to autograd where a backward exists.  The transform classes stay the
front end with the reference's signatures; the op boundary carries the sample
programs as a uint8 CPU tensor of ``tb_sample_ops`` records (``include/texbias.h``).

Reference interfaces each op replaces (file:line under the reference root):
  texbias::kspace_filter     Fourier.shift_fourier -> k-space op(s) -> inv_shift_fourier(...).real
                             source_code/filters_and_operators.py:236-252, 370-393, 503-515,
                             663-705, 906-983; stylization_layers.py:79-116
  texbias::salt_and_pepper_  SaltAndPepper.salt_and_pepper  filters_and_operators.py:465-482
  texbias::kspace_mask       a hand-built mask multiplied into Fourier.shift_fourier(x)  :594-632
  texbias::kspace_mask_learn the same with the mask as a trainable tensor (autograd w.r.t. image and mask;
                             the reference's only trainable k-space object has d/d alpha = 0 and its
                             drivers update it by finite differences, Gibbs_GD)
  texbias::kspace_mask_grad  the mask gradient on its own
  texbias::kspace_cmask, kspace_cmask_learn, kspace_cmask_grad   the same three for a complex64 mask (a phase
                             ramp or any complex factor multiplied into Fourier.shift_fourier(x)  :594-632)
  texbias::shift_fourier     Fourier.shift_fourier      filters_and_operators.py:594-612 (float32 -> complex64)
  texbias::inv_shift_fourier Fourier.inv_shift_fourier  filters_and_operators.py:614-632 (complex64 -> float32;
                             autograd: each is the other's adjoint up to N)
  texbias::radial_power      the radially binned power spectrum the reference's notebooks look at by eye
                             (show_slice_and_fourier); autograd w.r.t. the image
  texbias::radial_filter     a mask that is a radial profile p(|f|) -- disk_mask (:136-197) is the 0/1 step --
                             with autograd w.r.t. the image and the profile (the GD_work.ipynb variant of
                             the Gibbs layer, trained by gradient instead of Gibbs_GD's finite differences)
  texbias::radial_grad, radial_mask, radial_bin   the profile gradient, the expansion and its adjoint alone
  texbias::gibbs_layer       GibbsNoiseLayer.forward / _apply_mask  stylization_layers.py:79-116
                             (autograd: the filter is self-adjoint; d/d alpha = 0 as in the reference)
  texbias::kspace_spikes     spike_layer.forward  stylization_layers.py:143-151 (KSpaceSpikeNoise._set_spike,
                             filters_and_operators.py:906-983) with the log-intensity read on the device; autograd
                             w.r.t. the image and the log-intensity in closed form (the reference's drivers update
                             it by finite differences, spikes11_layer_domain_GD.py:260-275)
  texbias::kspace_spikes_grad   the two gradients on their own
  texbias::amp_mix           what a user of Fourier.shift_fourier / inv_shift_fourier (:594-632) composes by hand
                             for amplitude mixing (abs, angle, polar between the two): the phase of x with the
                             amplitude moved towards a partner's, fused, with autograd w.r.t. both images
  texbias::amp_mix_grad      its two gradients on their own
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import kprog as K
from ._abi import TbSampleOps, programs_array
from . import runtime as rt

_REC = C.sizeof(TbSampleOps)


def pack_programs(programs: Sequence[Sequence]) -> torch.Tensor:
    """list (per sample) of op lists -> uint8 CPU tensor [B, sizeof(tb_sample_ops)]; with a program
    longer than TB_MAX_OPS, [passes, B, sizeof(tb_sample_ops)] (cut by ``kprog.split_program``:
    needs the op's frequency geometry, so such programs go through ``pack_programs_split``)."""
    arr = programs_array(programs)
    buf = np.frombuffer(C.string_at(C.addressof(arr), C.sizeof(arr)), dtype=np.uint8).copy()
    return torch.from_numpy(buf).reshape(len(programs), _REC)


def pack_programs_split(programs: Sequence[Sequence], hwd: Sequence[int]) -> torch.Tensor:
    """``pack_programs`` for programs of any length: [passes, B, REC] when one exceeds TB_MAX_OPS."""
    from ._abi import TB_MAX_OPS
    if all(len(p) <= TB_MAX_OPS for p in programs):
        return pack_programs(programs)
    parts = [K.split_program(list(p), hwd) for p in programs]
    npass = max(len(c) for c in parts)
    return torch.stack([pack_programs([c[i] if i < len(c) else [] for c in parts]) for i in range(npass)])


def unpack_programs(t: torch.Tensor) -> List[TbSampleOps]:
    raw = bytes(t.contiguous().cpu().numpy().tobytes())
    n = t.shape[0]
    arr = (TbSampleOps * n).from_buffer_copy(raw)
    return list(arr)


def _as_prog_lists(recs: List[TbSampleOps]):
    return [[r.op[j] for j in range(r.n)] for r in recs]


@torch.library.custom_op("texbias::kspace_filter", mutates_args=())
def kspace_filter(x: torch.Tensor, n_dims: int, programs: torch.Tensor, channels: int,
                  pad: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """y = Re(IFFT(program_b(FFT(x)))) over the trailing ``n_dims`` axes of [B*channels..., *spatial]
    (last axis padded by ``pad`` zero columns); also the per-sample (min, max) order-preserving keys
    (int32 [B, 2]) that salt-and-pepper uses."""
    passes = [programs] if programs.dim() == 2 else list(programs)   # [passes, B, REC]: split programs
    progs = _as_prog_lists(unpack_programs(passes[0]))
    mm = torch.empty((len(progs), 2), dtype=torch.int32, device=x.device)
    y = rt._kspace_filter_pass(x, n_dims, progs, channels, pad=pad, minmax=mm)
    view = y[..., : x.shape[-1]] if pad else y
    for p in passes[1:]:
        rt._kspace_filter_pass(view, n_dims, _as_prog_lists(unpack_programs(p)), channels, out=view, minmax=mm)
    return y, mm


@kspace_filter.register_fake
def _kspace_filter_fake(x, n_dims, programs, channels, pad=0):
    shape = tuple(x.shape[:-1]) + (x.shape[-1] + pad,)
    return x.new_empty(shape), x.new_empty((programs.shape[-2], 2), dtype=torch.int32)


@torch.library.custom_op("texbias::salt_and_pepper_", mutates_args=("x",))
def salt_and_pepper_(x: torch.Tensor, minmax: torch.Tensor, thresholds: torch.Tensor, seed: int, offset: int,
                     per_sample_dims: int) -> None:
    """In place: voxels with u <= lo -> min/2, lo < u <= hi -> max/2 of their sample (keys from
    ``minmax``); u from the device Philox stream (seed, offset).  thresholds: float32 CPU [B, 2]."""
    thr = [(float(a), float(b)) for a, b in thresholds.tolist()]
    rt.salt_and_pepper(x, per_sample_dims, thr, minmax, out=x, seed=seed, offset=offset)


@salt_and_pepper_.register_fake
def _salt_and_pepper_fake(x, minmax, thresholds, seed, offset, per_sample_dims):
    return None


def kspace_filter_programs(x: torch.Tensor, n_dims: int, programs: Sequence[Sequence], channels: int,
                           pad: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Convenience: the op with Python op lists."""
    return torch.ops.texbias.kspace_filter(x, n_dims, pack_programs(programs), channels, pad)


@torch.library.custom_op("texbias::kspace_mask", mutates_args=())
def kspace_mask(x: torch.Tensor, mask: torch.Tensor, n_dims: int, channels: int, pad: int = 0) -> torch.Tensor:
    """y = Re(IFFT(ifftshift(mask * fftshift(FFT(x))))) over the trailing ``n_dims`` axes of
    [B*channels..., *spatial] (last axis padded by ``pad`` zero columns) with the caller's real mask,
    laid out like ``Fourier.shift_fourier(x, n_dims)``: ``spatial`` or ``(channels,) + spatial``, float32,
    contiguous, on x's device.  One fused pass; the kernel reads ``mask`` on the current stream."""
    return rt.kspace_mask(x, mask, n_dims, pad=pad, channels=channels)


@kspace_mask.register_fake
def _kspace_mask_fake(x, mask, n_dims, channels, pad=0):
    return x.new_empty(tuple(x.shape[:-1]) + (x.shape[-1] + pad,))


def _kspace_mask_setup(ctx, inputs, output):
    x, mask, n_dims, channels, pad = inputs
    if mask.requires_grad:
        raise ValueError("texbias::kspace_mask has no gradient w.r.t. the mask (a learnable mask is not supported)")
    ctx.save_for_backward(mask)
    ctx.n_dims, ctx.channels, ctx.d = n_dims, channels, x.shape[-1]


def _kspace_mask_backward(ctx, gy):
    # the symmetrised real mask makes x -> y self-adjoint; the zero pad columns take no gradient
    (mask,) = ctx.saved_tensors
    return torch.ops.texbias.kspace_mask(gy[..., : ctx.d], mask, ctx.n_dims, ctx.channels, 0), None, None, None, None


kspace_mask.register_autograd(_kspace_mask_backward, setup_context=_kspace_mask_setup)


@torch.library.custom_op("texbias::kspace_mask_grad", mutates_args=())
def kspace_mask_grad(x: torch.Tensor, g: torch.Tensor, n_dims: int, channels: int, mask_channels: int) -> torch.Tensor:
    """Gradient of ``kspace_mask(x, M)`` with respect to the mask for the upstream gradient ``g`` (the
    image's shape, any strides with a contiguous last axis): ``spatial`` for ``mask_channels`` = 1 (summed
    over the channels), else ``(channels,) + spatial``; summed over the samples.  No autograd formula
    (double backward is not supported)."""
    return rt.kspace_mask_grad(x, g, n_dims, mask_channels, channels)


@kspace_mask_grad.register_fake
def _kspace_mask_grad_fake(x, g, n_dims, channels, mask_channels):
    spatial = tuple(x.shape[x.dim() - n_dims:])
    return x.new_empty(spatial if mask_channels == 1 else (mask_channels,) + spatial)


@torch.library.custom_op("texbias::kspace_mask_learn", mutates_args=())
def kspace_mask_learn(x: torch.Tensor, mask: torch.Tensor, n_dims: int, channels: int, pad: int = 0) -> torch.Tensor:
    """``texbias::kspace_mask`` (the same fused pass, bit for bit) for a learnable mask: autograd with
    respect to the image and to the mask.  Every element of the mask's centred layout is an independent
    variable."""
    return rt.kspace_mask_learn(x, mask, n_dims, pad=pad, channels=channels)


@kspace_mask_learn.register_fake
def _kspace_mask_learn_fake(x, mask, n_dims, channels, pad=0):
    return x.new_empty(tuple(x.shape[:-1]) + (x.shape[-1] + pad,))


def _kspace_mask_learn_setup(ctx, inputs, output):
    x, mask, n_dims, channels, pad = inputs
    ctx.save_for_backward(x, mask)
    ctx.n_dims, ctx.channels, ctx.d = n_dims, channels, x.shape[-1]
    ctx.cm = 1 if mask.dim() == n_dims else channels


@torch.autograd.function.once_differentiable
def _kspace_mask_learn_backward(ctx, gy):
    # image: the filter is self-adjoint; mask: Re(X conj G) / N per coefficient; the zero pad columns
    # take no gradient, and the view without them is read in place.  Once differentiable: a double
    # backward raises instead of dropping the mask's share of the second derivative.
    x, mask = ctx.saved_tensors
    g = gy[..., : ctx.d]
    gx = gm = None
    if ctx.needs_input_grad[0]:
        gx = torch.ops.texbias.kspace_mask(g, mask.detach(), ctx.n_dims, ctx.channels, 0)
    if ctx.needs_input_grad[1]:
        gm = torch.ops.texbias.kspace_mask_grad(x, g, ctx.n_dims, ctx.channels, ctx.cm)
    return gx, gm, None, None, None


kspace_mask_learn.register_autograd(_kspace_mask_learn_backward, setup_context=_kspace_mask_learn_setup)


@torch.library.custom_op("texbias::kspace_cmask", mutates_args=())
def kspace_cmask(x: torch.Tensor, mask: torch.Tensor, n_dims: int, channels: int, pad: int = 0,
                 conj: bool = False) -> torch.Tensor:
    """``texbias::kspace_mask`` with a complex64 mask (TB_OP_CMASK): y = Re(IFFT(ifftshift(mask *
    fftshift(FFT(x))))), ``spatial`` or ``(channels,) + spatial``, contiguous, on x's device.  ``conj``:
    conj(mask) instead, the adjoint of the same op, read from the same buffer."""
    return rt.kspace_cmask(x, mask, n_dims, pad=pad, channels=channels, conj=conj)


@kspace_cmask.register_fake
def _kspace_cmask_fake(x, mask, n_dims, channels, pad=0, conj=False):
    return x.new_empty(tuple(x.shape[:-1]) + (x.shape[-1] + pad,))


def _kspace_cmask_setup(ctx, inputs, output):
    x, mask, n_dims, channels, pad, conj = inputs
    if mask.requires_grad:
        raise ValueError("texbias::kspace_cmask has no gradient w.r.t. the mask (use texbias::kspace_cmask_learn)")
    ctx.save_for_backward(mask)
    ctx.n_dims, ctx.channels, ctx.d, ctx.conj = n_dims, channels, x.shape[-1], conj


def _kspace_cmask_backward(ctx, gy):
    # the adjoint of x -> Re(IFFT(M FFT x)) is g -> Re(IFFT(conj(M) FFT g)): the same op with the
    # conjugate flag toggled; the zero pad columns take no gradient
    (mask,) = ctx.saved_tensors
    gx = torch.ops.texbias.kspace_cmask(gy[..., : ctx.d], mask, ctx.n_dims, ctx.channels, 0, not ctx.conj)
    return gx, None, None, None, None, None


kspace_cmask.register_autograd(_kspace_cmask_backward, setup_context=_kspace_cmask_setup)


@torch.library.custom_op("texbias::kspace_cmask_grad", mutates_args=())
def kspace_cmask_grad(x: torch.Tensor, g: torch.Tensor, n_dims: int, channels: int, mask_channels: int) -> torch.Tensor:
    """Gradient of ``kspace_cmask(x, M)`` with respect to the complex mask for the upstream gradient ``g``:
    complex64, conj(FFT x) FFT g / N (torch's convention for a complex leaf), shapes and sums as
    ``kspace_mask_grad``.  No autograd formula (double backward is not supported)."""
    return rt.kspace_cmask_grad(x, g, n_dims, mask_channels, channels)


@kspace_cmask_grad.register_fake
def _kspace_cmask_grad_fake(x, g, n_dims, channels, mask_channels):
    spatial = tuple(x.shape[x.dim() - n_dims:])
    return x.new_empty(spatial if mask_channels == 1 else (mask_channels,) + spatial, dtype=torch.complex64)


@torch.library.custom_op("texbias::kspace_cmask_learn", mutates_args=())
def kspace_cmask_learn(x: torch.Tensor, mask: torch.Tensor, n_dims: int, channels: int, pad: int = 0) -> torch.Tensor:
    """``texbias::kspace_cmask`` (the same fused pass, bit for bit) for a learnable complex mask: autograd
    with respect to the image and to the mask."""
    return rt.kspace_cmask_learn(x, mask, n_dims, pad=pad, channels=channels)


@kspace_cmask_learn.register_fake
def _kspace_cmask_learn_fake(x, mask, n_dims, channels, pad=0):
    return x.new_empty(tuple(x.shape[:-1]) + (x.shape[-1] + pad,))


def _kspace_cmask_learn_setup(ctx, inputs, output):
    x, mask, n_dims, channels, pad = inputs
    ctx.save_for_backward(x, mask)
    ctx.n_dims, ctx.channels, ctx.d = n_dims, channels, x.shape[-1]
    ctx.cm = 1 if mask.dim() == n_dims else channels


@torch.autograd.function.once_differentiable
def _kspace_cmask_learn_backward(ctx, gy):
    # image: the op with the conjugate flag; mask: conj(X) G / N per coefficient.  Only the gradients
    # asked for are launched; once differentiable, as kspace_mask_learn.
    x, mask = ctx.saved_tensors
    g = gy[..., : ctx.d]
    gx = gm = None
    if ctx.needs_input_grad[0]:
        gx = torch.ops.texbias.kspace_cmask(g, mask.detach(), ctx.n_dims, ctx.channels, 0, True)
    if ctx.needs_input_grad[1]:
        gm = torch.ops.texbias.kspace_cmask_grad(x, g, ctx.n_dims, ctx.channels, ctx.cm)
    return gx, gm, None, None, None


kspace_cmask_learn.register_autograd(_kspace_cmask_learn_backward, setup_context=_kspace_cmask_learn_setup)


@torch.library.custom_op("texbias::shift_fourier", mutates_args=())
def shift_fourier(x: torch.Tensor, n_dims: int) -> torch.Tensor:
    """K = fftshift(fftn(x, dims), dims) over the trailing ``n_dims`` axes: float32 in, complex64 out in
    the centred layout of ``texbias::kspace_mask`` (``runtime.kspace_export``)."""
    return rt.kspace_export(x, n_dims)


@shift_fourier.register_fake
def _shift_fourier_fake(x, n_dims):
    return x.new_empty(x.shape, dtype=torch.complex64)


@torch.library.custom_op("texbias::inv_shift_fourier", mutates_args=())
def inv_shift_fourier(k: torch.Tensor, n_dims: int, pad: int = 0) -> torch.Tensor:
    """y = Re(ifftn(ifftshift(k, dims), dims)) over the trailing ``n_dims`` axes for any complex64 ``k``
    (last axis padded by ``pad`` zero columns): float32 out (``runtime.kspace_import``)."""
    return rt.kspace_import(k, n_dims, pad=pad)


@inv_shift_fourier.register_fake
def _inv_shift_fourier_fake(k, n_dims, pad=0):
    return k.new_empty(tuple(k.shape[:-1]) + (k.shape[-1] + pad,), dtype=torch.float32)


def _spatial_count(shape, n_dims: int) -> float:
    return float(int(np.prod([int(s) for s in shape[len(shape) - n_dims:]])))


# The two maps are each other's adjoint up to N = the number of transformed voxels: with the upstream
# gradient of a complex tensor in PyTorch's convention dL/dRe + i dL/dIm,
#   K = shift_fourier(x):      gx = N inv_shift_fourier(gK)
#   y = inv_shift_fourier(K):  gK = shift_fourier(gy[..., :D]) / N   (the zero pad columns take no gradient)
# Each backward is the other op, so both are differentiable any number of times.
def _shift_fourier_setup(ctx, inputs, output):
    x, n_dims = inputs
    ctx.n_dims, ctx.n = n_dims, _spatial_count(x.shape, n_dims)


def _shift_fourier_backward(ctx, gk):
    if not ctx.needs_input_grad[0]:
        return None, None
    return torch.ops.texbias.inv_shift_fourier(gk, ctx.n_dims, 0) * ctx.n, None


def _inv_shift_fourier_setup(ctx, inputs, output):
    k, n_dims, pad = inputs
    ctx.n_dims, ctx.d, ctx.n = n_dims, k.shape[-1], _spatial_count(k.shape, n_dims)


def _inv_shift_fourier_backward(ctx, gy):
    if not ctx.needs_input_grad[0]:
        return None, None, None
    return torch.ops.texbias.shift_fourier(gy[..., : ctx.d], ctx.n_dims) / ctx.n, None, None


shift_fourier.register_autograd(_shift_fourier_backward, setup_context=_shift_fourier_setup)
inv_shift_fourier.register_autograd(_inv_shift_fourier_backward, setup_context=_inv_shift_fourier_setup)


# ------------------------------------------------------------------ radial profiles (runtime.radial_*)
@torch.library.custom_op("texbias::radial_mask", mutates_args=())
def radial_mask(profile: torch.Tensor, spatial: Sequence[int], dr: float, mode: int) -> torch.Tensor:
    """Expand a radial profile [K] or [C, K] to the centred mask of ``texbias::kspace_mask``: ``spatial`` or
    ``(C,) + spatial``.  No autograd formula (``texbias::radial_filter`` has the gradient)."""
    return rt.radial_mask(profile, spatial, dr, mode)


@radial_mask.register_fake
def _radial_mask_fake(profile, spatial, dr, mode):
    sp = tuple(int(v) for v in spatial)
    return profile.new_empty(sp if profile.dim() == 1 else (profile.shape[0],) + sp)


@torch.library.custom_op("texbias::radial_bin", mutates_args=())
def radial_bin(a: torch.Tensor, n_dims: int, bins: int, dr: float, mode: int) -> torch.Tensor:
    """The adjoint of ``texbias::radial_mask``: a real centred array ``spatial`` or ``(C,) + spatial`` summed over
    its radial bins, [bins] or [C, bins].  No autograd formula."""
    return rt.radial_bin(a, n_dims, bins, dr, mode)


@radial_bin.register_fake
def _radial_bin_fake(a, n_dims, bins, dr, mode):
    return a.new_empty((bins,) if a.dim() == n_dims else (a.shape[0], bins))


@torch.library.custom_op("texbias::radial_grad", mutates_args=())
def radial_grad(x: torch.Tensor, g: torch.Tensor, n_dims: int, channels: int, profile_channels: int, bins: int,
                dr: float, mode: int) -> torch.Tensor:
    """Gradient of ``radial_filter(x, p)`` with respect to the profile for the upstream gradient ``g``: [bins] for
    ``profile_channels`` = 1 (summed over the channels), else [channels, bins]; summed over the samples.  No
    autograd formula (double backward is not supported)."""
    return rt.radial_grad(x, g, n_dims, profile_channels, bins, dr, mode, channels)


@radial_grad.register_fake
def _radial_grad_fake(x, g, n_dims, channels, profile_channels, bins, dr, mode):
    return x.new_empty((bins,) if profile_channels == 1 else (profile_channels, bins))


@torch.library.custom_op("texbias::radial_power", mutates_args=())
def radial_power(x: torch.Tensor, n_dims: int, bins: int, dr: float, mode: int) -> torch.Tensor:
    """Radially binned power spectrum of every volume of [*lead, *spatial]: [*lead, bins], with
    P.sum(-1) = (x**2).sum(spatial).  Autograd with respect to ``x``, once differentiable."""
    return rt.radial_power(x, n_dims, bins, dr, mode)


@radial_power.register_fake
def _radial_power_fake(x, n_dims, bins, dr, mode):
    return x.new_empty(tuple(x.shape[: x.dim() - n_dims]) + (bins,))


def _radial_power_setup(ctx, inputs, output):
    x, n_dims, bins, dr, mode = inputs
    ctx.save_for_backward(x)
    ctx.n_dims, ctx.dr, ctx.mode = n_dims, dr, mode


@torch.autograd.function.once_differentiable
def _radial_power_backward(ctx, gp):
    # P = x^T (F^H diag(w_k) F / N) x per volume, so gx = 2 Re(IFFT(M FFT x)) with M = expand(gP): one mask per
    # volume, run as one sample of B C channels with a [B C][H][W][D] mask
    (x,) = ctx.saved_tensors
    if not ctx.needs_input_grad[0]:
        return None, None, None, None, None
    spatial = tuple(x.shape[x.dim() - ctx.n_dims:])
    bc = int(np.prod(x.shape[: x.dim() - ctx.n_dims])) if x.dim() > ctx.n_dims else 1
    prof = gp.reshape(bc, gp.shape[-1]).to(torch.float32).contiguous()
    m = torch.ops.texbias.radial_mask(prof, list(spatial), ctx.dr, ctx.mode)
    gx = torch.ops.texbias.kspace_mask(x.reshape((1, bc) + spatial), m, ctx.n_dims, bc, 0)
    return gx.reshape(x.shape) * 2.0, None, None, None, None


radial_power.register_autograd(_radial_power_backward, setup_context=_radial_power_setup)


@torch.library.custom_op("texbias::radial_filter", mutates_args=())
def radial_filter(x: torch.Tensor, profile: torch.Tensor, n_dims: int, channels: int, dr: float, mode: int,
                  pad: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """y = kspace_mask(x, M) with M = radial_mask(profile): a k-space mask that is a function of radius, ``profile``
    [K] (shared by every channel) or [channels, K].  The profile is expanded once per call (4 Cp N bytes,
    independent of the batch size) and the image takes the existing TB_OP_MASK routes.  Returns (y, M); M is
    a fresh tensor, kept for the backward.  Autograd with respect to ``x`` and ``profile``, each launched only
    when asked for; once differentiable."""
    spatial = tuple(x.shape[x.dim() - n_dims:])
    m = rt.radial_mask(profile.detach(), spatial, dr, mode)
    return rt.kspace_mask(x, m, n_dims, pad=pad, channels=channels), m


@radial_filter.register_fake
def _radial_filter_fake(x, profile, n_dims, channels, dr, mode, pad=0):
    spatial = tuple(x.shape[x.dim() - n_dims:])
    return (x.new_empty(tuple(x.shape[:-1]) + (x.shape[-1] + pad,)),
            x.new_empty(spatial if profile.dim() == 1 else (profile.shape[0],) + spatial))


def _radial_filter_setup(ctx, inputs, output):
    x, profile, n_dims, channels, dr, mode, pad = inputs
    ctx.save_for_backward(x, output[1])
    ctx.mark_non_differentiable(output[1])
    ctx.n_dims, ctx.channels, ctx.d, ctx.dr, ctx.mode = n_dims, channels, x.shape[-1], dr, mode
    ctx.cp = 1 if profile.dim() == 1 else channels
    ctx.bins, ctx.pshape = profile.shape[-1], tuple(profile.shape)


@torch.autograd.function.once_differentiable
def _radial_filter_backward(ctx, gy, gm):
    # image: the real symmetric mask makes the filter self-adjoint; profile: the mask gradient summed over
    # shells, without the dense dM; the zero pad columns take no gradient
    x, m = ctx.saved_tensors
    g = gy[..., : ctx.d]
    gx = gp = None
    if ctx.needs_input_grad[0]:
        gx = torch.ops.texbias.kspace_mask(g, m, ctx.n_dims, ctx.channels, 0)
    if ctx.needs_input_grad[1]:
        gp = torch.ops.texbias.radial_grad(x, g, ctx.n_dims, ctx.channels, ctx.cp, ctx.bins, ctx.dr, ctx.mode)
        gp = gp.reshape(ctx.pshape)   # [1, K] for one channel
    return gx, gp, None, None, None, None, None


radial_filter.register_autograd(_radial_filter_backward, setup_context=_radial_filter_setup)


# ------------------------------------------------------------------ trainable spikes (runtime.kspace_spikes*)
@torch.library.custom_op("texbias::kspace_spikes", mutates_args=())
def kspace_spikes(x: torch.Tensor, log_intensity: torch.Tensor, loc: Sequence[int], n_dims: int, channels: int,
                  pad: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """The spike layer: |K(f_j)| := exp(log_intensity[j]) at S centred locations on every channel of
    [B*channels..., *spatial], phase kept (last axis padded by ``pad`` zero columns).  ``loc``: flat list of
    S * n_dims indices into the layout of ``Fourier.shift_fourier`` (the reference's ``loc``), no two at equal or
    conjugate frequencies; ``log_intensity``: float32 [S] on x's device, read by the kernels on the current stream
    (no host sync).  Returns (y, coef), coef float64 [*lead, S, 2] = K(f_j) of x, kept for the backward.  Autograd
    with respect to ``x`` and ``log_intensity``, each launched only when asked for; once differentiable."""
    return rt.kspace_spikes(x, log_intensity, loc, n_dims, channels, pad)


def _spikes_count(loc, n_dims: int) -> int:
    if n_dims < 1 or len(loc) % n_dims or not len(loc):
        raise ValueError(f"texbias::kspace_spikes: {len(loc)} location indices for {n_dims} transformed axes")
    return len(loc) // n_dims


@kspace_spikes.register_fake
def _kspace_spikes_fake(x, log_intensity, loc, n_dims, channels, pad=0):
    S = _spikes_count(loc, n_dims)
    lead = tuple(x.shape[: x.dim() - n_dims])
    return (x.new_empty(tuple(x.shape[:-1]) + (x.shape[-1] + pad,)),
            x.new_empty(lead + (S, 2), dtype=torch.float64))


@torch.library.custom_op("texbias::kspace_spikes_grad", mutates_args=())
def kspace_spikes_grad(g: torch.Tensor, coef: torch.Tensor, log_intensity: torch.Tensor, loc: Sequence[int],
                       n_dims: int, channels: int, image_grad: bool,
                       intensity_grad: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """The gradients of ``kspace_spikes`` for the upstream gradient ``g`` (the image's shape, any strides with a
    contiguous last axis) and the ``coef`` of its forward: (gx, dI), dI float32 [S] summed over every
    volume-channel.  ``image_grad`` False: no streaming pass is launched and gx is an empty tensor;
    ``intensity_grad`` False: the ordered sum is not launched and dI is an empty tensor.  No autograd formula
    (double backward is not supported)."""
    gx, dI = rt.kspace_spikes_grad(g, coef, log_intensity, loc, n_dims, channels, image_grad, intensity_grad)
    return (gx if image_grad else g.new_empty((0,))), (dI if intensity_grad else g.new_empty((0,)))


@kspace_spikes_grad.register_fake
def _kspace_spikes_grad_fake(g, coef, log_intensity, loc, n_dims, channels, image_grad, intensity_grad=True):
    S = _spikes_count(loc, n_dims)
    return g.new_empty(g.shape if image_grad else (0,)), g.new_empty((S,) if intensity_grad else (0,))


def _kspace_spikes_setup(ctx, inputs, output):
    x, log_intensity, loc, n_dims, channels, pad = inputs
    ctx.save_for_backward(output[1], log_intensity)
    ctx.mark_non_differentiable(output[1])
    ctx.loc, ctx.n_dims, ctx.channels, ctx.d = [int(v) for v in loc], n_dims, channels, x.shape[-1]


@torch.autograd.function.once_differentiable
def _kspace_spikes_backward(ctx, gy, gcoef):
    # one coefficient per spike of the upstream gradient, then Gamma_j and the dI shares (csrc/spike_grad.h); the
    # image gradient is one more plane-wave add and the intensity gradient one ordered sum, each launched only
    # when asked for; the zero pad columns take no gradient, and the view without them is read in place
    coef, log_intensity = ctx.saved_tensors
    gx = dI = None
    if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
        rx, rI = torch.ops.texbias.kspace_spikes_grad(gy[..., : ctx.d], coef, log_intensity.detach(), ctx.loc, ctx.n_dims,
                                                      ctx.channels, bool(ctx.needs_input_grad[0]),
                                                      bool(ctx.needs_input_grad[1]))
        gx = rx if ctx.needs_input_grad[0] else None
        dI = rI if ctx.needs_input_grad[1] else None
    return gx, dI, None, None, None, None


kspace_spikes.register_autograd(_kspace_spikes_backward, setup_context=_kspace_spikes_setup)


# amplitude mixing (csrc/ampmix.h): the phase of x's spectrum with an amplitude moved towards a partner's
@torch.library.custom_op("texbias::amp_mix", mutates_args=())
def amp_mix(x: torch.Tensor, y: torch.Tensor, mask: torch.Tensor, lam: torch.Tensor, perm: Optional[torch.Tensor],
            n_dims: int, channels: int, pad: int = 0) -> torch.Tensor:
    """out[b] = Re(ifftn(ifftshift(polar((1 - m) |X| + m |Y|, angle(X))))) over the trailing ``n_dims`` axes of
    [B, channels, *spatial], X = fftshift(fftn(x[b])), Y = fftshift(fftn(y[perm[b]])), m = lam[b] * mask:
    ``mask`` as in ``kspace_mask`` (``spatial`` or ``(channels,) + spatial``), ``lam`` float32 [B] and ``perm``
    int32 [B] (or None: identity) on x's device, read by the kernel on the current stream.  ``y`` may be ``x``
    itself: the partners are then rows of x and only one set of forward passes runs.  Autograd with respect
    to ``x`` and ``y``; ``lam`` and ``mask`` are constants (their gradients are None)."""
    return rt.kspace_ampmix(x, y, mask, lam, perm, n_dims, channels, pad)


@amp_mix.register_fake
def _amp_mix_fake(x, y, mask, lam, perm, n_dims, channels, pad=0):
    return x.new_empty(tuple(x.shape[:-1]) + (x.shape[-1] + pad,))


@torch.library.custom_op("texbias::amp_mix_grad", mutates_args=())
def amp_mix_grad(x: torch.Tensor, y: torch.Tensor, mask: torch.Tensor, lam: torch.Tensor,
                 perm: Optional[torch.Tensor], g: torch.Tensor, n_dims: int, channels: int,
                 need_gy: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """The gradients of ``amp_mix`` with respect to ``x`` and ``y`` for the upstream gradient ``g`` (x's shape,
    any strides with a contiguous last axis): (gx, gy); gy summed over equal partners in a fixed order.
    ``need_gy`` False: the partner's gradient is neither computed nor stored and gy is an empty tensor.  No
    autograd formula (double backward is not supported)."""
    gx, gy = rt.kspace_ampmix_grad(x, y, mask, lam, perm, g, n_dims, channels, need_gy)
    return gx, (gy if need_gy else g.new_empty((0,)))


@amp_mix_grad.register_fake
def _amp_mix_grad_fake(x, y, mask, lam, perm, g, n_dims, channels, need_gy):
    return x.new_empty(x.shape), x.new_empty(x.shape if need_gy else (0,))


def _amp_mix_setup(ctx, inputs, output):
    x, y, mask, lam, perm, n_dims, channels, pad = inputs
    if mask.requires_grad or lam.requires_grad:
        raise ValueError("texbias::amp_mix has no gradient w.r.t. the mask or lam (both are constants)")
    ctx.save_for_backward(x, y, mask, lam, perm)
    ctx.n_dims, ctx.channels, ctx.d = n_dims, channels, x.shape[-1]


@torch.autograd.function.once_differentiable
def _amp_mix_backward(ctx, go):
    # closed form per coefficient (csrc/ampmix.h); the partner's share only when y requires grad; the zero pad
    # columns take no gradient, and the view without them is read in place.  When y is x, autograd adds the
    # two returned gradients into the one leaf.
    x, y, mask, lam, perm = ctx.saved_tensors
    gx = gy = None
    if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
        need_gy = bool(ctx.needs_input_grad[1])
        rx, ry = torch.ops.texbias.amp_mix_grad(x, y, mask, lam, perm, go[..., : ctx.d], ctx.n_dims, ctx.channels,
                                                need_gy)
        gx = rx if ctx.needs_input_grad[0] else None
        gy = ry if need_gy else None
    return gx, gy, None, None, None, None, None, None


amp_mix.register_autograd(_amp_mix_backward, setup_context=_amp_mix_setup)


def _layer_apply(img: torch.Tensor, alpha: torch.Tensor) -> torch.Tensor:
    B = img.shape[0]
    n_dims = img.dim() - 1
    spatial = tuple(img.shape[1:])
    a = alpha.detach().reshape(-1)[:1].to(device=img.device, dtype=torch.float32).contiguous()
    # the kernel reads alpha from device memory (no host round trip for Gibbs_GD updates); `a`
    # aliases the alpha buffer or is a stream-ordered temporary, so the read is safe
    prog = [K.layer_op(0.0, spatial, alpha_ptr=a.data_ptr())]
    x = img if img.dtype == torch.float32 else img.float()
    y = rt.kspace_filter(x.reshape((B, 1) + spatial), n_dims, [prog] * B, 1)
    return y.reshape(img.shape)


@torch.library.custom_op("texbias::gibbs_layer", mutates_args=())
def gibbs_layer(img: torch.Tensor, alpha: torch.Tensor) -> torch.Tensor:
    """GibbsNoiseLayer's low-pass over all non-batch axes with the device-resident alpha."""
    return _layer_apply(img.contiguous(), alpha)


@gibbs_layer.register_fake
def _gibbs_layer_fake(img, alpha):
    return torch.empty_like(img, dtype=torch.float32)


def _gibbs_layer_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[1])


def _gibbs_layer_backward(ctx, gy):
    (alpha,) = ctx.saved_tensors
    return torch.ops.texbias.gibbs_layer(gy, alpha), torch.zeros_like(alpha)


gibbs_layer.register_autograd(_gibbs_layer_backward, setup_context=_gibbs_layer_setup)
