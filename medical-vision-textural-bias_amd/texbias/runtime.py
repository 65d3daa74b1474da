"""Device runtime: plans, workspaces and the batched launch wrappers over the C ABI.

Tensors are torch CUDA (HIP) tensors; launches go on the caller's current
stream (``torch.cuda.current_stream``) so they order with surrounding torch
work and graph-capture with it.  Raises if a tensor is not on a HIP device:
this is the product path and it has no CPU implementation.
"""
from __future__ import annotations

import ctypes as C
import threading
from collections import OrderedDict
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._abi import TB_MAX_BATCH, TB_MAX_OPS, programs_array
from ._lib import TexbiasError, check, lib
from .kprog import Geometry, cmask_op, geometry, mask_op, split_program, unshift

_plans: Dict[Tuple[int, int, int, int], "Plan"] = {}
_ws: "OrderedDict[Tuple[int, int], torch.Tensor]" = OrderedDict()
_ws_lock = threading.Lock()
_mm: Dict[int, torch.Tensor] = {}
_lock = threading.Lock()


class Plan:
    def __init__(self, device: torch.device, H: int, W: int, D: int):
        self.device, self.H, self.W, self.D = device, H, W, D
        h = C.c_void_p()
        with torch.cuda.device(device):
            check(lib().tb_plan_create(H, W, D, C.byref(h)), f"plan {H}x{W}x{D}")
        self.handle = h

    def radices(self, axis: int) -> List[int]:
        buf = (C.c_int * 8)()
        n = lib().tb_plan_radices(self.handle, axis, buf)
        return list(buf[:n])

    def workspace_bytes(self, bc: int) -> int:
        return int(lib().tb_workspace_bytes(self.handle, bc))

    def __del__(self):  # pragma: no cover - interpreter shutdown order
        try:
            if self.handle:
                lib().tb_plan_destroy(self.handle)
        except Exception:
            pass


def require_hip(t: torch.Tensor, what: str) -> None:
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise TexbiasError(f"{what}: expected a HIP (cuda) tensor, got {getattr(t, 'device', type(t))}")
    if t.dtype != torch.float32:
        raise TexbiasError(f"{what}: expected float32, got {t.dtype}")


def plan_for(device: torch.device, H: int, W: int, D: int) -> Plan:
    idx = device.index if device.index is not None else torch.cuda.current_device()
    key = (idx, H, W, D)
    p = _plans.get(key)
    if p is None:
        with _lock:
            p = _plans.get(key)
            if p is None:
                p = Plan(torch.device("cuda", idx), H, W, D)
                _plans[key] = p
    return p


def _ws_key(device: torch.device) -> Tuple[int, int]:
    """Workspaces are per (device, current stream): the launches of one stream are ordered, so they
    share one; launches from two streams (a side stream, a second thread) get separate scratch --
    the band passes keep their arrival counter and min/max partials in it."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    return idx, torch.cuda.current_stream(torch.device("cuda", idx)).cuda_stream


# Bounded LRU caches: a caller that makes a fresh stream per iteration (or per thread) would otherwise
# keep one spectrum-sized workspace per stream it ever used.  An evicted workspace was allocated on its
# own stream, so the caching allocator hands its memory out again only in that stream's order.
_WS_CAP = 8


def _cached_ws(cache: "OrderedDict[Tuple[int, int], torch.Tensor]", device: torch.device, nbytes: int) -> torch.Tensor:
    key = _ws_key(device)
    with _ws_lock:
        ws = cache.get(key)
        if ws is None or ws.numel() < nbytes:
            ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=torch.device("cuda", key[0]))
        cache[key] = ws
        cache.move_to_end(key)
        while len(cache) > _WS_CAP:
            cache.popitem(last=False)
    return ws


def workspace(device: torch.device, nbytes: int) -> torch.Tensor:
    return _cached_ws(_ws, device, nbytes)


_ws_prep: "OrderedDict[Tuple[int, int], torch.Tensor]" = OrderedDict()


def workspace_prep(device: torch.device, nbytes: int) -> torch.Tensor:
    """Small per-(device, stream) workspace of the preprocessing statistics (kept apart from the
    spectrum workspace so neither reallocates the other)."""
    return _cached_ws(_ws_prep, device, nbytes)


def _stream(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _bc_view(x: torch.Tensor, n_dims: int):
    """View [*lead, *spatial] as (BC, spatial strides) with a single bc stride, else None."""
    lead = x.shape[: x.dim() - n_dims]
    sp = x.shape[x.dim() - n_dims:]
    bc = int(np.prod(lead)) if lead else 1
    st = x.stride()
    lead_st = st[: x.dim() - n_dims]
    sp_st = st[x.dim() - n_dims:]
    # lead dims must collapse to one stride
    bstride = None
    if lead:
        exp = None
        for size, s in zip(reversed(lead), reversed(lead_st)):
            if size == 1:
                continue
            if exp is None:
                exp, bstride = s * size, s
            elif s != exp:
                return None
            else:
                exp = s * size
    if bstride is None:
        bstride = int(np.prod(sp))
    return bc, bstride, sp, sp_st


def _hwd_strides(geo: Geometry, sp_st: Sequence[int]) -> Tuple[int, int, int]:
    k = [sp_st[i] for i in geo.kept]
    if len(k) == 3:
        return k[0], k[1], k[2]
    if len(k) == 2:
        return k[0], 0, k[1]
    if len(k) == 1:
        return 0, 0, k[0]
    return 0, 0, 1


def kspace_filter(x: torch.Tensor, n_dims: int, programs: Sequence[Sequence], channels: int,
                  out: Optional[torch.Tensor] = None, pad: int = 0,
                  minmax: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = Re(IFFT(program_b(FFT(x)))) over the trailing ``n_dims`` axes.

    ``x``: [*lead, *spatial] float32 on a HIP device, lead = (B, C) flattened to B*C with
    ``channels`` = C; ``programs``: B lists of TbOp.  ``pad`` appends zero columns to the
    last axis of the output (U-Net padding).  ``minmax``: optional int32 [B, 2] device
    tensor receiving the per-sample (min, max) keys of the output.  Programs longer than one
    launch holds (TB_MAX_OPS) run as several passes cut where that is exact
    (``kprog.split_program``); the later passes filter the output in place.
    """
    require_hip(x, "kspace_filter")
    if all(len(p) <= TB_MAX_OPS for p in programs):
        return _kspace_filter_pass(x, n_dims, programs, channels, out, pad, minmax)
    hwd = geometry(x.shape[x.dim() - n_dims:]).hwd
    parts = [split_program(list(p), hwd) for p in programs]
    npass = max(len(c) for c in parts)
    passes = [[c[i] if i < len(c) else [] for c in parts] for i in range(npass)]
    y = _kspace_filter_pass(x, n_dims, passes[0], channels, out, pad, minmax)
    view = y[..., : x.shape[-1]] if pad else y
    for prog in passes[1:]:
        _kspace_filter_pass(view, n_dims, prog, channels, view, 0, minmax)
    return y


def planes_closed_form(x: torch.Tensor, n_dims: int, programs: Sequence[Sequence], channels: int,
                       out: Optional[torch.Tensor] = None, pad: int = 0,
                       minmax: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The closed-form spike route alone (``tb_planes_closed_form_f32``): ``kspace_filter`` for
    programs made only of spikes that do not touch; raises for any other program."""
    require_hip(x, "planes_closed_form")
    return _kspace_filter_pass(x, n_dims, programs, channels, out, pad, minmax, entry="tb_planes_closed_form_f32")


def _kspace_filter_pass(x: torch.Tensor, n_dims: int, programs: Sequence[Sequence], channels: int,
                        out: Optional[torch.Tensor] = None, pad: int = 0,
                        minmax: Optional[torch.Tensor] = None, entry: str = "tb_kspace_filter_f32") -> torch.Tensor:
    """One launch group of ``kspace_filter`` (every program at most TB_MAX_OPS ops)."""
    geo = geometry(x.shape[x.dim() - n_dims:])
    H, W, D = geo.hwd
    v = _bc_view(x, n_dims)
    if v is None or _hwd_strides(geo, v[3])[2] != 1:
        x = x.contiguous()
        v = _bc_view(x, n_dims)
    bc, bstride, sp, sp_st = v
    B = len(programs)
    if bc != B * channels:
        raise ValueError(f"{B} programs x {channels} channels != {bc} volumes")
    sh, sw, sd = _hwd_strides(geo, sp_st)
    if sd != 1:
        raise TexbiasError("innermost transformed axis must be contiguous")
    if out is None:
        osh = tuple(x.shape[:-1]) + (x.shape[-1] + pad,)
        out = torch.empty(osh, dtype=torch.float32, device=x.device)
    require_hip(out, "kspace_filter(out)")
    if pad and len(geo.kept) and geo.kept[-1] != n_dims - 1:
        raise TexbiasError("padding requires a non-singleton last axis")
    vo = _bc_view(out, n_dims)
    if vo is None:
        raise TexbiasError("output must collapse its leading axes")
    geo_o = Geometry(tuple(out.shape[out.dim() - n_dims:]), geo.kept)
    osh_, osw, osd = _hwd_strides(geo_o, vo[3])
    if osd != 1:
        raise TexbiasError("output innermost axis must be contiguous")
    plan = plan_for(x.device, H, W, D)
    nbytes = plan.workspace_bytes(bc)
    with torch.cuda.device(x.device):
        ws = workspace(x.device, nbytes)
        xs = (C.c_int64 * 3)(bstride, sh, sw)
        ys = (C.c_int64 * 3)(vo[1], osh_, osw)
        progs = programs_array(programs)
        mm_ptr = None
        if minmax is not None:
            if minmax.dtype != torch.int32 or minmax.numel() < 2 * B or minmax.device != x.device:
                raise TexbiasError("minmax must be an int32 [B,2] tensor on the input's device")
            mm_ptr = minmax.data_ptr()
        check(getattr(lib(), entry)(plan.handle, x.data_ptr(), xs, out.data_ptr(), ys, pad, ws.data_ptr(),
                                    ws.numel(), B, channels, C.addressof(progs), mm_ptr, _stream(x.device)), entry)
    return out


def mask_geometry(x: torch.Tensor, mask: torch.Tensor, n_dims: int, channels: Optional[int] = None,
                  learnable: bool = False) -> Tuple[int, int]:
    """Host-side check of a user k-space mask against the image ``x`` [*lead, *spatial]: returns
    (mask channels, image channels).  The mask is ``spatial`` (shared by every channel) or
    ``(C,) + spatial`` with C = ``channels`` (default: the image's last leading axis); float32,
    contiguous, on the image's device -- the kernels index it as M[Cm][H][W][D] with no copy, so
    nothing else is accepted.  A mask with ``requires_grad`` passes only with ``learnable`` (the
    ``kspace_mask_learn`` path, which has the gradient with respect to the mask)."""
    return _mask_geometry("kspace_mask", torch.float32, x, mask, n_dims, channels, learnable)


def cmask_geometry(x: torch.Tensor, mask: torch.Tensor, n_dims: int, channels: Optional[int] = None,
                   learnable: bool = False) -> Tuple[int, int]:
    """``mask_geometry`` for the complex mask of ``kspace_cmask`` (TB_OP_CMASK): the same shapes,
    complex64 (interleaved re, im: what the kernels load), contiguous, on the image's device."""
    return _mask_geometry("kspace_cmask", torch.complex64, x, mask, n_dims, channels, learnable)


def _mask_geometry(what, dtype, x, mask, n_dims, channels, learnable):
    if not isinstance(x, torch.Tensor) or not isinstance(mask, torch.Tensor):
        raise ValueError(f"{what}: image and mask must be torch tensors")
    if n_dims < 1 or x.dim() < n_dims:
        raise ValueError(f"{what}: {n_dims} transformed axes on a {x.dim()}-d image")
    spatial = tuple(x.shape[x.dim() - n_dims:])
    lead = x.shape[: x.dim() - n_dims]
    if channels is None:
        channels = int(lead[-1]) if len(lead) else 1
    channels = int(channels)
    if channels < 1 or (int(np.prod(lead)) if len(lead) else 1) % channels:
        raise ValueError(f"{what}: {channels} channels do not divide the leading axes {tuple(lead)}")
    if tuple(mask.shape) == spatial:
        cm = 1
    elif tuple(mask.shape) == (channels,) + spatial:
        cm = channels
    else:
        raise ValueError(f"{what}: mask shape {tuple(mask.shape)} is neither {spatial} nor "
                         f"{(channels,) + spatial}")
    if mask.dtype != dtype:
        raise ValueError(f"{what}: the mask must be {str(dtype)[6:]}, got {mask.dtype}")
    if not mask.is_contiguous():
        raise ValueError(f"{what}: the mask must be contiguous")
    if mask.device != x.device:
        raise ValueError(f"{what}: mask on {mask.device}, image on {x.device}")
    if mask.requires_grad and not learnable:
        raise ValueError(f"{what}: a mask with requires_grad is not supported (no gradient w.r.t. the mask)")
    return cm, channels


def kspace_mask(x: torch.Tensor, mask: torch.Tensor, n_dims: int, pad: int = 0,
                out: Optional[torch.Tensor] = None, channels: Optional[int] = None) -> torch.Tensor:
    """y = Re(IFFT(ifftshift(mask * fftshift(FFT(x))))) over the trailing ``n_dims`` axes in one fused
    round trip (TB_OP_MASK): ``mask`` is laid out like ``Fourier.shift_fourier(x, n_dims)``, shape
    ``spatial`` or ``(C,) + spatial`` (see ``mask_geometry``).  ``pad`` / ``out`` as ``kspace_filter``;
    ``out`` may be ``x``; ``channels``: see ``mask_geometry``.  The launch reads ``mask`` on the current
    stream, with no host sync."""
    return _kspace_mask(x, mask, n_dims, pad, out, channels, False)


def kspace_mask_learn(x: torch.Tensor, mask: torch.Tensor, n_dims: int, pad: int = 0,
                      channels: Optional[int] = None) -> torch.Tensor:
    """``kspace_mask`` for a mask that may require grad (the forward of ``torch.ops.texbias.kspace_mask_learn``;
    the gradient with respect to the mask is ``kspace_mask_grad``)."""
    return _kspace_mask(x, mask, n_dims, pad, None, channels, True)


def _kspace_mask(x, mask, n_dims, pad, out, channels, learnable):
    cm, channels = mask_geometry(x, mask, n_dims, channels, learnable)
    require_hip(x, "kspace_mask")
    hwd = geometry(x.shape[x.dim() - n_dims:]).hwd
    lead = x.shape[: x.dim() - n_dims]
    bc = int(np.prod(lead)) if len(lead) else 1
    prog = [mask_op(mask.data_ptr(), cm, hwd)]
    return _kspace_filter_pass(x, n_dims, [prog] * (bc // channels), channels, out, pad)


def kspace_cmask(x: torch.Tensor, mask: torch.Tensor, n_dims: int, pad: int = 0,
                 out: Optional[torch.Tensor] = None, channels: Optional[int] = None,
                 conj: bool = False) -> torch.Tensor:
    """``kspace_mask`` with a complex64 mask (TB_OP_CMASK): a phase ramp (sub-voxel shift, motion), a
    B0-like phase, a complex apodisation -- one fused round trip, no spectrum exported.  The ``.real``
    of the reference makes it the multiplication of every stored coefficient by
    (M[s(f)] + conj(M[s(-f)])) / 2.  ``conj``: use conj(mask), the adjoint of the same op (what the
    autograd with respect to the image runs), read from the same buffer."""
    return _kspace_cmask(x, mask, n_dims, pad, out, channels, False, conj)


def kspace_cmask_learn(x: torch.Tensor, mask: torch.Tensor, n_dims: int, pad: int = 0,
                       channels: Optional[int] = None) -> torch.Tensor:
    """``kspace_cmask`` for a mask that may require grad (the forward of
    ``torch.ops.texbias.kspace_cmask_learn``; the gradient with respect to the mask is ``kspace_cmask_grad``)."""
    return _kspace_cmask(x, mask, n_dims, pad, None, channels, True, False)


def _kspace_cmask(x, mask, n_dims, pad, out, channels, learnable, conj):
    cm, channels = cmask_geometry(x, mask, n_dims, channels, learnable)
    require_hip(x, "kspace_cmask")
    hwd = geometry(x.shape[x.dim() - n_dims:]).hwd
    lead = x.shape[: x.dim() - n_dims]
    bc = int(np.prod(lead)) if len(lead) else 1
    prog = [cmask_op(mask.data_ptr(), cm, hwd, conj=conj)]
    return _kspace_filter_pass(x, n_dims, [prog] * (bc // channels), channels, out, pad)


def kspace_mask_grad(x: torch.Tensor, g: torch.Tensor, n_dims: int, mask_channels: int,
                     channels: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Gradient of ``kspace_mask(x, M)`` with respect to the mask for an upstream gradient ``g`` (the
    image's shape): dM[s(f)] = sum Re(FFT(x)(f) conj(FFT(g)(f))) / N in the mask's centred layout, summed
    over the samples and, with ``mask_channels`` = 1, over the channels.  Returns ``spatial`` for
    ``mask_channels`` = 1, else ``(C,) + spatial`` with C = ``channels`` (default: the image's last
    leading axis).  ``x`` and ``g`` may have any strides with a contiguous last axis (``gy[..., :D]`` of
    a padded output is read in place).  Two forward passes and one per-coefficient pass on the current
    stream (``tb_kspace_mask_grad_f32``); every element is written once, so repeated calls agree bit
    for bit.  ``out``: a float32 contiguous tensor of the result's shape on the image's device to
    overwrite (it need not be zeroed)."""
    return _mask_grad("kspace_mask_grad", torch.float32, x, g, n_dims, mask_channels, channels, out)


def kspace_cmask_grad(x: torch.Tensor, g: torch.Tensor, n_dims: int, mask_channels: int,
                      channels: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Gradient of ``kspace_cmask(x, M)`` with respect to the complex mask, in torch.autograd's convention
    for a complex leaf: dM[s(f)] = sum conj(FFT(x)(f)) FFT(g)(f) / N, complex64, with dM[s(-f)] =
    conj(dM[s(f)]); its real part is ``kspace_mask_grad``'s.  Arguments, sums, strides and ``out``
    (complex64 here) as ``kspace_mask_grad``; ``tb_kspace_cmask_grad_f32``."""
    return _mask_grad("kspace_cmask_grad", torch.complex64, x, g, n_dims, mask_channels, channels, out)


def _grad_pair(what, x, g, n_dims, mask_channels, channels):
    """Host-side check of an (image, upstream gradient) pair and their in-place addressing: (x, xs, g, gs,
    spatial, channels, mask channels, volumes, geometry)."""
    if not isinstance(x, torch.Tensor) or not isinstance(g, torch.Tensor):
        raise ValueError(f"{what}: image and upstream gradient must be torch tensors")
    if n_dims < 1 or x.dim() < n_dims:
        raise ValueError(f"{what}: {n_dims} transformed axes on a {x.dim()}-d image")
    if tuple(g.shape) != tuple(x.shape):
        raise ValueError(f"{what}: upstream gradient {tuple(g.shape)} does not match the image {tuple(x.shape)}")
    if x.dtype != torch.float32 or g.dtype != torch.float32:
        raise ValueError(f"{what}: float32 tensors expected, got {x.dtype} and {g.dtype}")
    if g.device != x.device:
        raise ValueError(f"{what}: upstream gradient on {g.device}, image on {x.device}")
    spatial = tuple(x.shape[x.dim() - n_dims:])
    lead = x.shape[: x.dim() - n_dims]
    if channels is None:
        channels = int(lead[-1]) if len(lead) else 1
    channels, cm = int(channels), int(mask_channels)
    bc = int(np.prod(lead)) if len(lead) else 1
    if channels < 1 or bc % channels:
        raise ValueError(f"{what}: {channels} channels do not divide the leading axes {tuple(lead)}")
    if cm != 1 and cm != channels:
        raise ValueError(f"{what}: {cm} mask channels for {channels} image channels (1 or {channels})")
    require_hip(x, what)
    geo = geometry(spatial)
    H, W, D = geo.hwd

    def strided(t):
        v = _bc_view(t, n_dims)
        if v is None or _hwd_strides(geo, v[3])[2] != 1:
            t = t.contiguous()
            v = _bc_view(t, n_dims)
        return t, (C.c_int64 * 3)(v[1], *_hwd_strides(geo, v[3])[:2])

    x, xs = strided(x)
    g, gs = strided(g)
    return x, xs, g, gs, spatial, channels, cm, bc, geo


def _mask_grad(what, dtype, x, g, n_dims, mask_channels, channels, out):
    x, xs, g, gs, spatial, channels, cm, bc, geo = _grad_pair(what, x, g, n_dims, mask_channels, channels)
    H, W, D = geo.hwd
    shape = spatial if cm == 1 else (cm,) + spatial
    if out is None:
        dm = torch.empty(shape, dtype=dtype, device=x.device)
    else:
        dm = out
        if (not isinstance(dm, torch.Tensor) or tuple(dm.shape) != shape or dm.dtype != dtype
                or not dm.is_contiguous() or dm.device != x.device):
            raise ValueError(f"{what}: out must be a {str(dtype)[6:]} contiguous {shape} tensor on {x.device}")
    plan = plan_for(x.device, H, W, D)
    with torch.cuda.device(x.device):
        ws = workspace(x.device, int(lib().tb_mask_grad_workspace_bytes(plan.handle, bc)))
        name = "tb_kspace_mask_grad_f32" if dtype == torch.float32 else "tb_kspace_cmask_grad_f32"
        check(getattr(lib(), name)(plan.handle, x.data_ptr(), xs, g.data_ptr(), gs, dm.data_ptr(), cm, ws.data_ptr(),
                                   ws.numel(), bc // channels, channels, _stream(x.device)), name)
    return dm


def _spectrum_args(what: str, t: torch.Tensor, n_dims: int, dtype: torch.dtype) -> Tuple[Geometry, int]:
    """Host-side check of an export / import argument [*lead, *spatial]: (geometry, volumes)."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: a torch tensor is expected, got {type(t).__name__}")
    n_dims = int(n_dims)
    if n_dims < 1 or t.dim() < n_dims:
        raise ValueError(f"{what}: {n_dims} transformed axes on a {t.dim()}-d tensor")
    if t.dtype != dtype:
        raise ValueError(f"{what}: {dtype} expected, got {t.dtype}")
    lead = t.shape[: t.dim() - n_dims]
    if t.device.type != "cuda":
        raise TexbiasError(f"{what}: expected a HIP (cuda) tensor, got {t.device}")
    return geometry(tuple(t.shape[t.dim() - n_dims:])), (int(np.prod(lead)) if len(lead) else 1)


def _image_strides(t: torch.Tensor, n_dims: int, geo: Geometry):
    """(bc stride, h stride, w stride) of an image, or None when it is not addressable in place (leading
    axes that do not collapse, a strided last axis)."""
    v = _bc_view(t, n_dims)
    if v is None:
        return None
    sh, sw, sd = _hwd_strides(geo, v[3])
    if sd != 1:
        return None
    return (C.c_int64 * 3)(v[1], sh, sw)


def kspace_export(x: torch.Tensor, n_dims: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K = fftshift(fftn(x, dims), dims) over the trailing ``n_dims`` axes (``Fourier.shift_fourier``):
    ``x`` float32 [*lead, *spatial] with any strides and a contiguous last axis (read in place), K complex64
    of x's shape, contiguous, in the centred layout of ``kspace_mask``.  Pass A and one per-coefficient
    pass on the current stream (``tb_kspace_export_f32``); every element of K is written once, f and -f
    from one value, so repeated calls agree bit for bit.  ``out``: a complex64 contiguous tensor of x's
    shape on its device to overwrite (it need not be zeroed)."""
    geo, bc = _spectrum_args("kspace_export", x, n_dims, torch.float32)
    H, W, D = geo.hwd
    xs = _image_strides(x, n_dims, geo)
    if xs is None:
        x = x.contiguous()
        xs = _image_strides(x, n_dims, geo)
    if out is None:
        k = torch.empty(x.shape, dtype=torch.complex64, device=x.device)
    else:
        k = out
        if (not isinstance(k, torch.Tensor) or tuple(k.shape) != tuple(x.shape) or k.dtype != torch.complex64
                or not k.is_contiguous() or k.device != x.device):
            raise ValueError(f"kspace_export: out must be a complex64 contiguous {tuple(x.shape)} tensor on {x.device}")
    plan = plan_for(x.device, H, W, D)
    with torch.cuda.device(x.device):
        ws = workspace(x.device, int(lib().tb_spectrum_workspace_bytes(plan.handle, bc)))
        check(lib().tb_kspace_export_f32(plan.handle, x.data_ptr(), xs, k.data_ptr(), ws.data_ptr(), ws.numel(),
                                         bc, 1, _stream(x.device)), "tb_kspace_export_f32")
    return k


def kspace_import(k: torch.Tensor, n_dims: int, pad: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = Re(ifftn(ifftshift(k, dims), dims)) over the trailing ``n_dims`` axes
    (``Fourier.inv_shift_fourier``) for any complex64 ``k`` [*lead, *spatial] -- it need not be Hermitian:
    the result is the exact inverse of the symmetrised (k(f) + conj(k(-f))) / 2.  ``pad`` appends zero
    columns to the last axis.  One per-coefficient pass and pass C on the current stream
    (``tb_kspace_import_f32``).  ``out``: a float32 tensor [*lead, *spatial[:-1], D + pad] on k's device
    with a contiguous last axis; a strided view is written in place, bytes outside it are not touched."""
    geo, bc = _spectrum_args("kspace_import", k, n_dims, torch.complex64)
    H, W, D = geo.hwd
    pad = int(pad)
    if pad < 0:
        raise ValueError(f"kspace_import: pad must be >= 0, got {pad}")
    if pad and len(geo.kept) and geo.kept[-1] != n_dims - 1:
        raise ValueError("kspace_import: padding requires a non-singleton last axis")
    k = k.resolve_conj().contiguous()   # a lazily conjugated view shares its base's memory
    shape = tuple(k.shape[:-1]) + (k.shape[-1] + pad,)
    if out is None:
        y = torch.empty(shape, dtype=torch.float32, device=k.device)
    else:
        y = out
        if (not isinstance(y, torch.Tensor) or tuple(y.shape) != shape or y.dtype != torch.float32
                or y.device != k.device):
            raise ValueError(f"kspace_import: out must be a float32 {shape} tensor on {k.device}")
    ys = _image_strides(y, n_dims, geo)
    if ys is None:
        raise ValueError("kspace_import: out must collapse its leading axes and have a contiguous last axis")
    plan = plan_for(k.device, H, W, D)
    with torch.cuda.device(k.device):
        ws = workspace(k.device, int(lib().tb_spectrum_workspace_bytes(plan.handle, bc)))
        check(lib().tb_kspace_import_f32(plan.handle, k.data_ptr(), y.data_ptr(), ys, pad, ws.data_ptr(), ws.numel(),
                                         bc, 1, _stream(k.device)), "tb_kspace_import_f32")
    return y


# ------------------------------------------------------------------ amplitude mixing (tb_kspace_ampmix_*, csrc/ampmix.h)
def _ampmix_args(what, x, y, mask, lam, perm, n_dims, channels):
    """Host-side check of the arguments of amplitude mixing: (x, xs, y or None, ys, mask channels, channels,
    samples, geometry).  ``y`` that is ``x`` (the same storage, shape and strides) comes back as None: the
    partners are then rows of x and only one set of forward passes runs."""
    if not isinstance(y, torch.Tensor):
        raise ValueError(f"{what}: image and partner must be torch tensors")
    cm, channels = _mask_geometry(what, torch.float32, x, mask, n_dims, channels, False)
    if tuple(y.shape) != tuple(x.shape):
        raise ValueError(f"{what}: partner {tuple(y.shape)} does not match the image {tuple(x.shape)}")
    if x.dtype != torch.float32 or y.dtype != torch.float32:
        raise ValueError(f"{what}: float32 tensors expected, got {x.dtype} and {y.dtype}")
    if y.device != x.device:
        raise ValueError(f"{what}: partner on {y.device}, image on {x.device}")
    lead = x.shape[: x.dim() - n_dims]
    bc = int(np.prod(lead)) if len(lead) else 1
    B = bc // channels
    if not isinstance(lam, torch.Tensor) or lam.dtype != torch.float32 or tuple(lam.shape) != (B,) \
            or not lam.is_contiguous():
        raise ValueError(f"{what}: lam must be a float32 contiguous [{B}] tensor (one strength per sample)")
    if perm is not None and (not isinstance(perm, torch.Tensor) or perm.dtype != torch.int32
                             or tuple(perm.shape) != (B,) or not perm.is_contiguous()):
        raise ValueError(f"{what}: perm must be None or an int32 contiguous [{B}] tensor (one partner per sample)")
    for name, t in (("lam", lam), ("perm", perm)):
        if t is not None and t.device != x.device:
            raise ValueError(f"{what}: {name} on {t.device}, image on {x.device} (both are read by the kernel)")
    require_hip(x, what)
    geo = geometry(tuple(x.shape[x.dim() - n_dims:]))
    same = y is x or (y.data_ptr() == x.data_ptr() and y.stride() == x.stride())

    def strided(t):
        s = _image_strides(t, n_dims, geo)
        if s is None:
            t = t.contiguous()
            s = _image_strides(t, n_dims, geo)
        return t, s

    x, xs = strided(x)
    if same:
        return x, xs, None, None, cm, channels, B, geo
    y, ys = strided(y)
    return x, xs, y, ys, cm, channels, B, geo


def kspace_ampmix(x: torch.Tensor, y: torch.Tensor, mask: torch.Tensor, lam: torch.Tensor,
                  perm: Optional[torch.Tensor], n_dims: int, channels: Optional[int] = None, pad: int = 0,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Amplitude mixing over the trailing ``n_dims`` axes of ``x`` [B, C, *spatial]: sample b keeps the phase of
    its spectrum and takes the amplitude (1 - m) |X| + m |Y| with Y the spectrum of ``y[perm[b]]`` and
    m = ``lam[b]`` * ``mask`` (``mask`` as in ``kspace_mask``; ``lam`` float32 [B] and ``perm`` int32 [B] or
    None on x's device, read by the kernel on the current stream -- no host read).  ``y`` may be ``x``
    itself (batch-internal mixing, one set of forward passes).  ``perm`` values outside [0, B) are clamped
    by the kernel; the caller owes a valid index.  ``pad`` / ``out`` as ``kspace_import``.  No spectrum is
    stored outside the workspace (``tb_kspace_ampmix_f32``)."""
    what = "kspace_ampmix"
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{what}: image and partner must be torch tensors")
    x, xs, y, ys, cm, channels, B, geo = _ampmix_args(what, x, y, mask, lam, perm, n_dims, channels)
    H, W, D = geo.hwd
    pad = int(pad)
    if pad < 0:
        raise ValueError(f"{what}: pad must be >= 0, got {pad}")
    if pad and len(geo.kept) and geo.kept[-1] != n_dims - 1:
        raise ValueError(f"{what}: padding requires a non-singleton last axis")
    shape = tuple(x.shape[:-1]) + (x.shape[-1] + pad,)
    if out is None:
        o = torch.empty(shape, dtype=torch.float32, device=x.device)
    else:
        o = out
        if not isinstance(o, torch.Tensor) or tuple(o.shape) != shape or o.dtype != torch.float32 or o.device != x.device:
            raise ValueError(f"{what}: out must be a float32 {shape} tensor on {x.device}")
    os_ = _image_strides(o, n_dims, geo)
    if os_ is None:
        raise ValueError(f"{what}: out must collapse its leading axes and have a contiguous last axis")
    plan = plan_for(x.device, H, W, D)
    with torch.cuda.device(x.device):
        ws = workspace(x.device, int(lib().tb_ampmix_workspace_bytes(plan.handle, B * channels, 0, 0)))
        check(lib().tb_kspace_ampmix_f32(plan.handle, x.data_ptr(), xs, None if y is None else y.data_ptr(), ys,
                                         None if perm is None else perm.data_ptr(), mask.data_ptr(), cm,
                                         lam.data_ptr(), o.data_ptr(), os_, pad, ws.data_ptr(), ws.numel(), B, channels,
                                         _stream(x.device)), "tb_kspace_ampmix_f32")
    return o


def ampmix_workspace_bytes(x: torch.Tensor, n_dims: int, with_g: bool, with_gy: bool) -> int:
    """Workspace bytes of amplitude mixing for the volumes of ``x`` [*lead, *spatial]: the forward
    (``with_g`` False), the gradient with respect to x, and with ``with_gy`` also to y."""
    geo, bc = _spectrum_args("ampmix_workspace_bytes", x, n_dims, torch.float32)
    plan = plan_for(x.device, *geo.hwd)
    return int(lib().tb_ampmix_workspace_bytes(plan.handle, bc, 1 if with_g else 0, 1 if with_gy else 0))


def kspace_ampmix_grad(x: torch.Tensor, y: torch.Tensor, mask: torch.Tensor, lam: torch.Tensor,
                       perm: Optional[torch.Tensor], g: torch.Tensor, n_dims: int, channels: Optional[int] = None,
                       need_gy: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Gradients of ``kspace_ampmix`` with respect to ``x`` and ``y`` for the upstream gradient ``g`` (x's shape,
    any strides with a contiguous last axis): (gx, gy), both of x's shape.  gy[j] is the sum over the samples
    b with ``perm[b]`` = j in the order of b (no atomics: repeated calls agree bit for bit); with ``need_gy``
    False it is None, and neither its buffer nor its passes exist.  When ``y`` is ``x`` the two are still
    returned apart: the gradient of the batch-internal mix is their sum.  Where |X(f)| = 0 the tangential term
    of gx is dropped, where |Y(f)| = 0 the coefficient adds nothing to gy (``tb_kspace_ampmix_bwd_f32``)."""
    what = "kspace_ampmix_grad"
    if not isinstance(x, torch.Tensor) or not isinstance(g, torch.Tensor):
        raise ValueError(f"{what}: image and upstream gradient must be torch tensors")
    if tuple(g.shape) != tuple(x.shape) or g.dtype != torch.float32 or g.device != x.device:
        raise ValueError(f"{what}: the upstream gradient must be a float32 {tuple(x.shape)} tensor on {x.device}")
    x, xs, y, ys, cm, channels, B, geo = _ampmix_args(what, x, y, mask, lam, perm, n_dims, channels)
    H, W, D = geo.hwd
    gs = _image_strides(g, n_dims, geo)
    if gs is None:
        g = g.contiguous()
        gs = _image_strides(g, n_dims, geo)
    gx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    gy = torch.empty(x.shape, dtype=torch.float32, device=x.device) if need_gy else None
    gxs = _image_strides(gx, n_dims, geo)
    plan = plan_for(x.device, H, W, D)
    with torch.cuda.device(x.device):
        ws = workspace(x.device, int(lib().tb_ampmix_workspace_bytes(plan.handle, B * channels, 1, 1 if need_gy else 0)))
        check(lib().tb_kspace_ampmix_bwd_f32(plan.handle, x.data_ptr(), xs, None if y is None else y.data_ptr(), ys,
                                             None if perm is None else perm.data_ptr(), mask.data_ptr(), cm,
                                             lam.data_ptr(), g.data_ptr(), gs, gx.data_ptr(), gxs,
                                             None if gy is None else gy.data_ptr(), gxs, ws.data_ptr(), ws.numel(), B,
                                             channels, _stream(x.device)), "tb_kspace_ampmix_bwd_f32")
    return gx, gy


# ------------------------------------------------------------------ radial profiles (tb_radial_*, csrc/radial.h)
RADIAL_MODES = {"nearest": 0, "linear": 1}
RADIAL_MAX_BINS = 2048


def radial_params(what: str, bins, dr, mode) -> Tuple[int, float, int]:
    """Host-side check of (bins, bin width, mode): ``mode`` is 0 / "nearest" or 1 / "linear"."""
    if isinstance(mode, str):
        if mode not in RADIAL_MODES:
            raise ValueError(f"{what}: mode must be 'nearest' or 'linear', got {mode!r}")
        mode = RADIAL_MODES[mode]
    if isinstance(mode, bool) or mode not in (0, 1):
        raise ValueError(f"{what}: mode must be 0 (nearest) or 1 (linear), got {mode!r}")
    bins, dr = int(bins), float(dr)
    if bins < 1 or bins > RADIAL_MAX_BINS:
        raise ValueError(f"{what}: 1 <= bins <= {RADIAL_MAX_BINS} expected, got {bins}")
    if not np.isfinite(dr) or dr <= 0.0:
        raise ValueError(f"{what}: the bin width dr must be finite and > 0, got {dr}")
    return bins, dr, int(mode)


def _radial_out(what, out, shape, device):
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if (not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(shape) or out.dtype != torch.float32
            or not out.is_contiguous() or out.device != device):
        raise ValueError(f"{what}: out must be a float32 contiguous {tuple(shape)} tensor on {device}")
    return out


def radial_power(x: torch.Tensor, n_dims: int, bins: int, dr: float = 1.0, mode=0,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Radially binned power spectrum of every volume of ``x`` [*lead, *spatial] (float32, any strides with a
    contiguous last axis): P[..., k] = sum_f w_k(f) |FFT(x)(f)|^2 / N over ``bins`` shells of width ``dr`` of the
    integer radius of the centred layout (``include/texbias.h``), so that P.sum(-1) = (x**2).sum(spatial).
    One forward pass and one fused shell reduction in a fixed order (``tb_kspace_radial_power_f32``): no
    spectrum is stored, repeated calls agree bit for bit.  Returns float32 [*lead, bins]."""
    what = "radial_power"
    K, dr, mode = radial_params(what, bins, dr, mode)
    geo, bc = _spectrum_args(what, x, n_dims, torch.float32)
    H, W, D = geo.hwd
    xs = _image_strides(x, n_dims, geo)
    if xs is None:
        x = x.contiguous()
        xs = _image_strides(x, n_dims, geo)
    lead = tuple(x.shape[: x.dim() - n_dims])
    ch = int(lead[-1]) if lead else 1   # launch groups of whole samples, as the other entry points
    P = _radial_out(what, out, lead + (K,), x.device)
    plan = plan_for(x.device, H, W, D)
    with torch.cuda.device(x.device):
        ws = workspace(x.device, int(lib().tb_radial_workspace_bytes(plan.handle, bc, K, 0)))
        check(lib().tb_kspace_radial_power_f32(plan.handle, x.data_ptr(), xs, P.data_ptr(), K, dr, mode, ws.data_ptr(),
                                               ws.numel(), bc // ch, ch, _stream(x.device)),
              "tb_kspace_radial_power_f32")
    return P


def radial_grad(x: torch.Tensor, g: torch.Tensor, n_dims: int, profile_channels: int, bins: int, dr: float = 1.0,
                mode=1, channels: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Gradient of ``kspace_mask(x, radial_mask(p))`` with respect to the radial profile p for an upstream
    gradient ``g``: dp[k] = sum_f w_k(f) Re(FFT(x)(f) conj(FFT(g)(f))) / N, summed over the samples and, with
    ``profile_channels`` = 1, over the channels -- ``radial_bin(kspace_mask_grad(x, g))`` without the dense dM.
    Arguments and strides as ``kspace_mask_grad``.  Returns float32 [bins] or [C, bins]
    (``tb_kspace_radial_grad_f32``)."""
    what = "radial_grad"
    K, dr, mode = radial_params(what, bins, dr, mode)
    x, xs, g, gs, spatial, channels, cp, bc, geo = _grad_pair(what, x, g, n_dims, profile_channels, channels)
    H, W, D = geo.hwd
    dp = _radial_out(what, out, (K,) if cp == 1 else (cp, K), x.device)
    plan = plan_for(x.device, H, W, D)
    with torch.cuda.device(x.device):
        ws = workspace(x.device, int(lib().tb_radial_workspace_bytes(plan.handle, bc, K, 1)))
        check(lib().tb_kspace_radial_grad_f32(plan.handle, x.data_ptr(), xs, g.data_ptr(), gs, dp.data_ptr(), cp, K, dr,
                                              mode, ws.data_ptr(), ws.numel(), bc // channels, channels,
                                              _stream(x.device)), "tb_kspace_radial_grad_f32")
    return dp


def _radial_profile(what, p):
    if not isinstance(p, torch.Tensor):
        raise ValueError(f"{what}: a torch tensor is expected, got {type(p).__name__}")
    if p.dim() not in (1, 2) or p.dtype != torch.float32:
        raise ValueError(f"{what}: a float32 profile [K] or [C, K] is expected, got {p.dtype} {tuple(p.shape)}")
    if p.device.type != "cuda":
        raise TexbiasError(f"{what}: expected a HIP (cuda) tensor, got {p.device}")
    return p.contiguous()


def radial_mask(profile: torch.Tensor, spatial: Sequence[int], dr: float = 1.0, mode=1,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Expand a radial profile [K] or [C, K] (float32, on the device) to the centred mask of ``kspace_mask``:
    M[s] = sum_k w_k(s) p[k], shape ``spatial`` or ``(C,) + spatial`` (``tb_radial_mask_f32``)."""
    what = "radial_mask"
    p = _radial_profile(what, profile)
    K, dr, mode = radial_params(what, p.shape[-1], dr, mode)
    spatial = tuple(int(s) for s in spatial)
    H, W, D = geometry(spatial).hwd
    cp = 1 if p.dim() == 1 else int(p.shape[0])
    M = _radial_out(what, out, spatial if p.dim() == 1 else (cp,) + spatial, p.device)
    plan = plan_for(p.device, H, W, D)
    with torch.cuda.device(p.device):
        check(lib().tb_radial_mask_f32(plan.handle, p.data_ptr(), cp, K, dr, mode, M.data_ptr(), _stream(p.device)),
              "tb_radial_mask_f32")
    return M


def radial_bin(a: torch.Tensor, n_dims: int, bins: int, dr: float = 1.0, mode=1,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The adjoint of ``radial_mask``: q[k] = sum_s w_k(s) a[s] for a real array in the centred layout,
    ``spatial`` (-> [bins]) or ``(C,) + spatial`` (-> [C, bins]), float32; float64 sums in a fixed order
    (``tb_radial_bin_f32``).  ``radial_bin(ones)`` gives the shell counts."""
    what = "radial_bin"
    K, dr, mode = radial_params(what, bins, dr, mode)
    if not isinstance(a, torch.Tensor):
        raise ValueError(f"{what}: a torch tensor is expected, got {type(a).__name__}")
    if a.dim() not in (n_dims, n_dims + 1) or a.dtype != torch.float32:
        raise ValueError(f"{what}: a float32 array spatial or (C,) + spatial with {n_dims} spatial axes is expected, "
                         f"got {a.dtype} {tuple(a.shape)}")
    if a.device.type != "cuda":
        raise TexbiasError(f"{what}: expected a HIP (cuda) tensor, got {a.device}")
    a = a.contiguous()
    H, W, D = geometry(tuple(a.shape[a.dim() - n_dims:])).hwd
    cm = 1 if a.dim() == n_dims else int(a.shape[0])
    q = _radial_out(what, out, (K,) if a.dim() == n_dims else (cm, K), a.device)
    plan = plan_for(a.device, H, W, D)
    with torch.cuda.device(a.device):
        ws = workspace(a.device, int(lib().tb_radial_workspace_bytes(plan.handle, cm, K, 0)))
        check(lib().tb_radial_bin_f32(plan.handle, a.data_ptr(), cm, K, dr, mode, q.data_ptr(), ws.data_ptr(),
                                      ws.numel(), _stream(a.device)), "tb_radial_bin_f32")
    return q


def set_radial_fused(enable: bool) -> None:
    """The fused shell reduction for ``radial_power`` / ``radial_grad`` when True (default), else the composed
    route for every plan: ``kspace_mask_grad`` into the workspace, then the dense bin reduction
    (tb_set_radial_fused; a test switch)."""
    check(lib().tb_set_radial_fused(1 if enable else 0))


# ------------------------------------------------------------------ trainable spikes (tb_kspace_spikes_*, csrc/spike_grad.h)
def spikes_touch(a: Sequence[int], b: Sequence[int], n: Sequence[int]) -> bool:
    """Two unshifted frequencies reach the same stored coefficient: equal, or conjugate (a = -b mod n)."""
    a, b = tuple(int(v) for v in a), tuple(int(v) for v in b)
    return a == b or a == tuple((m - v) % m for v, m in zip(b, n))


def spike_locations(what: str, loc: Sequence[int], spatial: Sequence[int]) -> List[Tuple[int, int, int]]:
    """Host-side check of the spikes of one call: ``loc`` is a flat list of S * n_dims indices into the CENTRED
    layout of ``Fourier.shift_fourier`` (the reference's ``loc``).  Returns the S unshifted (kh, kw, kd) of
    ``TB_OP_SPIKE``.  IndexError for an index out of bounds; ValueError for a count outside 1..TB_MAX_OPS or
    two spikes at equal or conjugate frequencies.  Touches no device."""
    spatial = tuple(int(s) for s in spatial)
    geo = geometry(spatial)
    loc = [int(v) for v in loc]
    nd = len(spatial)
    if nd < 1 or not loc or len(loc) % nd:
        raise ValueError(f"{what}: {len(loc)} location indices for {nd} transformed axes")
    S = len(loc) // nd
    if not 1 <= S <= TB_MAX_OPS:
        raise ValueError(f"{what}: {S} spikes (1 to {TB_MAX_OPS} are supported)")
    out: List[Tuple[int, int, int]] = []
    for j in range(S):
        idx = loc[j * nd:(j + 1) * nd]
        for s, n in zip(idx, spatial):
            if not 0 <= s < n:
                raise IndexError(f"{what}: spike index {tuple(idx)} out of bounds for {spatial}")
        f = geo.to_hwd(unshift(idx, spatial))
        for q, e in enumerate(out):
            if spikes_touch(f, e, geo.hwd):
                raise ValueError(f"{what}: spikes {q} and {j} are at equal or conjugate frequencies")
        out.append(f)
    return out


def spike_intensity(what: str, log_intensity, S: int, device=None) -> None:
    """Host-side check of the layer's log-intensities: a float32 tensor [S] (on ``device`` when given)."""
    if not isinstance(log_intensity, torch.Tensor):
        raise ValueError(f"{what}: log_intensity must be a torch tensor, got {type(log_intensity).__name__}")
    if tuple(log_intensity.shape) != (S,):
        raise ValueError(f"{what}: log_intensity {tuple(log_intensity.shape)} for {S} spikes (expected ({S},))")
    if log_intensity.dtype != torch.float32:
        raise ValueError(f"{what}: log_intensity must be float32, got {log_intensity.dtype}")
    if device is not None and log_intensity.device != device:
        raise ValueError(f"{what}: log_intensity on {log_intensity.device}, image on {device}")


def _spikes_args(what, t, log_intensity, loc, n_dims, channels):
    """Common host-side checks of the two spike launchers: (unshifted locations as int32[S][3], S, geometry,
    volumes, channels)."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: a torch tensor is expected, got {type(t).__name__}")
    n_dims, channels = int(n_dims), int(channels)
    if n_dims < 1 or t.dim() < n_dims:
        raise ValueError(f"{what}: {n_dims} transformed axes on a {t.dim()}-d tensor")
    spatial = tuple(t.shape[t.dim() - n_dims:])
    lead = t.shape[: t.dim() - n_dims]
    bc = int(np.prod(lead)) if len(lead) else 1
    if channels < 1 or bc % channels:
        raise ValueError(f"{what}: {channels} channels do not divide the leading axes {tuple(lead)}")
    f = spike_locations(what, loc, spatial)
    spike_intensity(what, log_intensity, len(f), t.device)
    if t.dtype != torch.float32:
        raise ValueError(f"{what}: float32 expected, got {t.dtype}")
    return f, len(f), geometry(spatial), bc, channels


def _spikes_loc_array(f):
    return (C.c_int32 * (3 * len(f)))(*[v for k in f for v in k])


def kspace_spikes(x: torch.Tensor, log_intensity: torch.Tensor, loc: Sequence[int], n_dims: int, channels: int,
                  pad: int = 0, minmax: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The spike layer on the closed-form route with a device-resident log-intensity: |K(f_j)| := exp(I_j) at the S
    centred locations ``loc`` (flat, S * n_dims indices) on every channel of ``x`` [*lead, *spatial], phase kept.
    ``log_intensity``: float32 [S] on x's device, read when the kernels run (no host sync: a captured graph
    replays with the values then in the tensor).  Returns (y, coef): y as ``kspace_filter`` (``pad`` zero
    columns), coef float64 [*lead, S, 2] = the coefficients K(f_j) of x, which ``kspace_spikes_grad`` needs
    (``tb_kspace_spikes_f32``)."""
    what = "kspace_spikes"
    f, S, geo, bc, channels = _spikes_args(what, x, log_intensity, loc, n_dims, channels)
    pad = int(pad)
    if pad < 0:
        raise ValueError(f"{what}: pad must be >= 0, got {pad}")
    require_hip(x, what)
    H, W, D = geo.hwd
    if pad and len(geo.kept) and geo.kept[-1] != n_dims - 1:
        raise TexbiasError("padding requires a non-singleton last axis")
    xs = _image_strides(x, n_dims, geo)
    if xs is None:
        x = x.contiguous()
        xs = _image_strides(x, n_dims, geo)
    y = torch.empty(tuple(x.shape[:-1]) + (x.shape[-1] + pad,), dtype=torch.float32, device=x.device)
    ys = _image_strides(y, n_dims, geo)
    coef = torch.empty(tuple(x.shape[: x.dim() - n_dims]) + (S, 2), dtype=torch.float64, device=x.device)
    logi = log_intensity.detach().contiguous()
    mm_ptr = None
    if minmax is not None:
        if minmax.dtype != torch.int32 or minmax.numel() < 2 * (bc // channels) or minmax.device != x.device:
            raise TexbiasError("minmax must be an int32 [B,2] tensor on the input's device")
        mm_ptr = minmax.data_ptr()
    plan = plan_for(x.device, H, W, D)
    with torch.cuda.device(x.device):
        ws = workspace(x.device, int(lib().tb_spikes_workspace_bytes(plan.handle, bc)))
        check(lib().tb_kspace_spikes_f32(plan.handle, x.data_ptr(), xs, y.data_ptr(), ys, pad, ws.data_ptr(), ws.numel(),
                                         bc // channels, channels, S, _spikes_loc_array(f), logi.data_ptr(),
                                         coef.data_ptr(), mm_ptr, _stream(x.device)), "tb_kspace_spikes_f32")
    return y, coef


def kspace_spikes_grad(g: torch.Tensor, coef: torch.Tensor, log_intensity: torch.Tensor, loc: Sequence[int],
                       n_dims: int, channels: int, image_grad: bool = True, intensity_grad: bool = True,
                       gx_out: Optional[torch.Tensor] = None,
                       dI_out: Optional[torch.Tensor] = None) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """The gradients of ``kspace_spikes`` for an upstream gradient ``g`` (the image's shape, any strides with a
    contiguous last axis: ``gy[..., :D]`` of a padded output is read in place) and the ``coef`` of its forward:
    (gx, dI) with gx = g + Re(sum_j Gamma_j e^{i theta_j}) / N (``image_grad``, one more read and write of the
    volume; None otherwise and no streaming pass is launched) and dI float32 [S], summed over every
    volume-channel in index order in float64 (``intensity_grad``).  No floating-point atomics: repeated calls
    agree bit for bit (``tb_kspace_spikes_bwd_f32``).  ``gx_out`` / ``dI_out``: float32 contiguous tensors of the
    results' shapes on g's device to overwrite (they need not be zeroed)."""
    what = "kspace_spikes_grad"
    f, S, geo, bc, channels = _spikes_args(what, g, log_intensity, loc, n_dims, channels)
    lead = tuple(g.shape[: g.dim() - n_dims])
    if (not isinstance(coef, torch.Tensor) or tuple(coef.shape) != lead + (S, 2) or coef.dtype != torch.float64
            or coef.device != g.device):
        raise ValueError(f"{what}: coef must be a float64 {lead + (S, 2)} tensor on {g.device}")
    require_hip(g, what)
    H, W, D = geo.hwd
    gs = _image_strides(g, n_dims, geo)
    if gs is None:
        g = g.contiguous()
        gs = _image_strides(g, n_dims, geo)
    coef = coef.contiguous()
    logi = log_intensity.detach().contiguous()
    def result(out, shape, name):
        if out is None:
            return torch.empty(shape, dtype=torch.float32, device=g.device)
        if (not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(shape) or out.dtype != torch.float32
                or not out.is_contiguous() or out.device != g.device):
            raise ValueError(f"{what}: {name} must be a float32 contiguous {tuple(shape)} tensor on {g.device}")
        return out

    gx = result(gx_out, g.shape, "gx_out") if image_grad else None
    dI = result(dI_out, (S,), "dI_out") if intensity_grad else None
    plan = plan_for(g.device, H, W, D)
    with torch.cuda.device(g.device):
        ws = workspace(g.device, int(lib().tb_spikes_workspace_bytes(plan.handle, bc)))
        check(lib().tb_kspace_spikes_bwd_f32(
            plan.handle, g.data_ptr(), gs, bc // channels, channels, S, _spikes_loc_array(f), logi.data_ptr(),
            coef.data_ptr(), gx.data_ptr() if image_grad else None,
            _image_strides(gx, n_dims, geo) if image_grad else None, dI.data_ptr() if intensity_grad else None,
            ws.data_ptr(), ws.numel(), _stream(g.device)), "tb_kspace_spikes_bwd_f32")
    return gx, dI


def minmax_buffer(device: torch.device, B: int) -> torch.Tensor:
    idx = device.index if device.index is not None else torch.cuda.current_device()
    m = _mm.get(idx)
    if m is None or m.shape[0] < B:
        m = torch.empty((max(B, 8), 2), dtype=torch.int32, device=torch.device("cuda", idx))
        _mm[idx] = m
    return m[:B]


def _rows_geometry(x: torch.Tensor, per_sample_dims: int):
    """(B, rows, len, ld, sb) of x viewed as B samples of rows x len (last axis contiguous)."""
    if x.stride(-1) != 1:
        raise TexbiasError("last axis must be contiguous")
    B = int(np.prod(x.shape[: x.dim() - per_sample_dims])) if x.dim() > per_sample_dims else 1
    inner = x.shape[x.dim() - per_sample_dims:]
    ln = int(inner[-1])
    rows = int(np.prod(inner[:-1])) if len(inner) > 1 else 1
    ld = x.stride(-2) if x.dim() >= 2 else ln
    # rows must be uniformly strided by ld within a sample
    exp = ld
    for size, s in zip(reversed(inner[:-1]), reversed(x.stride()[x.dim() - per_sample_dims:-1])):
        if size != 1 and s != exp:
            return None
        exp = s * size if size != 1 else exp
    sb = x.stride(x.dim() - per_sample_dims - 1) if x.dim() > per_sample_dims else rows * ld
    if B > 1:
        lead = x.shape[: x.dim() - per_sample_dims]
        lst = x.stride()[: x.dim() - per_sample_dims]
        e = None
        for size, s in zip(reversed(lead), reversed(lst)):
            if size == 1:
                continue
            if e is None:
                e, sb = s * size, s
            elif s != e:
                return None
            else:
                e = s * size
    return B, rows, ln, ld, sb


def minmax_keys(x: torch.Tensor, per_sample_dims: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    require_hip(x, "minmax")
    g = _rows_geometry(x, per_sample_dims)
    if g is None:
        x = x.contiguous()
        g = _rows_geometry(x, per_sample_dims)
    B, rows, ln, ld, sb = g
    mm = out if out is not None else torch.empty((B, 2), dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        check(lib().tb_minmax_f32(x.data_ptr(), mm.data_ptr(), B, rows, ln, ld, sb, _stream(x.device)), "tb_minmax_f32")
    return mm


def keys_to_float(mm: torch.Tensor) -> np.ndarray:
    L = lib()
    return np.array([[L.tb_key_to_float(int(v) & 0xFFFFFFFF) for v in row] for row in mm.cpu().tolist()],
                    np.float32)


def salt_and_pepper(x: torch.Tensor, per_sample_dims: int, thresholds: Sequence[Tuple[float, float]],
                    minmax: torch.Tensor, out: Optional[torch.Tensor] = None, u: Optional[torch.Tensor] = None,
                    cls: Optional[torch.Tensor] = None, seed: int = 0, offset: int = 0) -> torch.Tensor:
    """SaltAndPepper.salt_and_pepper over B samples.  out may be x (sparse in-place scatter)."""
    require_hip(x, "salt_and_pepper")
    if out is None:
        out = torch.empty_like(x)
    require_hip(out, "salt_and_pepper(out)")
    g = _rows_geometry(x, per_sample_dims)
    go = _rows_geometry(out, per_sample_dims)
    if g is None or go is None or g != go:
        raise TexbiasError("salt_and_pepper: input/output must share a row geometry")
    B, rows, ln, ld, sb = g
    if len(thresholds) != B:
        raise ValueError("one (lo, hi) threshold pair per sample")
    thr = np.asarray(thresholds, np.float32).reshape(B, 2)
    thr_c = (C.c_float * (2 * B))(*thr.ravel().tolist())
    for t, name in ((u, "u"),):
        if t is not None:
            require_hip(t, name)
            if _rows_geometry(t, per_sample_dims) != g:
                raise TexbiasError("u must share the input's geometry")
    if cls is not None and (cls.dtype != torch.int8 or cls.shape != x.shape or cls.stride() != x.stride()):
        raise TexbiasError("cls must be int8 with the input's shape and strides")
    with torch.cuda.device(x.device):
        check(lib().tb_salt_pepper_f32(x.data_ptr(), out.data_ptr(), cls.data_ptr() if cls is not None else None,
                                       u.data_ptr() if u is not None else None, seed & (2 ** 64 - 1),
                                       offset & (2 ** 64 - 1), thr_c, minmax.data_ptr(), B, rows, ln, ld, sb,
                                       _stream(x.device)), "tb_salt_pepper_f32")
    return out


def disk_mask_tensor(shape: Sequence[int], r, dim: int, inside_off: bool, device: torch.device) -> torch.Tensor:
    """disk_mask.binary_mask_{2d,3d} (filters_and_operators.py:136-197) built on the device."""
    shape = tuple(int(s) for s in shape)
    grid = shape[-dim:]
    outer = int(np.prod(shape[:-dim])) if len(shape) > dim else 1
    n0, n1, n2 = (1,) + grid if dim == 2 else grid
    m = torch.empty(shape, dtype=torch.float32, device=device)
    if isinstance(r, (int, np.integer)) and not isinstance(r, bool):
        int_r, r2i, r2f = 1, int(r) * int(r), 0.0
    else:
        int_r, r2i = 0, 0
        r2 = float(r) ** 2
        r2f = float(np.float32(r2)) if np.isfinite(r2) else float("inf")
    with torch.cuda.device(device):
        check(lib().tb_disk_mask_f32(m.data_ptr(), outer, n0, n1, n2, int_r, r2i, r2f, 1 if inside_off else 0,
                                     _stream(device)), "tb_disk_mask_f32")
    return m


def logabs_sums(x: torch.Tensor, n_dims: int, programs: Sequence[Sequence], channels: int) -> torch.Tensor:
    """Sum over the full spectrum of log(|k|+1e-10) per volume-channel (float64 [B*C])."""
    require_hip(x, "logabs_sums")
    geo = geometry(x.shape[x.dim() - n_dims:])
    H, W, D = geo.hwd
    x = x.contiguous()
    bc, bstride, sp, sp_st = _bc_view(x, n_dims)
    sh, sw, sd = _hwd_strides(geo, sp_st)
    plan = plan_for(x.device, H, W, D)
    out = torch.empty(bc, dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        ws = workspace(x.device, plan.workspace_bytes(bc))
        xs = (C.c_int64 * 3)(bstride, sh, sw)
        progs = programs_array(programs)
        check(lib().tb_kspace_logabs_sum_f32(plan.handle, x.data_ptr(), xs, ws.data_ptr(), ws.numel(), len(programs),
                                             channels, C.addressof(progs), out.data_ptr(), _stream(x.device)),
              "tb_kspace_logabs_sum_f32")
    return out


def set_compiled_plans(enable: bool) -> None:
    """Passes A/C on the compile-time slab plans (240x155, 128x128) when True (default), else the
    generic run-time-planned kernels (tb_set_compiled_plans)."""
    check(lib().tb_set_compiled_plans(1 if enable else 0))


def set_band_plans(enable: bool) -> None:
    """Band-limited passes A'/B'/C' for low-pass programs when True (default), else the full
    spectrum passes for every program (tb_set_band_plans)."""
    check(lib().tb_set_band_plans(1 if enable else 0))


def set_point_plans(enable: bool) -> None:
    """Spike-only programs (plane waves, k-space spikes) in closed form when True (default), else
    on the full-spectrum passes (tb_set_point_plans)."""
    check(lib().tb_set_point_plans(1 if enable else 0))


def set_wrap_plans(enable: bool) -> None:
    """Wrap-only programs on the separable route (2-tap H/W combine + D circulant, one image read
    and write) when True (default), else on the full-spectrum passes (tb_set_wrap_plans)."""
    check(lib().tb_set_wrap_plans(1 if enable else 0))


def set_half_units(enable: bool) -> None:
    """Full-spectrum passes A / C as half units (row parity) over a split spectrum where the plan
    has them (240 x 240 x 155) when True (default), else whole slabs (tb_set_half_units)."""
    check(lib().tb_set_half_units(1 if enable else 0))


def set_band_inv16(enable: bool) -> None:
    """Pass C' synthesis in split f16 on the matrix cores when True (default, where the launch's
    V rows fit), else the f32 MFMA synthesis (tb_set_band_inv16)."""
    check(lib().tb_set_band_inv16(1 if enable else 0))


def set_chain_chunk(n: int) -> None:
    """Channel-volumes per pass A -> B -> C chain (tb_set_chain_chunk): n > 0 chunks, 0 = whole
    batch group per pass, n < 0 = default (Infinity-Cache-sized chunks)."""
    check(lib().tb_set_chain_chunk(int(n)))


def set_pass_timing(enable: bool) -> None:
    check(lib().tb_set_pass_timing(1 if enable else 0))


def pass_times_ms() -> Tuple[List[float], List[int]]:
    ms = (C.c_float * 4)()
    cnt = (C.c_int * 4)()
    check(lib().tb_get_pass_times_ms(ms, cnt))
    return list(ms), list(cnt)


def pass_stats() -> Tuple[List[float], List[int], List[float], List[str]]:
    """Per pass slot (0 forward, 1 k-space, 2 inverse, 3 salt-and-pepper / min-max) since timing
    was enabled: summed ms, launch count, summed algorithmic bytes, last kernel name; clears."""
    ms = (C.c_float * 4)()
    cnt = (C.c_int * 4)()
    nb = (C.c_double * 4)()
    names = [lib().tb_pass_kernel(i).decode() for i in range(4)]
    check(lib().tb_get_pass_stats(ms, cnt, nb))
    return list(ms), list(cnt), list(nb), names
