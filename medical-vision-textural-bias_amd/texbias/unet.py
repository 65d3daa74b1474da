"""3-D residual U-Net equivalent to the MONAI 0.5 ``UNet`` the reference trains.

The reference builds ``monai.networks.nets.UNet(dimensions=3, in_channels, out_channels,
channels=(16, 32, 64, 128, 256), strides=(2, 2, 2, 2), num_res_units=2)``
(e.g. 10_scripts/20_Gibbs_filters/stylized_gibbs12p5.py:192-199).  MONAI is not a
dependency here; the module tree below reproduces the architecture printed in
source_code/test.ipynb:754-1010 (cell 21) module for module, so parameter shapes,
counts and default initialisation match (parity with MONAI's numerics is unpinned:
MONAI is not installed in this image).

Blocks (MONAI 0.5 semantics):
* ``Convolution`` = Conv3d / ConvTranspose3d -> InstanceNorm3d(affine=False) -> Dropout(0) -> PReLU
  ("NDA" order; on HIP tensors one fused texbias kernel pair, ``texbias.norm``), or the bare conv
  when ``conv_only``;
* ``ResidualUnit`` = ``subunits`` Convolutions (first one strided) + residual path (strided 3^3
  conv, 1^3 conv when only the channel count changes, else identity), summed;
* ``SkipConnection`` = cat([x, sub(x)], dim=1).

On HIP float32 tensors the blocks run as fused autograd functions over the texbias kernels
(``texbias.conv`` routes each convolution, ``texbias.norm`` the ADN):
* ``Convolution`` with an ADN: conv -> ADN in one function whose backward gets the conv's bias gradient
  out of the ADN backward's store pass (no channel-sum sweep);
* a strided ``ResidualUnit`` (unit0 and the residual are both Conv3d(cin -> c, 3, stride 2)): ONE stacked
  convolution with 2c outputs, the residual half summed into the last ADN's store, one stacked input and
  weight gradient in the backward (no gradient-accumulation add);
* an identity-residual ``ResidualUnit``: the residual summed into the ADN store (or after the bare conv).
Parameters and state dicts are those of the plain modules.
"""
from __future__ import annotations

import os
from typing import Sequence

import torch
import torch.nn as nn

from . import conv as _conv
from .conv import Conv3d, ConvTranspose3d
from . import norm as _norm
from .norm import adn_backward, adn_forward, instnorm_prelu

FUSED = os.environ.get("TEXBIAS_FUSED_UNITS", "1") != "0"


def _fusable(x: torch.Tensor, conv: nn.Module, adn) -> bool:
    if not (FUSED and _norm.ENABLED and x.is_cuda and x.dtype == torch.float32 and
            isinstance(conv, (Conv3d, ConvTranspose3d)) and conv.groups == 1 and conv.dilation == (1, 1, 1) and
            _conv.custom_backward_applies(x, conv.weight)):
        return False
    if isinstance(conv, Conv3d) and conv.padding_mode != "zeros":
        return False
    return adn is None or adn.D.p == 0.0 or not adn.training


class _ConvADNFn(torch.autograd.Function):
    """y = prelu(instance_norm(conv(x))) (+ res): MONAI Convolution "NDA" (+ the ResidualUnit's sum)."""

    @staticmethod
    def forward(ctx, x, w, b, a, route, eps, res, res_is_x, out=None):
        z = route.forward(x.contiguous(), w, b)
        y, mean, rstd = adn_forward(z, a, eps, res=res, out=out)
        ctx.save_for_backward(x, w, a, z, mean, rstd)
        ctx.route, ctx.has_b, ctx.has_res, ctx.res_is_x = route, b is not None, res is not None, res_is_x
        return y

    @staticmethod
    def backward(ctx, g):
        x, w, a, z, mean, rstd = ctx.saved_tensors
        n = ctx.needs_input_grad
        g = _norm._plain(g)  # a channel slice of the skip concatenation's gradient is read in place
        dz, da, db = adn_backward(z, g, mean, rstd, a, need_w=n[3], need_bias=ctx.has_b and n[2])
        gw = ctx.route.weight_grad(dz, x, w) if n[1] else None
        if ctx.res_is_x:  # identity residual: dX = dconv(dZ) + dY in the input-gradient kernel's store
            gx = ctx.route.input_grad(dz, x, w, add=g) if n[0] else None
            return gx, gw, db, da, None, None, None, None, None
        gx = ctx.route.input_grad(dz, x, w) if n[0] else None
        return gx, gw, db, da, None, None, (g if ctx.has_res and n[6] else None), None, None


class _ConvResFn(torch.autograd.Function):
    """y = conv(x) + x: the identity-residual unit with a bare conv (the top ResidualUnit(3, 3, conv_only))."""

    @staticmethod
    def forward(ctx, x, w, b, route):
        x = x.contiguous()
        y = route.forward(x, w, b, add=x)
        ctx.save_for_backward(x, w)
        ctx.route, ctx.has_b = route, b is not None
        return y

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        n = ctx.needs_input_grad
        g = g.contiguous()
        gx = ctx.route.input_grad(g, x, w, add=g) if n[0] else None
        need_b = ctx.has_b and n[2]
        gb = None
        if n[1] and need_b:  # the weight-gradient sweep sums g on the way where its route can
            gw, gb = ctx.route.weight_bias_grad(g, x, w)
        else:
            gw = ctx.route.weight_grad(g, x, w) if n[1] else None
        if need_b and gb is None:
            gb = _conv.channel_sum(g)
        return gx, gw, gb, None


def _adjacent(a: torch.Tensor, b: torch.Tensor):
    """[a; b] along dim 0 without a copy when b's storage directly follows a's (``ResidualUnit`` keeps the
    unit-0 and residual parameters of a strided unit that way), else None."""
    if not (a.is_contiguous() and b.is_contiguous() and a.shape[1:] == b.shape[1:] and a.dtype == b.dtype and
            a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr() and
            b.storage_offset() == a.storage_offset() + a.numel()):
        return None
    return torch.empty(0, dtype=a.dtype, device=a.device).set_(
        a.untyped_storage(), a.storage_offset(), (a.shape[0] + b.shape[0],) + tuple(a.shape[1:]))


class _StackedUnitFn(torch.autograd.Function):
    """A strided ResidualUnit: [unit0 | residual] = conv(x, [W0; Wr], stride 2) as one convolution,
    a0 = ADN0(unit0), out = ADN1(conv1(a0)) + residual."""

    @staticmethod
    def forward(ctx, x, w0, b0, wr, br, a0w, w1, b1, a1w, unit, eps, skip, skip_in=None):
        c = w0.shape[0]
        w_st = _adjacent(w0, wr)
        if w_st is None:
            w_st = torch.cat([w0, wr], 0)
        b_st = None
        if b0 is not None and br is not None:
            b_st = _adjacent(b0, br)
            if b_st is None:
                b_st = torch.cat([b0, br], 0)
        x = x.contiguous()
        r_st = unit.stacked_route(x, w_st)
        y2 = r_st.forward(x, w_st, b_st)                      # [N, 2c, ...]
        z0, res = y2[:, :c], y2[:, c:]
        a0, m0, s0 = adn_forward(z0, a0w, eps)
        conv1 = list(unit.conv.children())[1].conv
        r1 = _conv.route_of(conv1, a0)
        z1 = r1.forward(a0, w1, b1)
        out, m1, s1 = adn_forward(z1, a1w, eps, res=res)
        ctx.save_for_backward(x, w_st, a0w, w1, a1w, y2, a0, z1, m0, s0, m1, s1)
        ctx.cfg = (c, r_st, r1, b0 is not None, b1 is not None)
        ctx.skip = skip
        ctx.skip_in = skip_in  # the hand-over dict of the stacked unit that made x, if one did
        return out

    @staticmethod
    def backward(ctx, g):
        x, w_st, a0w, w1, a1w, y2, a0, z1, m0, s0, m1, s1 = ctx.saved_tensors
        c, r_st, r1, has_b0, has_b1 = ctx.cfg
        n = ctx.needs_input_grad
        dy2, gd = ctx.skip.pop("dy2", None), ctx.skip.pop("gx", None)
        gs = ctx.skip.pop("g", None)
        if dy2 is not None and gd is not None and gs is None and dy2.shape == y2.shape and \
                g.data_ptr() == gd.data_ptr() and \
                g.shape == gd.shape and g.stride() == gd.stride():
            pass  # g is the downstream unit's input gradient + the skip share, already in dy2[:, c:]
        elif gs is not None:  # the skip concatenation's share of this output's gradient, summed straight into
            dy2 = torch.empty_like(y2)
            g = torch.add(g, gs, out=dy2[:, c:])  # the residual conv's half of the stacked output gradient
        else:
            dy2 = torch.empty_like(y2)
            g = g.contiguous()
            dy2[:, c:].copy_(g)                               # the residual conv's output gradient
        # the residual conv's bias gradient (g summed over n and the voxels) out of the ADN's statistics sweep
        dbr = torch.empty(c, dtype=g.dtype, device=g.device) if has_b0 and n[4] else None
        dz1, da1, db1 = adn_backward(z1, g, m1, s1, a1w, need_w=n[8], need_bias=has_b1, dysum_out=dbr)
        da0 = r1.input_grad(dz1, a0, w1)
        gw1 = r1.weight_grad(dz1, a0, w1) if n[6] else None
        _, dw0a, db0 = adn_backward(y2[:, :c], da0, m0, s0, a0w, need_w=n[5], need_bias=has_b0,
                                    dx_out=dy2[:, :c])
        up = ctx.skip_in
        gu = up.get("g") if up is not None else None
        if n[0] and gu is not None and gu.shape == x.shape and \
                ((_conv.CONVT_DX_ADD and r_st.dx == "convT64") or (_conv.CONVT_STACK_DX_ADD and r_st.dx == "convTs")):
            # x is a stacked unit's output and its skip share gu is waiting: the kernel writes dX + gu into
            # channels [cu, 2 cu) of that unit's stacked output-gradient buffer, which that unit's backward
            # takes over when this very slice comes back to it as its output gradient (no add pass, no copy)
            cu = x.shape[1]
            buf = torch.empty((x.shape[0], 2 * cu) + tuple(x.shape[2:]), dtype=x.dtype, device=x.device)
            gx = _alias(buf, cu, 2 * cu)
            r_st.input_grad(dy2, x, w_st, add=gu, out=gx)
            del up["g"]
            up["dy2"], up["gx"] = buf, gx
        else:
            gx = r_st.input_grad(dy2, x, w_st) if n[0] else None
        gw_st = r_st.weight_grad(dy2, x, w_st) if (n[1] or n[3]) else None
        return (gx, gw_st[:c] if gw_st is not None else None, db0, gw_st[c:] if gw_st is not None else None, dbr,
                dw0a, gw1, db1 if n[7] else None, da1, None, None, None, None)


class ADN(nn.Sequential):
    def __init__(self, channels: int, dropout: float = 0.0):
        super().__init__()
        self.add_module("N", nn.InstanceNorm3d(channels, eps=1e-5, affine=False, track_running_stats=False))
        self.add_module("D", nn.Dropout(p=dropout))
        self.add_module("A", nn.PReLU(num_parameters=1))

    def forward(self, x):
        # On the GPU the N -> D(0) -> A chain is one fused texbias op (two HBM sweeps per direction).
        if _norm.ENABLED and x.is_cuda and x.dtype == torch.float32 and (self.D.p == 0.0 or not self.training):
            return instnorm_prelu(x, self.A.weight, self.N.eps)
        return super().forward(x)


class Convolution(nn.Sequential):
    def __init__(self, cin: int, cout: int, strides: int = 1, kernel_size: int = 3, conv_only: bool = False,
                 is_transposed: bool = False, dropout: float = 0.0):
        super().__init__()
        pad = (kernel_size - 1) // 2
        if is_transposed:
            conv = ConvTranspose3d(cin, cout, kernel_size, stride=strides, padding=pad, output_padding=strides - 1)
        else:
            conv = Conv3d(cin, cout, kernel_size, stride=strides, padding=pad)
        self.add_module("conv", conv)
        if not conv_only:
            self.add_module("adn", ADN(cout, dropout))

    def fused(self, x, res=None, out=None):
        """conv -> ADN (+ res) as one autograd function, or None when the fused path does not apply.
        ``out``: storage to write the result into (an alias, see ``_alias``)."""
        adn = getattr(self, "adn", None)
        if adn is None or not _fusable(x, self.conv, adn):
            return None
        return _ConvADNFn.apply(x, self.conv.weight, self.conv.bias, adn.A.weight, _conv.route_of(self.conv, x),
                                adn.N.eps, res, res is x, out)

    def forward(self, x):
        y = self.fused(x)
        return y if y is not None else super().forward(x)


class ResidualUnit(nn.Module):
    def __init__(self, cin: int, cout: int, strides: int = 1, kernel_size: int = 3, subunits: int = 2,
                 last_conv_only: bool = False, dropout: float = 0.0):
        super().__init__()
        self.conv = nn.Sequential()
        sch, sst = cin, strides
        subunits = max(1, subunits)
        for su in range(subunits):
            conv_only = last_conv_only and su == subunits - 1
            self.conv.add_module(f"unit{su}", Convolution(sch, cout, sst, kernel_size, conv_only=conv_only,
                                                          dropout=dropout))
            sch, sst = cout, 1
        if strides != 1 or cin != cout:
            k, p = (kernel_size, (kernel_size - 1) // 2) if strides != 1 else (1, 0)
            self.residual = Conv3d(cin, cout, k, stride=strides, padding=p)
        else:
            self.residual = nn.Identity()
        self._register_state_dict_hook(ResidualUnit._unshare_packed)

    @staticmethod
    def _unshare_packed(module, state_dict, prefix, local_metadata):
        """state_dict of a packed unit: its unit-0 / residual tensors as copies of their own, so a checkpoint
        holds no shared storages (safetensors refuses them); ``keep_vars=True`` callers get the Parameters."""
        for k in ("conv.unit0.conv.weight", "conv.unit0.conv.bias", "residual.weight", "residual.bias"):
            v = state_dict.get(prefix + k)
            if v is not None and not isinstance(v, nn.Parameter) and v.untyped_storage().nbytes() != \
                    v.numel() * v.element_size():
                state_dict[prefix + k] = v.clone()
        return state_dict

    def forward(self, x):
        units = list(self.conv.children())
        if isinstance(self.residual, Conv3d) and len(units) == 2 and all(hasattr(u, "adn") for u in units):
            u0, u1 = units
            r = self.residual
            if r.stride == u0.conv.stride and r.kernel_size == u0.conv.kernel_size and r.padding == u0.conv.padding \
                    and isinstance(u0.conv, Conv3d) and _fusable(x, u0.conv, u0.adn) and _fusable(x, r, None) and \
                    _fusable(x, u1.conv, u1.adn) and (r.bias is None) == (u0.conv.bias is None) and \
                    u0.adn.N.eps == u1.adn.N.eps and r.padding_mode == "zeros":
                skip = {}
                y = _StackedUnitFn.apply(x, u0.conv.weight, u0.conv.bias, r.weight, r.bias, u0.adn.A.weight,
                                         u1.conv.weight, u1.conv.bias, u1.adn.A.weight, self, u0.adn.N.eps, skip,
                                         getattr(x, "_tb_skip", None))
                y._tb_skip = skip  # a skip concatenation of y hands its gradient share over (_SkipCatFn)
                return y
        if isinstance(self.residual, nn.Identity) and len(units) == 1 and hasattr(units[0], "adn"):
            out = self.__dict__.pop("_tb_out", None)
            if out is not None and tuple(out.shape) != tuple(x.shape[:1]) + (units[0].conv.out_channels,) + \
                    tuple(x.shape[2:]):
                out = None
            y = units[0].fused(x, res=x, out=out)
            if y is not None:
                return y
        if isinstance(self.residual, nn.Identity) and len(units) == 1 and not hasattr(units[0], "adn") and \
                _fusable(x, units[0].conv, None):
            c = units[0].conv
            return _ConvResFn.apply(x, c.weight, c.bias, _conv.route_of(c, x))
        res = self.residual(x)
        return self.conv(x) + res

    def pack_parameters(self) -> bool:
        """Explicit setup, never called by ``forward``: move a strided unit's unit-0 and residual conv
        weights (and biases) into one storage each, unit 0's first, so the stacked convolution reads them as
        one tensor with no per-step concatenation (``_adjacent``; without packing ``forward`` concatenates).
        The Parameter objects stay the same (optimizer state is unaffected), but afterwards the two pairs
        share a storage (``state_dict`` returns copies of those four tensors, so checkpoints -- torch.save or
        safetensors -- hold no shared storage).  Skipped (returns False) under inference mode or when
        a tensor is not a plain leaf Parameter.  ``TrainStep`` calls it once, before DDP and the optimizer."""
        units = list(self.conv.children())
        if not (isinstance(self.residual, Conv3d) and len(units) == 2 and hasattr(units[0], "conv")):
            return False
        c0, r = units[0].conv, self.residual
        if torch.is_inference_mode_enabled() or not isinstance(c0, Conv3d) or r.stride != c0.stride or \
                r.kernel_size != c0.kernel_size or r.padding != c0.padding:
            return False  # only the units forward runs as one stacked convolution
        packed = False
        with torch.no_grad():
            for n in ("weight", "bias"):
                a, b = getattr(c0, n), getattr(r, n)
                if a is None or b is None or a.shape[1:] != b.shape[1:] or a.dtype != b.dtype or a.device != b.device:
                    continue
                if not (isinstance(a, nn.Parameter) and isinstance(b, nn.Parameter) and a.is_leaf and b.is_leaf) \
                        or a.is_inference() or b.is_inference():
                    continue
                if _adjacent(a, b) is None:
                    st = torch.cat([a.detach(), b.detach()], 0)
                    a.data, b.data = st[:a.shape[0]], st[a.shape[0]:]
                packed = True
        return packed

    def stacked_route(self, x: torch.Tensor, w_st: torch.Tensor) -> "_conv.Route":
        """The route of the stacked [unit0; residual] convolution for this input (cached per shape)."""
        r = self.residual
        key = ("stacked", tuple(x.shape), x.dtype, x.device, x.data_ptr() % 16 == 0)
        cache = self.__dict__.setdefault("_tb_routes", {})
        rt = cache.get(key)
        if rt is None:
            rt = _conv.Route(x, w_st, r.stride, r.padding, (0, 0, 0), False)
            cache[key] = rt
        return rt


def pack_parameters(model: nn.Module) -> int:
    """``ResidualUnit.pack_parameters`` on every strided unit of ``model``; returns how many were packed."""
    return sum(1 for m in model.modules() if isinstance(m, ResidualUnit) and m.pack_parameters())


def _alias(buf: torch.Tensor, c0: int, c1: int) -> torch.Tensor:
    """Channels [c0, c1) of ``buf`` as a tensor of its own that shares the storage but is not an autograd
    view (its own version counter): a kernel writes into it through the raw pointer."""
    sh = (buf.shape[0], c1 - c0) + tuple(buf.shape[2:])
    return torch.empty(0, dtype=buf.dtype, device=buf.device).set_(
        buf.untyped_storage(), buf.storage_offset() + c0 * buf.stride(1), sh, buf.stride())


class _SkipCatFn(torch.autograd.Function):
    """cat([x, s], 1) where s already sits in channels [c, c + cs) of ``buf``: only x is copied.  When x
    comes from a stacked ResidualUnit (``skip``: its hand-over dict), x's gradient share g[:, :c] is handed
    to that unit's backward, which sums it with the submodule's share straight into its stacked output
    gradient (no autograd accumulation pass, no copy); autograd runs this backward before the submodule's
    and the unit's, since both need the gradient of s first."""

    @staticmethod
    def forward(ctx, x, s, buf, skip=None):
        c = x.shape[1]
        _alias(buf, 0, c).copy_(x)
        ctx.c, ctx.skip = c, skip
        return _alias(buf, 0, buf.shape[1])

    @staticmethod
    def backward(ctx, g):
        if ctx.skip is not None and ctx.needs_input_grad[0]:
            ctx.skip["g"] = g[:, :ctx.c]
            return None, g[:, ctx.c:], None, None
        return g[:, :ctx.c], g[:, ctx.c:], None, None


class SkipConnection(nn.Module):
    def __init__(self, submodule: nn.Module):
        super().__init__()
        self.submodule = submodule

    def _tail_unit(self):
        """The identity-residual unit whose output ends the submodule (``_up``'s ResidualUnit), if any."""
        m = self.submodule
        if isinstance(m, nn.Sequential) and len(m) > 0 and isinstance(m[-1], nn.Sequential) and len(m[-1]) == 2:
            ru = m[-1][1]
            if isinstance(ru, ResidualUnit) and isinstance(ru.residual, nn.Identity):
                return ru
        return None

    def forward(self, x):
        # On the fused HIP path the submodule's last unit writes its output straight into the concatenation's
        # upper channels (one copy instead of two)
        ru = self._tail_unit() if (FUSED and x.is_cuda and x.dtype == torch.float32) else None
        if ru is not None:
            cs = list(ru.conv.children())[0].conv.out_channels
            buf = torch.empty((x.shape[0], x.shape[1] + cs) + tuple(x.shape[2:]), dtype=x.dtype, device=x.device)
            tail = _alias(buf, x.shape[1], x.shape[1] + cs)
            ru._tb_out = tail
            try:
                s = self.submodule(x)
            finally:
                ru.__dict__.pop("_tb_out", None)
            if s.data_ptr() == tail.data_ptr() and s.shape == tail.shape:
                return _SkipCatFn.apply(x, s, buf, getattr(x, "_tb_skip", None))
            return torch.cat([x, s], dim=1)
        return torch.cat([x, self.submodule(x)], dim=1)


class UNet(nn.Module):
    """``UNet(dimensions=3, in_channels, out_channels, channels, strides, num_res_units=2)``."""

    def __init__(self, dimensions: int = 3, in_channels: int = 1, out_channels: int = 1,
                 channels: Sequence[int] = (16, 32, 64, 128, 256), strides: Sequence[int] = (2, 2, 2, 2),
                 kernel_size: int = 3, up_kernel_size: int = 3, num_res_units: int = 2, dropout: float = 0.0):
        super().__init__()
        if dimensions != 3:
            raise ValueError("only the 3-D U-Net of the reference is provided")
        if len(channels) < 2 or len(strides) != len(channels) - 1:
            raise ValueError("len(strides) must be len(channels) - 1 >= 1")
        if num_res_units < 1:
            raise ValueError("the reference configuration uses residual units (num_res_units >= 1)")
        self.nru, self.k, self.uk, self.dropout = num_res_units, kernel_size, up_kernel_size, dropout

        def block(cin, cout, chs, sts, is_top):
            c, s = chs[0], sts[0]
            if len(chs) > 2:
                sub = block(c, c, chs[1:], sts[1:], False)
                upc = c * 2
            else:
                sub = self._down(c, chs[1], 1)
                upc = c + chs[1]
            return nn.Sequential(self._down(cin, c, s), SkipConnection(sub), self._up(upc, cout, s, is_top))

        self.model = block(in_channels, out_channels, tuple(channels), tuple(strides), True)

    def _down(self, cin, cout, s):
        return ResidualUnit(cin, cout, s, self.k, self.nru, dropout=self.dropout)

    def _up(self, cin, cout, s, is_top):
        conv = Convolution(cin, cout, s, self.uk, conv_only=False, is_transposed=True, dropout=self.dropout)
        ru = ResidualUnit(cout, cout, 1, self.k, subunits=1, last_conv_only=is_top, dropout=self.dropout)
        return nn.Sequential(conv, ru)

    def forward(self, x):
        return self.model(x)
