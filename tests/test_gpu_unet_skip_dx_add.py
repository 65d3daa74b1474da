"""The level-1 / level-2 pair of the U-Net with the skip share summed in the transposed-conv kernel's store
(``conv.CONVT_DX_ADD``, ``texbias.unet._StackedUnitFn``): ResidualUnit(4 -> 16, stride 2), then a SkipConnection
around ResidualUnit(16 -> 32, stride 2) and its up path (ConvTranspose3d(32 -> 16) -> ADN -> identity-residual
unit), input 1 x 4 x 8 x 8 x 16.

The level-2 unit's stacked input gradient (Conv3d(16 -> 64, stride 2), on the ``convT64`` route) is written, with
the skip concatenation's share of the level-1 output's gradient added in the kernel's store, straight into
channels [16, 32) of the level-1 unit's stacked output-gradient buffer; the level-1 backward takes that buffer
over instead of running its add pass.

* On against off: off rounds dX to float32, then adds the share (one rounding); on adds the share to the same
  float32 dX in the kernel's registers (one rounding): the sums are the same, so every gradient is expected bit
  for bit equal where the kernels downstream are deterministic.  The bar allows what two runs of the off path
  differ by (kernels that sum with atomics), and never less than 8 x 2^-24 of the largest value.
* On against the float64 restatement of tests/_unet_ref.py: the bars of tests/test_gpu_unet_blocks.py."""
import copy

import pytest
import torch
import torch.nn as nn

import _unet_ref as R
from test_gpu_unet_blocks import _init, _judge, _three_runs

pytestmark = pytest.mark.gpu

SHAPE = (1, 4, 8, 8, 16)


def _pair(seed):
    from texbias import unet
    up = nn.Sequential(unet.Convolution(32, 16, 2, is_transposed=True), unet.ResidualUnit(16, 16, 1, subunits=1))
    return _init(nn.Sequential(unet.ResidualUnit(4, 16, 2),
                               unet.SkipConnection(nn.Sequential(unet.ResidualUnit(16, 32, 2), up))), seed)


def _ref(sd, x):
    d, inter = R.residual_unit(sd, "0", x, 2)
    u, sub = R.residual_unit(sd, "1.submodule.0", d, 2)
    inter.update(sub)
    s, sub = R.up_block(sd, "1.submodule.1", u, False)
    inter.update(sub)
    return torch.cat([d, s], dim=1), inter


def _spy(conv, monkeypatch):
    """Count the transposed-conv calls that write into a handed-over buffer."""
    calls = []
    real = conv.convT_mfma

    def spy(x, w, b, add=None, out=None):
        calls.append((add is not None, out is not None))
        return real(x, w, b, add=add, out=out)

    monkeypatch.setattr(conv, "convT_mfma", spy)
    return calls


def _grads(m, x0, g):
    m = copy.deepcopy(m)
    x = x0.clone().requires_grad_(True)
    y = m(x)
    y.backward(g)
    out = {"output": y.detach(), "input": x.grad}
    out.update({n: p.grad for n, p in m.named_parameters()})
    return out


def test_on_equals_off(gpu, monkeypatch):
    from texbias import conv
    m = _pair(seed=40)
    x0 = torch.randn(SHAPE, device="cuda") * 1.5 + 0.3
    with torch.no_grad():
        g = torch.randn_like(copy.deepcopy(m)(x0))
    calls = _spy(conv, monkeypatch)
    assert conv.CONVT_DX_ADD
    on = _grads(m, x0, g)
    assert calls.count((True, True)) == 1, calls   # the level-2 unit's input gradient took the skip share
    del calls[:]
    monkeypatch.setattr(conv, "CONVT_DX_ADD", False)
    off, off2 = _grads(m, x0, g), _grads(m, x0, g)
    assert (True, True) not in calls and (False, True) not in calls, calls
    for n in on:
        scale = off[n].abs().max().item()
        e_on = (on[n] - off[n]).abs().max().item()
        e_off = (off2[n] - off[n]).abs().max().item()
        print(f"  {n}: on-off {e_on:.3e} off-off {e_off:.3e} scale {scale:.3e}")
        assert e_on <= max(e_off, 8 * 2.0 ** -24 * scale), (n, e_on, e_off, scale)


def test_on_against_float64(gpu, heartbeat, monkeypatch):
    from texbias import conv
    m = _pair(seed=41)
    calls = _spy(conv, monkeypatch)
    y, ours, a32, r64, inter, names = _three_runs(m, _ref, SHAPE, monkeypatch)
    assert calls.count((True, True)) == 1, calls
    assert "SkipCatFn" in type(y.grad_fn).__name__
    _judge("pair", "skip-dx-add", ours, a32, r64, inter, names)
