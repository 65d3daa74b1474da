"""The whole U-Net (channels 16 .. 256, four stride-2 levels) at 1 x 4 x 32 x 32 x 32 with the deep transposed
products on k_convT_stack (``conv.CONVT_STACK``: the up2 128 -> 32 and up3 384 -> 64 forwards, the input gradients
of the stacked 32 -> 128 and 64 -> 256 stride-2 units) and the skip share summed in that kernel's store
(``conv.CONVT_STACK_DX_ADD``), on against off.  The gates (least positions per layer, set from measurements at the
C3 shapes) are opened for the test's small grids (4^3 and 2^3).

* Route on against off, each against the float64 restatement of tests/_unet_ref.py: the bars of
  tests/test_gpu_unet_blocks.py (``_judge``) with the off arm in ATen's place -- the on arm's error within 4 x (tensors)
  or 10 x (scalar PReLU weights, zero-gradient biases) of max(the off arm's, the floor); the loss sum(y g) likewise.
* The skip-add switch alone, on against off: the same sums in the kernel's store as in the add pass, so every
  gradient is expected bit for bit equal; the bar is that of tests/test_gpu_unet_skip_dx_add.py (what two runs of
  the off path differ by, never less than 8 x 2^-24 of the largest value)."""
import copy

import pytest
import torch

import _unet_ref as R
from test_gpu_unet_blocks import _init, _judge

pytestmark = pytest.mark.gpu

SHAPE = (1, 4, 32, 32, 32)
OPEN = {(128, 32): 1, (256, 64): 1, (384, 64): 1}


def _net(seed):
    from texbias import unet
    return _init(unet.UNet(3, 4, 3), seed)


def _spy(conv, monkeypatch):
    calls = []
    real = conv.convT_stack

    def spy(x, w, b, add=None, out=None):
        calls.append((tuple(w.shape[:2]), add is not None, out is not None))
        return real(x, w, b, add=add, out=out)

    monkeypatch.setattr(conv, "convT_stack", spy)
    return calls


def _grads(m, x0, g):
    m = copy.deepcopy(m)   # fresh route caches per arm
    x = x0.clone().requires_grad_(True)
    y = m(x)
    y.backward(g)
    out = {"output": y.detach(), "input": x.grad, "loss": (y.detach() * g).sum()}
    out.update({n: p.grad for n, p in m.named_parameters()})
    return out


def _open(conv, monkeypatch):
    monkeypatch.setattr(conv, "CONVT_STACK_FWD_MIN_POS", dict(OPEN))
    monkeypatch.setattr(conv, "CONVT_STACK_DX_MIN_POS", dict(OPEN))


def test_route_on_against_off(gpu, monkeypatch):
    from texbias import conv
    m = _net(seed=50)
    x0 = torch.randn(SHAPE, device="cuda") * 1.5 + 0.3
    with torch.no_grad():
        g = torch.randn_like(copy.deepcopy(m)(x0))
    _open(conv, monkeypatch)
    monkeypatch.setattr(conv, "CONVT_STACK", True)
    monkeypatch.setattr(conv, "CONVT_STACK_DX_ADD", True)
    calls = _spy(conv, monkeypatch)
    on = _grads(m, x0, g)
    assert sorted(calls) == [((128, 32), False, False), ((128, 32), True, True), ((256, 64), True, True),
                             ((384, 64), False, False)], calls
    del calls[:]
    monkeypatch.setattr(conv, "CONVT_STACK", False)
    off = _grads(m, x0, g)
    assert not calls
    sd = {n: p.detach().double().requires_grad_(True) for n, p in m.named_parameters()}
    x64 = x0.double().requires_grad_(True)
    y64, inter = R.unet(sd, "model", x64, 4)
    y64.backward(g.double())
    r64 = {"output": y64.detach(), "input": x64.grad}
    r64.update({n: p.grad for n, p in sd.items()})
    l64 = (y64.detach() * g.double()).sum().item()
    lscale = (y64.detach() * g.double()).abs().sum().item()
    e_on, e_off = abs(on.pop("loss").item() - l64), abs(off.pop("loss").item() - l64)
    print(f"  loss: on {e_on:.3e} off {e_off:.3e} of sum|y g| {lscale:.3e}")
    assert e_on <= 4 * max(e_off, 1e-6 * lscale)
    _judge("unet-32", "convTs", on, off, r64, inter, [n for n, _ in m.named_parameters()])


def test_skip_add_on_equals_off(gpu, monkeypatch):
    from texbias import conv
    m = _net(seed=51)
    x0 = torch.randn(SHAPE, device="cuda") * 1.5 + 0.3
    with torch.no_grad():
        g = torch.randn_like(copy.deepcopy(m)(x0))
    _open(conv, monkeypatch)
    monkeypatch.setattr(conv, "CONVT_STACK", True)
    monkeypatch.setattr(conv, "CONVT_STACK_DX_ADD", True)
    calls = _spy(conv, monkeypatch)
    on = _grads(m, x0, g)
    assert sum(1 for c in calls if c[1] and c[2]) == 2, calls
    del calls[:]
    monkeypatch.setattr(conv, "CONVT_STACK_DX_ADD", False)
    off, off2 = _grads(m, x0, g), _grads(m, x0, g)
    assert len(calls) == 8 and not any(c[1] or c[2] for c in calls), calls
    for n in on:
        scale = off[n].abs().max().item()
        e_on = (on[n] - off[n]).abs().max().item()
        e_off = (off2[n] - off[n]).abs().max().item()
        print(f"  {n}: on-off {e_on:.3e} off-off {e_off:.3e} scale {scale:.3e}")
        assert e_on <= max(e_off, 8 * 2.0 ** -24 * scale), (n, e_on, e_off, scale)
