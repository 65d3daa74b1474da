"""The float64 restatement of the U-Net blocks (tests/_unet_ref.py) against the ``texbias.unet`` modules on the
CPU in float64, where the modules take their plain ``nn`` path: output, input gradient and every parameter
gradient agree to 1e-12 of the tensor's largest value.

A conv bias ahead of an InstanceNorm has the true gradient 0 (the norm removes the mean), so its computed
value is the float64 rounding of sum dz (about 1e-14 here) and has no scale of its own: it is compared, and
bounded, against the size of the terms it sums, 1e-12 x sum |dz|."""
import pytest
import torch

import _unet_ref as R


def _init(m, seed):
    """PReLU slopes away from the init value 0.25."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("A.weight"):
                p.copy_(torch.rand(p.shape, generator=g) * 0.7 - 0.3)
    return m


def _compare(m, ref_fn, shape, seed):
    torch.manual_seed(seed)
    m = _init(m, seed).double()
    x = (torch.randn(shape, dtype=torch.float64) * 1.5 + 0.3).requires_grad_(True)
    y = m(x)
    g = torch.randn_like(y)
    names = [n for n, _ in m.named_parameters()]
    grads = torch.autograd.grad(y, [x] + list(m.parameters()), g)
    sd = {n: p.detach().clone().requires_grad_(True) for n, p in m.named_parameters()}
    xr = x.detach().clone().requires_grad_(True)
    yr, inter = ref_fn(sd, xr)
    (yr * g).sum().backward()

    def close(a, b, what, scale=None):
        scale = b.abs().max().item() if scale is None else scale
        err = (a - b).abs().max().item()
        assert scale > 0 and err <= 1e-12 * scale, (what, err, scale)

    assert y.shape == yr.shape
    close(y.detach(), yr.detach(), "output")
    close(grads[0], xr.grad, "input gradient")
    scalars, zero_b, tensors = R.split_params(names, inter)
    assert set(scalars) == {n for n in names if n.endswith("A.weight")}
    for n, gm in zip(names, grads[1:]):
        gr = sd[n].grad
        assert gr is not None and gr.shape == gm.shape, n
        if n in zero_b:
            cond = R.bias_cond(inter[zero_b[n]])
            close(gm, gr, n, scale=cond)
            assert gr.abs().max().item() <= 1e-12 * cond, (n, gr.abs().max().item(), cond)  # analytically zero
        else:
            close(gm, gr, n)
    for n, c in scalars.items():
        assert R.prelu_cond(inter[c]) > 0, n
    return zero_b, tensors


def test_strided_unit():
    from texbias import unet
    zero_b, tensors = _compare(unet.ResidualUnit(4, 16, 2), lambda sd, x: R.residual_unit(sd, "", x, 2),
                               (2, 4, 6, 8, 10), 0)
    assert set(zero_b) == {"conv.unit0.conv.bias", "conv.unit1.conv.bias"}
    assert "residual.bias" in tensors and "residual.weight" in tensors


def test_bottom_unit_pointwise_residual():
    from texbias import unet
    m = unet.ResidualUnit(128, 256, 1)
    assert tuple(m.residual.weight.shape[2:]) == (1, 1, 1)
    _compare(m, lambda sd, x: R.residual_unit(sd, "", x, 1), (2, 128, 2, 2, 2), 1)


@pytest.mark.parametrize("top", [True, False])
def test_up_block(top):
    from texbias import unet
    m = torch.nn.Sequential(unet.Convolution(8, 4, 2, is_transposed=True),
                            unet.ResidualUnit(4, 4, 1, subunits=1, last_conv_only=top))
    zero_b, tensors = _compare(m, lambda sd, x: R.up_block(sd, "", x, top), (2, 8, 3, 4, 5), 2)
    # the top unit's bare conv keeps a real bias gradient; below the top it sits ahead of a norm
    assert ("1.conv.unit0.conv.bias" in tensors) == top
    assert "0.conv.bias" in zero_b


def test_mini_unet():
    from texbias import unet
    m = unet.UNet(3, 4, 3, (16, 32, 64), (2, 2))
    zero_b, tensors = _compare(m, lambda sd, x: R.unet(sd, "model", x, 2), (2, 4, 8, 12, 20), 3)
    biases = {n for n, _ in m.named_parameters() if n.endswith("bias")}
    real = {"model.0.residual.bias", "model.1.submodule.0.residual.bias", "model.1.submodule.1.submodule.residual.bias",
            "model.2.1.conv.unit0.conv.bias"}
    assert biases - set(zero_b) == real
