"""The few-channel full-resolution kernels at their edges, called directly (texbias.conv.small_conv,
conv_s2_fewin, convT_fewout): single planes and rows, widths that are no multiple of the 4 outputs a
thread owns, second z and row blocks of one plane / one row, the widest row, every residual mode of the
z-march (none, a separate tensor, the input itself) and weight counts that end at different places of a
16-pair weight batch.  Against a float64 reference, by the rule of tests/test_gpu_conv_up.py: the error vs
float64 within 4x max(ATen float32's error, 1e-6 of the largest value)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def conv(gpu):
    from texbias import conv
    return conv


def close64(ours, ref32, ref64):
    scale = ref64.abs().max().item()
    e_ours = (ours.double() - ref64).abs().max().item()
    e_ref = (ref32.double() - ref64).abs().max().item()
    assert e_ours <= 4 * max(e_ref, 1e-6 * scale), (e_ours, e_ref, scale)


SMALL = [(3, 3, (1, 1, 1, 5)),      # a single plane, a single row, W no multiple of 4
         (3, 3, (2, 9, 7, 10)),     # a second z block of one plane, a second row block of one row
         (3, 3, (1, 8, 6, 168)),    # the widest row: 252 of 256 threads
         (4, 4, (1, 17, 13, 36)),
         (2, 3, (1, 10, 8, 17)),
         (1, 4, (2, 5, 13, 17)),
         (4, 2, (1, 7, 9, 160))]


def _small_case(cin, cout, shape, seed=0):
    torch.manual_seed(seed)
    x = torch.randn((shape[0], cin) + shape[1:], device="cuda")
    w = torch.randn((cout, cin, 3, 3, 3), device="cuda") * (1.0 / (27 * cin) ** 0.5)
    b = torch.randn(cout, device="cuda")
    return x, w, b


@pytest.mark.parametrize("cin,cout,shape,mode", [c + (m,) for c in SMALL for m in ("none", "separate", "input")
                                                 if m != "input" or c[0] == c[1]])  # conv(x) + x: the input's shape
def test_small_conv(conv, cin, cout, shape, mode):
    x, w, b = _small_case(cin, cout, shape)
    add = None if mode == "none" else x if mode == "input" else \
        torch.randn((shape[0], cout) + shape[1:], device="cuda")
    y = conv.small_conv(x, w, b, add=add)
    ref = F.conv3d(x, w, b, padding=1)
    ref64 = F.conv3d(x.double(), w.double(), b.double(), padding=1)
    if add is not None:
        ref, ref64 = ref + add, ref64 + add.double()
    close64(y, ref, ref64)


@pytest.mark.parametrize("cin,cout,shape", [c for c in SMALL if c[0] == c[1]])
def test_small_conv_residual_from_input_bitwise(conv, cin, cout, shape):
    """add = x takes the residual from the staged plane; add = a copy of x loads it: the same sum."""
    x, w, b = _small_case(cin, cout, shape, seed=1)
    assert torch.equal(conv.small_conv(x, w, b, add=x), conv.small_conv(x, w, b, add=x.clone()))


@pytest.mark.parametrize("cin,cout,shape", [c for c in SMALL if c[0] == c[1]])
def test_small_conv_input_grad_with_residual(conv, cin, cout, shape):
    """The input gradient of conv(x) + x as the flipped-weight call with add = g."""
    x, w, _ = _small_case(cin, cout, shape, seed=2)
    g = torch.randn_like(x)
    dx = conv.small_conv(g, w.flip(2, 3, 4).transpose(0, 1).contiguous(), None, add=g)
    x32 = x.clone().requires_grad_(True)
    ref, = torch.autograd.grad(F.conv3d(x32, w, None, padding=1) + x32, x32, g)
    x64 = x.double().requires_grad_(True)
    ref64, = torch.autograd.grad(F.conv3d(x64, w.double(), None, padding=1) + x64, x64, g.double())
    close64(dx, ref, ref64)


# weights per output pair: 27 cin, ending inside a 16-pair batch at 27 / 54 / 81 / 108 mod 16
@pytest.mark.parametrize("shape", [(1, 6, 4, 8), (2, 12, 10, 32), (1, 4, 6, 160)])
@pytest.mark.parametrize("cin,mout", [(4, 32), (3, 32), (1, 32), (2, 16), (3, 16)])
def test_conv_s2_fewin(conv, cin, mout, shape):
    """(4, 32) runs the 512-thread form (the halves of the block split the output pairs)."""
    torch.manual_seed(3)
    x = torch.randn((shape[0], cin) + shape[1:], device="cuda")
    w = torch.randn((mout, cin, 3, 3, 3), device="cuda") * (1.0 / (27 * cin) ** 0.5)
    b = torch.randn(mout, device="cuda")
    y = conv.conv_s2_fewin(x, conv.s2_pairs(w), b, mout)
    ref = F.conv3d(x, w, b, stride=2, padding=1)
    ref64 = F.conv3d(x.double(), w.double(), b.double(), stride=2, padding=1)
    close64(y, ref, ref64)


# (2, 6, 5, 20) and (1, 1, 1, 4): the 512-thread form with a last partial row block; Wi = 80: 6 rows of 80
@pytest.mark.parametrize("shape", [(1, 1, 1, 4), (2, 6, 5, 20), (1, 4, 7, 80)])
@pytest.mark.parametrize("cin,cout", [(32, 3), (16, 3), (32, 4), (16, 1)])
def test_convT_fewout(conv, cin, cout, shape):
    """Forward on k_convT_fewout, input gradient through the layer's Route (k_conv_s2_fewin)."""
    torch.manual_seed(4)
    x = torch.randn((shape[0], cin) + shape[1:], device="cuda")
    w = torch.randn((cin, cout, 3, 3, 3), device="cuda") * (1.0 / (27 * cin) ** 0.5)
    b = torch.randn(cout, device="cuda")
    kw = dict(stride=2, padding=1, output_padding=1)
    y = conv.convT_fewout(x, w, b)
    x32 = x.clone().requires_grad_(True)
    ref = F.conv_transpose3d(x32, w, b, **kw)
    x64 = x.double().requires_grad_(True)
    ref64 = F.conv_transpose3d(x64, w.double(), b.double(), **kw)
    close64(y, ref.detach(), ref64.detach())
    route = conv.Route(x, w, (2, 2, 2), (1, 1, 1), (1, 1, 1), True)
    assert route.kind == "fewout" and route.dx == "fewout"
    g = torch.randn_like(y)
    gx = route.input_grad(g, x, w)
    gxr, = torch.autograd.grad(ref, x32, g)
    gx64, = torch.autograd.grad(ref64, x64, g.double())
    close64(gx, gxr, gx64)
