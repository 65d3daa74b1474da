"""Fused Dice statistics (tb_dice_sums_f32 / _bwd) against the plain PyTorch formula of
DiceLoss(sigmoid=True, squared_pred=True) -- forward value and input gradient (float32)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


def _against_cpu64(loss, x, t):
    """The fused loss and its input gradient vs the plain formula on the CPU in float64 (DiceLoss.forward's
    own fallback); returns the fused (loss, gradient, upstream gradient)."""
    lf = loss(x, t)
    gup = torch.rand(lf.shape, device="cuda") + 0.5
    gf, = torch.autograd.grad(lf, x, gup)
    xc = x.detach().cpu().double().requires_grad_(True)
    lr = loss(xc, t.cpu().double())   # CPU float64: the plain formula
    gr, = torch.autograd.grad(lr, xc, gup.cpu().double())
    assert lf.shape == lr.shape
    torch.testing.assert_close(lf.cpu().double(), lr, rtol=0, atol=1e-5)
    torch.testing.assert_close(gf.cpu().double(), gr, rtol=1e-4, atol=1e-7)
    return lf, gf, gup


# The reductions take 16384-voxel chunks per block.  The last four shapes: S = 105 (scalar path, one partial
# chunk), S = 17408 (float4 path, one full chunk and a ragged one: the finalize sums two partials), S = 17391
# (scalar path over two chunks), S = 16388 (a second chunk of exactly one float4).
@pytest.mark.parametrize("shape,squared,batch,red", [((2, 3, 24, 20, 18), True, False, "mean"),
                                                     ((1, 2, 16, 9, 7), False, False, "mean"),
                                                     ((2, 3, 12, 10, 8), True, True, "mean"),
                                                     ((2, 3, 12, 10, 8), True, False, "sum"),
                                                     ((3, 2, 8, 6, 4), True, False, "none"),
                                                     ((3, 2, 8, 6, 4), False, True, "none"),
                                                     ((1, 2, 3, 5, 7), True, False, "mean"),
                                                     ((2, 2, 17, 32, 32), True, False, "mean"),
                                                     ((1, 3, 33, 31, 17), True, False, "none"),
                                                     ((1, 2, 17, 241, 4), False, True, "sum")])
def test_dice_fused_matches_plain(gpu, shape, squared, batch, red):
    """The fused loss (sums sweep + one-launch finalize, and the one-launch gradient of the sums) vs the
    plain formula on the CPU in float64, every reduction."""
    from texbias.losses import DiceLoss
    torch.manual_seed(0)
    x = torch.randn(shape, device="cuda", requires_grad=True)
    t = (torch.rand(shape, device="cuda") > 0.6).float()
    loss = DiceLoss(sigmoid=True, squared_pred=squared, batch=batch, reduction=red)
    _against_cpu64(loss, x, t)


@pytest.mark.parametrize("variant", ["soft_target", "smooth", "empty_target"])
def test_dice_fused_matches_plain_variants(gpu, variant):
    """Same bars over two chunks: soft targets (t^2 != t), smoothing terms other than the default, and an
    all-zero target under logits of -8 (the sums are the smoothing terms' size)."""
    from texbias.losses import DiceLoss
    torch.manual_seed(1)
    shape = (2, 2, 17, 32, 32)
    kw = {}
    x = torch.randn(shape, device="cuda")
    t = (torch.rand(shape, device="cuda") > 0.6).float()
    if variant == "soft_target":
        t = torch.rand(shape, device="cuda")
    elif variant == "smooth":
        kw = dict(smooth_nr=1e-3, smooth_dr=0.5)
    else:
        x, t = torch.full(shape, -8.0, device="cuda"), torch.zeros(shape, device="cuda")
    loss = DiceLoss(sigmoid=True, squared_pred=True, **kw)
    _against_cpu64(loss, x.requires_grad_(True), t)


def test_dice_misaligned_operands(gpu):
    """x and t as contiguous views one float into a larger storage (data_ptr % 16 == 4): S % 4 == 0 over two
    chunks, but the float4 path must not be taken.  Against CPU float64, and bit-identical on a second call."""
    from texbias.losses import DiceLoss
    torch.manual_seed(2)
    shape = (2, 2, 17, 32, 32)
    n = math.prod(shape)
    assert math.prod(shape[2:]) % 4 == 0 and math.prod(shape[2:]) > 16384
    x = torch.randn(n + 1, device="cuda")[1:].view(shape).detach().requires_grad_(True)
    t = (torch.rand(n + 1, device="cuda") > 0.6).float()[1:].view(shape)
    assert x.data_ptr() % 16 == 4 and t.data_ptr() % 16 == 4 and x.is_contiguous() and t.is_contiguous()
    loss = DiceLoss(sigmoid=True, squared_pred=True)
    lf, gf, gup = _against_cpu64(loss, x, t)
    lf2 = loss(x, t)
    gf2, = torch.autograd.grad(lf2, x, gup)
    assert torch.equal(lf2, lf) and torch.equal(gf2, gf)
