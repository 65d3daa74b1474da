"""ConvTranspose3d(64 -> 16, 3, stride 2, padding 1, output_padding 1) in split precision on the bf16 matrix
cores (csrc/conv_up.hip, k_convT_split; csrc/split_bf16.h) behind tb_convT3d_mfma_{,add_}f32: forward with
bias, the stacked stride-2 Conv3d(16 -> 64)'s input gradient, `add` and `out` as tensors of their own and as
channel slices [16, 32) of 32-channel tensors, integer data bit for bit against float64, small and tiny inputs,
a z segment three times round the 2-slot plane ring, run-to-run bit equality, and the f32 kernel where the split
kernel has no plan.

Bar: close64 of tests/test_gpu_conv_mfma_split.py -- the error against float64 within 4 x max(ATen float32's,
1e-6 of the largest value).  The kernel that ran is read from the profiler's kernel names, so a silent fall back
to the other kernel fails.

Shapes are (N, Di, Hi, Wi).  The host plan (ct_plan in csrc/conv_up.hip) serves Cin = 64 at 32 <= Wi <= 60: two
input rows per step up to Wi = 40, one above.  On the f32 kernel (k_convT_mfma64), by that plan:
  * (1, 1, 1, 4), (1, 4, 3, 12), (2, 5, 6, 20), (3, 6, 172, 8): rows narrower than 32 measured slower or within
    the spread on the split kernel (one or two position tiles per step; the width sweep of profiles/r21);
  * (1, 3, 3, 64), the widest row the entry accepts: the 2-slot ring of one row (+ 1) at 65 positions, 99 840 B,
    and the 65 536 B of partial tiles exceed 160 KiB -- the shape `test_no_plan_runs_f32_kernel` takes;
  * Cin = 32 (the input gradient of Conv3d(16 -> 32, stride 2)): the kernel's two-group form is not built.
These cases assert the f32 kernel's name and keep the accuracy bar.  What they were listed to exercise runs on the
split kernel at the narrowest rows it serves: (1, 1, 1, 32) one row, every neighbour absent, Di shorter than the
ring; (1, 4, 3, 36) tiles that straddle rows and a last partial tile (72 positions); (2, 5, 6, 32) mid-size;
(1, 3, 3, 60) the widest planned row (one row per step); (3, 6, 172, 32) 258 (n, row block) columns on 256 CUs,
one z segment of 6 planes, three times round the 2-slot ring.

Worst close64 ratio e_ours / max(e_aten, 1e-6 max|y|) measured on MI355X (bar: 4): 0.381."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SPLIT, F32 = "k_convT_split", "k_convT_mfma64"
S0, S1, S2, S3, S4, S5 = (1, 1, 1, 4), (2, 3, 5, 40), (1, 4, 3, 12), (2, 5, 6, 20), (1, 3, 3, 64), (3, 6, 172, 8)
W0, W2, W3, W4, W5 = (1, 1, 1, 32), (1, 4, 3, 36), (2, 5, 6, 32), (1, 3, 3, 60), (3, 6, 172, 32)  # their split-kernel kin
ALL = [S0, S1, S2, S3, S4, S5, W0, W2, W3, W4, W5]


@pytest.fixture(scope="module")
def conv(gpu):
    from texbias import conv
    return conv


def kernels(fn):
    """(fn's result, the names of the kernels it launched)"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    return out, [e.key for e in prof.key_averages() if e.device_time_total > 0]


def ran(names, want, other):
    assert any(want in k for k in names) and not any(other in k for k in names), names


def gate(shape, cin=64):
    """(the kernel the host plan names for a shape, the other one)"""
    return (SPLIT, F32) if cin == 64 and 32 <= shape[3] <= 60 else (F32, SPLIT)


def close64(ours, ref32, ref64, what=""):
    scale = ref64.abs().max().item()
    e_ours = (ours.double() - ref64).abs().max().item()
    e_ref = (ref32.double() - ref64).abs().max().item()
    print(f"close64 {what}: ours {e_ours:.3e} aten {e_ref:.3e} scale {scale:.3e} "
          f"ratio {e_ours / max(e_ref, 1e-6 * scale):.3f}")
    assert e_ours <= 4 * max(e_ref, 1e-6 * scale), (e_ours, e_ref, scale)


_cache = {}


def convT(x, w, b):
    return F.conv_transpose3d(x, w, b, stride=2, padding=1, output_padding=1)


def data(shape, scale=1.0, integer=False):
    """x, w, b and the forward references (ATen float32, float64) of a shape, made once"""
    key = (shape, scale, integer)
    if key not in _cache:
        gen = torch.Generator(device="cuda").manual_seed(9876 + sum(shape))
        N, D, H, W = shape
        if integer:  # |sum| <= 8 taps x 64 channels x 4 x 2 + 4 < 2^24 and every value a bf16: exact on either kernel
            x = torch.randint(-4, 5, (N, 64, D, H, W), device="cuda", generator=gen).float()
            w = torch.randint(-2, 3, (64, 16, 3, 3, 3), device="cuda", generator=gen).float()
            b = torch.randint(-4, 5, (16,), device="cuda", generator=gen).float()
        else:
            x = torch.randn((N, 64, D, H, W), device="cuda", generator=gen) * scale
            w = torch.randn((64, 16, 3, 3, 3), device="cuda", generator=gen) * (1.0 / (8 * 64) ** 0.5)
            b = torch.randn(16, device="cuda", generator=gen) * scale
        d = dict(x=x, w=w, b=b)
        d["y32"], d["y64"] = convT(x, w, b), convT(x.double(), w.double(), b.double())
        _cache[key] = d
    return _cache[key]


@pytest.mark.parametrize("shape", ALL)
def test_forward_bias(conv, shape):
    """One partial tile with every neighbour absent and Di shorter than the ring; the C3 row width with Hi no
    multiple of the rows per step; tiles that straddle rows; a mid-size case; the widest row; 258 (n, row block)
    columns, one z segment of 6 planes per block -- each on the kernel the host plan names (module docstring)."""
    d = data(shape)
    y, names = kernels(lambda: conv.convT_mfma(d["x"], d["w"], d["b"]))
    ran(names, *gate(shape))
    close64(y, d["y32"], d["y64"], f"fwd {shape}")


@pytest.mark.parametrize("shape", [S1, S2, W2])
def test_stacked_input_gradient(conv, shape):
    """The input gradient of the stacked Conv3d(16 -> 64, stride 2) (weight [64, 16, 3, 3, 3] read as that
    layer's) against float64 autograd."""
    gen = torch.Generator(device="cuda").manual_seed(55)
    N, D, H, W = shape
    gy = torch.randn((N, 64, D, H, W), device="cuda", generator=gen)
    w = torch.randn((64, 16, 3, 3, 3), device="cuda", generator=gen) * (1.0 / (27 * 16) ** 0.5)
    x32 = torch.zeros((N, 16, 2 * D, 2 * H, 2 * W), device="cuda", requires_grad=True)
    x64 = x32.detach().double().requires_grad_(True)
    g32, = torch.autograd.grad(F.conv3d(x32, w, None, stride=2, padding=1), x32, gy)
    g64, = torch.autograd.grad(F.conv3d(x64, w.double(), None, stride=2, padding=1), x64, gy.double())
    g, names = kernels(lambda: conv.convT_mfma(gy, w, None))
    ran(names, *gate(shape))
    close64(g, g32, g64, f"stacked dgrad {shape}")


@pytest.mark.parametrize("shape", [(1, 6, 8, 8), (2, 3, 7, 12)])
def test_cin32_through_s2_input_gradient(conv, shape):
    """Cin = 32 through the stride-2 Conv3d(16 -> 32) layer's input gradient: the f32 kernel (the split kernel's
    two-group form is not built), and its accuracy."""
    torch.manual_seed(6)
    N, D, H, W = shape
    x = torch.randn((N, 16, 2 * D, 2 * H, 2 * W), device="cuda", requires_grad=True)
    ours = conv.Conv3d(16, 32, 3, stride=2, padding=1).cuda()
    y = ours(x)
    g = torch.randn_like(y)
    assert conv.s2_dgrad_applies(g, x, ours.weight, ours.stride, ours.padding)
    (gx,), names = kernels(lambda: torch.autograd.grad(y, (x,), g))
    ran(names, F32, SPLIT)
    x64 = x.detach().double().requires_grad_(True)
    gx64, = torch.autograd.grad(F.conv3d(x64, ours.weight.double(), ours.bias.double(), stride=2, padding=1), x64,
                                g.double())
    xr = x.detach().clone().requires_grad_(True)
    gxr, = torch.autograd.grad(F.conv3d(xr, ours.weight, ours.bias, stride=2, padding=1), xr, g)
    close64(gx, gxr, gx64, f"Cin 32 dgrad {shape}")


@pytest.mark.parametrize("shape", [S1, S3, W3])
@pytest.mark.parametrize("sliced", [False, True])
def test_add_and_out(conv, shape, sliced):
    """`add` summed in the store and `out` written in place: tensors of their own, and channels [16, 32) of
    32-channel tensors, whose other half comes back bit for bit unchanged."""
    d = data(shape)
    N, D, H, W = shape
    gen = torch.Generator(device="cuda").manual_seed(78)
    wide_a = torch.randn((N, 32, 2 * D, 2 * H, 2 * W), device="cuda", generator=gen)
    wide_o = torch.randn((N, 32, 2 * D, 2 * H, 2 * W), device="cuda", generator=gen)
    before = wide_o.clone()
    add = wide_a[:, 16:] if sliced else wide_a[:, 16:].contiguous()
    out = wide_o[:, 16:] if sliced else torch.empty_like(d["y32"])
    y, names = kernels(lambda: conv.convT_mfma(d["x"], d["w"], d["b"], add=add, out=out))
    ran(names, *gate(shape))
    assert y.data_ptr() == out.data_ptr()
    close64(y, d["y32"] + add, d["y64"] + add.double(), f"add/out {shape} sliced={sliced}")
    assert torch.equal(wide_o[:, :16], before[:, :16])
    if not sliced:
        assert torch.equal(wide_o, before)
    # `add` alone, and `out` alone
    y2 = conv.convT_mfma(d["x"], d["w"], d["b"], add=add)
    assert torch.equal(y2, y)
    y3 = conv.convT_mfma(d["x"], d["w"], d["b"], out=out)
    close64(y3, d["y32"], d["y64"], f"out {shape} sliced={sliced}")
    assert torch.equal(wide_o[:, :16], before[:, :16])


def test_add_and_out_f32_kernel(conv):
    """The f32 kernel honours `add` and the sample strides too, with one input row per step (the widest row, no
    split plan); `test_add_and_out` at (2, 5, 6, 20) is its two-row form."""
    d = data(S4)
    N, D, H, W = S4
    gen = torch.Generator(device="cuda").manual_seed(79)
    wide_a = torch.randn((N, 32, 2 * D, 2 * H, 2 * W), device="cuda", generator=gen)
    wide_o = torch.randn((N, 32, 2 * D, 2 * H, 2 * W), device="cuda", generator=gen)
    before = wide_o.clone()
    y, names = kernels(lambda: conv.convT_mfma(d["x"], d["w"], d["b"], add=wide_a[:, 16:], out=wide_o[:, 16:]))
    ran(names, F32, SPLIT)
    close64(y, d["y32"] + wide_a[:, 16:], d["y64"] + wide_a[:, 16:].double(), "add/out f32 kernel")
    assert torch.equal(wide_o[:, :16], before[:, :16])


@pytest.mark.parametrize("shape", [S1, S2, S5, W0, W2, W4, W5])
def test_integer_data_exact(conv, shape):
    """Integer x, w and bias, exact in bf16 and in every f32 sum: the result equals float64 bit for bit, so no
    lane, tap, class, channel or group is misplaced."""
    d = data(shape, integer=True)
    y, names = kernels(lambda: conv.convT_mfma(d["x"], d["w"], d["b"]))
    ran(names, *gate(shape))
    assert torch.equal(y.double(), d["y64"])


@pytest.mark.parametrize("shape", [S1, W2])
@pytest.mark.parametrize("scale", [1e-6, 2.0 ** -100])
def test_scaled_inputs(conv, shape, scale):
    """Inputs (and bias) scaled by 1e-6 and 2^-100, weights unscaled: the parts keep f32's exponent."""
    d = data(shape, scale)
    y, names = kernels(lambda: conv.convT_mfma(d["x"], d["w"], d["b"]))
    ran(names, SPLIT, F32)
    close64(y, d["y32"], d["y64"], f"{shape} scale {scale:.3e}")


def test_two_calls_bit_equal(conv):
    """No atomics, a fixed order of operations: two calls agree bit for bit, with and without `add`."""
    for shape in (S1, W5):
        d = data(shape)
        a, b = conv.convT_mfma(d["x"], d["w"], d["b"]), conv.convT_mfma(d["x"], d["w"], d["b"])
        assert torch.equal(a, b)
        add = d["y32"]
        a, b = conv.convT_mfma(d["x"], d["w"], d["b"], add=add), conv.convT_mfma(d["x"], d["w"], d["b"], add=add)
        assert torch.equal(a, b)


def test_no_plan_runs_f32_kernel(conv):
    """Wi = 64 (ct_plan: one row per step still needs 99 840 B of ring + 65 536 B of partial tiles): the f32 MFMA
    kernel runs (its name, and its accuracy)."""
    d = data(S4)
    y, names = kernels(lambda: conv.convT_mfma(d["x"], d["w"], d["b"]))
    ran(names, F32, SPLIT)
    close64(y, d["y32"], d["y64"], f"{S4} (f32 kernel)")
