"""The 16 -> 16 full-resolution conv in split precision on the bf16 matrix cores (csrc/conv_up.hip,
k_conv16_split; csrc/split_bf16.h) behind tb_conv3d_fwd16_{,add_,dgrad_}f32: forward with bias, `add` (a
separate tensor and a 16-channel slice of a wider one), the input gradient (flipped, transposed weight),
small and tiny inputs, persistent step shares, run-to-run bit equality, and the f32 kernel past the LDS limit.

Bar: close64 of tests/test_gpu_conv_up.py -- the error against float64 within 4 x max(ATen float32's,
1e-6 of the largest value).  The kernel that ran is read from the profiler's kernel names, so a fall back to
the f32 kernel (k_conv3d_fwd16) fails.

Worst close64 ratio e_ours / max(e_aten, 1e-6 max|y|) measured on MI355X (bar: 4): 0.340
(the input gradient at (2, 5, 7, 80))."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SPLIT, F32 = "k_conv16_split", "k_conv3d_fwd16"
S1, S2, S3, S4, S5 = (1, 1, 1, 16), (1, 2, 4, 16), (2, 5, 7, 80), (1, 3, 3, 96), (2, 104, 30, 16)


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


def close64(ours, ref32, ref64, what=""):
    scale = ref64.abs().max().item()
    e_ours = (ours.double() - ref64).abs().max().item()
    e_ref = (ref32.double() - ref64).abs().max().item()
    print(f"close64 {what}: ours {e_ours:.3e} aten {e_ref:.3e} scale {scale:.3e} "
          f"ratio {e_ours / max(e_ref, 1e-6 * scale):.3f}")
    assert e_ours <= 4 * max(e_ref, 1e-6 * scale), (e_ours, e_ref, scale)


_cache = {}


def data(shape, scale=1.0):
    """x, w, b, g and the forward / input-gradient references (ATen float32, float64) of a shape, made once"""
    key = (shape, scale)
    if key not in _cache:
        gen = torch.Generator(device="cuda").manual_seed(1234 + sum(shape))
        N, D, H, W = shape
        x = torch.randn((N, 16, D, H, W), device="cuda", generator=gen) * scale
        w = torch.randn((16, 16, 3, 3, 3), device="cuda", generator=gen) * (1.0 / 432 ** 0.5)
        b = torch.randn(16, device="cuda", generator=gen) * scale
        d = dict(x=x, w=w, b=b)
        d["y32"], d["y64"] = F.conv3d(x, w, b, padding=1), F.conv3d(x.double(), w.double(), b.double(), padding=1)
        d["g32"] = F.conv_transpose3d(x, w, None, padding=1)
        d["g64"] = F.conv_transpose3d(x.double(), w.double(), None, padding=1)
        _cache[key] = d
    return _cache[key]


@pytest.mark.parametrize("shape", [S1, S2, S3, S4, S5])
def test_forward_bias(conv, shape):
    """Cases 1 - 5: one tile with every neighbour absent; D shorter than the ring and H no multiple of 3; the
    C3 row width with a partial last row block; W = 96, the widest row whose ring fits (3 slots); 2080
    block-steps >= 8 x 256 CUs: persistent shares that cross column boundaries."""
    d = data(shape)
    y, names = kernels(lambda: conv.conv_fwd16(d["x"], d["w"], d["b"]))
    ran(names, SPLIT, F32)
    close64(y, d["y32"], d["y64"], f"fwd {shape}")


@pytest.mark.parametrize("sliced", [False, True])
def test_forward_add(conv, sliced):
    """Cases 6, 7: `add` as a separate tensor, and as the upper 16 channels of a 32-channel tensor (read in
    place by the input-gradient entry, add_sn = 32 D H W)."""
    d = data(S3)
    gen = torch.Generator(device="cuda").manual_seed(77)
    wide = torch.randn((S3[0], 32) + S3[1:], device="cuda", generator=gen)
    add = wide[:, 16:] if sliced else wide[:, 16:].contiguous()
    if sliced:  # the strided `add` enters through the input-gradient entry point
        y, names = kernels(lambda: conv.conv_fwd16_dgrad(d["x"], d["w"], add))
        r32, r64 = d["g32"] + add, d["g64"] + add.double()
    else:
        y, names = kernels(lambda: conv.conv_fwd16(d["x"], d["w"], d["b"], add))
        r32, r64 = d["y32"] + add, d["y64"] + add.double()
    ran(names, SPLIT, F32)
    close64(y, r32, r64, f"add sliced={sliced}")


@pytest.mark.parametrize("with_add", [False, True])
def test_input_gradient(conv, with_add):
    """Case 8: the input gradient (A = W[c][m][26 - t]) with and without `add`."""
    d = data(S3)
    add = torch.randn(d["x"].shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(78)) \
        if with_add else None
    y, names = kernels(lambda: conv.conv_fwd16_dgrad(d["x"], d["w"], add))
    ran(names, SPLIT, F32)
    r32, r64 = d["g32"], d["g64"]
    if with_add:
        r32, r64 = r32 + add, r64 + add.double()
    close64(y, r32, r64, f"dgrad add={with_add}")


@pytest.mark.parametrize("scale", [1e-6, 2.0 ** -100])
def test_scaled_inputs(conv, scale):
    """Case 9: inputs (and bias) scaled by 1e-6 and 2^-100, weights unscaled: the parts keep f32's exponent."""
    d = data(S3, scale)
    y, names = kernels(lambda: conv.conv_fwd16(d["x"], d["w"], d["b"]))
    ran(names, SPLIT, F32)
    close64(y, d["y32"], d["y64"], f"scale {scale:.3e}")
    g = conv.conv_fwd16_dgrad(d["x"], d["w"])
    close64(g, d["g32"], d["g64"], f"dgrad scale {scale:.3e}")


def test_two_calls_bit_equal(conv):
    """Case 10: no atomics, a fixed order of operations: two calls agree bit for bit (forward with add, and
    the persistent-share shape)."""
    d = data(S3)
    add = d["g32"]
    a, b = conv.conv_fwd16(d["x"], d["w"], d["b"], add), conv.conv_fwd16(d["x"], d["w"], d["b"], add)
    assert torch.equal(a, b)
    d = data(S5)
    a, b = conv.conv_fwd16_dgrad(d["x"], d["w"]), conv.conv_fwd16_dgrad(d["x"], d["w"])
    assert torch.equal(a, b)


def test_ring_past_lds_runs_f32_kernel(conv):
    """W = 112: three plane slots of 3 x 5 x 117 x 32 B = 168 480 B exceed the 160 KB of LDS: the f32 MFMA kernel
    runs (its name, and its accuracy)."""
    d = data((1, 3, 3, 112))
    y, names = kernels(lambda: conv.conv_fwd16(d["x"], d["w"], d["b"]))
    ran(names, F32, SPLIT)
    close64(y, d["y32"], d["y64"], "W = 112 (f32 kernel)")
