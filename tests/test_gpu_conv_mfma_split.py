"""The 32 -> 32 and 64 -> 64 stride-1 3x3x3 convs in split precision on the bf16 matrix cores (csrc/conv_up.hip,
k_conv_mfma_split; csrc/split_bf16.h) behind tb_conv3d_mfma_{,add_,dgrad_}f32: forward with bias, `add` (a
separate tensor and a C-channel slice of a 2C-channel one), the input gradient (flipped, transposed weight),
integer data bit for bit against float64, small and tiny inputs, z segments longer than the plane ring,
run-to-run bit equality, and the f32 kernel where the split kernel has no plan.

Bar: close64 of tests/test_gpu_conv_up.py -- the error against float64 within 4 x max(ATen float32's,
1e-6 of the largest value).  The kernel that ran is read from the profiler's kernel names, so a fall back to
the f32 kernel (k_conv3d_mfma_s1) fails.

Shapes are (N, D, H, W).  The host plan (xs_plan in csrc/conv_up.hip) takes the most rows per step, up to
4, whose staging tasks fit 512 threads and whose 3-slot ring and partial tiles fit 160 KiB: C = 32 serves
16 <= W <= 64 (narrower rows measured slower and stay on the f32 kernel), C = 64 W <= 36.  The long-march shapes
give one z segment of 6 planes per block on 256 CUs (3 ring slots + 2 = 5).

Worst close64 ratio e_ours / max(e_aten, 1e-6 max|y|) measured on MI355X (bar: 4): 0.250 on the split kernel
(the input gradient at (3, 6, 172, 16) and at (2, 3, 5, 40) scaled by 1e-6), 0.550 on the f32 kernel (C = 64, W = 40)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SPLIT, F32 = "k_conv_mfma_split", "k_conv3d_mfma_s1"
A1, A2, A3, A4 = (32, (1, 1, 1, 4)), (32, (2, 3, 5, 40)), (32, (3, 6, 172, 16)), (32, (1, 3, 3, 64))
B0, B1, B2, B3, B4 = (64, (1, 1, 1, 4)), (64, (2, 4, 5, 20)), (64, (1, 3, 3, 8)), (64, (2, 12, 40, 20)), (64, (1, 3, 3, 36))
ALL = [A1, A2, A3, A4, B0, B1, B2, B3, B4]
PAST = [(64, (1, 3, 3, 40)), (64, (1, 3, 3, 48))]


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


def gate(case):
    """(the kernel the host gate names for a case, the other one): C = 32 rows narrower than 16 stay on the f32
    kernel (the split form measured slower at W = 8)"""
    return (F32, SPLIT) if case[0] == 32 and case[1][3] < 16 else (SPLIT, F32)


def close64(ours, ref32, ref64, what=""):
    scale = ref64.abs().max().item()
    e_ours = (ours.double() - ref64).abs().max().item()
    e_ref = (ref32.double() - ref64).abs().max().item()
    print(f"close64 {what}: ours {e_ours:.3e} aten {e_ref:.3e} scale {scale:.3e} "
          f"ratio {e_ours / max(e_ref, 1e-6 * scale):.3f}")
    assert e_ours <= 4 * max(e_ref, 1e-6 * scale), (e_ours, e_ref, scale)


_cache = {}


def data(case, scale=1.0, integer=False):
    """x, w, b and the forward / input-gradient references (ATen float32, float64) of a case, made once"""
    key = (case, scale, integer)
    if key not in _cache:
        C, shape = case
        gen = torch.Generator(device="cuda").manual_seed(4321 + C + sum(shape))
        N, D, H, W = shape
        if integer:  # |sum| <= 27 C * 4 * 2 + 4 < 2^24 and every value a bf16: exact on either kernel
            x = torch.randint(-4, 5, (N, C, D, H, W), device="cuda", generator=gen).float()
            w = torch.randint(-2, 3, (C, C, 3, 3, 3), device="cuda", generator=gen).float()
            b = torch.randint(-4, 5, (C,), device="cuda", generator=gen).float()
        else:
            x = torch.randn((N, C, D, H, W), device="cuda", generator=gen) * scale
            w = torch.randn((C, C, 3, 3, 3), device="cuda", generator=gen) * (1.0 / (27 * C) ** 0.5)
            b = torch.randn(C, device="cuda", generator=gen) * scale
        d = dict(x=x, w=w, b=b)
        d["y32"], d["y64"] = F.conv3d(x, w, b, padding=1), F.conv3d(x.double(), w.double(), b.double(), padding=1)
        d["g32"] = F.conv_transpose3d(x, w, None, padding=1)
        d["g64"] = F.conv_transpose3d(x.double(), w.double(), None, padding=1)
        _cache[key] = d
    return _cache[key]


@pytest.mark.parametrize("case", ALL)
def test_forward_bias(conv, case):
    """One partial tile with every neighbour absent and D shorter than the ring (C = 32 at W = 4 is the f32
    kernel's by the host gate, C = 64 the split kernel's); the C3 row widths (40 and 20: tiles that straddle
    rows, H no multiple of the rows per step, four output-tile groups at C = 64); z segments of 6 planes, twice
    round the ring; the widest rows the split kernel takes."""
    d = data(case)
    y, names = kernels(lambda: conv.conv_mfma(d["x"], d["w"], d["b"]))
    ran(names, *gate(case))
    close64(y, d["y32"], d["y64"], f"fwd {case}")


@pytest.mark.parametrize("case", ALL)
def test_input_gradient(conv, case):
    """The input gradient (A = W[c][m][26 - t]) at every shape."""
    d = data(case)
    g, names = kernels(lambda: conv.conv_mfma_dgrad(d["x"], d["w"]))
    ran(names, *gate(case))
    close64(g, d["g32"], d["g64"], f"dgrad {case}")


@pytest.mark.parametrize("case", [A2, B1])
def test_forward_add(conv, case):
    """Forward with bias and `add` as a separate tensor."""
    d = data(case)
    add = torch.randn(d["x"].shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(77))
    y, names = kernels(lambda: conv.conv_mfma(d["x"], d["w"], d["b"], add))
    ran(names, SPLIT, F32)
    close64(y, d["y32"] + add, d["y64"] + add.double(), f"add {case}")


@pytest.mark.parametrize("case", [A2, B1])
@pytest.mark.parametrize("sliced", [False, True])
def test_input_gradient_add(conv, case, sliced):
    """The input gradient with `add`: a tensor of its own, and the upper C channels of a 2C-channel tensor read
    in place (add_sn = 2 C D H W)."""
    d = data(case)
    C, shape = case
    gen = torch.Generator(device="cuda").manual_seed(78)
    wide = torch.randn((shape[0], 2 * C) + shape[1:], device="cuda", generator=gen)
    add = wide[:, C:] if sliced else wide[:, C:].contiguous()
    g, names = kernels(lambda: conv.conv_mfma_dgrad(d["x"], d["w"], add))
    ran(names, SPLIT, F32)
    close64(g, d["g32"] + add, d["g64"] + add.double(), f"dgrad add {case} sliced={sliced}")


@pytest.mark.parametrize("case", [A2, B1, B3])
def test_integer_data_exact(conv, case):
    """Integer x, w and bias, exact in bf16 and in every f32 sum: the forward result and the input gradient equal
    float64 bit for bit, so no lane, tap, channel or group is misplaced."""
    d = data(case, integer=True)
    y, names = kernels(lambda: conv.conv_mfma(d["x"], d["w"], d["b"]))
    ran(names, SPLIT, F32)
    assert torch.equal(y.double(), d["y64"])
    g, names = kernels(lambda: conv.conv_mfma_dgrad(d["x"], d["w"]))
    ran(names, SPLIT, F32)
    assert torch.equal(g.double(), d["g64"])


@pytest.mark.parametrize("case", [A2, B1])
@pytest.mark.parametrize("scale", [1e-6, 2.0 ** -100])
def test_scaled_inputs(conv, case, scale):
    """Inputs (and bias) scaled by 1e-6 and 2^-100, weights unscaled: the parts keep f32's exponent."""
    d = data(case, scale)
    y, names = kernels(lambda: conv.conv_mfma(d["x"], d["w"], d["b"]))
    ran(names, SPLIT, F32)
    close64(y, d["y32"], d["y64"], f"{case} scale {scale:.3e}")
    g = conv.conv_mfma_dgrad(d["x"], d["w"])
    close64(g, d["g32"], d["g64"], f"dgrad {case} scale {scale:.3e}")


def test_two_calls_bit_equal(conv):
    """No atomics, a fixed order of operations: two calls agree bit for bit (forward with add, and the input
    gradient at the long-march shapes)."""
    for case in (A2, B1):
        d = data(case)
        add = d["g32"]
        a, b = conv.conv_mfma(d["x"], d["w"], d["b"], add), conv.conv_mfma(d["x"], d["w"], d["b"], add)
        assert torch.equal(a, b)
    for case in (A3, B3):
        d = data(case)
        a, b = conv.conv_mfma_dgrad(d["x"], d["w"]), conv.conv_mfma_dgrad(d["x"], d["w"])
        assert torch.equal(a, b)


@pytest.mark.parametrize("case", PAST)
def test_no_plan_runs_f32_kernel(conv, case):
    """C = 64 at W = 40 (one row per step: 155 520 B of ring + 12 288 B of partial tiles exceed 160 KiB) and at
    W = 48, the widest row the entry accepts (576 staging tasks for 512 threads): the f32 MFMA kernel runs
    (its name, and its accuracy)."""
    d = data(case)
    y, names = kernels(lambda: conv.conv_mfma(d["x"], d["w"], d["b"]))
    ran(names, F32, SPLIT)
    close64(y, d["y32"], d["y64"], f"{case} (f32 kernel)")
    g, names = kernels(lambda: conv.conv_mfma_dgrad(d["x"], d["w"]))
    ran(names, F32, SPLIT)
    close64(g, d["g32"], d["g64"], f"dgrad {case} (f32 kernel)")
