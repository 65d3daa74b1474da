"""The conv GEMM on the split-precision tile (csrc/gemm_core.h SplitTile, csrc/conv_gemm.hip) through
conv.conv_gemm, against float64 ATen: every forward tile class, conv stride 1 / 2 / 1x1x1, the stride-1 input
gradient, the sub-pixel ConvTranspose3d (an empty k slice included), channel and position counts that divide no
tile, a 24-element tail stage, odd and even stage counts, split k and the direct store, `add` aliasing a
channel-sliced output, integer operands (exact), scaled / huge / infinite values, run-to-run bit equality.

Bar: close64 -- the error against float64 within 4 x max(ATen float32's, 1e-6 of the largest value).  The kernel
that ran is read from the profiler: M > 64 runs k_conv_gemm<128, 128, 2, 512, true> (the split tile), M <= 64 the
f32 tiles (<64, 64, 2, 256, false>, <32, 128, 1, 256, false>), which the per-layer timings left there.

The weight gradient (conv.wgrad_gemm) stays on the f32 tile, unchanged: tests/test_gpu_wgrad_gemm.py is its test.

Worst close64 ratio e_ours / max(e_aten, 1e-6 max|y|) measured on MI355X (bar: 4): 0.155 on the split tile
(8 -> 136 at 26^3, the direct store), 0.183 over all cases (24 -> 40, the f32 64 x 64 tile)."""
import re

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


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


def tile_of(M):
    return "128,128,2,512,true" if M > 64 else ("64,64,2,256,false" if M > 32 else "32,128,1,256,false")


def ran(names, M):
    """exactly the tile kernel of M's class ran"""
    tiles = [re.sub(r"\s+", "", k) for k in names if "k_conv_gemm<" in k]
    assert len(tiles) == 1 and f"k_conv_gemm<{tile_of(M)}>" in tiles[0], names


def close64(ours, ref32, ref64, what=""):
    scale = ref64.abs().max().item()
    e_ours = (ours.double() - ref64).abs().max().item()
    e_ref = (ref32.double() - ref64).abs().max().item()
    print(f"close64 {what}: ours {e_ours:.3e} aten {e_ref:.3e} scale {scale:.3e} "
          f"ratio {e_ours / max(e_ref, 1e-6 * scale):.3f}")
    assert e_ours <= 4 * max(e_ref, 1e-6 * scale), (e_ours, e_ref, scale)


def ref(mode, x, w, b, s, k):
    """ATen's result of the mode in x's dtype"""
    p = (k - 1) // 2
    if mode == "conv":
        return F.conv3d(x, w, b, stride=s, padding=p)
    if mode == "dgrad":  # the input gradient of a stride-1 conv with weight w
        return F.conv_transpose3d(x, w, b, stride=1, padding=p)
    return F.conv_transpose3d(x, w, b, stride=2, padding=1, output_padding=1)


def wshape(mode, cin, M, k):
    return (M, cin, k, k, k) if mode == "conv" else (cin, M, k, k, k)


# (mode, GEMM Cin, M, input (N, D, H, W), stride, k)
CASES = [
    ("conv", 8, 24, (1, 9, 3, 5), 1, 3),       # M <= 32
    ("conv", 24, 40, (2, 5, 7, 6), 1, 3),      # M <= 64: 40 channels, 420 positions
    ("conv", 128, 128, (1, 5, 5, 4), 1, 3),    # M > 64, stride 1
    ("conv", 64, 128, (2, 6, 6, 4), 2, 3),     # stride 2
    ("conv", 128, 256, (2, 5, 5, 4), 1, 1),    # 1x1x1
    ("conv", 24, 136, (2, 5, 7, 6), 1, 3),     # 136 channels (a partial second m tile), 420 positions (3.3 tiles)
    ("conv", 8, 72, (1, 7, 5, 9), 1, 3),       # K = 216: a 24-element tail stage
    ("conv", 8, 136, (1, 26, 26, 26), 1, 3),   # 276 blocks: no split k, the kernel's own store (bias there)
    ("dgrad", 128, 128, (1, 5, 5, 4), 1, 3),   # input gradient of a stride-1 conv
    ("dgrad", 16, 72, (2, 3, 5, 4), 1, 3),
    ("convT", 384, 64, (2, 5, 5, 4), 2, 3),    # CONVT_EMPTY of tests/test_gpu_conv_gemm.py (f32 tile)
    ("convT", 384, 72, (2, 5, 5, 4), 2, 3),    # the same on the split tile
    ("convT", 16, 136, (1, 3, 4, 5), 2, 3),    # the input gradient of a stride-2 conv 136 -> 16
    ("conv", 72, 384, (2, 6, 6, 4), 2, 3),     # the input gradient of ConvTranspose3d 384 -> 72
]

_cache = {}


def data(case, scale=1.0, integer=False):
    """x, w, b and the ATen float32 / float64 results of a case, made once"""
    key = (case, scale, integer)
    if key not in _cache:
        mode, cin, M, shape, s, k = case
        gen = torch.Generator(device="cuda").manual_seed(4321 + cin + M + sum(shape))
        xs, ws = (shape[0], cin) + shape[1:], wshape(mode, cin, M, k)
        if integer:
            x = torch.randint(-8, 9, xs, device="cuda", generator=gen).float()
            w = torch.randint(-8, 9, ws, device="cuda", generator=gen).float()
            b = torch.randint(-8, 9, (M,), device="cuda", generator=gen).float()
        else:
            x = torch.randn(xs, device="cuda", generator=gen) * scale
            w = torch.randn(ws, device="cuda", generator=gen) * (1.0 / (cin * k ** 3) ** 0.5)
            b = torch.randn(M, device="cuda", generator=gen) * scale
        d = dict(x=x, w=w, b=b, y32=ref(mode, x, w, b, s, k), y64=ref(mode, x.double(), w.double(), b.double(), s, k))
        _cache[key] = d
    return _cache[key]


def run(conv, case, d, **kw):
    mode, cin, M, shape, s, k = case
    return conv.conv_gemm(d["x"], d["w"], d["b"], mode, s, k, **kw)


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}-{'x'.join(map(str, c[3]))}-s{c[4]}k{c[5]}")
def test_against_float64(conv, case):
    d = data(case)
    y, names = kernels(lambda: run(conv, case, d))
    ran(names, case[2])
    assert y.shape == d["y32"].shape
    close64(y, d["y32"], d["y64"], str(case))


def test_cases_reach_pipeline_corners(conv):
    """No kernel runs: the planner's answers for the split-tile cases above -- an odd and an even number of
    stages per block, split k (k_cg_reduce) and the direct store, and a sub-pixel class whose K ends before the
    last k slice (a block that runs no stage and stores zeros)."""
    stages, splits = set(), set()
    for mode, cin, M, shape, s, k in CASES:
        if M <= 64:
            continue
        cfg = conv.conv_gemm_config((shape[0], cin) + shape[1:], M, mode, s, k)
        assert (cfg["BM"], cfg["BP"]) == (128, 128) and cfg["kper"] % 32 == 0
        stages.add(cfg["kper"] // 32)
        splits.add(cfg["nsplit"] > 1)
    assert any(n % 2 == 1 for n in stages) and any(n % 2 == 0 for n in stages), stages
    assert splits == {False, True}
    cfg = conv.conv_gemm_config((2, 384, 5, 5, 4), 72, "convT", 2, 3)
    assert cfg["nsplit"] > 1 and (cfg["nsplit"] - 1) * cfg["kper"] >= 384, cfg


def test_add_aliasing_channel_slice(conv):
    """`add` aliasing an output that is a channel slice of a wider buffer: the slice is conv + its old value,
    the neighbouring channels are untouched bit for bit."""
    case = ("conv", 32, 72, (2, 6, 8, 4), 2, 3)
    d = data(case)
    gen = torch.Generator(device="cuda").manual_seed(5)
    buf = torch.randn((2, 104, 3, 4, 2), device="cuda", generator=gen)
    keep = buf.clone()
    out = buf[:, 16:88]
    _, names = kernels(lambda: run(conv, case, d, add=out, out=out))
    ran(names, 72)
    close64(buf[:, 16:88], d["y32"] + keep[:, 16:88], d["y64"] + keep[:, 16:88].double(), "add = out, sliced")
    assert torch.equal(buf[:, :16], keep[:, :16]) and torch.equal(buf[:, 88:], keep[:, 88:])


def test_add_in_the_kernels_store(conv):
    """No split k: bias and an aliasing `add` are summed in the tile kernel's own store."""
    case = ("conv", 8, 136, (1, 26, 26, 26), 1, 3)
    d = data(case)
    acc = torch.randn(d["y32"].shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(6))
    acc0 = acc.clone()
    _, names = kernels(lambda: run(conv, case, d, add=acc, out=acc))
    ran(names, 136)
    assert not any("k_cg_reduce" in k for k in names), names
    close64(acc, d["y32"] + acc0, d["y64"] + acc0.double(), "add = out, direct store")


@pytest.mark.parametrize("case", [("conv", 24, 136, (2, 5, 7, 6), 1, 3), ("convT", 384, 72, (2, 5, 5, 4), 2, 3)],
                         ids=["conv", "convT"])
def test_integer_operands_exact(conv, case):
    """Integer operands in [-8, 8]: x1 = x2 = 0, every product and partial sum is an exact f32, so the result
    equals float64's; a layout, tap-mask or k-order slip is a wrong integer."""
    d = data(case, integer=True)
    y, names = kernels(lambda: run(conv, case, d))
    ran(names, case[2])
    assert torch.equal(y.double(), d["y64"])


VC = ("conv", 128, 128, (1, 5, 5, 4), 1, 3)


@pytest.mark.parametrize("scale", [2.0 ** -100, 2.0 ** 60])
def test_scaled_operands(conv, scale):
    d = data(VC, scale)
    y, names = kernels(lambda: run(conv, VC, d))
    ran(names, VC[2])
    close64(y, d["y32"], d["y64"], f"scale {scale:.3e}")


def test_huge_element_stays_finite(conv):
    """One input element at 3e38 (above the largest finite bf16's neighbourhood: split3_pk clamps the leading
    part), the weight scaled by 2^-10 so that every result is finite."""
    d = data(VC)
    x = d["x"].clone()
    x[0, 77, 2, 3, 1] = 3e38
    w = d["w"] * 2.0 ** -10
    y = conv.conv_gemm(x, w, d["b"], "conv", 1, 3)
    y32, y64 = ref("conv", x, w, d["b"], 1, 3), ref("conv", x.double(), w.double(), d["b"].double(), 1, 3)
    assert torch.isfinite(y64).all() and torch.isfinite(y).all()
    close64(y, y32, y64, "3e38")


def test_infinite_element(conv):
    """One +Inf input element: every output it reaches is non-finite, every other output meets the bar."""
    d = data(VC)
    x = d["x"].clone()
    x[0, 5, 2, 2, 2] = float("inf")
    y = conv.conv_gemm(x, d["w"], d["b"], "conv", 1, 3)
    reached = ~torch.isfinite(ref("conv", x.double(), d["w"].double(), d["b"].double(), 1, 3))
    assert reached.any() and not reached.all()
    assert (~torch.isfinite(y) == reached).all()
    keep = ~reached
    close64(torch.where(keep, y, 0), torch.where(keep, d["y32"], 0), torch.where(keep, d["y64"], 0), "+Inf, the rest")


@pytest.mark.parametrize("case", [("conv", 128, 128, (1, 5, 5, 4), 1, 3), ("convT", 384, 72, (2, 5, 5, 4), 2, 3),
                                  ("conv", 8, 136, (1, 26, 26, 26), 1, 3)], ids=["conv", "convT", "direct"])
def test_two_calls_bit_equal(conv, case):
    d = data(case)
    assert torch.equal(run(conv, case, d), run(conv, case, d))
