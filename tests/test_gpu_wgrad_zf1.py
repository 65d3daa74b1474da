"""The few-channel stride-1 weight gradient (k_conv3d_wgrad_zf1: 16-byte operand reads, 16-column k groups)
and the bias gradient summed out of the same sweep (tb_conv3d_wgrad_bias_ws_f32), through the entry points the
U-Net's backward uses (texbias.conv.wgrad_bias / wgrad), against float64 references on small shapes."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

# (M, Cc), (N, D, H, W): one k group per row; W just above 128 (WV 40); the C3 row length with odd H (a row
# block past H); a wide row (WV 64); a k count that is no multiple of the 2x unrolled group loop with M < 3 and
# Cc = 5 (absent MFMA rows and columns); a single channel pair; and z segments of unequal length: with YB = 2
# rows per block N nyb = 2 * 20 = 40 row blocks, and on 256 CUs (512 resident blocks) the planner's cost
# ceil(40 ZS / 512) (zlen + 2) is least at zlen = 3 -- ZS = 10 segments of 3, ..., 3, 1 planes for D = 28.
SHAPES = [((3, 3), (2, 5, 6, 8)), ((3, 3), (1, 7, 5, 132)), ((3, 3), (1, 6, 7, 160)), ((3, 3), (1, 4, 3, 240)),
          ((2, 5), (2, 9, 4, 20)), ((1, 1), (1, 3, 2, 4)), ((3, 3), (2, 28, 40, 8))]
IDS = ["one-group", "w132", "w160-oddH", "w240", "m2c5-w20", "single", "uneven-z"]


@pytest.fixture(scope="module")
def conv(gpu):
    from texbias import conv as C
    return C


def test_uneven_z_plan(conv):
    """The plan the "uneven-z" shape relies on (SHAPES' comment), from the planner itself."""
    (M, Cc), (N, D, H, W) = SHAPES[IDS.index("uneven-z")]
    p = conv.wgrad_plan((N, M, D, H, W), (N, Cc, D, H, W), 1)
    assert (p["kind"], p["YB"], p["zlen"], p["ZS"]) == (3, 2, 3, 10) and D % p["zlen"] == 1


@pytest.fixture(scope="module")
def cases(conv):
    """Per shape, computed once: inputs, two calls of wgrad_bias, and the float64 / ATen float32 references."""
    out = {}
    for (M, Cc), (N, D, H, W) in SHAPES:
        torch.manual_seed(7)
        x = torch.randn((N, Cc, D, H, W), device="cuda")
        g = torch.randn((N, M, D, H, W), device="cuda") + 0.25
        wsh = (M, Cc, 3, 3, 3)
        first = conv.wgrad_bias(g, x, wsh, 1, 1)
        second = conv.wgrad_bias(g, x, wsh, 1, 1)
        w = torch.zeros(wsh, device="cuda", requires_grad=True)
        ref, = torch.autograd.grad(torch.nn.functional.conv3d(x, w, padding=1), w, g)
        w64 = torch.zeros(wsh, device="cuda", dtype=torch.float64, requires_grad=True)
        r64, = torch.autograd.grad(torch.nn.functional.conv3d(x.double(), w64, padding=1), w64, g.double())
        out[((M, Cc), (N, D, H, W))] = dict(x=x, g=g, first=first, second=second, ref=ref, r64=r64,
                                            b64=g.double().sum(dim=(0, 2, 3, 4)))
    torch.cuda.synchronize()
    return out


def _meets_f64_bar(ours, ref, r64):
    """tests/test_gpu_conv.py's bar: max |ours - r64| <= 4 max(max |ATen f32 - r64|, 1e-6 scale)."""
    scale = r64.abs().max().item()
    e, er = (ours.double() - r64).abs().max().item(), (ref.double() - r64).abs().max().item()
    print(f"max|ours - r64| {e:.3e}  max|ATen - r64| {er:.3e}  scale {scale:.3e}")
    return e <= 4 * max(er, 1e-6 * scale)


def _bias_close(a, b64, voxels):
    """tests/test_gpu_norm.py's channel_sum bar: rtol 1e-6, atol 1e-6 sqrt(voxels per channel)."""
    print(f"max|gb - f64| {(a.double() - b64).abs().max().item():.3e}  atol {1e-6 * math.sqrt(voxels):.3e}")
    torch.testing.assert_close(a.double(), b64, rtol=1e-6, atol=1e-6 * math.sqrt(voxels))


@pytest.mark.parametrize("key", SHAPES, ids=IDS)
def test_dw_against_float64(cases, key):
    c = cases[key]
    assert _meets_f64_bar(c["first"][0], c["ref"], c["r64"])


@pytest.mark.parametrize("key", SHAPES, ids=IDS)
def test_dw_and_bias_repeat_bitwise(cases, key):
    c = cases[key]
    assert torch.equal(c["first"][0], c["second"][0])
    assert c["first"][1] is not None and torch.equal(c["first"][1], c["second"][1])


@pytest.mark.parametrize("key", SHAPES, ids=IDS)
def test_bias_sum_against_float64(conv, cases, key):
    c = cases[key]
    gb = c["first"][1]
    assert gb is not None, "the zf1 route sums the bias"
    vox = c["g"][:, 0].numel()
    _bias_close(gb, c["b64"], vox)
    # the fallback a None result leads to (channel_sum) gives the same sum within the same bar
    _bias_close(gb, conv.channel_sum(c["g"]).double(), vox)


@pytest.mark.parametrize("key", SHAPES, ids=IDS)
def test_plain_ws_entry_matches(conv, cases, key):
    """tb_conv3d_wgrad_ws_f32 (no bias output) runs the same kernel: the same bits."""
    (M, Cc), _ = key
    c = cases[key]
    assert torch.equal(conv.wgrad(c["g"], c["x"], (M, Cc, 3, 3, 3), 1, 1), c["first"][0])


def test_bias_not_done_reports_zero(cases):
    """Without room for the partials (the plain workspace size) dW is still produced and *bias_done is 0; a
    route that does not sum the bias says so in the size query."""
    import ctypes
    from texbias._lib import lib
    key = SHAPES[0]
    (M, Cc), (N, D, H, W) = key
    c = cases[key]
    dims = (N, M, Cc, D, H, W, D, H, W, 1, 1)
    sums = ctypes.c_int(-1)
    nb_bias = int(lib().tb_conv3d_wgrad_bias_ws_bytes(*dims, ctypes.byref(sums)))
    nb = int(lib().tb_conv3d_wgrad_ws_bytes(*dims))
    assert sums.value == 1 and nb_bias >= nb + 8 * M
    st = torch.cuda.current_stream().cuda_stream
    ws = torch.empty(nb_bias, dtype=torch.uint8, device="cuda")
    dW = torch.empty((M, Cc, 27), device="cuda")
    gb = torch.full((M,), 123.0, device="cuda")
    done = ctypes.c_int(-1)
    assert lib().tb_conv3d_wgrad_bias_ws_f32(c["g"].data_ptr(), c["x"].data_ptr(), dW.data_ptr(), gb.data_ptr(), *dims,
                                             ws.data_ptr(), nb, ctypes.byref(done), st) == 0
    torch.cuda.synchronize()
    assert done.value == 0 and torch.equal(gb, torch.full_like(gb, 123.0))
    assert torch.equal(dW.view(M, Cc, 3, 3, 3), c["first"][0])
    dims16 = (1, 16, 16, 6, 6, 16, 6, 6, 16, 1, 1)   # the 16-channel z-march: no bias sum
    assert int(lib().tb_conv3d_wgrad_bias_ws_bytes(*dims16, ctypes.byref(sums))) == \
        int(lib().tb_conv3d_wgrad_ws_bytes(*dims16)) and sums.value == 0


def test_atomic_entry_still_meets_bar(cases):
    """tb_conv3d_wgrad_f32 (float atomics, no workspace) on the same kernel."""
    from texbias._lib import lib
    key = SHAPES[4]
    (M, Cc), (N, D, H, W) = key
    c = cases[key]
    dW = torch.empty((M, Cc, 3, 3, 3), device="cuda")
    assert lib().tb_conv3d_wgrad_f32(c["g"].data_ptr(), c["x"].data_ptr(), dW.data_ptr(), N, M, Cc, D, H, W, D, H, W, 1, 1,
                                     torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert _meets_f64_bar(dW, c["ref"], c["r64"])


def test_conv_res_unit_round_trip(conv, monkeypatch):
    """y = conv(x) + x (the top ResidualUnit(3, 3, conv_only)) at 2 x 3 x 8 x 6 x 8: gw, gb, gx against the float64
    model, with the bias gradient out of the weight-gradient sweep (channel_sum is not called)."""
    from texbias import unet as U
    calls = []
    real = conv.channel_sum
    monkeypatch.setattr(conv, "channel_sum", lambda g: (calls.append(1), real(g))[1])
    torch.manual_seed(11)
    mod = conv.Conv3d(3, 3, 3, padding=1).cuda()
    x = torch.randn((2, 3, 8, 6, 8), device="cuda", requires_grad=True)
    y = U._ConvResFn.apply(x, mod.weight, mod.bias, conv.route_of(mod, x))
    g = torch.randn_like(y) + 0.25
    gx, gw, gb = torch.autograd.grad(y, (x, mod.weight, mod.bias), g)
    assert not calls

    def model(dtype):
        xx = x.detach().to(dtype).requires_grad_(True)
        w, b = mod.weight.detach().to(dtype).requires_grad_(True), mod.bias.detach().to(dtype).requires_grad_(True)
        yy = torch.nn.functional.conv3d(xx, w, b, padding=1) + xx
        return torch.autograd.grad(yy, (xx, w, b), g.to(dtype))

    (rx, rw, rb), (r64x, r64w, r64b) = model(torch.float32), model(torch.float64)
    assert _meets_f64_bar(gw, rw, r64w)
    assert _meets_f64_bar(gx, rx, r64x)
    _bias_close(gb, r64b, g[:, 0].numel())
