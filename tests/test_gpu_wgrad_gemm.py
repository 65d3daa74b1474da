"""The deep-level weight gradient as an implicit GEMM (csrc/conv_wgrad_gemm.hip, tb_conv3d_wgrad_gemm_f32)
against a float64 ``aten.convolution_backward``: 3x3x3 at stride 1 and 2, 1x1x1, the ConvTranspose3d role
swap, partial tiles in both dimensions, reductions shorter than one stage, sample boundaries and stage
tails, and the six deep layers of the C3 step.  Error vs float64 within 4x max(PyTorch float32's own error,
1e-6 of the largest value) (``close64`` of tests/test_gpu_conv_gemm.py).  Also: bitwise repeatability, operands
that are channel slices of wider buffers, a forced split against the planned one, and the route."""
import copy
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def conv(gpu):
    from texbias import conv
    return conv


def close64(ours, ref32, ref64):
    scale = ref64.abs().max().item()
    e_ours = (ours.double() - ref64).abs().max().item()
    e_ref = (ref32.double() - ref64).abs().max().item()
    print(f"err ours {e_ours:.3e} torch-f32 {e_ref:.3e} scale {scale:.3e}")
    assert e_ours <= 4 * max(e_ref, 1e-6 * scale), (e_ours, e_ref, scale)


# (N, Cin, Cout, input D x H x W, stride, k, transposed)
SMALL = [
    (2, 128, 128, (3, 5, 10), 1, 3, False),  # rows of 10; 150 positions per sample: a tail stage, the sample boundary
    (2, 128, 256, (2, 3, 5), 1, 3, False),   # every position touches a border in some axis
    (1, 256, 256, (3, 3, 2), 1, 3, False),   # reduction shorter than one stage
    (2, 64, 256, (6, 6, 4), 2, 3, False),    # the stacked stride-2 form; 64-wide column tiles
    (2, 384, 64, (3, 5, 2), 2, 3, True),     # role swap (output_padding 1); M = 384
    (2, 128, 256, (3, 5, 4), 1, 1, False),   # 1x1x1
    (2, 24, 40, (5, 7, 6), 1, 3, False),     # channel counts that divide no tile
]
C3 = [
    (2, 64, 256, (30, 30, 20), 2, 3, False), (2, 128, 128, (15, 15, 10), 1, 3, False),
    (2, 128, 256, (15, 15, 10), 1, 3, False), (2, 256, 256, (15, 15, 10), 1, 3, False),
    (2, 128, 256, (15, 15, 10), 1, 1, False), (2, 384, 64, (15, 15, 10), 2, 3, True),
]


@functools.lru_cache(maxsize=None)
def _case(case):
    """G, X (the kernel's operands), the weight's shape and the float32 / float64 ATen weight gradients;
    computed once per case and shared (never modified)."""
    n, cin, cout, sp, s, k, tr = case
    torch.manual_seed(hash(case) % 1000)
    p = (k - 1) // 2
    x = torch.randn((n, cin) + sp, device="cuda")
    if tr:
        wshape = (cin, cout, k, k, k)
        gy = torch.randn((n, cout) + tuple(2 * d for d in sp), device="cuda")
    else:
        wshape = (cout, cin, k, k, k)
        gy = torch.randn((n, cout) + tuple((d + 2 * p - k) // s + 1 for d in sp), device="cuda")
    op = [1] * 3 if tr else [0] * 3

    def ref(dt):
        w = torch.zeros(wshape, device="cuda", dtype=dt)
        return torch.ops.aten.convolution_backward(gy.to(dt), x.to(dt), w, None, [s] * 3, [p] * 3, [1] * 3, tr, op, 1,
                                                   [False, True, False])[1]

    G, X = (x, gy) if tr else (gy, x)
    return G, X, wshape, ref(torch.float32), ref(torch.float64)


@pytest.mark.parametrize("case", SMALL + C3)
def test_matches_float64(conv, case):
    G, X, wshape, r32, r64 = _case(case)
    s, k, tr = case[4:]
    cfg = conv.wgrad_gemm_config(G.shape, X.shape, s, k)
    if cfg is not None:
        print("config", cfg)
        dW = conv.wgrad_gemm(G, X, wshape, s, k)
    else:  # the plan declines: the route keeps its earlier weight gradient
        x, gy = (G, X) if tr else (X, G)
        w = torch.zeros(wshape, device="cuda")
        r = conv.Route(x, w, (s,) * 3, ((k - 1) // 2,) * 3, (1, 1, 1) if tr else (0, 0, 0), tr)
        assert not r.wgg
        dW = r.weight_grad(gy, x, w)
    # every case of this file has a plan (partial tiles are masked in both dimensions)
    assert cfg is not None
    assert dW.shape == r64.shape
    close64(dW, r32, r64)


@pytest.mark.parametrize("case", [SMALL[0], SMALL[3], C3[2]])
def test_bitwise_repeatable(conv, case):
    G, X, wshape, _, _ = _case(case)
    a = conv.wgrad_gemm(G, X, wshape, case[4], case[5])
    b = conv.wgrad_gemm(G, X, wshape, case[4], case[5])
    assert torch.equal(a, b)


@pytest.mark.parametrize("case", [SMALL[0], SMALL[3], SMALL[4]])
def test_channel_slices_read_in_place(conv, case):
    """X (and G) as channel slices of wider buffers, batch stride passed: bitwise the contiguous call."""
    G, X, wshape, _, _ = _case(case)
    s, k = case[4], case[5]
    want = conv.wgrad_gemm(G, X, wshape, s, k)
    xb = torch.randn((X.shape[0], X.shape[1] + 24) + tuple(X.shape[2:]), device="cuda")
    xb[:, 8:8 + X.shape[1]] = X
    gb = torch.randn((G.shape[0], G.shape[1] + 5) + tuple(G.shape[2:]), device="cuda")
    gb[:, 5:] = G
    xs, gs = xb[:, 8:8 + X.shape[1]], gb[:, 5:]
    assert not xs.is_contiguous() and not gs.is_contiguous()
    assert conv._chan_plain(xs) is xs and conv._chan_plain(gs) is gs
    assert torch.equal(conv.wgrad_gemm(G, xs, wshape, s, k), want)
    assert torch.equal(conv.wgrad_gemm(gs, xs, wshape, s, k), want)


@pytest.mark.parametrize("case", [SMALL[0], C3[1], C3[3]])
def test_forced_single_slice_agrees(conv, case):
    """One slice per sample against the planned split (and a deliberately fine one): all within the bar."""
    G, X, wshape, r32, r64 = _case(case)
    s, k = case[4], case[5]
    n = case[0]
    assert conv.wgrad_gemm_config(G.shape, X.shape, s, k, sps=1)["nsplit"] == n
    fine = conv.wgrad_gemm_config(G.shape, X.shape, s, k, sps=7)
    assert fine["nsplit"] > n and fine["kper"] % 32 == 0
    for sps in (1, 7):
        close64(conv.wgrad_gemm(G, X, wshape, s, k, sps=sps), r32, r64)


def test_config_and_declined_shapes(conv):
    """Tiles by channel count, slices never straddling a sample, and shapes the entry refuses."""
    from texbias._lib import TexbiasError
    cfg = conv.wgrad_gemm_config((2, 256, 15, 15, 10), (2, 256, 15, 15, 10), 1, 3)
    assert (cfg["BM"], cfg["BP"]) == (128, 128) and cfg["nsplit"] % 2 == 0
    assert cfg["blocks"] == 2 * 2 * 27 * cfg["nsplit"] and cfg["blocks"] >= 256
    cfg = conv.wgrad_gemm_config((2, 384, 15, 15, 10), (2, 64, 30, 30, 20), 2, 3)
    assert (cfg["BM"], cfg["BP"]) == (128, 64)
    cfg = conv.wgrad_gemm_config((2, 40, 5, 7, 6), (2, 24, 5, 7, 6), 1, 3)
    assert (cfg["BM"], cfg["BP"]) == (64, 64)
    assert conv.wgrad_gemm_config((1, 8, 4, 4, 4), (1, 8, 4, 4, 4), 2, 1) is None       # 1x1x1 is stride 1 only
    assert conv.wgrad_gemm_config((1, 8, 4, 4, 4), (1, 8, 8, 8, 8), 3, 3) is None       # stride 3
    assert conv.wgrad_gemm_config((1, 8, 128, 128, 128), (1, 8, 128, 128, 128), 1, 3) is None  # 2^21 positions
    g = torch.randn((1, 8, 4, 4, 4), device="cuda")
    with pytest.raises(TexbiasError):
        conv.wgrad_gemm(g, g, (8, 8, 1, 1, 1), 2, 1)


def test_route_runs_the_gemm_weight_gradient(conv, monkeypatch):
    """The bottom ResidualUnit (128 -> 256, 256 -> 256, 1x1x1 residual) at a deep-level shape: with WGRAD_GEMM its
    three weight gradients run on the new entry, without it none does, and both match float64 within the bar."""
    from texbias import unet
    torch.manual_seed(11)
    base = unet.ResidualUnit(128, 256, strides=1).cuda()
    x = torch.randn((2, 128, 8, 13, 10), device="cuda")  # 1040 positions per sample: inside the gate
    calls = []
    real = conv.wgrad_gemm

    def counted(*a, **k):
        calls.append(a[2])
        return real(*a, **k)
    monkeypatch.setattr(conv, "wgrad_gemm", counted)

    def grads(mod, inp):
        y = mod(inp)
        torch.manual_seed(12)
        g = torch.randn(y.shape, device="cuda").to(y.dtype)
        (y * g).sum().backward()
        return {n: p.grad for n, p in mod.named_parameters()}

    on = copy.deepcopy(base)
    g_on = grads(on, x)
    assert sorted(tuple(c) for c in calls) == sorted([(256, 128, 3, 3, 3), (256, 256, 3, 3, 3), (256, 128, 1, 1, 1)])
    routes = [r for m in on.modules() for r in m.__dict__.get("_tb_routes", {}).values()]
    assert routes and all(r.wgg and r.fast_w for r in routes)
    del calls[:]
    monkeypatch.setattr(conv, "WGRAD_GEMM", False)
    off = copy.deepcopy(base)
    g_off = grads(off, x)
    assert not calls
    assert not any(r.wgg for m in off.modules() for r in m.__dict__.get("_tb_routes", {}).values())
    g_64 = grads(copy.deepcopy(base).double(), x.double())
    for n in g_64:
        if n.endswith("weight") and g_64[n].dim() == 5:
            close64(g_on[n], g_off[n], g_64[n])
