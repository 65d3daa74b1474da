"""ConvTranspose3d(Cin -> 32 / 64, 3, stride 2, padding 1, output_padding 1) with the eight sub-pixel classes stacked
over one gather, in split precision on the bf16 matrix cores (csrc/conv_stack.hip, k_convT_stack, behind
tb_convT3d_stack_f32 / texbias.conv.convT_stack): forward with and without bias, the stacked stride-2 Conv3d's input
gradient, `add` and `out` as tensors of their own and as channel slices of wider tensors, k split over channel
slices (k_cts_reduce) and in one slice (the store from the block), integer data bit for bit, scaled and non-finite
inputs, run-to-run bit equality, refusals and the Route's fall back.

Reference: float64 torch.nn.functional.conv_transpose3d on the CPU.  Bar: close64 of tests/test_gpu_convT_split.py
-- the error against float64 within 4 x max(ATen float32's, 1e-6 of the largest value).

Grids (Di, Hi, Wi) against the block's 64 positions: 1 x 1 x 1 (every neighbour outside the volume), 2 x 3 x 5 (30
positions: less than a tile, odd extents), 3 x 5 x 12 (180: two tiles and a partial one), 1 x 5 x 13 (65: one past
the tile), and N = 2 of 2 x 3 x 5 (the sample boundary at position 30 of tile 0).  The plan splits 384 -> 64 on
these grids over 6 channel slices and 128 -> 32 over 4; 32 -> 32 has one channel block, so one slice, and
`slices(1)` forces the one-slice store for the wider layers (the form the C3 shapes run).

Worst close64 ratio e_ours / max(e_aten, 1e-6 max|y|) measured on MI355X (bar: 4): 0.445 (profiles/r25/README.md)."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CH = [(128, 32), (256, 64), (384, 64), (32, 32)]
GRIDS = [(1, 1, 1, 1), (1, 2, 3, 5), (1, 3, 5, 12), (1, 1, 5, 13), (2, 2, 3, 5)]


@pytest.fixture(scope="module")
def conv(gpu):
    from texbias import conv
    return conv


@contextlib.contextmanager
def slices(n):
    from texbias._lib import lib
    from texbias import conv
    lib().tb_convT3d_stack_set_split(n)
    conv._cts_ws_bytes.cache_clear()
    try:
        yield
    finally:
        lib().tb_convT3d_stack_set_split(0)
        conv._cts_ws_bytes.cache_clear()


def close64(ours, ref32, ref64, what=""):
    ref64 = ref64.to(ours.device)
    scale = ref64.abs().max().item()
    e_ours = (ours.double() - ref64).abs().max().item()
    e_ref = (ref32.double() - ref64).abs().max().item()
    print(f"close64 {what}: ours {e_ours:.3e} aten {e_ref:.3e} scale {scale:.3e} "
          f"ratio {e_ours / max(e_ref, 1e-6 * scale):.3f}")
    assert e_ours <= 4 * max(e_ref, 1e-6 * scale), (e_ours, e_ref, scale)


def convT(x, w, b):
    return F.conv_transpose3d(x, w, b, stride=2, padding=1, output_padding=1)


_cache = {}


def data(ch, grid, scale=1.0, integer=False):
    """x, w, b and the forward references (ATen float32 on the GPU, float64 on the CPU), made once"""
    key = (ch, grid, scale, integer)
    if key not in _cache:
        cin, cout = ch
        N, D, H, W = grid
        gen = torch.Generator(device="cuda").manual_seed(4321 + cin + sum(grid))
        if integer:  # |sum| <= 8 taps x 384 x 4 x 2 + 4 < 2^24 and every value a bf16: exact
            x = torch.randint(-4, 5, (N, cin, D, H, W), device="cuda", generator=gen).float()
            w = torch.randint(-2, 3, (cin, cout, 3, 3, 3), device="cuda", generator=gen).float()
            b = torch.randint(-4, 5, (cout,), device="cuda", generator=gen).float()
        else:
            x = torch.randn((N, cin, D, H, W), device="cuda", generator=gen) * scale
            w = torch.randn((cin, cout, 3, 3, 3), device="cuda", generator=gen) * (1.0 / (8 * cin) ** 0.5)
            b = torch.randn(cout, device="cuda", generator=gen) * scale
        d = dict(x=x, w=w, b=b)
        d["y32"] = convT(x, w, b)
        d["y64"] = convT(x.double().cpu(), w.double().cpu(), b.double().cpu())
        _cache[key] = d
    return _cache[key]


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("ch", CH)
def test_forward_bias(conv, ch, grid):
    d = data(ch, grid)
    y = conv.convT_stack(d["x"], d["w"], d["b"])
    close64(y, d["y32"], d["y64"], f"fwd {ch} {grid}")


def test_slice_counts(conv):
    """The plan's k slices at the test shapes: at least 3 for 384 -> 64 and 128 -> 32 (the reduce kernel runs), one
    for 32 -> 32 (the block stores), and the slices cover the channel blocks exactly once."""
    for ch, lo, hi in (((384, 64), 3, 8), ((128, 32), 3, 8), ((32, 32), 1, 1)):
        for grid in GRIDS:
            cfg = conv.convT_stack_config((grid[0], ch[0]) + grid[1:], ch[1])
            assert lo <= cfg["nsplit"] <= hi, (ch, grid, cfg)
            cb = ch[0] // 32
            assert (cfg["nsplit"] - 1) * cfg["cper"] < cb <= cfg["nsplit"] * cfg["cper"], cfg
            assert cfg["positions"] == grid[0] * grid[1] * grid[2] * grid[3]
    with slices(1):
        assert conv.convT_stack_config((1, 384, 3, 5, 12), 64)["nsplit"] == 1


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("ch", CH[:3])
def test_forward_one_slice(conv, ch, grid):
    """The same through the one-slice form: the whole k loop in one block, the float2 store from the block."""
    d = data(ch, grid)
    with slices(1):
        assert conv.convT_stack_config(d["x"].shape, ch[1])["nsplit"] == 1
        y = conv.convT_stack(d["x"], d["w"], d["b"])
    close64(y, d["y32"], d["y64"], f"fwd one slice {ch} {grid}")


@pytest.mark.parametrize("ch", [(128, 32), (32, 32)])
def test_no_bias(conv, ch):
    d = data(ch, GRIDS[2])
    y = conv.convT_stack(d["x"], d["w"], None)
    b5 = d["b"].view(1, -1, 1, 1, 1)
    close64(y, d["y32"] - b5, d["y64"] - b5.double().cpu(), f"no bias {ch}")


@pytest.mark.parametrize("ch,grid", [((128, 32), (2, 2, 3, 5)), ((256, 64), (1, 3, 5, 12)), ((128, 32), (1, 1, 5, 13))])
def test_stacked_input_gradient(conv, ch, grid):
    """A stride-2 Conv3d(Cout -> Cin)'s weight [Cin, Cout, 3, 3, 3] read as that layer's: its input gradient against
    float64 autograd through conv3d."""
    cin, cout = ch
    N, D, H, W = grid
    gen = torch.Generator(device="cuda").manual_seed(55)
    gy = torch.randn((N, cin, D, H, W), device="cuda", generator=gen)
    w = torch.randn((cin, cout, 3, 3, 3), device="cuda", generator=gen) * (1.0 / (27 * cout) ** 0.5)
    x32 = torch.zeros((N, cout, 2 * D, 2 * H, 2 * W), device="cuda", requires_grad=True)
    x64 = x32.detach().double().cpu().requires_grad_(True)
    g32, = torch.autograd.grad(F.conv3d(x32, w, None, stride=2, padding=1), x32, gy)
    g64, = torch.autograd.grad(F.conv3d(x64, w.double().cpu(), None, stride=2, padding=1), x64, gy.double().cpu())
    close64(conv.convT_stack(gy, w, None), g32, g64, f"stacked dgrad {ch} {grid}")


@pytest.mark.parametrize("one_slice", [False, True])
@pytest.mark.parametrize("sliced", [False, True])
@pytest.mark.parametrize("ch,grid", [((128, 32), (2, 2, 3, 5)), ((384, 64), (1, 3, 5, 12))])
def test_add_and_out(conv, ch, grid, sliced, one_slice):
    """`add` summed in the store and `out` written in place: tensors of their own, and channel slices of wider
    tensors with distinct sample strides, whose other channels come back bit for bit unchanged."""
    d = data(ch, grid)
    cout = ch[1]
    N, D, H, W = grid
    gen = torch.Generator(device="cuda").manual_seed(78)
    wide_a = torch.randn((N, 2 * cout + 2, 2 * D, 2 * H, 2 * W), device="cuda", generator=gen)
    wide_o = torch.randn((N, 3 * cout, 2 * D, 2 * H, 2 * W), device="cuda", generator=gen)
    before = wide_o.clone()
    add = wide_a[:, 2:2 + cout] if sliced else wide_a[:, 2:2 + cout].contiguous()
    out = wide_o[:, cout:2 * cout] if sliced else torch.empty_like(d["y32"])
    with slices(1 if one_slice else 0):
        y = conv.convT_stack(d["x"], d["w"], d["b"], add=add, out=out)
        y2 = conv.convT_stack(d["x"], d["w"], d["b"], add=add)
    assert y.data_ptr() == out.data_ptr()
    close64(y, d["y32"] + add, d["y64"] + add.double().cpu(), f"add/out {ch} {grid} sliced={sliced}")
    assert torch.equal(y2, y)
    assert torch.equal(wide_o[:, :cout], before[:, :cout]) and torch.equal(wide_o[:, 2 * cout:], before[:, 2 * cout:])
    if not sliced:
        assert torch.equal(wide_o, before)


@pytest.mark.parametrize("one_slice", [False, True])
@pytest.mark.parametrize("ch,grid", [(ch, GRIDS[2]) for ch in CH] + [((128, 32), g) for g in GRIDS] +
                         [((384, 64), GRIDS[4])])
def test_integer_data_exact(conv, ch, grid, one_slice):
    """Integer x, w and bias, exact in bf16 and in every f32 sum: the result equals float64 bit for bit, so no tap,
    class, offset, channel block, slice or accumulator row is misplaced."""
    d = data(ch, grid, integer=True)
    with slices(1 if one_slice else 0):
        y = conv.convT_stack(d["x"], d["w"], d["b"])
    assert torch.equal(y.double().cpu(), d["y64"])


@pytest.mark.parametrize("scale", [2.0 ** -100, 2.0 ** 60])
@pytest.mark.parametrize("ch", [(128, 32), (384, 64)])
def test_scaled_inputs(conv, ch, scale):
    d = data(ch, GRIDS[2], scale)
    y = conv.convT_stack(d["x"], d["w"], d["b"])
    close64(y, d["y32"], d["y64"], f"{ch} scale {scale:.3e}")


@pytest.mark.parametrize("one_slice", [False, True])
def test_one_inf_input(conv, one_slice):
    """One +Inf input element: non-finite exactly where float64 is."""
    d = data((128, 32), GRIDS[2])
    x = d["x"].clone()
    x[0, 37, 1, 2, 7] = float("inf")
    with slices(1 if one_slice else 0):
        y = conv.convT_stack(x, d["w"], d["b"])
    y64 = convT(x.double().cpu(), d["w"].double().cpu(), d["b"].double().cpu())
    assert torch.equal(~torch.isfinite(y).cpu(), ~torch.isfinite(y64))
    assert (~torch.isfinite(y64)).sum().item() > 0
    fin = torch.isfinite(y64)
    close64(torch.where(fin.cuda(), y, torch.zeros_like(y)), torch.where(fin.cuda(), d["y32"], torch.zeros_like(y)),
            torch.where(fin, d["y64"], torch.zeros_like(y64)), "finite part")


def test_two_calls_bit_equal(conv):
    """No atomics, a fixed order of operations: two calls agree bit for bit, split and in one slice, with `add`."""
    for ch, grid in (((384, 64), GRIDS[2]), ((128, 32), GRIDS[4])):
        d = data(ch, grid)
        for n in (0, 1):
            with slices(n):
                a, b = conv.convT_stack(d["x"], d["w"], d["b"]), conv.convT_stack(d["x"], d["w"], d["b"])
                assert torch.equal(a, b)
                a = conv.convT_stack(d["x"], d["w"], d["b"], add=d["y32"])
                b = conv.convT_stack(d["x"], d["w"], d["b"], add=d["y32"])
                assert torch.equal(a, b)


@pytest.mark.parametrize("cin,cout", [(64, 16), (40, 32), (128, 48)])
def test_refused_channels(conv, cin, cout):
    """Cout outside {32, 64} and Cin no multiple of 32: TB_ERR_UNSUPPORTED_SIZE, no plan, and the output untouched."""
    from texbias._abi import TB_ERR_UNSUPPORTED_SIZE
    x = torch.randn((1, cin, 2, 3, 4), device="cuda")
    w = torch.randn((cin, cout, 3, 3, 3), device="cuda")
    out = torch.full((1, cout, 4, 6, 8), 7.0, device="cuda")
    rc, _ = conv.convT_stack_rc(x, w, None, out=out)
    torch.cuda.synchronize()
    assert rc == TB_ERR_UNSUPPORTED_SIZE and bool((out == 7.0).all())
    assert conv.convT_stack_config(x.shape, cout) is None


def test_route_and_fall_back(conv, monkeypatch):
    """Through Route: with the gates open the transposed forward and the stride-2 unit's input gradient take
    ``convTs`` and agree with ATen; refused shapes (Cout 16, Cin 40, odd extents of a stride-2 input gradient) and
    the switch off keep the earlier route."""
    monkeypatch.setattr(conv, "CONVT_STACK_FWD_MIN_POS", {(128, 32): 1, (64, 16): 1, (40, 32): 1})
    monkeypatch.setattr(conv, "CONVT_STACK_DX_MIN_POS", {(128, 32): 1, (128, 16): 1})
    torch.manual_seed(3)

    def up(cin, cout, sp):
        m = conv.ConvTranspose3d(cin, cout, 3, stride=2, padding=1, output_padding=1).cuda()
        x = torch.randn((1, cin) + sp, device="cuda")
        return m, x, conv.Route(x, m.weight, m.stride, m.padding, m.output_padding, True)

    m, x, r = up(128, 32, (2, 3, 5))
    assert (r.kind, r.dx) == ("convTs", "aten")
    y = m(x)
    yr = convT(x, m.weight, m.bias)
    assert (y - yr).abs().max().item() <= 2e-5 * yr.abs().max().item()
    assert up(64, 16, (2, 3, 5))[2].kind != "convTs" and up(40, 32, (2, 3, 5))[2].kind != "convTs"

    def down(cin, cout, sp):
        m = conv.Conv3d(cin, cout, 3, stride=2, padding=1).cuda()
        x = torch.randn((1, cin) + sp, device="cuda", requires_grad=True)
        return m, x, conv.Route(x, m.weight, m.stride, m.padding, (0, 0, 0), False)

    m, x, r = down(32, 128, (4, 6, 10))
    assert r.dx == "convTs"
    y = m(x)
    g = torch.randn_like(y)
    gx, = torch.autograd.grad(y, (x,), g)
    xr = x.detach().clone().requires_grad_(True)
    gr, = torch.autograd.grad(F.conv3d(xr, m.weight, m.bias, stride=2, padding=1), xr, g)
    assert (gx - gr).abs().max().item() <= 2e-5 * gr.abs().max().item()
    assert down(32, 128, (4, 5, 10))[2].dx != "convTs"      # odd extent
    assert down(16, 128, (4, 6, 16))[2].dx != "convTs"      # Cout 16
    monkeypatch.setattr(conv, "CONVT_STACK", False)
    assert up(128, 32, (2, 3, 5))[2].kind == "aten" and down(32, 128, (4, 6, 10))[2].dx == "aten"
