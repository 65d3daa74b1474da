"""The fused U-Net units of ``texbias.unet`` (_StackedUnitFn, _ConvADNFn, _ConvResFn, _SkipCatFn) against a
float64 restatement (tests/_unet_ref.py) at the smallest shapes that take each ``conv.Route`` kind.

Every case makes three runs with the same weights, input and upstream gradient: ours (float32, every switch at
its default; the fused function must have run), aten32 (a deepcopy with ``conv.ENABLED = norm.ENABLED = False``:
MIOpen / ATen) and ref64 (the restatement in float64 on the GPU).  Bars, all against ref64:
* tensors (output, input gradient, 5-D weight gradients, residual conv bias, the top bare conv's bias): the
  ``close64`` rule of tests/test_gpu_conv_up.py, e_ours <= 4 max(e_aten32, 1e-6 max|ref64|);
* scalar PReLU weight gradients, against their conditioning: |g - g64| / sum_{n <= 0} |n dy| within
  10 max(ATen's, 1e-6) (the rule of test_train_step_full_volume_matches_aten);
* biases of convs ahead of an ADN (true value 0): |db - db64| / sum |dz64| within 10 max(ATen's, 1e-6), and
  the tensor is returned, not None.
Each case prints its ratios e_ours / max(e_aten32, floor) per tensor before it asserts, and one "WORST" line.

Worst measured ratios on an MI355X (tensor rule, bar 4 / scalar rule, bar 10 / zero-bias rule, bar 10); no floor
was raised:
* strided units: 0.72 (case A packed, the output) / 0.015 (A, unit 1's PReLU weight) / 0.001 (A2, unit 1's bias);
* up blocks: 0.64 (F1, the output) / 0.011 (F2, the ConvTranspose3d's PReLU weight) / below 0.001;
* mini U-Nets: 0.79 (16 x 16 x 32, the bottom unit's conv1 weight) / 0.030 (8 x 12 x 20) / below 0.001.
The tensor ratios moved by about 0.05 between two runs (case A's output: 0.56 and 0.51).
"""
import copy

import pytest
import torch
import torch.nn as nn

import _unet_ref as R

pytestmark = pytest.mark.gpu

# name: (cin, c, x shape, stacked conv (kind, dx), conv1 (kind, dx), wgg) -- the route kinds follow from the
# gates of texbias.conv at these shapes; None = not asserted
STRIDED = {
    "A": (4, 16, (2, 4, 8, 12, 32), ("fewin", "aten"), ("fwd16", "fwd16"), None),
    "A2": (4, 16, (1, 4, 6, 10, 20), ("fewin", "aten"), ("gemm", "gemm"), None),        # halved W = 10
    "A3": (4, 16, (1, 4, 7, 9, 10), ("aten", "aten"), ("gemm", "gemm"), None),          # odd extents
    "B": (16, 32, (2, 16, 8, 12, 16), ("gemm", "convT64"), ("mfma", "mfma"), None),     # stacked weight 64 x 16
    "B2": (16, 32, (1, 16, 6, 6, 12), ("gemm", "aten"), ("gemm", "gemm"), None),        # W % 8 != 0; halved W = 6
    "C": (32, 64, (2, 32, 6, 8, 8), ("gemm", "aten"), ("mfma", "mfma"), None),
    "D": (64, 128, (1, 64, 4, 6, 8), ("gemm", "aten"), ("gemm", "gemm"), None),
    "D2": (64, 128, (1, 64, 16, 24, 24), None, None, True),   # 1152 output positions: the WGRAD_GEMM_* gate
}

# name: (cin, c, top, x shape, ConvTranspose3d (kind, dx), unit conv (kind, dx))
UP = {
    "F1": (64, 16, False, (2, 64, 4, 6, 8), ("convT64", "gemm"), ("fwd16", "fwd16")),   # add in the store
    "F5": (64, 16, False, (1, 64, 3, 5, 5), ("aten", "aten"), ("gemm", "gemm")),        # add= of the dgrad form
    "F2": (128, 32, False, (1, 128, 3, 4, 4), ("aten", "aten"), ("mfma", "mfma")),      # generic add
    "F3": (384, 64, False, (1, 384, 2, 3, 4), ("aten", "aten"), ("mfma", "mfma")),
    # bias gradient from the weight-gradient sweep; output S = 34560: two full ADN chunks and a ragged one
    "F4": (32, 3, True, (1, 32, 10, 12, 36), ("fewout", "fewout"), ("small", "small")),
}

FWD_KINDS = {"fewin", "fwd16", "mfma", "small", "fewout", "convT64", "gemm", "aten"}
DX_KINDS = {"fwd16", "mfma", "small", "fewout", "convT64", "gemm", "aten"}


def _init(m, seed):
    """Default conv initialisation; PReLU slopes from [-0.3, 0.4], so that none is the init value 0.25."""
    torch.manual_seed(seed)
    m = m.cuda()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("A.weight"):
                p.uniform_(-0.3, 0.4)
    return m


def _strided(name, seed=0):
    from texbias import unet
    cin, c = STRIDED[name][:2]
    return _init(unet.ResidualUnit(cin, c, 2), seed)


def _up(name, seed=0):
    from texbias import unet
    cin, c, top = UP[name][:3]
    return _init(nn.Sequential(unet.Convolution(cin, c, 2, is_transposed=True),
                               unet.ResidualUnit(c, c, 1, subunits=1, last_conv_only=top)), seed)


def _one_route(mod):
    routes = list(mod.__dict__.get("_tb_routes", {}).values())
    assert len(routes) == 1, (type(mod).__name__, len(routes))
    return routes[0]


def _strided_routes(m):
    return _one_route(m), _one_route(m.conv.unit1.conv)


def _up_routes(m):
    return _one_route(m[0].conv), _one_route(m[1].conv.unit0.conv)


def _three_runs(m, ref_fn, shape, monkeypatch, frozen=(), freeze_x=False, before_ours=None):
    """ours / aten32 / ref64 with the same weights, input and upstream gradient.  Returns
    (y, ours, a32, r64, inter, names): dicts name -> tensor with "output" and "input" beside the parameter
    names; frozen entries of ``ours`` are None."""
    from texbias import conv, norm
    aten = copy.deepcopy(m)            # before any forward: no cached routes, no packed storage
    if before_ours is not None:
        before_ours(m)
    for n, p in m.named_parameters():
        p.requires_grad_(n not in frozen)
    x0 = torch.randn(shape, device="cuda") * 1.5 + 0.3
    x = x0.clone().requires_grad_(not freeze_x)
    y = m(x)
    g = torch.randn_like(y)
    y.backward(g)
    ours = {"output": y.detach(), "input": x.grad}
    ours.update({n: p.grad for n, p in m.named_parameters()})
    with monkeypatch.context() as mp:
        mp.setattr(conv, "ENABLED", False)
        mp.setattr(norm, "ENABLED", False)
        xa = x0.clone().requires_grad_(True)
        ya = aten(xa)
        ya.backward(g)
    a32 = {"output": ya.detach(), "input": xa.grad}
    a32.update({n: p.grad for n, p in aten.named_parameters()})
    sd = {n: p.detach().double().requires_grad_(True) for n, p in m.named_parameters()}
    x64 = x0.double().requires_grad_(True)
    y64, inter = ref_fn(sd, x64)
    y64.backward(g.double())
    r64 = {"output": y64.detach(), "input": x64.grad}
    r64.update({n: p.grad for n, p in sd.items()})
    return y, ours, a32, r64, inter, [n for n, _ in m.named_parameters()]


def _judge(label, kind, ours, a32, r64, inter, names, skip=()):
    """Print every ratio, then assert the three bars; ``skip``: names left out (frozen in ``ours``)."""
    scalars, zero_b, tensors = R.split_params(names, inter)
    bad, worst = [], {"tensor": (0.0, ""), "scalar": (0.0, ""), "zero_bias": (0.0, "")}

    def note(cls, n, e_o, e_a, floor, bar, extra=""):
        ratio = e_o / max(e_a, floor)
        print(f"  {label} {cls:9s} {n}: ours {e_o:.3e} aten32 {e_a:.3e} floor {floor:.3e} ratio {ratio:.3f}{extra}")
        if ratio > worst[cls][0]:
            worst[cls] = (ratio, n)
        if not ratio <= bar:        # (also catches nan)
            bad.append((cls, n, e_o, e_a, floor))

    for n in ["output", "input"] + names:
        if n in skip:
            continue
        assert ours[n] is not None, f"{label}: {n} has no gradient"
        assert a32[n] is not None and r64[n] is not None, n
        assert ours[n].shape == r64[n].shape, n
        o, a, r = ours[n].double(), a32[n].double(), r64[n]
        if n in scalars:
            cond = R.prelu_cond(inter[scalars[n]])
            assert cond > 0, n
            note("scalar", n, (o - r).abs().item() / cond, (a - r).abs().item() / cond, 1e-6, 10.0,
                 f" (|g64| {r.abs().item():.3e} cond {cond:.3e})")
        elif n in zero_b:
            cond = R.bias_cond(inter[zero_b[n]])
            assert cond > 0, n
            note("zero_bias", n, (o - r).abs().max().item() / cond, (a - r).abs().max().item() / cond, 1e-6, 10.0)
        else:
            scale = r.abs().max().item()
            assert scale > 0, n
            note("tensor", n, (o - r).abs().max().item(), (a - r).abs().max().item(), 1e-6 * scale, 4.0,
                 f" (scale {scale:.3e})")
    print(f"WORST {kind} {label}: " + " ".join(f"{c}={v[0]:.3f}[{v[1]}]" for c, v in worst.items()))
    assert not bad, (label, bad)


# ------------------------------------------------------------------ strided units: _StackedUnitFn
def _check_strided_routes(name, m):
    _, _, _, st, c1, wgg = STRIDED[name]
    r_st, r1 = _strided_routes(m)
    got = ((r_st.kind, r_st.dx), (r1.kind, r1.dx), (r_st.wgg, r1.wgg))
    print(f"  {name} routes: stacked {got[0]} conv1 {got[1]} wgg {got[2]}")
    if st is not None:
        assert got[0] == st and got[1] == c1, (name, got)
    if wgg is not None:
        assert got[2] == (wgg, wgg), (name, got)


@pytest.mark.parametrize("name,packed", [(n, False) for n in STRIDED] + [("A", True)])
def test_strided_unit(gpu, heartbeat, monkeypatch, name, packed):
    """ResidualUnit(cin, c, 2) as one stacked convolution: output and every gradient against float64."""
    m = _strided(name, seed=10)
    shape = STRIDED[name][2]

    def pack(mod):
        assert mod.pack_parameters()

    y, ours, a32, r64, inter, names = _three_runs(m, lambda sd, x: R.residual_unit(sd, "", x, 2), shape,
                                                  monkeypatch, before_ours=pack if packed else None)
    assert "StackedUnitFn" in type(y.grad_fn).__name__
    _check_strided_routes(name, m)
    _judge(name + ("-packed" if packed else ""), "strided", ours, a32, r64, inter, names)


def test_strided_unit_partial_needs_input_grad(gpu, heartbeat, monkeypatch):
    """Case B with unit 0's conv weight, unit 0's PReLU weight and the input frozen: the remaining gradients
    meet the same bars and the frozen ones stay None."""
    frozen = ("conv.unit0.conv.weight", "conv.unit0.adn.A.weight")
    m = _strided("B", seed=11)
    y, ours, a32, r64, inter, names = _three_runs(m, lambda sd, x: R.residual_unit(sd, "", x, 2), STRIDED["B"][2],
                                                  monkeypatch, frozen=frozen, freeze_x=True)
    assert "StackedUnitFn" in type(y.grad_fn).__name__
    for n in frozen + ("input",):
        assert ours[n] is None, n
    _judge("B-partial", "strided", ours, a32, r64, inter, names, skip=frozen + ("input",))


# ------------------------------------------------------------------ up blocks: _ConvADNFn (x 2) / _ConvResFn
def _check_up_routes(name, m):
    _, _, _, _, ct, uc = UP[name]
    rt, ru = _up_routes(m)
    got = ((rt.kind, rt.dx), (ru.kind, ru.dx))
    print(f"  {name} routes: convT {got[0]} unit conv {got[1]}")
    assert got == (ct, uc), (name, got)


@pytest.mark.parametrize("name", list(UP))
def test_up_block(gpu, heartbeat, monkeypatch, name):
    """ConvTranspose3d -> ADN -> identity-residual unit: output and every gradient against float64."""
    m = _up(name, seed=20)
    top, shape = UP[name][2], UP[name][3]
    y, ours, a32, r64, inter, names = _three_runs(m, lambda sd, x: R.up_block(sd, "", x, top), shape, monkeypatch)
    assert ("ConvResFn" if top else "ConvADNFn") in type(y.grad_fn).__name__
    _check_up_routes(name, m)
    _judge(name, "up", ours, a32, r64, inter, names)


def test_up_block_only_prelu_weights(gpu, heartbeat, monkeypatch):
    """Case F1 with only the PReLU weights requiring a gradient."""
    m = _up("F1", seed=21)
    frozen = tuple(n for n, _ in m.named_parameters() if not n.endswith("A.weight"))
    y, ours, a32, r64, inter, names = _three_runs(m, lambda sd, x: R.up_block(sd, "", x, False), UP["F1"][3],
                                                  monkeypatch, frozen=frozen, freeze_x=True)
    assert "ConvADNFn" in type(y.grad_fn).__name__
    for n in frozen + ("input",):
        assert ours[n] is None, n
    assert len(names) - len(frozen) == 2
    _judge("F1-prelu-only", "up", ours, a32, r64, inter, names, skip=frozen + ("input",))


# ------------------------------------------------------------------ route coverage
def test_route_union(gpu):
    """The cases above take every forward and every input-gradient kind a unit can be built from."""
    fwd, dx = set(), set()
    x_of = lambda shape: torch.randn(shape, device="cuda")  # noqa: E731
    with torch.no_grad():
        for name in STRIDED:
            m = _strided(name)
            m(x_of(STRIDED[name][2]))
            _check_strided_routes(name, m)
            for r in _strided_routes(m):
                fwd.add(r.kind), dx.add(r.dx)
        for name in UP:
            m = _up(name)
            m(x_of(UP[name][3]))
            _check_up_routes(name, m)
            for r in _up_routes(m):
                fwd.add(r.kind), dx.add(r.dx)
    assert fwd >= FWD_KINDS and dx >= DX_KINDS, (sorted(fwd), sorted(dx))


# ------------------------------------------------------------------ mini U-Nets: _SkipCatFn and every unit together
@pytest.mark.parametrize("shape", [(2, 4, 16, 16, 32), (2, 4, 8, 12, 20)])
def test_mini_unet(gpu, heartbeat, monkeypatch, shape):
    """UNet(3, 4, 3, (16, 32, 64), (2, 2)): the skip hand-over, the in-place concatenation buffer and every
    unit together; output, input gradient and every parameter gradient against float64."""
    from texbias import unet
    m = _init(unet.UNet(3, 4, 3, (16, 32, 64), (2, 2)), seed=30)
    down, skip = m.model[0], m.model[1]
    assert skip._tail_unit() is not None
    seen = {}   # the first forward's tensors: ours (the aten32 deepcopy carries the hooks along)

    def keep(key):
        def hook(mod, inputs, out):
            seen.setdefault(key, out)
        return hook

    hooks = [down.register_forward_hook(keep("down")), skip.submodule.register_forward_hook(keep("sub")),
             skip.register_forward_hook(keep("cat"))]
    y, ours, a32, r64, inter, names = _three_runs(m, lambda sd, x: R.unet(sd, "model", x, 2), shape, monkeypatch)
    for h in hooks:
        h.remove()
    d, s, cat = seen["down"], seen["sub"], seen["cat"]
    assert "StackedUnitFn" in type(d.grad_fn).__name__ and isinstance(getattr(d, "_tb_skip", None), dict)
    assert not d._tb_skip, "the hand-over dict is emptied by the unit's backward"
    assert "SkipCatFn" in type(cat.grad_fn).__name__
    # the submodule's output already sits in the upper channels of the concatenation
    assert s.data_ptr() == cat.data_ptr() + d.shape[1] * cat.stride(1) * cat.element_size()
    assert torch.equal(cat[:, :d.shape[1]], d) and torch.equal(cat[:, d.shape[1]:], s)
    assert "ConvResFn" in type(y.grad_fn).__name__
    with torch.no_grad():
        x = torch.randn(shape, device="cuda") * 1.5 + 0.3
        y0 = m(x)
    assert torch.equal(y0, m(x))
    _judge(f"unet-{'x'.join(map(str, shape[2:]))}", "unet", ours, a32, r64, inter, names)
