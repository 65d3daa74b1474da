"""The trainable spike layer on the GPU: k_spike_delta / k_spike_gamma / k_spike_dI_sum around the closed-form
route's k_point_dft and k_point_apply, the custom ops (autograd, opcheck, torch.compile, HIP-graph capture with a
live intensity), LearnedSpikeLayer under TrainStep, and the C ABI's argument checks.

Semantics (restated in tests/_spikes_ref.py, checked there against autograd of the reference's expression):
  y = x + Re(sum_j (A_j u - K_j) e^{i theta_j}) / N,  dI_j = sum_bc A_j p / N,
  gx = g + Re(sum_j u (-p + i q (A_j / m - 1)) e^{i theta_j}) / N,  p + i q = conj(u) G_j.
Bars: <= 2e-6 of max|y| against the host program of the same spikes on the closed-form route (the project's bar
between routes; not bit equality: the device forms exp(I) itself); <= 1e-5 of the largest value against float64 for
y and gx; dI against its conditioning, |dI - dI64| <= 1e-5 sum_bc A_j |G_j| / N (the sum over volume-channels
cancels, as DESIGN treats the PReLU scalars); dI against sum g (y(I + ln 2) - y(I)) from two forward calls, the
same bar plus the float32 rounding of the two outputs, 4 2^-24 sum|g| max|y| (derived, not measured).
Largest |dI - dI64| / (sum_bc A_j |G_j| / N) seen on an MI355X: 1.7e-07 (bar 1e-5).

Spectrum of y: the reference writes K(f_j) alone and takes ``.real``, which halves the change of a coefficient
whose conjugate partner it left untouched, FFT(y)(f_j) = (A_j u + K_j) / 2; |FFT(y)(f_j)| = A_j holds only at a
self-conjugate f_j (DC, Nyquist).  The check is made on the coefficient the layer set, c_j = 2 FFT(y)(f_j) -
FFT(x)(f_j) (FFT(y)(f_j) itself at a self-conjugate f_j): |c_j| = exp(I_j) to 1e-5 relative, phase that of
FFT(x)(f_j).  The issue sets no bar for the phase; the one used is derived, not measured: both float32 spectra are
good to 1e-5 of their largest coefficient (the project's bar against float64), c_j's is A_j itself and FFT(x)'s is
max|K|, so the two unit phasors may differ by 1e-5 (1 + max|K| / |K(f_j)|), with the float64 |K| in it.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import _spikes_ref as R

pytestmark = pytest.mark.gpu

TOL, TOL_ROUTE = 1e-5, 2e-6
LN2 = math.log(2.0)


@pytest.fixture(scope="module")
def rt(gpu):
    from texbias import ops  # noqa: F401  (registers torch.ops.texbias.*)
    from texbias import runtime
    return runtime


# (image shape, transformed axes, channels, pad)
SHAPES = {
    "odd_d_pad": ((2, 3, 24, 20, 15), 3, 3, 5),          # odd D, partial last quads, a padded output
    "odd_hw": ((1, 2, 31, 17, 30), 3, 2, 0),
    "lead_singleton": ((2, 1, 1, 16, 12, 10), 4, 1, 0),  # the reference's call of the layer: (1, H, W, D) transformed
    "two_groups": ((9, 1, 8, 8, 8), 3, 1, 0),            # more than TB_MAX_BATCH samples
}
KINDS = ["dc", "nyquist", "kd0", "generic", "three"]


def _locs(spatial, kind):
    nd = len(spatial)
    generic = tuple(0 if n == 1 else min(n - 1, n // 2 + 2 + a) for a, n in enumerate(spatial))
    kd0 = tuple(0 if n == 1 else (n // 2 if a == nd - 1 else (1 if a == nd - 3 else n - 1))
                for a, n in enumerate(spatial))
    one = {"dc": R.centre(spatial), "nyquist": R.nyquist(spatial), "kd0": kd0, "generic": generic}
    return [one["generic"], one["nyquist"], one["kd0"]] if kind == "three" else [one[kind]]


_cache = {}


def _case(rt, name, kind):
    """Forward, backward and the float64 closed form of one case, computed once."""
    key = (name, kind)
    if key in _cache:
        return _cache[key]
    shape, n_dims, ch, pad = SHAPES[name]
    spatial = shape[len(shape) - n_dims:]
    locs = _locs(spatial, kind)
    flat = [v for l in locs for v in l]
    rng = np.random.default_rng(1000 + 10 * list(SHAPES).index(name) + KINDS.index(kind))
    x = rng.standard_normal(shape).astype(np.float32)
    g = rng.standard_normal(shape).astype(np.float32)
    I = rng.uniform(6.0, 12.0, len(locs)).astype(np.float32)
    xd, Id = torch.from_numpy(x).cuda(), torch.from_numpy(I).cuda()
    D = shape[-1]
    gp = torch.zeros(shape[:-1] + (D + pad,), device="cuda")
    gp[..., :D] = torch.from_numpy(g).cuda()
    gview = gp[..., :D]                                   # pad > 0: a strided view of a (D + pad)-column gradient
    y, coef = rt.kspace_spikes(xd, Id, flat, n_dims, ch, pad)
    gx_out = torch.full(shape, float("nan"), device="cuda")
    dI_out = torch.full((len(locs),), float("nan"), device="cuda")
    gx, dI = rt.kspace_spikes_grad(gview, coef, Id, flat, n_dims, ch, True, True, gx_out=gx_out, dI_out=dI_out)
    assert gx.data_ptr() == gx_out.data_ptr() and dI.data_ptr() == dI_out.data_ptr()
    ref = R.closed_form(x, g, I, locs, n_dims)
    c = dict(shape=shape, n_dims=n_dims, ch=ch, pad=pad, spatial=spatial, locs=locs, flat=flat, x=x, g=g, I=I, xd=xd,
             Id=Id, gview=gview, y=y, coef=coef, gx=gx, dI=dI, ref=ref)
    _cache[key] = c
    return c


CASES = [(n, k) for n in SHAPES for k in KINDS]
CASE_IDS = [f"{n}-{k}" for n, k in CASES]


@pytest.mark.parametrize("name,kind", CASES, ids=CASE_IDS)
def test_forward_matches_the_host_program_and_float64(rt, name, kind):
    from texbias import kprog as K
    c = _case(rt, name, kind)
    D, pad = c["shape"][-1], c["pad"]
    geo = K.geometry(c["spatial"])
    prog = [K.spike_op(l, geo, float(i)) for l, i in zip(c["locs"], c["I"])]
    for op in prog[1:]:
        op.reserved = 1
    B = int(np.prod(c["shape"][: len(c["shape"]) - c["n_dims"]])) // c["ch"]
    yh = rt.planes_closed_form(c["xd"], c["n_dims"], [prog] * B, c["ch"], pad=pad)     # the closed-form route alone
    y = c["y"].cpu().numpy().astype(np.float64)
    assert y.shape == c["shape"][:-1] + (D + pad,)
    scale = np.abs(c["ref"]["y"]).max()
    e_route = np.abs(y - yh.cpu().numpy()).max() / scale
    e64 = np.abs(y[..., :D] - c["ref"]["y"]).max() / scale
    print(f"vs host program {e_route:.3e}  vs float64 {e64:.3e}")
    assert e_route <= TOL_ROUTE
    assert e64 <= TOL
    if pad:
        assert np.all(y[..., D:] == 0.0)
    K64 = c["ref"]["K"]
    assert np.abs(c["coef"].cpu().numpy().view(np.complex128)[..., 0] - K64).max() <= TOL * np.abs(K64).max()


@pytest.mark.parametrize("name,kind", CASES, ids=CASE_IDS)
def test_gradients_match_float64_and_are_written_once(rt, name, kind):
    c = _case(rt, name, kind)
    gx, dI = c["gx"].cpu().numpy(), c["dI"].cpu().numpy()
    assert not np.isnan(gx).any() and not np.isnan(dI).any()          # NaN-filled buffers come back fully written
    ref = c["ref"]
    egx = np.abs(gx - ref["gx"]).max() / np.abs(ref["gx"]).max()
    ratio = np.abs(dI - ref["dI"]) / ref["dI_scale"]
    print(f"gx {egx:.3e}  |dI - dI64| / (sum A|G| / N) {ratio.max():.3e}  (dI {dI}, float64 {ref['dI']})")
    assert egx <= TOL
    assert ratio.max() <= TOL
    gx2, dI2 = rt.kspace_spikes_grad(c["gview"], c["coef"], c["Id"], c["flat"], c["n_dims"], c["ch"])
    assert torch.equal(gx2, c["gx"]) and torch.equal(dI2, c["dI"])    # fixed order, no atomics: bit-reproducible
    # the intensity gradient alone is the same number
    none, dI3 = rt.kspace_spikes_grad(c["gview"], c["coef"], c["Id"], c["flat"], c["n_dims"], c["ch"], image_grad=False)
    assert none is None and torch.equal(dI3, c["dI"])


@pytest.mark.parametrize("name,kind", CASES, ids=CASE_IDS)
def test_intensity_gradient_matches_the_doubled_forward(rt, name, kind):
    """y(I_j + ln 2) - y(I_j) = dy/dI_j exactly, so sum g (y(I_j + ln 2) - y(I_j)) = dI_j with no FFT reference."""
    c = _case(rt, name, kind)
    D = c["shape"][-1]
    y0 = c["y"][..., :D].cpu().numpy().astype(np.float64)
    g64 = c["g"].astype(np.float64)
    dI = c["dI"].cpu().numpy().astype(np.float64)
    for j in range(len(c["locs"])):
        I2 = c["I"].copy()
        I2[j] = np.float32(I2[j] + np.float32(LN2))
        y1 = rt.kspace_spikes(c["xd"], torch.from_numpy(I2).cuda(), c["flat"], c["n_dims"], c["ch"], c["pad"])[0]
        y1 = y1[..., :D].cpu().numpy().astype(np.float64)
        est = (g64 * (y1 - y0)).sum()
        bar = TOL * c["ref"]["dI_scale"][j] + 4.0 * 2.0 ** -24 * np.abs(g64).sum() * max(np.abs(y0).max(), np.abs(y1).max())
        print(f"spike {j}: dI {dI[j]:.6e}  sum g dy {est:.6e}  |diff| {abs(dI[j] - est):.3e}  bar {bar:.3e}")
        assert abs(dI[j] - est) <= bar


@pytest.mark.parametrize("name,kind", CASES, ids=CASE_IDS)
def test_output_spectrum_has_the_set_modulus_and_the_input_phase(rt, name, kind):
    c = _case(rt, name, kind)
    D, nd = c["shape"][-1], c["n_dims"]
    ky = rt.kspace_export(c["y"][..., :D], nd).cpu().numpy().astype(np.complex128)
    kx = rt.kspace_export(c["xd"], nd).cpu().numpy().astype(np.complex128)
    ax = tuple(range(-nd, 0))
    kx64 = np.fft.fftshift(np.fft.fftn(c["x"].astype(np.float64), axes=ax), axes=ax)
    for j, loc in enumerate(c["locs"]):
        cj = R.set_coefficient(ky, kx, loc, c["spatial"])
        vx = kx[(Ellipsis,) + tuple(loc)]
        A = math.exp(float(c["I"][j]))
        e_mod = np.abs(np.abs(cj) / A - 1.0).max()
        # a float32 spectrum is good to ~1e-5 of its largest coefficient (A after the spike, max|K| before)
        vx64 = kx64[(Ellipsis,) + tuple(loc)]
        bar = TOL * (1.0 + np.abs(kx64).max() / np.abs(vx64).min())
        e_ph = np.abs(cj / np.abs(cj) - vx / np.abs(vx)).max()
        print(f"spike {j}: |c| / A - 1 = {e_mod:.3e}  phase {e_ph:.3e} (bar {bar:.3e})")
        assert e_mod <= TOL
        assert e_ph <= bar


def test_only_the_requested_gradients_are_launched(rt):
    from texbias.spikes import LearnedSpikeLayer
    shape = (2, 3, 24, 20, 15)
    rng = np.random.default_rng(7)
    xd = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda()
    gd = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda()
    layer = LearnedSpikeLayer([7.0, 9.0], n_spikes=2, seed=3).cuda()
    y = layer(xd)
    assert layer.last_loc is not None and len(layer.last_loc) == 2
    rt.set_pass_timing(True)
    try:
        y.backward(gd)
        _, cnt, _, names = rt.pass_stats()
    finally:
        rt.set_pass_timing(False)
    # only the parameter requires grad: one read of g, the coefficients, the ordered sum -- no streaming pass
    assert xd.grad is None
    # (a slot's name outlives its launches, so the launch counts say which slots ran: slot 2 is the apply's alone)
    assert cnt == [1, 1, 0, 1], (cnt, names)
    assert names[0] == "k_point_dft" and names[1] == "k_spike_gamma" and names[3] == "k_spike_dI_sum", names
    assert "k_point_apply" not in (names[0], names[1], names[3])
    flat = [v for l in layer.last_loc for v in l]
    coef = rt.kspace_spikes(xd, layer.log_intensity.detach(), flat, 3, 3)[1]
    want = rt.kspace_spikes_grad(gd, coef, layer.log_intensity.detach(), flat, 3, 3, image_grad=False)[1]
    assert torch.equal(layer.log_intensity.grad, want)
    # only the image requires grad: the streaming pass is there, and no dI is handed to autograd
    layer.log_intensity.requires_grad_(False)
    xr = xd.clone().requires_grad_(True)
    y = layer(xr, loc=layer.last_loc)
    rt.set_pass_timing(True)
    try:
        y.backward(gd)
        _, cnt, _, names = rt.pass_stats()
    finally:
        rt.set_pass_timing(False)
    assert cnt == [1, 1, 1, 0] and names[2] == "k_point_apply", (cnt, names)     # and no ordered sum
    assert torch.equal(layer.log_intensity.grad, want)   # untouched
    assert torch.equal(xr.grad, rt.kspace_spikes_grad(gd, coef, layer.log_intensity, flat, 3, 3)[0])
    # both: every slot once
    layer.log_intensity.requires_grad_(True)
    layer.log_intensity.grad = None
    xr.grad = None
    y = layer(xr, loc=layer.last_loc)
    rt.set_pass_timing(True)
    try:
        y.backward(gd)
        _, cnt, _, names = rt.pass_stats()
    finally:
        rt.set_pass_timing(False)
    assert cnt == [1, 1, 1, 1] and names[2] == "k_point_apply" and names[3] == "k_spike_dI_sum", (cnt, names)
    assert torch.equal(layer.log_intensity.grad, want)


def test_layer_pad_and_launcher_minmax(rt):
    """``forward(x, loc, pad)`` writes the U-Net's zero columns, and the launcher's ``minmax`` receives the
    per-sample (min, max) keys of the output without them, in two launch groups too."""
    from texbias._lib import lib
    from texbias.spikes import LearnedSpikeLayer
    rng = np.random.default_rng(12)
    for shape, pad in (((2, 3, 24, 20, 15), 5), ((9, 1, 8, 8, 8), 0)):
        xd = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda()
        layer = LearnedSpikeLayer(9.0, seed=4).cuda()
        loc = [(shape[2] // 2 + 1, 3, 2)]
        with torch.no_grad():
            y = layer(xd, loc=loc, pad=pad)
        assert tuple(y.shape) == shape[:-1] + (shape[-1] + pad,)
        mm = torch.full((shape[0], 2), -1, dtype=torch.int32, device="cuda")
        y2, _ = rt.kspace_spikes(xd, layer.log_intensity.detach(), list(loc[0]), 3, shape[1], pad, minmax=mm)
        assert torch.equal(y2, y)
        if pad:
            assert torch.all(y[..., shape[-1]:] == 0)
        body = y[..., : shape[-1]].reshape(shape[0], -1)
        keys = mm.cpu().numpy().view(np.uint32)
        got = np.array([[lib().tb_key_to_float(int(k)) for k in row] for row in keys], np.float32)
        want = torch.stack([body.min(1).values, body.max(1).values], 1).cpu().numpy()
        assert np.array_equal(got, want), (got, want)


def test_opcheck(rt):
    shape = (2, 3, 24, 20, 15)
    rng = np.random.default_rng(8)
    xd = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda()
    gd = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda()
    Id = torch.tensor([7.0, 9.5], device="cuda")
    flat = [3, 4, 5, 12, 10, 7]
    utils = ("test_schema", "test_faketensor", "test_autograd_registration")
    torch.library.opcheck(torch.ops.texbias.kspace_spikes.default, (xd, Id, flat, 3, 3, 5), test_utils=utils)
    torch.library.opcheck(torch.ops.texbias.kspace_spikes.default,
                          (xd.clone().requires_grad_(True), Id.clone().requires_grad_(True), flat, 3, 3, 0),
                          test_utils=utils)
    coef = torch.ops.texbias.kspace_spikes(xd, Id, flat, 3, 3, 0)[1]
    for image_grad, intensity_grad in ((True, True), (False, True), (True, False)):
        torch.library.opcheck(torch.ops.texbias.kspace_spikes_grad.default,
                              (gd, coef, Id, flat, 3, 3, image_grad, intensity_grad), test_utils=utils)


def test_compile_fullgraph_with_backward(rt):
    shape, flat = (2, 3, 24, 20, 15), [3, 4, 5, 12, 10, 7]
    rng = np.random.default_rng(9)
    x = rng.standard_normal(shape).astype(np.float32)
    w = rng.standard_normal(shape[:-1] + (20,)).astype(np.float32)   # the padded output's weights in the loss

    def fn(xd, Id):
        y = torch.ops.texbias.kspace_spikes(xd, Id, flat, 3, 3, 5)[0]
        return y * 2.0 + 1.0

    def run(compiled):
        f = torch.compile(fn, fullgraph=True, backend="aot_eager") if compiled else fn
        xd = torch.from_numpy(x).cuda().requires_grad_(True)
        Id = torch.tensor([7.0, 9.5], device="cuda", requires_grad=True)
        y = f(xd, Id)
        (y * torch.from_numpy(w).cuda()).sum().backward()
        return y.detach(), xd.grad, Id.grad

    ref = run(False)
    torch._dynamo.reset()
    got = run(True)
    for a, b in zip(got, ref):
        torch.testing.assert_close(a, b, rtol=0, atol=0)
    gy = 2.0 * w.astype(np.float64)[..., :15]
    c = R.closed_form(x, gy, [7.0, 9.5], [(3, 4, 5), (12, 10, 7)], 3)
    assert np.abs(ref[1].cpu().numpy() - c["gx"]).max() <= TOL * np.abs(c["gx"]).max()
    assert np.all(np.abs(ref[2].cpu().numpy() - c["dI"]) <= TOL * c["dI_scale"])


def test_graph_capture_reads_the_live_intensity(rt):
    from texbias.spikes import LearnedSpikeLayer
    shape, loc = (2, 1, 16, 12, 10), [(9, 7, 6)]
    x = np.random.default_rng(10).standard_normal(shape).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    layer = LearnedSpikeLayer(8.0).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():   # warm up: plan and workspace
        layer(xd, loc=loc)
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr), torch.no_grad():   # one stream, no parallel branches
        out = layer(xd, loc=loc)
    gr.replay()
    torch.cuda.synchronize()
    y0 = out.clone()
    with torch.no_grad():
        assert torch.equal(y0, layer(xd, loc=loc))          # replay is bit-equal to eager
        layer.log_intensity.add_(LN2)                        # in place: the captured launch reads this buffer
    gr.replay()
    torch.cuda.synchronize()
    d = (out.double() - y0.double()).cpu().numpy()
    # y(I + ln 2) - y(I) = dy/dI = Re(A u e^{i theta}) / N
    c = R.closed_form(x, x, [8.0], loc, 3)
    K = c["K"][..., 0]
    want = (math.exp(8.0) * (K / np.abs(K))[..., None, None, None] * R.plane(loc[0], shape[2:])).real / np.prod(shape[2:])
    e = np.abs(d - want).max() / np.abs(c["y"]).max()
    print(f"replay difference vs dy/dI: {e:.3e} of max|y|")
    assert np.abs(want).max() > 0.1 * np.abs(c["y"]).max()   # the difference is not lost in the bar
    assert e <= TOL


def test_layer_trains_under_train_step(rt):
    from texbias.spikes import LearnedSpikeLayer
    from texbias.train import TrainStep
    from texbias import optim
    loc = [(9, 7, 6)]

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.spike = LearnedSpikeLayer(8.0, seed=0)
            self.head = torch.nn.Conv3d(1, 1, 3, padding=1)

        def forward(self, x):
            return self.head(self.spike(x, loc=loc))

    torch.manual_seed(0)
    rng = np.random.default_rng(11)
    x = torch.from_numpy(rng.standard_normal((2, 1, 16, 16, 16)).astype(np.float32)).cuda()
    labels = torch.from_numpy((rng.random((2, 1, 16, 16, 16)) > 0.5).astype(np.float32)).cuda()
    step = TrainStep(Net(), torch.device("cuda:0"))
    assert isinstance(step.opt, optim.Adam)
    p = step.module.spike.log_intensity
    assert any(q is p for grp in step.opt.param_groups for q in grp["params"])
    step.loss_fn(step.model(x), labels).backward()
    dI0 = p.grad.clone()
    before = p.detach().clone()
    assert torch.isfinite(dI0).all() and float(dI0.abs()) > 0.0
    for _ in range(3):
        loss = step(x, labels)
    after = p.detach()
    print(f"dI {float(dI0):.4e}  I {float(before):.6f} -> {float(after):.6f}  loss {float(loss):.5f}")
    assert torch.isfinite(after).all() and torch.isfinite(loss)
    assert float((after - before) * dI0) < 0.0               # moved against the gradient


# ------------------------------------------------------------------------------------------------- C ABI
BAD = ["s0", "s_big", "freq_high", "freq_negative", "equal", "conjugate", "null_logi", "null_loc", "null_coef_bwd",
       "short_ws", "null_ws", "small_d"]


@pytest.mark.parametrize("bad", BAD)
def test_c_abi_argument_checks(rt, bad):
    """The documented codes before any launch: NaN-filled outputs stay NaN."""
    from texbias._abi import TB_ERR_INVALID_ARG, TB_ERR_UNSUPPORTED_SIZE, TB_ERR_WORKSPACE, TB_MAX_OPS, TB_OK
    from texbias._lib import lib
    B, Cc, H, W, D = 1, 2, 12, 10, (3 if bad == "small_d" else 9)
    x = torch.randn((B, Cc, H, W, D), device="cuda")
    y = torch.full_like(x, float("nan"))
    gx = torch.full_like(x, float("nan"))
    S = 2
    coef = torch.zeros((B, Cc, TB_MAX_OPS + 1, 2), dtype=torch.float64, device="cuda")
    logi = torch.full((TB_MAX_OPS + 1,), 7.0, device="cuda")
    dI = torch.full((TB_MAX_OPS + 1,), float("nan"), device="cuda")
    plan = rt.plan_for(x.device, H, W, D)
    need = int(lib().tb_spikes_workspace_bytes(plan.handle, B * Cc))
    assert need > 0 and int(lib().tb_spikes_workspace_bytes(plan.handle, 0)) == 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    st = (C.c_int64 * 3)(H * W * D, W * D, D)
    stream = torch.cuda.current_stream().cuda_stream
    loc = [1, 2, 0, 3, 4, 1] + [5, 0, 0, 6, 0, 0, 4, 1, 0, 3, 1, 0, 2, 1, 0]
    a = dict(S=S, loc=True, logi=logi.data_ptr(), coef=coef.data_ptr(), ws=ws.data_ptr(), n=need)
    want, fwd, bwd = TB_ERR_INVALID_ARG, True, True
    if bad == "s0":
        a["S"] = 0
    elif bad == "s_big":
        a["S"] = TB_MAX_OPS + 1
    elif bad == "freq_high":
        loc[4] = W
    elif bad == "freq_negative":
        loc[2] = -1
    elif bad == "equal":
        loc[3:6] = loc[0:3]
    elif bad == "conjugate":
        loc[3:6] = [H - 1, W - 2, 0]
    elif bad == "null_logi":
        a["logi"] = None
    elif bad == "null_loc":
        a["loc"] = False
    elif bad == "null_coef_bwd":
        a["coef"], fwd = None, False
    elif bad == "short_ws":
        a["n"], want = need - 1, TB_ERR_WORKSPACE
    elif bad == "null_ws":
        a["ws"], want = None, TB_ERR_WORKSPACE
    elif bad == "small_d":
        loc[2] = loc[5] = 0
        want = TB_ERR_UNSUPPORTED_SIZE
    larr = (C.c_int32 * len(loc))(*loc) if a["loc"] else None
    if fwd:
        rc = lib().tb_kspace_spikes_f32(plan.handle, x.data_ptr(), st, y.data_ptr(), st, 0, a["ws"], a["n"], B, Cc,
                                        a["S"], larr, a["logi"], a["coef"], None, stream)
        assert rc == want, rc
    if bwd:
        rc = lib().tb_kspace_spikes_bwd_f32(plan.handle, x.data_ptr(), st, B, Cc, a["S"], larr, a["logi"], a["coef"],
                                            gx.data_ptr(), st, dI.data_ptr(), a["ws"], a["n"], stream)
        assert rc == want, rc
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and torch.isnan(gx).all() and torch.isnan(dI).all()
    if bad == "s0":   # the same arguments with a valid count run
        assert lib().tb_kspace_spikes_f32(plan.handle, x.data_ptr(), st, y.data_ptr(), st, 0, a["ws"], a["n"], B, Cc, S,
                                          larr, a["logi"], a["coef"], None, stream) == TB_OK
        assert lib().tb_kspace_spikes_bwd_f32(plan.handle, x.data_ptr(), st, B, Cc, S, larr, a["logi"], a["coef"], None,
                                              None, dI.data_ptr(), a["ws"], a["n"], stream) == TB_OK
        torch.cuda.synchronize()
        assert not torch.isnan(y).any() and torch.isnan(gx).all() and not torch.isnan(dI[:S]).any()
        assert torch.isnan(dI[S:]).all()
