"""Value classes (tests/_value_cases.py) on every k-space route of tb_kspace_filter_f32, against the float64
restatement ``ref64`` of the same program.

Bar, per (sample, channel): e_ours <= 4 max(e_ref32, 1e-6 scale), scale = max(max|x_bc|, max|y64_bc|), ref32 the
same restatement in float32 on torch.fft; the output finite; the pad columns (pad = 3) exactly zero; the
min / max keys equal to the output's own min / max per sample; an all-zero sample or channel under a linear
program gives an all-zero output.  The kernel that ran is asserted from ``rt.pass_stats()``; the split-f16
instantiation of pass A' (k_band_fwd<1, 1, 155, true>), which the pass name does not tell from the f32 one,
from the profiler's kernel names.

Routes, shapes (B from the class, C = 2) and programs (lin = disk + wrap(0.5), chain = disk + kept-phase spike
outside the box + wrap(0.5), inbox = disk + kept-phase spike inside the box, spike / spike2 = one / two kept-
phase spikes, hp = disk(3.0, inside_off), gibbs = Gibbs(0.85), wrap0 / wrap5 = wrap(0) / wrap(0.5)):

    full    band / point / wrap plans off            12x10x15                 lin chain spike hp gibbs
    band    k_band_fwd (f32) + k_band_inv16          24x20x15, 31x17x30       lin chain inbox      (disk 4.5)
    band32  k_band_fwd (f32) + k_band_inv            24x20x15, 31x17x30       lin chain inbox
    f16     k_band_fwd<.., 155, true> + k_band_inv16 24x20x155                lin chain
            (W = 20: one full and one 4-row strip)
    even    k_wrap_even                              16x12x10                 wrap0 wrap5
    odd     k_wrap_dgemm                             6x10x7, 16x12x15         wrap0 wrap5
    point   k_point_dft / k_point_delta / k_point_apply   12x10x15            spike spike2
    generic k_gen_dft (band / point / wrap plans off)     37x41x43            lin spike

Cells that are absent: spikes on the wrap route and masks on the closed-form route (the routes do not take
those programs).  Every class runs in every other cell.  ``constant`` under spike / spike2 / inbox has no reference
phase (V.phase_free: the exact coefficient is 0 and a transform's rounding noise decides the angle): on the
full-spectrum route, whose radix 2 / 3 / 5 butterflies cancel a constant exactly, it keeps the whole bar; on the
band, closed-form and direct-DFT routes the same bar is taken on the magnitudes of the output's spectrum
(V.close64_mag: the wave's amplitude at the spike and its partner, DC, and every other coefficient at the floor),
with the finite, pad and key checks as everywhere.

Worst e_ours / max(e_ref32, 1e-6 scale) measured on MI355X (bar: 4), per route, and the cell it comes from:
    full     3.002  12x10x15 spike dc_heavy      (e_ref32 = 5.9 floors)
    band     0.945  31x17x30 inbox tiny_channel
    band32   0.857  31x17x30 inbox tiny_channel
    f16      0.400  24x20x155 chain empty_channel
    even     0.106  16x12x10 wrap5 dc_heavy
    odd      0.157  16x12x15 wrap5 dc_heavy
    point    0.502  12x10x15 spike tiny_channel
    generic  1.223  37x41x43 spike dc_heavy      (e_ref32 = 3.9 floors)
band / band32 31x17x30 inbox ``dc_heavy`` (a coefficient of 19.5 under a DC term of 1.6e7, the kept phase conditioned
by 8.1e5) was at 12.4 while pass A' summed the raw rows; with the row's first value taken off before the D product
(k_band_fwd, run-time D) it is at 0.31 / 0.34.  The phase-free ``constant`` cells: band 0.010 / 0.028, band32 0.003 /
0.028, point 0.011 / 0.008, generic 0.041; on the full route, with its phase, 0.143.
"""
import re

import numpy as np
import pytest
import torch

import _value_cases as V

pytestmark = pytest.mark.gpu
PAD = 3

ROUTES = {
    "full": dict(shapes=[(12, 10, 15)], kinds=["lin", "chain", "spike", "hp", "gibbs"], r=3.5),
    "band": dict(shapes=[(24, 20, 15), (31, 17, 30)], kinds=["lin", "chain", "inbox"], r=4.5),
    "band32": dict(shapes=[(24, 20, 15), (31, 17, 30)], kinds=["lin", "chain", "inbox"], r=4.5),
    "f16": dict(shapes=[(24, 20, 155)], kinds=["lin", "chain"], r=4.5),
    "even": dict(shapes=[(16, 12, 10)], kinds=["wrap0", "wrap5"], r=0.0),
    "odd": dict(shapes=[(6, 10, 7), (16, 12, 15)], kinds=["wrap0", "wrap5"], r=0.0),
    "point": dict(shapes=[(12, 10, 15)], kinds=["spike", "spike2"], r=0.0),
    "generic": dict(shapes=[(37, 41, 43)], kinds=["lin", "spike"], r=3.5),
}
CELLS = [(route, hwd, kind) for route, d in ROUTES.items() for hwd in d["shapes"] for kind in d["kinds"]]


def cell_id(c):
    return f"{c[0]}-{'x'.join(map(str, c[1]))}-{c[2]}"


@pytest.fixture(scope="module")
def rt(gpu):
    from texbias import runtime
    return runtime


def run(rt, route, x, ops):
    """(y, keys, pass names) of one launch on a route"""
    off = route in ("full", "generic")
    xd = torch.from_numpy(x).cuda()
    mm = torch.empty((x.shape[0], 2), dtype=torch.int32, device="cuda")
    try:
        if off:
            rt.set_band_plans(False)
            rt.set_point_plans(False)
            rt.set_wrap_plans(False)
        if route == "band32":
            rt.set_band_inv16(False)
        rt.set_pass_timing(True)
        y = rt.kspace_filter(xd, 3, ops, x.shape[1], pad=PAD, minmax=mm)
        torch.cuda.synchronize()
        names = rt.pass_stats()[3]
    finally:
        rt.set_pass_timing(False)
        rt.set_band_inv16(True)
        rt.set_band_plans(True)
        rt.set_point_plans(True)
        rt.set_wrap_plans(True)
    return y, mm, names


def check_kernels(route, names):
    if route == "full":
        assert names[0] == "k_slab_fwd" and names[1] == "k_kspace" and names[2] == "k_slab_inv", names
    elif route in ("band", "f16"):
        assert names[0] == "k_band_fwd" and names[2] == "k_band_inv16", names
    elif route == "band32":
        assert names[0] == "k_band_fwd" and names[2] == "k_band_inv", names
    elif route == "even":
        assert names[2] == "k_wrap_even", names
    elif route == "odd":
        assert names[2] == "k_wrap_dgemm", names
    elif route == "point":
        assert names[0].startswith("k_point_dft") and names[1] == "k_point_delta" and names[2] == "k_point_apply", names
    else:
        assert names[1] == "k_gen_dft", names


def check_keys(rt, y, mm, D):
    v = y[..., :D].reshape(y.shape[0], -1)
    m = rt.keys_to_float(mm)
    np.testing.assert_array_equal(m[:, 0], v.min(1).values.cpu().numpy())
    np.testing.assert_array_equal(m[:, 1], v.max(1).values.cpu().numpy())


@pytest.mark.parametrize("name", V.CLASSES)
@pytest.mark.parametrize("cell", CELLS, ids=cell_id)
def test_value_class(rt, cell, name):
    route, hwd, kind = cell
    x, progs, y64, y32 = V.case(name, hwd, kind, ROUTES[route]["r"])
    y, mm, names = run(rt, route, x, V.to_ops(progs, hwd))
    check_kernels(route, names)
    D = hwd[2]
    yh = y.cpu().numpy()
    assert np.isfinite(yh).all(), f"non-finite output: {np.count_nonzero(~np.isfinite(yh))} values"
    assert not yh[..., D:].any(), "pad columns"
    if V.phase_free(name, kind) and route != "full":   # no reference phase, and no exact cancellation
        V.close64_mag(yh[..., :D], x, y64, y32, f"{cell_id(cell)} {name}")
    else:
        V.close64(yh[..., :D], x, y64, y32, f"{cell_id(cell)} {name}")
    check_keys(rt, y, mm, D)
    if kind in V.LINEAR:   # an all-zero sample / channel stays all zero
        for b in range(x.shape[0]):
            for c in range(x.shape[1]):
                if not x[b, c].any():
                    assert not yh[b, c].any(), (b, c)


@pytest.mark.parametrize("name,kind", [("randn", "lin"), ("empty_sample", "chain")])
def test_f16_variant_runs(rt, name, kind):
    """(a one-sample linear launch and a B = 2 launch of the chain program)  24 x 20 x 155 (contiguous, D = 155, <= 16 kd columns, < 16 kw rows) takes the split-f16 D product of
    pass A' and the split-f16 synthesis of pass C': the instantiations by their template arguments."""
    from torch.profiler import ProfilerActivity, profile
    hwd = (24, 20, 155)
    x, progs, _, _ = V.case(name, hwd, kind, 4.5)
    xd = torch.from_numpy(x).cuda()
    ops = V.to_ops(progs, hwd)
    rt.kspace_filter(xd, 3, ops, x.shape[1], pad=PAD)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        rt.kspace_filter(xd, 3, ops, x.shape[1], pad=PAD)
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages() if e.device_time_total > 0]
    print(names)
    assert any(re.search(r"k_band_fwd<1, 1, 155, (true|\(bool\)1)>", k) for k in names), names
    assert any("k_band_inv16<" in k for k in names), names
