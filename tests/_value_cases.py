"""Value classes for the k-space routes, their programs and float64 / float32 references -- test
infrastructure (tests/test_value_cases_cpu.py on the host emulator, tests/test_gpu_value_classes.py on
the device).  Plain numpy / torch, no GPU, nothing of the library but the op constructors.

Every other k-space test feeds unit-scale ``randn``.  The classes here are what volumes look like
instead: exact-zero background, raw intensities of 10^3, empty channels and samples, one hot voxel, a
single impulse, whole-image powers of two from 2^-100 to 2^60, and images whose tail (or one whole
channel) lies 2^-120 .. 2^-140 below the rest -- the inputs of the value-dependent steps of the kernels
(the per-strip / per-unit power-of-two scales of the split-f16 products, the phase normalisation of a
kept-phase spike).

A program is a list of plain tuples, turned into ops by ``to_ops`` and restated by ``ref64`` / ``ref32``:
    ("disk", r, inside_off)   ("gibbs", alpha)   ("wrap", alpha)   ("spike", idx_shifted, log_amp)
The bar is ``close64`` per (sample, channel): e_ours <= 4 max(e_ref32, 1e-6 scale), scale = max(max|x_bc|,
max|y64_bc|) -- max|x| because a high-pass of a constant has y ~ 0, per channel because a tiny channel
must not hide behind its neighbour.
"""
from __future__ import annotations

import numpy as np

from oracle import filters_oracle as O

C = 2
SCALED = (-100, -24, 24, 60)
HALO = (-120, -140)
CLASSES = (["randn"] + [f"scaled[{k}]" for k in SCALED] +
           ["brain", "empty_channel", "empty_sample", "constant", "dc_heavy", "hot_voxel", "impulse"] +
           [f"halo[{e}]" for e in HALO] + ["tiny_channel"])
TINY = 2.0 ** -114      # a strip / unit whose max |x| is in (0, TINY) had the scale 2^(14 - ex) = inf
STRIP = 16              # rows of one k_band_fwd strip (band.h BAND_FWD_ROWS)


# ----------------------------------------------------------------- generators
def _randn(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def strips(x):
    """max |x| of every 16-row strip of every (bc, h) slab: [B C, H, ceil(W / 16)]"""
    B, Cc, H, W, D = x.shape
    a = np.abs(x.reshape(B * Cc, H, W, D)).max(axis=3)
    return np.stack([a[:, :, w0:w0 + STRIP].max(axis=2) for w0 in range(0, W, STRIP)], axis=2)


def wrap_units(x):
    """max |x| of every k_wrap_dgemm unit (rows 4 gq .. 4 gq + 3 of both W halves in the slabs hq and
    hq + H / 2 of one channel-volume; even H and W): [B C, H / 2, ceil(W / 8)]"""
    B, Cc, H, W, D = x.shape
    a = np.abs(x.reshape(B * Cc, 2, H // 2, 2, W // 2, D)).max(axis=(1, 3, 5))
    return np.stack([a[:, :, g:g + 4].max(axis=2) for g in range(0, W // 2, 4)], axis=2)


def make(name: str, hwd, seed: int = 0) -> np.ndarray:
    """float32 [B, C, H, W, D] of a class (B = 2 for ``empty_sample``, else 1; C = 2); each class asserts
    its own claim about the data."""
    H, W, D = hwd
    B = 2 if name == "empty_sample" else 1
    shape = (B, C, H, W, D)
    g = _randn(shape, seed + 17 * sum(hwd))
    if name == "randn":
        x = g
    elif name.startswith("scaled["):
        x = np.ldexp(g, int(name[7:-1])).astype(np.float32)
        assert np.isfinite(x).all() and np.abs(x).max() > 0
    elif name == "brain":
        ax = [(np.arange(n) - (n - 1) / 2) / (0.36 * n) for n in hwd]
        inside = (ax[0][:, None, None] ** 2 + ax[1][None, :, None] ** 2 + ax[2][None, None, :] ** 2) < 1.0
        x = np.where(inside, np.float32(1000) + np.float32(400) * np.abs(g), np.float32(0)).astype(np.float32)
        assert np.count_nonzero(x == 0) >= 0.5 * x.size
        lo, hi = strips(x), strips(np.where(x == 0, np.float32(1), np.float32(0)))
        assert (lo == 0).any(), "no all-zero strip"
        assert ((lo > 0) & (hi > 0)).any(), "no strip with zeros next to values"
    elif name == "empty_channel":
        x = g.copy()
        x[:, 0] = 0
    elif name == "empty_sample":
        x = g.copy()
        x[1] = 0
    elif name == "constant":
        x = np.full(shape, 1000.0, np.float32)
    elif name == "dc_heavy":
        x = (np.float32(1000) + g).astype(np.float32)
    elif name == "hot_voxel":
        x = g.copy()
        for c in range(C):
            x[0, c, (H // 3 + c) % H, W // 2, (2 * D) // 3] = 1e6
    elif name == "impulse":
        x = np.zeros(shape, np.float32)
        for c in range(C):
            x[0, c, (H // 3 + c) % H, W // 4 + 1, D // 2 + 1] = 1.0
        assert x[:, :, 0, 0, 0].max() == 0
    elif name.startswith("halo["):
        e = int(name[5:-1])
        x = g.copy()
        x[:, :, H // 2:] = np.ldexp(g[:, :, H // 2:], e)
        s = strips(x)[:, H // 2:]
        assert (s > 0).all() and (s < TINY).all(), "a halo strip outside (0, 2^-114)"
        assert (strips(x)[:, : H // 2] > 0.5).all()
        if e < -126:
            assert np.abs(x[:, :, H // 2:]).max() < 2.0 ** -126     # float32 subnormals
    elif name == "tiny_channel":
        x = g.copy()
        x[:, 0] = np.ldexp(g[:, 0], -120)
        s = strips(x).reshape(B, C, H, -1)[:, 0]
        assert (s > 0).all() and (s < TINY).all()
        if H % 2 == 0 and W % 2 == 0:
            # A wrap unit pairs the slabs h and h + H / 2, so no unit of ``halo`` is all halo: the wrap
            # route's tiny units are those of this class's channel 0, every one of them.
            u = wrap_units(x).reshape(B, C, H // 2, -1)[:, 0]
            assert (u > 0).all() and (u < TINY).all()
    else:
        raise KeyError(name)
    assert x.dtype == np.float32 and x.shape == shape
    return x


# ----------------------------------------------------------------- programs
def log_amp(xb) -> float:
    """log(0.25 N max|x|) of a sample [C, H, W, D] (2.0 for an all-zero one): the spike's plane wave is a
    quarter of the image's largest value in every class."""
    m = float(np.abs(xb).max())
    n = int(np.prod(xb.shape[1:]))
    return float(np.log(0.25 * n * m)) if m > 0 else 2.0


def spike_idx(hwd, where="out"):
    """fftshift-ed index of a spike: ``out`` at 0.8 n (outside every low-pass box used here), ``in`` at
    (+1, +1, +2) off the centre (inside them), ``b`` a second one that touches neither."""
    if where == "out":
        return tuple(int(n * 0.8) for n in hwd)
    if where == "in":
        return (hwd[0] // 2 + 1, hwd[1] // 2 + 1, hwd[2] // 2 + 2)
    return (hwd[0] // 4, hwd[1] // 2 + 2, hwd[2] // 4 + 1)


def programs(kind: str, x, r=3.5):
    """One program per sample of x for a named kind (the spike amplitude follows the sample)."""
    hwd = x.shape[2:]
    out = []
    for b in range(x.shape[0]):
        la = log_amp(x[b])
        p = {
            "lin": [("disk", r, False), ("wrap", 0.5)],
            "chain": [("disk", r, False), ("spike", spike_idx(hwd, "out"), la), ("wrap", 0.5)],
            "inbox": [("disk", r, False), ("spike", spike_idx(hwd, "in"), la)],
            "spike": [("spike", (3, 4, 5), la)],
            "spike2": [("spike", (3, 4, 5), la), ("spike", spike_idx(hwd, "b"), la - 1.0)],
            "hp": [("disk", 3.0, True)],
            "gibbs": [("gibbs", 0.85)],
            "wrap0": [("wrap", 0.0)],
            "wrap5": [("wrap", 0.5)],
        }[kind]
        out.append(p)
    return out


LINEAR = ("lin", "hp", "gibbs", "wrap0", "wrap5")
RAW_PHASE = ("spike", "spike2", "inbox")    # a kept-phase spike reads a coefficient that no mask has zeroed


def phase_condition(x, idx) -> float:
    """sum|x| / |k(idx)| over the (sample, channel) volumes of x, the largest: the factor by which a
    transform's backward error grows in the kept phase of a spike at idx.  0 for an all-zero volume (every
    transform returns exactly 0 there, and angle(0) = 0), inf where the exact coefficient is 0 but the
    volume is not."""
    ax = (-3, -2, -1)
    k = np.fft.fftshift(np.fft.fftn(np.asarray(x, np.float64), axes=ax), axes=ax)
    worst = 0.0
    for b in range(x.shape[0]):
        for c in range(x.shape[1]):
            s = float(np.abs(x[b, c]).sum(dtype=np.float64))
            m = float(np.abs(k[b, c][tuple(idx)]))
            if s > 0:
                worst = max(worst, s / m if m > 0 else np.inf)
    return worst


def phase_free(name: str, kind: str) -> bool:
    """Cells whose kept phase has no reference value: a kept-phase spike on an unmasked coefficient of
    ``constant``.  Every coefficient of a constant but DC is exactly 0, yet a rounding transform returns 0 there
    only where its roundings happen to cancel (numpy's does at 12 x 10 x 15 and does not at 37 x 41 x 43), else
    noise of any angle: the phase that ref64 would keep is its own FFT's accident (phase_condition = inf; see
    tests/test_value_cases_cpu.py::test_kept_phase_conditioning).  Where the transform under test cancels a
    constant exactly (the mixed-radix full-spectrum passes and the emulator at the radix 2 / 3 / 5 / 7 shapes
    used here) the cell keeps the whole bar; elsewhere it is compared free of the phase (``close64_mag``).  A
    spike behind a mask that zeroes its coefficient (``chain``) reads an exact 0 in every transform."""
    return name == "constant" and kind in RAW_PHASE


def to_ops(progs, hwd):
    from texbias import kprog as K
    geo = K.geometry(hwd)
    res = []
    for p in progs:
        ops = []
        for op in p:
            if op[0] == "disk":
                ops.append(K.disk_op(op[1], op[2]))
            elif op[0] == "gibbs":
                ops.append(K.gibbs_op(op[1], hwd))
            elif op[0] == "wrap":
                ops.append(K.wrap_op(op[1]))
            else:
                ops.append(K.spike_op(op[1], geo, op[2]))
        res.append(ops)
    return res


# ----------------------------------------------------------------- references
def _wrap_mask(hwd, alpha):
    """WrapArtifact as one mask: alpha on the odd fftshift-ed indices of each axis (O.wrap_artifact)"""
    m = np.ones(hwd, np.float64)
    a = float(np.float32(alpha))
    m[1::2, :, :] *= a
    m[:, 1::2, :] *= a
    m[:, :, 1::2] *= a
    return m


def _mask(op, hwd):
    if op[0] == "disk":
        return O.disk_mask(hwd, op[1], 3, op[2]).astype(np.float64)
    if op[0] == "gibbs":
        return O.gibbs_mask(hwd, op[1]).astype(np.float64)
    return _wrap_mask(hwd, op[1])


def _real_part(k, xp):
    """The spectrum of Re(ifftn(k)) over the last three axes, k fftshift-ed: (k(f) + conj(k(-f))) / 2, taken in
    the spectrum so that a coefficient that is exactly 0 stays 0 (a round trip through the image would
    leave rounding noise there, whose angle a later kept-phase spike would read)."""
    ax = (-3, -2, -1)
    if xp is np:
        u = np.fft.ifftshift(k, axes=ax)
        m = np.conj(np.roll(np.flip(u, axis=ax), 1, axis=ax))
        return np.fft.fftshift(0.5 * (u + m), axes=ax)
    u = xp.fft.ifftshift(k, dim=ax)
    m = xp.conj(xp.roll(xp.flip(u, dims=ax), shifts=(1, 1, 1), dims=ax))
    return xp.fft.fftshift(0.5 * (u + m), dim=ax)


def ref64(x, progs) -> np.ndarray:
    """float64 restatement: fftn in complex128; the 0/1 masks of oracle.filters_oracle and the wrap mask;
    a spike replaces one coefficient (|k| := exp(val), the phase of the float64 coefficient, angle(0) = 0)
    and the `.real` of the inverse gives its conjugate partner the other half, as O.spikes_exact; between
    ops that `.real` is taken in the spectrum (after a spike, and after the Gibbs mask, which is not
    symmetric on an even axis); ifftn(...).real."""
    x = np.asarray(x, np.float64)
    ax = (-3, -2, -1)
    y = np.empty_like(x)
    for b, prog in enumerate(progs):
        hwd = x.shape[2:]
        k = np.fft.fftshift(np.fft.fftn(x[b], axes=ax), axes=ax)
        for i, op in enumerate(prog):
            if op[0] == "spike":
                sel = (slice(None),) + tuple(op[1])
                kk = k[sel]
                ph = np.where(kk == 0, 0.0, np.angle(kk))
                k[sel] = np.exp(np.float64(np.float32(op[2]))) * np.exp(1j * ph)
            else:
                k = k * _mask(op, hwd)
            if op[0] in ("spike", "gibbs") and i + 1 < len(prog):
                k = _real_part(k, np)
        y[b] = np.fft.ifftn(np.fft.ifftshift(k, axes=ax), axes=ax).real
    return y


def ref32(x, progs) -> np.ndarray:
    """The same restatement in float32 / complex64 on torch.fft."""
    import torch
    xt = torch.from_numpy(np.ascontiguousarray(x, np.float32))
    ax = (-3, -2, -1)
    y = torch.empty_like(xt)
    for b, prog in enumerate(progs):
        hwd = tuple(xt.shape[2:])
        k = torch.fft.fftshift(torch.fft.fftn(xt[b], dim=ax), dim=ax)
        for i, op in enumerate(prog):
            if op[0] == "spike":
                h, w, d = op[1]
                kk = k[:, h, w, d]
                ph = torch.where(kk == 0, torch.zeros_like(kk.real), torch.angle(kk))
                amp = torch.exp(torch.tensor(np.float32(op[2])))
                k[:, h, w, d] = torch.polar(amp.expand_as(ph).contiguous(), ph)
            else:
                k = k * torch.from_numpy(_mask(op, hwd).astype(np.float32))
            if op[0] in ("spike", "gibbs") and i + 1 < len(prog):
                k = _real_part(k, torch)
        y[b] = torch.fft.ifftn(torch.fft.ifftshift(k, dim=ax), dim=ax).real
    return y.numpy()


_refs = {}


def case(name, hwd, kind, r=3.5):
    """(x, programs, y64, y32) of a cell, made once and shared (read-only)"""
    key = (name, tuple(hwd), kind, r)
    if key not in _refs:
        x = make(name, hwd)
        progs = programs(kind, x, r)
        y64, y32 = ref64(x, progs), ref32(x, progs)
        for a in (x, y64, y32):
            a.setflags(write=False)
        _refs[key] = (x, progs, y64, y32)
    return _refs[key]


# ----------------------------------------------------------------- the bar
def ratios(ours, x, y64, y32):
    """per (sample, channel): e_ours / max(e_ref32, 1e-6 scale), with e_ref32 / (1e-6 scale) next to it"""
    B, Cc = x.shape[:2]
    out = np.empty((B, Cc, 2))
    for b in range(B):
        for c in range(Cc):
            scale = max(np.abs(x[b, c]).max(), np.abs(y64[b, c]).max())
            e_o = np.abs(np.asarray(ours[b, c], np.float64) - y64[b, c]).max()
            e_r = np.abs(np.asarray(y32[b, c], np.float64) - y64[b, c]).max()
            floor = 1e-6 * float(scale) if scale > 0 else 0.0
            den = max(e_r, floor)
            out[b, c, 0] = (e_o / den) if den > 0 else (0.0 if e_o == 0 else np.inf)
            out[b, c, 1] = (e_r / floor) if floor > 0 else (0.0 if e_r == 0 else np.inf)
    return out


def close64_mag(ours, x, y64, y32, what="") -> float:
    """The bar without the spike's phase: max | |F(ours)| - |F(y64)| | / N over all coefficients F = fftn of a
    (sample, channel) in place of max |ours - y64|, against the same figure of ref32 and the same floor.
    | |F(a)| - |F(b)| | <= sum |a - b| <= N max |a - b|, so an output inside the image bar is inside this one;
    what it no longer sees is the angle of a coefficient.  The wave's amplitude at the spike and its partner,
    the DC term and every other coefficient (which stays at the floor) are all held."""
    ours = np.asarray(ours, np.float64)
    assert np.isfinite(ours).all(), f"{what}: non-finite output"
    ax = (-3, -2, -1)
    n = float(np.prod(x.shape[2:]))
    worst = 0.0
    for b in range(x.shape[0]):
        for c in range(x.shape[1]):
            m64 = np.abs(np.fft.fftn(y64[b, c], axes=ax))
            e_o = np.abs(np.abs(np.fft.fftn(ours[b, c], axes=ax)) - m64).max() / n
            e_r = np.abs(np.abs(np.fft.fftn(np.asarray(y32[b, c], np.float64), axes=ax)) - m64).max() / n
            scale = max(np.abs(x[b, c]).max(), np.abs(y64[b, c]).max())
            den = max(e_r, 1e-6 * float(scale))
            worst = max(worst, (e_o / den) if den > 0 else (0.0 if e_o == 0 else np.inf))
    print(f"close64_mag {what}: worst = {worst:.3f}")
    assert worst <= 4.0, (what, worst)
    return worst


def close64(ours, x, y64, y32, what="") -> float:
    """Asserts the bar on every (sample, channel) and returns the worst ratio (bar: 4)."""
    assert np.isfinite(np.asarray(ours)).all(), f"{what}: non-finite output"
    r = ratios(ours, x, y64, y32)
    worst = float(r[..., 0].max())
    print(f"close64 {what}: worst e_ours / max(e_ref32, 1e-6 scale) = {worst:.3f} "
          f"(e_ref32 / floor {float(r[..., 1].max()):.3f})")
    assert worst <= 4.0, (what, r[..., 0].tolist())
    return worst
