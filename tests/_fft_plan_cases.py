"""The case table of the mixed-radix plan sweeps (tests/test_emu_fft_plans.py on the host emulator,
tests/test_gpu_fft_plans.py on the device) -- test infrastructure.

The run-time planner (csrc/plan_host.h factorize()) takes 19 radices and up to 8 stages per axis, and
the three axes run three different bodies (D: pair-packed rows; W: columns of the slab; H: pass B, its
last stage fused with the op program).  The table places every length on one axis at a time, next to
two small composite axes, so each case names one plan of one body.

Nothing here reads the library: the factorisation is restated, and the coverage conditions
(tests/test_emu_fft_plans.py::test_table_coverage) are computed from that restatement.
"""
from __future__ import annotations

import numpy as np

# csrc/plan_host.h kRadixPref, restated: fewest stages first, the odd primes >= 7 last
RADIX_PREF = (16, 15, 12, 10, 9, 8, 6, 5, 4, 3, 2, 7, 11, 13, 17, 19, 23, 29, 31)
PRIMES = (7, 11, 13, 17, 19, 23, 29, 31)
STREAMED = (11, 13, 17, 19, 23, 29, 31)     # fft_core.h IsStreamed: the second compiled radix set


def expected_radices(n: int):
    """factorize(): greedily the first radix of the preference order that divides what is left.
    None for a length with a prime factor above 31."""
    out, m = [], int(n)
    while m > 1:
        for r in RADIX_PREF:
            if m % r == 0:
                out.append(r)
                m //= r
                break
        else:
            return None
    return out


SINGLE = [2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 15, 16, 11, 13, 17, 19, 23, 29, 31]
PRIME_LAST = [22, 26, 33, 34, 38, 39, 46, 55, 58, 62, 77, 91, 176, 208]
PRIME_FIRST = [49, 121, 143, 169, 221, 289, 323, 361, 437, 529, 667, 841, 899, 961]   # its twiddles run
DEEP = [98, 147, 242, 686]          # 2.7.7, 3.7.7, 2.11.11, 2.7.7.7
LENGTHS = SINGLE + PRIME_LAST + PRIME_FIRST + [256] + DEEP

AXES = (0, 1, 2)
AXIS_NAME = "HWD"


def shape_for(n: int, axis: int):
    """(H, W, D) with `n` on `axis`: the other two axes stay small composites, so every slab and tile
    is far below the LDS and H <= the mask-gradient tile limit (no case leaves the mixed-radix route)."""
    s = [6, 8, 10] if n <= 100 else [6, 4, 6]
    s[axis] = n
    return tuple(s)


# (spatial shape as the caller passes it, transformed axes): every (length, axis), two channel-volumes each
CASES = [(shape_for(n, a), 3) for n in LENGTHS for a in AXES]
# squeezed axes: [H, D] images (W = 1) and a single row (H = W = 1)
EXTRA = [((26, 33), 2), ((22, 6), 2), ((1, 1, 143), 3)]
ALL_CASES = CASES + EXTRA
CHANNELS = 2


def case_id(case):
    return "x".join(str(s) for s in case[0])


# the fused-filter subset: every streamed prime alone, as the first, the last and a middle stage
FILTER_LENGTHS = [11, 13, 17, 19, 23, 29, 31, 22, 143, 169, 98, 242, 686]


def filter_shape_for(n: int, axis: int):
    s = [10, 8, 12]
    s[axis] = n
    return tuple(s)


FILTER_CASES = [filter_shape_for(n, a) for n in FILTER_LENGTHS for a in AXES]


def spike_index(hwd):
    """Centred index (2, -3, +3) off the centre, wrapped into the axis where it is shorter than that
    (squared distance >= 14 either way: outside the radius-3 disk)."""
    H, W, D = hwd
    return ((H // 2 + 2) % H, (W // 2 - 3) % W, (D // 2 + 3) % D)


def filter_program(hwd):
    """High-pass disk, one spike outside it, wrap: an op that reads the coefficient's position on every
    axis, one that hits a single coefficient and its mirror, one that reads the parity of the position."""
    from texbias import kprog as K
    return [K.disk_op(3.0, inside_off=True), K.spike_op(spike_index(hwd), K.geometry(hwd), 9.0), K.wrap_op(0.5)]


def filter_reference(x, hwd):
    """x: [C, H, W, D] float32."""
    from oracle import filters_oracle as O
    return O.wrap_artifact(O.plane_waves(O.fourier_disk(x, 3.0, inside_off=True), spike_index(hwd), 9.0), 0.5)


# The host picks one of two compiled radix sets per kernel: SMALL, or ALL (with the streamed primes), once
# for the W / D passes and once for the H pass.  (H, W, D) per corner (set of W / D, set of H).
SMALL, ALL = "small", "all"
CORNERS = [
    ((SMALL, SMALL), (12, 10, 9)),     # control
    ((SMALL, ALL), (22, 8, 6)),
    ((SMALL, ALL), (143, 4, 6)),
    ((ALL, SMALL), (6, 26, 10)),
    ((ALL, SMALL), (6, 8, 31)),
    ((ALL, ALL), (13, 19, 23)),
    ((ALL, ALL), (29, 4, 33)),
]
PRIME_ROWS = [(p, 8, 6) for p in STREAMED]     # one streamed radix alone on H: the one-radix pass B


def corner_of(hwd):
    def rset(*ns):
        return ALL if any(r in STREAMED for n in ns for r in expected_radices(n)) else SMALL
    return rset(hwd[1], hwd[2]), rset(hwd[0])


# ----------------------------------------------------------------- data and float64 references
def image(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def spectrum(shape, seed):
    rng = np.random.default_rng(seed)   # not Hermitian: the import symmetrises
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def ref_export(x, n_dims):
    ax = tuple(range(-n_dims, 0))
    return np.fft.fftshift(np.fft.fftn(np.asarray(x, np.float64), axes=ax), axes=ax)


def ref_import(k, n_dims):
    ax = tuple(range(-n_dims, 0))
    return np.fft.ifftn(np.fft.ifftshift(np.asarray(k, np.complex128), axes=ax), axes=ax).real


def crelerr(a, b) -> float:
    a, b = np.asarray(a, np.complex128), np.asarray(b, np.complex128)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30))


def mirror_defect(k, n_dims):
    """Elements that differ from the conjugate of their mirror K(-f) (flip and roll by one in the
    unshifted layout), over the columns kd whose mirror is not a stored coefficient of its own (kd != 0,
    and kd != D/2 for even D): there f and -f are the two stores of one value."""
    ax = tuple(range(-n_dims, 0))
    u = np.fft.ifftshift(k, axes=ax)
    m = np.conj(np.roll(np.flip(u, axis=ax), 1, axis=ax))
    D = k.shape[-1]
    kd = [i for i in range(1, D) if 2 * i != D]
    return int(np.count_nonzero(u[..., kd] != m[..., kd]))


# ----------------------------------------------------------------- coverage of the table, from expected_radices
def coverage(lengths=None):
    """What the plans of `lengths` visit: single-stage radices, primes as a non-last / last / middle
    stage (a middle stage has a prefix product P > 1 and a block length L > 1), stage counts."""
    cov = {"single": set(), "non_last": set(), "last": set(), "middle": set(), "stages": set()}
    for n in (LENGTHS if lengths is None else lengths):
        r = expected_radices(n)
        assert r is not None, n
        cov["stages"].add(len(r))
        if len(r) == 1:
            cov["single"].add(r[0])
        else:
            cov["last"].add(r[-1])      # of a plan with stages before it
        cov["non_last"].update(r[:-1])
        cov["middle"].update(r[1:-1])
    return cov
