#!/usr/bin/env python3
"""HIP-event timings of the four deep transposed-conv products of the C3 step (batch 2), one arm per process:

  up2 fwd   ConvTranspose3d(128 -> 32) forward at 30 x 30 x 20 (with bias)
  dn2 dx    the stacked Conv3d(32 -> 128, stride 2)'s input gradient = convT 128 -> 32 at 30 x 30 x 20
  up3 fwd   ConvTranspose3d(384 -> 64) forward at 15 x 15 x 10 (with bias)
  dn3 dx    the stacked Conv3d(64 -> 256, stride 2)'s input gradient = convT 256 -> 64 at 15 x 15 x 10

Arms: ``aten`` (the route without texbias.conv.CONVT_STACK: MIOpen / CK, with bench.py's seeded find db and
cudnn.benchmark), ``stack`` (k_convT_stack), and for the two input gradients ``stack_add`` (the skip share summed in
the kernel's store, written into a channel slice of the upstream buffer) against ``stack_sepadd`` (kernel, then one
torch.add into that slice) and ``aten_sepadd``.  Protocol of profiles/r21: 1 GiB written between calls, events
around one call, 3 warm-up + 10 timed calls; prints median, min and max in us.  ``--split N`` forces N k slices."""
import argparse
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "medical-vision-textural-bias_amd"), ROOT]
_seed = os.path.join(ROOT, "miopen_db")
_user = os.path.join(_seed, "user")
os.makedirs(_user, exist_ok=True)
os.makedirs(os.path.join(_seed, "kcache"), exist_ok=True)
for _n in os.listdir(_seed):
    if _n.endswith("db.txt") and not os.path.exists(os.path.join(_user, _n)):
        shutil.copyfile(os.path.join(_seed, _n), os.path.join(_user, _n))
os.environ.setdefault("MIOPEN_USER_DB_PATH", _user)
os.environ.setdefault("MIOPEN_CUSTOM_CACHE_DIR", os.path.join(_seed, "kcache"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from texbias import conv as C  # noqa: E402
from texbias._lib import lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--arm", required=True, choices=["aten", "stack", "stack_add", "stack_sepadd", "aten_sepadd"])
ap.add_argument("--split", type=int, default=0)
ap.add_argument("--calls", type=int, default=10)
args = ap.parse_args()
torch.backends.cudnn.benchmark = True
lib().tb_convT3d_stack_set_split(args.split)
_flush = torch.empty(1 << 28, device="cuda")

CALLS = [("up2 fwd", 128, 32, (30, 30, 20), True), ("dn2 dx", 128, 32, (30, 30, 20), False),
         ("up3 fwd", 384, 64, (15, 15, 10), True), ("dn3 dx", 256, 64, (15, 15, 10), False)]


def timeit(fn, n):
    ts = []
    for _ in range(n + 3):
        _flush.add_(1.0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts = sorted(ts[3:])
    return ts[len(ts) // 2], ts[0], ts[-1]


for name, cin, cout, sp, fwd in CALLS:
    N = 2
    if fwd and args.arm in ("stack_add", "stack_sepadd", "aten_sepadd"):
        continue
    x = torch.randn((N, cin) + sp, device="cuda")
    w = torch.randn((cin, cout, 3, 3, 3), device="cuda") * (1.0 / (8 * cin) ** 0.5)
    b = torch.randn(cout, device="cuda") if fwd else None
    osp = tuple(2 * n for n in sp)
    wide = torch.randn((N, 2 * cout) + osp, device="cuda")   # the skip concatenation's gradient; [:, :cout] the share
    buf = torch.empty_like(wide)                             # the upstream unit's stacked output-gradient buffer
    xin = torch.empty((N, cout) + osp, device="cuda")        # the stride-2 conv's input (its shape only)
    if args.arm == "aten":
        if fwd:
            fn = lambda: F.conv_transpose3d(x, w, b, stride=2, padding=1, output_padding=1)  # noqa: E731
        else:
            fn = lambda: torch.ops.aten.convolution_backward(  # noqa: E731
                x, xin, w, None, [2] * 3, [1] * 3, [1] * 3, False, [0] * 3, 1, [True, False, False])[0]
    elif args.arm == "aten_sepadd":
        fn = lambda: torch.add(torch.ops.aten.convolution_backward(  # noqa: E731
            x, xin, w, None, [2] * 3, [1] * 3, [1] * 3, False, [0] * 3, 1, [True, False, False])[0], wide[:, :cout],
            out=buf[:, cout:])
    elif args.arm == "stack":
        fn = lambda: C.convT_stack(x, w, b)  # noqa: E731
    elif args.arm == "stack_add":
        fn = lambda: C.convT_stack(x, w, None, add=wide[:, :cout], out=buf[:, cout:])  # noqa: E731
    else:
        fn = lambda: torch.add(C.convT_stack(x, w, None), wide[:, :cout], out=buf[:, cout:])  # noqa: E731
    med, lo, hi = timeit(fn, args.calls)
    fl = 2 * cin * cout * 27 * N * sp[0] * sp[1] * sp[2]
    ns = C.convT_stack_config(x.shape, cout)["nsplit"] if args.arm.startswith("stack") else 0
    print(f"{name:8s} {args.arm:12s} slices {ns}  median {med:8.1f} us  min {lo:8.1f}  max {hi:8.1f}  "
          f"{fl / med / 1e6:6.1f} TF/s", flush=True)
