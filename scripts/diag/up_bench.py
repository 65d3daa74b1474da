#!/usr/bin/env python3
"""HIP-event timings of the direct full-resolution stride-2 kernels (csrc/conv_up.hip) at the bench shapes."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "medical-vision-textural-bias_amd"), ROOT]
import argparse  # noqa: E402
import inspect  # noqa: E402

import torch  # noqa: E402

from texbias import conv as C  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--flush", action="store_true", help="write 1 GiB between timed calls (cold L2 / MALL)")
ap.add_argument("--convt", action="store_true", help="only the ConvTranspose3d(64 -> 16) arms: forward, stacked "
                "input gradient, and that gradient + the skip share into a channel slice")
ap.add_argument("--sweep", action="store_true", help="--convt at 2 x 64 x 32 x 32 x W, W = 8 .. 64")
args = ap.parse_args()
_flush = torch.empty(1 << 28, device="cuda") if args.flush else None


def timeit(fn, n=10):
    ts = []
    for _ in range(n + 3):
        if _flush is not None:
            _flush.add_(1.0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts = sorted(ts[3:])
    return ts[len(ts) // 2] * 1e3


def convt_arms(N, D, H, W, tag):
    """FLOP per call: 2 x 64 x 16 x 27 x N D H W (every tap of every input position is one multiply-add)."""
    fl = 2 * 64 * 16 * 27 * N * D * H * W
    x = torch.randn((N, 64, D, H, W), device="cuda")
    w = torch.randn((64, 16, 3, 3, 3), device="cuda")
    t = timeit(lambda: C.convT_mfma(x, w, None))
    print(f"convT 64->16 {tag} {D}x{H}x{W} fwd/dgrad        {t:8.1f} us  {fl / t / 1e6:6.1f} TF/s", flush=True)
    # the level-1 skip share: dX + g into channels [16, 32) of the stacked output-gradient buffer
    wide = torch.randn((N, 32, 2 * D, 2 * H, 2 * W), device="cuda")
    buf = torch.empty_like(wide)
    g = wide[:, :16]
    if "out" in inspect.signature(C.convT_mfma).parameters:
        t = timeit(lambda: C.convT_mfma(x, w, None, add=g, out=buf[:, 16:]))
        print(f"convT 64->16 {tag} {D}x{H}x{W} dgrad + add in store {t:8.1f} us", flush=True)
    t = timeit(lambda: torch.add(C.convT_mfma(x, w, None), g, out=buf[:, 16:]))
    print(f"convT 64->16 {tag} {D}x{H}x{W} dgrad, separate add  {t:8.1f} us", flush=True)


if args.convt or args.sweep:
    if args.sweep:
        for W in (8, 12, 16, 20, 24, 32, 40, 48, 64):
            try:
                convt_arms(2, 32, 32, W, "sweep")
            except RuntimeError as e:  # a width the library refuses
                print(f"convT 64->16 sweep 32x32x{W}: {e}", flush=True)
    else:
        convt_arms(2, 60, 60, 40, "C3")
    sys.exit(0)


x = torch.randn((2, 4, 240, 240, 160), device="cuda")
w = torch.randn((16, 4, 3, 3, 3), device="cuda")
K = C.s2_pairs(w)
t = timeit(lambda: C.conv_s2_fewin(x, K, None, 16))
print(f"conv_s2_fewin 4->16 (entry conv fwd)      {t:8.1f} us  {2 * 16 * 4 * 27 * 2 * 120 * 120 * 80 / t / 1e6:6.1f} TF/s")
xt = torch.randn((2, 32, 120, 120, 80), device="cuda")
wt = torch.randn((32, 3, 3, 3, 3), device="cuda")
t = timeit(lambda: C.convT_fewout(xt, wt, None))
print(f"convT_fewout 32->3 (exit convT fwd)       {t:8.1f} us  {2 * 32 * 3 * 27 * 2 * 120 * 120 * 80 / t / 1e6:6.1f} TF/s")
gy = torch.randn((2, 3, 240, 240, 160), device="cuda")
Kt = C.s2_pairs(wt)
t = timeit(lambda: C.conv_s2_fewin(gy, Kt, None, 32))
print(f"conv_s2_fewin 3->32 (exit convT dgrad)    {t:8.1f} us  {2 * 32 * 3 * 27 * 2 * 120 * 120 * 80 / t / 1e6:6.1f} TF/s")
x16 = torch.randn((2, 16, 120, 120, 80), device="cuda")
w16 = torch.randn((16, 16, 3, 3, 3), device="cuda")
t = timeit(lambda: C.conv_fwd16(x16, w16, None))
print(f"conv_fwd16 16->16 (120x120x80)            {t:8.1f} us  {2 * 16 * 16 * 27 * 2 * 120 * 120 * 80 / t / 1e6:6.1f} TF/s")
t = timeit(lambda: torch.nn.functional.conv3d(x16, w16, None, padding=1))
print(f"  MIOpen conv3d 16->16                    {t:8.1f} us")
x64 = torch.randn((2, 64, 60, 60, 40), device="cuda")
w64 = torch.randn((64, 16, 3, 3, 3), device="cuda")
t = timeit(lambda: C.convT_mfma64(x64, w64, None))
print(f"convT_mfma64 64->16 (up1 convT fwd)       {t:8.1f} us  {2 * 64 * 16 * 27 * 2 * 60 * 60 * 40 / t / 1e6:6.1f} TF/s")
t = timeit(lambda: torch.nn.functional.conv_transpose3d(x64, w64, None, stride=2, padding=1, output_padding=1))
print(f"  MIOpen conv_transpose3d 64->16          {t:8.1f} us")
for ch, sh in ((32, (2, 32, 60, 60, 40)), (64, (2, 64, 30, 30, 20))):
    xc = torch.randn(sh, device="cuda")
    wc = torch.randn((ch, ch, 3, 3, 3), device="cuda")
    fl = 2 * ch * ch * 27 * 2 * sh[2] * sh[3] * sh[4]
    t = timeit(lambda: C.conv_mfma(xc, wc, None))
    print(f"conv_mfma {ch}->{ch} {sh[2:]}        {t:8.1f} us  {fl / t / 1e6:6.1f} TF/s")
    t = timeit(lambda: torch.nn.functional.conv3d(xc, wc, None, padding=1))
    print(f"  MIOpen conv3d {ch}->{ch}                    {t:8.1f} us")
gy32 = torch.randn((2, 32, 60, 60, 40), device="cuda")
w32 = torch.randn((32, 16, 3, 3, 3), device="cuda")
t = timeit(lambda: C.convT_mfma(gy32, w32, None))
print(f"convT_mfma 32->16 (down1 s2 dgrad)        {t:8.1f} us  {2 * 32 * 16 * 27 * 2 * 60 * 60 * 40 / t / 1e6:6.1f} TF/s")
t = timeit(lambda: torch.nn.functional.conv_transpose3d(gy32, w32, None, stride=2, padding=1, output_padding=1))
print(f"  MIOpen conv_transpose3d 32->16          {t:8.1f} us")
