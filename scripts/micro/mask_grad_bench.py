#!/usr/bin/env python3
"""Mask-gradient pass against the same gradient composed from torch.fft, measurement tool.

At 2 x 4 x 240 x 240 x 155, for a shared mask (Cm = 1) and a per-channel one (Cm = 4):
  ours   runtime.kspace_mask_grad, per stage (tb_set_pass_timing: HIP events around each stage on the
         launch stream; slot 0 = the two forward passes A, slot 1 = k_kspace_maskgrad) and end to end
         (device events around the call)
  fft    rfftn of x and of g over the spatial axes, Re(X conj G) / N, summed over the samples (and the
         channels for Cm = 1), on the same device: the half-spectrum gradient, without the scatter to
         the centred full layout (so it does a little less than `ours`)

One run (--child KIND CM) is one process: warm-up, then --iters timed calls, one JSON line with the
median / min / max.  Without --child the script starts the runs as fresh child processes, `--runs`
rounds alternating ours / fft for both mask kinds, stops at the first child that fails, and prints the
median of the run medians with the min-max spread, the algorithmic bytes (two passes A, two spectrum
reads, Cm H W D 4 written) and the fraction of an 8 TB/s roofline they give.

Usage: python scripts/micro/mask_grad_bench.py [--runs 5] [--iters 20]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "medical-vision-textural-bias_amd"), ROOT):
    sys.path.insert(0, p)

SHAPE = (2, 4, 240, 240, 155)
PEAK = 8.0e12


def algorithmic_bytes(cm: int) -> float:
    B, C, H, W, D = SHAPE
    vox, spec = B * C * H * W * D * 4.0, B * C * H * W * (D // 2 + 1) * 8.0
    return 2.0 * (vox + spec) + 2.0 * spec + cm * H * W * D * 4.0


def child(a) -> None:
    import torch
    from texbias import runtime as rt
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    x, g = torch.randn(SHAPE, device=dev), torch.randn(SHAPE, device=dev)
    cm, n = a.child[1], float(SHAPE[2] * SHAPE[3] * SHAPE[4])
    out = torch.empty(SHAPE[2:] if cm == 1 else (cm,) + SHAPE[2:], device=dev)

    def ours():
        rt.kspace_mask_grad(x, g, 3, cm, out=out)

    def fft():
        X, G = torch.fft.rfftn(x, dim=(-3, -2, -1)), torch.fft.rfftn(g, dim=(-3, -2, -1))
        v = X.real * G.real + X.imag * G.imag
        return (v.sum(dim=(0, 1)) if cm == 1 else v.sum(dim=0)) / n

    fn = ours if a.child[0] == "ours" else fft
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    total, s0, s1 = [], [], []
    if a.child[0] == "ours":
        rt.set_pass_timing(True)
    for _ in range(a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        total.append(e0.elapsed_time(e1) * 1e3)
        if a.child[0] == "ours":
            ms, _, _, names = rt.pass_stats()
            s0.append(ms[0] * 1e3)
            s1.append(ms[1] * 1e3)
    res = {"kind": a.child[0], "cm": cm}
    for k, v in (("total", total), ("fwd", s0), ("maskgrad", s1)):
        if v:
            res[k] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    if a.child[0] == "ours":
        res["kernels"] = names[:2]
    print(json.dumps(res), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--child", nargs=2, default=None)
    a = ap.parse_args()
    if a.child:
        a.child = (a.child[0], int(a.child[1]))
        child(a)
        return
    rows = {}
    for r in range(a.runs):
        for cm in (1, SHAPE[1]):
            for kind in ("ours", "fft"):
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, str(cm), "--iters",
                                    str(a.iters)], capture_output=True, text=True, timeout=300)
                if p.returncode != 0:
                    print(p.stdout[-2000:], p.stderr[-2000:])
                    sys.exit(f"child {kind} {cm} failed with {p.returncode}")
                d = json.loads(p.stdout.strip().splitlines()[-1])
                print(json.dumps(d), flush=True)
                for k in ("total", "fwd", "maskgrad"):
                    if k in d:
                        rows.setdefault((kind, cm, k), []).append(d[k]["median"])
    print("\nmedian of run medians, us (min - max over the runs)")
    for (kind, cm, k), v in sorted(rows.items()):
        print(f"{kind:5s} Cm={cm} {k:9s} {statistics.median(v):9.1f} ({min(v):.1f} - {max(v):.1f})")
    for cm in (1, SHAPE[1]):
        t = statistics.median(rows[("ours", cm, "fwd")]) + statistics.median(rows[("ours", cm, "maskgrad")])
        nb = algorithmic_bytes(cm)
        print(f"Cm={cm}: algorithmic bytes {nb / 1e6:.1f} MB, {nb / PEAK * 1e6:.1f} us at 8 TB/s, stages sum {t:.1f} us: "
              f"{nb / PEAK * 1e6 / t:.3f} of the roofline; composed torch.fft / ours (end to end) "
              f"{statistics.median(rows[('fft', cm, 'total')]) / statistics.median(rows[('ours', cm, 'total')]):.2f}")


if __name__ == "__main__":
    main()
