#!/usr/bin/env python3
"""Radial reductions (shell power spectrum, profile gradient) against their composed forms, measurement tool.

At 2 x 4 x 240 x 240 x 155 with K = 188 bins, dr = 1, linear weights, a shared profile for the gradient:
  power     fused     runtime.radial_power (pass A, k_radial_power, k_radial_sum)
            composed  the same call after set_radial_fused(False): the mask gradient with g = x into the
                      workspace one sample at a time, then k_radial_bin
            fft       torch.fft.fftn -> abs()**2 -> index_add with precomputed bins and weights
  gradient  fused     runtime.radial_grad (two passes A, k_radial_grad, k_radial_sum)
            composed  after set_radial_fused(False): k_kspace_maskgrad writes dM, k_radial_bin reads it
            fft       fftn of x and g -> Re(X conj G) summed over samples and channels -> index_add
            maskgrad  runtime.kspace_mask_grad alone (Cm = 1), the parent's pass, measured in the same session
Per stage (tb_set_pass_timing: HIP events around each stage on the launch stream; slot 0 = passes A, slot 1 =
the per-coefficient pass, slot 2 = the ordered sum / the dense bin reduction) and end to end (device events
around the call).

One run (--child WHAT KIND) is one process: warm-up, then --iters timed calls, one JSON line with the median /
min / max.  Without --child the script starts the runs as fresh child processes, `--runs` rounds alternating
the variants, stops at the first child that fails, and prints the median of the run medians with the min-max
spread.

Usage: python scripts/micro/radial_bench.py [--runs 5] [--iters 20]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "medical-vision-textural-bias_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

SHAPE = (2, 4, 240, 240, 155)
K, DR, MODE = 188, 1.0, 1
VARIANTS = [("power", "fused"), ("power", "composed"), ("power", "fft"),
            ("grad", "fused"), ("grad", "composed"), ("grad", "fft"), ("grad", "maskgrad")]


def child(a) -> None:
    import numpy as np
    import torch
    from texbias import runtime as rt
    what, kind = a.child
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    x, g = torch.randn(SHAPE, device=dev), torch.randn(SHAPE, device=dev)
    n = float(SHAPE[2] * SHAPE[3] * SHAPE[4])
    ax = (-3, -2, -1)
    if kind == "fft":
        import _radial_ref as R
        b0, w0, w1 = R.weights(SHAPE[2:], K, DR, MODE)
        b0 = np.fft.ifftshift(b0)                                  # unshifted layout: no fftshift of the spectrum
        w0, w1 = np.fft.ifftshift(w0), np.fft.ifftshift(w1)
        i0 = torch.from_numpy(b0.reshape(-1)).to(dev)
        i1 = torch.from_numpy(np.minimum(b0 + 1, K - 1).reshape(-1)).to(dev)
        t0, t1 = torch.from_numpy(w0.reshape(-1)).to(dev), torch.from_numpy(w1.reshape(-1)).to(dev)
    if kind == "composed":
        rt.set_radial_fused(False)
    out_p = torch.empty(SHAPE[:2] + (K,), device=dev)
    out_g = torch.empty((K,), device=dev)
    out_m = torch.empty(SHAPE[2:], device=dev)

    def binned(v):                                                 # v [rows, N] -> [rows, K]
        q = torch.zeros((v.shape[0], K), device=dev)
        return q.index_add_(1, i0, v * t0).index_add_(1, i1, v * t1)

    def power():
        if kind == "fft":
            X = torch.fft.fftn(x, dim=ax)
            return binned((X.real ** 2 + X.imag ** 2).reshape(SHAPE[0] * SHAPE[1], -1)) / n
        return rt.radial_power(x, 3, K, DR, MODE, out=out_p)

    def grad():
        if kind == "fft":
            X, G = torch.fft.fftn(x, dim=ax), torch.fft.fftn(g, dim=ax)
            return binned((X.real * G.real + X.imag * G.imag).sum(dim=(0, 1)).reshape(1, -1)) / n
        if kind == "maskgrad":
            return rt.kspace_mask_grad(x, g, 3, 1, out=out_m)
        return rt.radial_grad(x, g, 3, 1, K, DR, MODE, out=out_g)

    fn = power if what == "power" else grad
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    total, stages = [], [[], [], []]
    ours = kind != "fft"
    if ours:
        rt.set_pass_timing(True)
    for _ in range(a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        total.append(e0.elapsed_time(e1) * 1e3)
        if ours:
            ms, _, _, names = rt.pass_stats()
            for s in range(3):
                stages[s].append(ms[s] * 1e3)
    res = {"what": what, "kind": kind}
    for k, v in (("total", total), ("s0", stages[0]), ("s1", stages[1]), ("s2", stages[2])):
        if v:
            res[k] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    if ours:
        res["kernels"] = names[:3]
    print(json.dumps(res), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--child", nargs=2, default=None)
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    rows = {}
    for r in range(a.runs):
        for what, kind in VARIANTS:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, kind, "--iters", str(a.iters)],
                               capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                print(p.stdout[-2000:], p.stderr[-2000:])
                sys.exit(f"child {what} {kind} failed with {p.returncode}")
            d = json.loads(p.stdout.strip().splitlines()[-1])
            print(json.dumps(d), flush=True)
            for k in ("total", "s0", "s1", "s2"):
                if k in d:
                    rows.setdefault((what, kind, k), []).append(d[k]["median"])
    print("\nmedian of run medians, us (min - max over the runs)")
    for (what, kind, k), v in sorted(rows.items()):
        print(f"{what:5s} {kind:8s} {k:5s} {statistics.median(v):9.1f} ({min(v):.1f} - {max(v):.1f})")


if __name__ == "__main__":
    main()
