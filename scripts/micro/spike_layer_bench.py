#!/usr/bin/env python3
"""The trainable spike layer against the paths it replaces, measurement tool.

At 2 x 1 x 240 x 240 x 155 (the spike drivers are one-channel) and 2 x 4 x 240 x 240 x 155, one spike:
  fwdC   new       runtime.kspace_spikes (k_point_dft, k_spike_delta, k_point_apply): the intensity read on the device
         host      runtime.kspace_filter with the host program of the same spike (k_point_dft, k_point_delta,
                   k_point_apply), the parent's forward -- two of the three kernels are shared
  bwdC   dI        runtime.kspace_spikes_grad, intensity gradient alone (k_point_dft on g, k_spike_gamma,
                   k_spike_dI_sum): 4 N bytes
         dI_gx     the same with the image gradient (+ k_point_apply on g): 4 N + 8 N bytes
  train  learned   one TrainStep of a U-Net behind a LearnedSpikeLayer (analytic intensity gradient)
         spike_gd  the parent's step: TrainStep of Spikes_UNet, then train.spike_gd (two more forwards of filter and
                   U-Net); both at the drivers' crop 2 x 1 x 128 x 128 x 64 (bench.py --model spike-layer)
Per stage (tb_set_pass_timing: slot 0 = k_point_dft, slot 1 = the coefficient kernel, slot 2 = k_point_apply,
slot 3 = k_spike_dI_sum), end to end (device events around the call) and on the host alone ("host": wall time
until the call has returned, launches queued but not waited for).

One run (--child WHAT KIND) is one process: warm-up, then --iters timed calls, one JSON line with the median /
min / max.  Without --child the script starts the runs as fresh child processes, `--runs` rounds alternating
the variants, stops at the first child that fails, and prints the median of the run medians with the min-max
spread.

Usage: python scripts/micro/spike_layer_bench.py [--runs 5] [--iters 20] [--only fwd,bwd,train]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "medical-vision-textural-bias_amd"), ROOT):
    sys.path.insert(0, p)

SPATIAL = (240, 240, 155)
CROP = (2, 1, 128, 128, 64)
LOC = (100, 131, 60)
LOG_I = 11.0
VARIANTS = [("fwd1", "new"), ("fwd1", "host"), ("fwd4", "new"), ("fwd4", "host"),
            ("bwd1", "dI"), ("bwd1", "dI_gx"), ("bwd4", "dI"), ("bwd4", "dI_gx"),
            ("train", "learned"), ("train", "spike_gd")]


def child(a) -> None:
    what, kind = a.child
    if what == "train":
        import bench  # noqa: F401 - the seeded MIOpen databases, before torch starts MIOpen
    import torch
    from texbias import kprog as K
    from texbias import runtime as rt
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    timed = what != "train"
    if what == "train":
        import stylization_layers as SL
        from texbias.spikes import LearnedSpikeLayer
        from texbias.train import TrainStep, spike_gd
        from texbias.unet import UNet
        x = torch.randn(CROP, device=dev)
        y = (torch.rand(CROP, device=dev) > 0.5).float()
        torch.backends.cudnn.benchmark = True

        class LearnedSpikesUNet(torch.nn.Module):   # Spikes_UNet with the trainable layer in front
            def __init__(self):
                super().__init__()
                self.spike = LearnedSpikeLayer(LOG_I, seed=0)
                self.ResUnet = UNet(dimensions=3, in_channels=1, out_channels=1, channels=(16, 32, 64, 128, 256),
                                    strides=(2, 2, 2, 2), num_res_units=2)

            def forward(self, img):
                return self.ResUnet(self.spike(img))

        if kind == "learned":
            step = TrainStep(LearnedSpikesUNet(), dev)

            def fn():
                return step(x, y)
        else:
            step = TrainStep(SL.Spikes_UNet(LOG_I), dev)

            def fn():
                loss = step(x, y)
                spike_gd(x, y, step.model, step.loss_fn)
                return loss
    else:
        C = int(what[-1])
        shape = (2, C) + SPATIAL
        x, g = torch.randn(shape, device=dev), torch.randn(shape, device=dev)
        logi = torch.full((1,), LOG_I, device=dev)
        flat = list(LOC)
        if what.startswith("fwd"):
            prog = [[K.spike_op(LOC, K.geometry(SPATIAL), LOG_I)]] * 2

            def fn():
                if kind == "host":
                    return rt.kspace_filter(x, 3, prog, C)
                return rt.kspace_spikes(x, logi, flat, 3, C)
        else:
            coef = rt.kspace_spikes(x, logi, flat, 3, C)[1]
            gx = torch.empty(shape, device=dev)
            dI = torch.empty((1,), device=dev)

            def fn():
                return rt.kspace_spikes_grad(g, coef, logi, flat, 3, C, kind == "dI_gx", True, gx_out=gx, dI_out=dI)

    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    total, host, stages = [], [], [[], [], [], []]
    if timed:
        rt.set_pass_timing(True)
    for _ in range(a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        fn()
        host.append((time.perf_counter() - t0) * 1e6)
        e1.record()
        torch.cuda.synchronize()
        total.append(e0.elapsed_time(e1) * 1e3)
        if timed:
            ms, _, _, names = rt.pass_stats()
            for s in range(4):
                stages[s].append(ms[s] * 1e3)
    res = {"what": what, "kind": kind}
    for k, v in (("total", total), ("host", host), ("s0", stages[0]), ("s1", stages[1]), ("s2", stages[2]),
                 ("s3", stages[3])):
        if v:
            res[k] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    if timed:
        res["kernels"] = names[:4]   # a slot's name outlives its launches: s3 = 0 means the slot was not used
    print(json.dumps(res), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", type=str, default="fwd,bwd,train")
    ap.add_argument("--child", nargs=2, default=None)
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    only = tuple(a.only.split(","))
    rows = {}
    for r in range(a.runs):
        for what, kind in VARIANTS:
            if not what.startswith(only):
                continue
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, kind, "--iters", str(a.iters)],
                               capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                print(p.stdout[-2000:], p.stderr[-2000:])
                sys.exit(f"child {what} {kind} failed with {p.returncode}")
            d = json.loads(p.stdout.strip().splitlines()[-1])
            print(json.dumps(d), flush=True)
            for k in ("total", "host", "s0", "s1", "s2", "s3"):
                if k in d:
                    rows.setdefault((what, kind, k), []).append(d[k]["median"])
    print("\nmedian of run medians, us (min - max over the runs)")
    for (what, kind, k), v in sorted(rows.items()):
        print(f"{what:5s} {kind:8s} {k:5s} {statistics.median(v):9.1f} ({min(v):.1f} - {max(v):.1f})")


if __name__ == "__main__":
    main()
