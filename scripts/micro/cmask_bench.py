#!/usr/bin/env python3
"""The fused complex k-space mask (TB_OP_CMASK) against its alternatives, measurement tool.

At 2 x 4 x 240 x 240 x 155, alternated call by call in the same process on the same device:
  forward   cmask     runtime.kspace_cmask, one mask shared by the channels (71 MB complex64)
            cmaskc    the same with a per-channel mask (4 x 71 MB)
            compose   inv_shift_fourier(shift_fourier(x) * M) on the library's spectrum ops
            fft       ifftn(ifftshift(fftshift(fftn(x)) * M)).real on torch.fft
  gradient  cgrad     runtime.kspace_cmask_grad, shared      cgradc   per channel
            rgrad     runtime.kspace_mask_grad (real mask), shared      rgradc   per channel
            fftgrad   torch.autograd through the torch.fft expression, shared complex leaf
End to end by device events around the call; for the library's own calls also per stage
(tb_set_pass_timing: slot 0 = forward pass(es) A, slot 1 = pass B / the gradient pass, slot 2 = pass C).

One run (--child) is one process: warm-up, then --iters timed calls of each, one JSON line.  Without
--child the script starts --runs fresh child processes, stops at the first that fails, and prints the
median of the run medians with the min-max spread, and the verdict the feature is held to: the fused
median below the composition's by more than the larger of the two spreads.

Usage: python scripts/micro/cmask_bench.py [--runs 5] [--iters 10]
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
DIMS = (-3, -2, -1)
FWD = ("cmask", "cmaskc", "compose", "fft")
GRAD = ("cgrad", "cgradc", "rgrad", "rgradc", "fftgrad")
OURS = ("cmask", "cmaskc", "compose", "cgrad", "cgradc", "rgrad", "rgradc")


def child(a) -> None:
    import torch
    from texbias import runtime as rt
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    sp, Cc = SHAPE[2:], SHAPE[1]
    x = torch.randn(SHAPE, device=dev)
    g = torch.randn(SHAPE, device=dev)
    m1 = torch.polar(torch.rand(sp, device=dev) * 1.5, (torch.rand(sp, device=dev) * 2 - 1) * torch.pi)
    m4 = torch.polar(torch.rand((Cc,) + sp, device=dev) * 1.5, (torch.rand((Cc,) + sp, device=dev) * 2 - 1) * torch.pi)
    yout = torch.empty(SHAPE, device=dev)
    kout = torch.empty(SHAPE, dtype=torch.complex64, device=dev)
    d1 = torch.empty(sp, dtype=torch.complex64, device=dev)
    d4 = torch.empty((Cc,) + sp, dtype=torch.complex64, device=dev)
    r1 = torch.empty(sp, device=dev)
    r4 = torch.empty((Cc,) + sp, device=dev)

    def fftgrad():
        M = m1.detach().clone().requires_grad_(True)
        k = torch.fft.fftshift(torch.fft.fftn(x, dim=DIMS), dim=DIMS)
        y = torch.fft.ifftn(torch.fft.ifftshift(k * M, dim=DIMS), dim=DIMS).real
        return torch.autograd.grad(y, M, g)[0]

    fns = {
        "cmask": lambda: rt.kspace_cmask(x, m1, 3, out=yout),
        "cmaskc": lambda: rt.kspace_cmask(x, m4, 3, out=yout),
        "compose": lambda: rt.kspace_import(rt.kspace_export(x, 3, out=kout) * m1, 3, out=yout),
        "fft": lambda: torch.fft.ifftn(torch.fft.ifftshift(
            torch.fft.fftshift(torch.fft.fftn(x, dim=DIMS), dim=DIMS) * m1, dim=DIMS), dim=DIMS).real,
        "cgrad": lambda: rt.kspace_cmask_grad(x, g, 3, 1, out=d1),
        "cgradc": lambda: rt.kspace_cmask_grad(x, g, 3, Cc, out=d4),
        "rgrad": lambda: rt.kspace_mask_grad(x, g, 3, 1, out=r1),
        "rgradc": lambda: rt.kspace_mask_grad(x, g, 3, Cc, out=r4),
        "fftgrad": fftgrad,
    }
    res = {}
    for group in (FWD, GRAD):
        for name in group:
            for _ in range(2):
                fns[name]()
        torch.cuda.synchronize()
        t = {name: [] for name in group}
        stage = {name: [[], [], []] for name in group if name in OURS}
        kern = {}
        for _ in range(a.iters):
            for name in group:
                ours = name in OURS
                if ours:
                    rt.set_pass_timing(True)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fns[name]()
                e1.record()
                torch.cuda.synchronize()
                t[name].append(e0.elapsed_time(e1) * 1e3)
                if ours:
                    ms, _, _, names = rt.pass_stats()
                    rt.set_pass_timing(False)
                    kern[name] = list(names[:3])
                    for s in range(3):
                        stage[name][s].append(ms[s] * 1e3)
        for name in group:
            res[name] = {"median": statistics.median(t[name]), "min": min(t[name]), "max": max(t[name])}
            if name in OURS:
                res[name]["stages"] = [statistics.median(v) for v in stage[name]]
                res[name]["kernels"] = kern[name]
    print(json.dumps(res), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    rows, kern = {}, {}
    for r in range(a.runs):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--iters", str(a.iters)],
                           capture_output=True, text=True, timeout=300)
        if p.returncode != 0:
            print(p.stdout[-2000:], p.stderr[-2000:])
            sys.exit(f"run {r} failed with {p.returncode}: no further runs are started")
        d = json.loads(p.stdout.strip().splitlines()[-1])
        print(json.dumps(d), flush=True)
        for name in FWD + GRAD:
            rows.setdefault((name, "end to end"), []).append(d[name]["median"])
            if name in OURS:
                kern[name] = d[name]["kernels"]
                for s in range(3):
                    rows.setdefault((name, f"stage{s}"), []).append(d[name]["stages"][s])
    print("\n| call | what | median of run medians (us) | min | max |")
    print("|---|---|---|---|---|")
    for (name, what), v in rows.items():
        k = ""
        if what.startswith("stage") and name in kern:
            k = f" {kern[name][int(what[-1])]}"
        print(f"| {name} | {what}{k} | {statistics.median(v):.1f} | {min(v):.1f} | {max(v):.1f} |")
    med = {k: statistics.median(v) for k, v in rows.items()}
    spr = {k: max(v) - min(v) for k, v in rows.items()}
    for name in ("cmask", "cmaskc"):
        a_, b_ = (name, "end to end"), ("compose", "end to end")
        gain, lim = med[b_] - med[a_], max(spr[a_], spr[b_])
        print(f"{name}: compose - fused = {gain:+.1f} us, larger spread {lim:.1f} us -> "
              f"{'EARNS its place' if gain > lim else 'does NOT earn its place'}; "
              f"compose / fused {med[b_] / med[a_]:.2f}, torch.fft / fused {med[('fft', 'end to end')] / med[a_]:.2f}")
    for name, real in (("cgrad", "rgrad"), ("cgradc", "rgradc")):
        print(f"{name}: torch.fft autograd / ours {med[('fftgrad', 'end to end')] / med[(name, 'end to end')]:.2f}, "
              f"complex / real gradient {med[(name, 'end to end')] / med[(real, 'end to end')]:.3f}")


if __name__ == "__main__":
    main()
