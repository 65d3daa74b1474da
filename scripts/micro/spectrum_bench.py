#!/usr/bin/env python3
"""Centred-spectrum export / import against the same maps composed from torch.fft, measurement tool.

At 2 x 4 x 240 x 240 x 155, three things, each alternated call by call with its torch.fft form on the
same device in the same process:
  export     runtime.kspace_export(x)                       | fftshift(fftn(x))
  import     runtime.kspace_import(k)                       | ifftn(ifftshift(k)).real
  roundtrip  import(export(x) * m), m complex [H, W, D]     | ifftn(ifftshift(fftshift(fftn(x)) * m)).real
End to end by device events around the call; for ours also per stage (tb_set_pass_timing: HIP events
around each stage on the launch stream; slot 0 = forward pass A, slot 1 = k_kspace_export /
k_kspace_import, slot 2 = inverse pass C).

One run (--child) is one process: warm-up, then --iters timed calls of each, one JSON line.  Without
--child the script starts --runs fresh child processes, stops at the first that fails, and prints the
median of the run medians with the min-max spread, the algorithmic bytes (N voxels, N_h = H W (D/2+1)
stored coefficients per volume: export 4N + 8N_h for pass A, 8N_h + 8N for the export pass; import the
mirror image) and the fraction of an 8 TB/s roofline they give.

Usage: python scripts/micro/spectrum_bench.py [--runs 5] [--iters 20]
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
DIMS = (-3, -2, -1)
WHAT = ("export", "import", "roundtrip")


def algorithmic_bytes(what: str) -> float:
    B, C, H, W, D = SHAPE
    n, nh = float(B * C * H * W * D), float(B * C * H * W * (D // 2 + 1))
    one = (4.0 * n + 8.0 * nh) + (8.0 * nh + 8.0 * n)      # slab pass + per-coefficient pass
    if what == "roundtrip":
        return 2.0 * one + 2.0 * 8.0 * n                   # and the multiply: K read, K written (m is small)
    return one


def child(a) -> None:
    import torch
    from texbias import runtime as rt
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    x = torch.randn(SHAPE, device=dev)
    k = torch.randn(SHAPE, device=dev) + 1j * torch.randn(SHAPE, device=dev)
    m = torch.randn(SHAPE[2:], device=dev) + 1j * torch.randn(SHAPE[2:], device=dev)
    kout = torch.empty(SHAPE, dtype=torch.complex64, device=dev)
    yout = torch.empty(SHAPE, device=dev)

    fns = {
        ("export", "ours"): lambda: rt.kspace_export(x, 3, out=kout),
        ("export", "fft"): lambda: torch.fft.fftshift(torch.fft.fftn(x, dim=DIMS), dim=DIMS),
        ("import", "ours"): lambda: rt.kspace_import(k, 3, out=yout),
        ("import", "fft"): lambda: torch.fft.ifftn(torch.fft.ifftshift(k, dim=DIMS), dim=DIMS).real,
        ("roundtrip", "ours"): lambda: rt.kspace_import(rt.kspace_export(x, 3, out=kout) * m, 3, out=yout),
        ("roundtrip", "fft"): lambda: torch.fft.ifftn(torch.fft.ifftshift(
            torch.fft.fftshift(torch.fft.fftn(x, dim=DIMS), dim=DIMS) * m, dim=DIMS), dim=DIMS).real,
    }
    res = {}
    for what in WHAT:
        for kind in ("ours", "fft"):
            for _ in range(3):
                fns[(what, kind)]()
        torch.cuda.synchronize()
        t = {"ours": [], "fft": []}
        stage = [[], [], []]
        for _ in range(a.iters):
            for kind in ("ours", "fft"):
                if kind == "ours":
                    rt.set_pass_timing(True)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fns[(what, kind)]()
                e1.record()
                torch.cuda.synchronize()
                t[kind].append(e0.elapsed_time(e1) * 1e3)
                if kind == "ours":
                    ms, _, _, names = rt.pass_stats()
                    rt.set_pass_timing(False)
                    for s in range(3):
                        stage[s].append(ms[s] * 1e3)
        res[what] = {kind: {"median": statistics.median(v), "min": min(v), "max": max(v)} for kind, v in t.items()}
        res[what]["stages"] = [statistics.median(v) for v in stage]
    print(json.dumps(res), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    rows = {}
    for r in range(a.runs):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--iters", str(a.iters)],
                           capture_output=True, text=True, timeout=300)
        if p.returncode != 0:
            print(p.stdout[-2000:], p.stderr[-2000:])
            sys.exit(f"run {r} failed with {p.returncode}")
        d = json.loads(p.stdout.strip().splitlines()[-1])
        print(json.dumps(d), flush=True)
        for what in WHAT:
            for kind in ("ours", "fft"):
                rows.setdefault((what, kind), []).append(d[what][kind]["median"])
            for s in range(3):
                rows.setdefault((what, f"stage{s}"), []).append(d[what]["stages"][s])
    print("\nmedian of run medians, us (min - max over the runs)")
    for (what, kind), v in sorted(rows.items()):
        print(f"{what:9s} {kind:7s} {statistics.median(v):9.1f} ({min(v):.1f} - {max(v):.1f})")
    for what in WHAT:
        ours, fft = statistics.median(rows[(what, "ours")]), statistics.median(rows[(what, "fft")])
        t = sum(statistics.median(rows[(what, f"stage{s}")]) for s in range(3))
        nb = algorithmic_bytes(what)
        print(f"{what}: algorithmic bytes {nb / 1e6:.1f} MB, {nb / PEAK * 1e6:.1f} us at 8 TB/s; stages sum {t:.1f} us; "
              f"end to end {nb / PEAK * 1e6 / ours:.3f} of the roofline; torch.fft / ours {fft / ours:.2f}")


if __name__ == "__main__":
    main()
