#!/usr/bin/env python3
"""Pass-B time of the full-spectrum route with and without a user mask (TB_OP_MASK), measurement tool.

Times pass B alone (tb_set_pass_timing: HIP events around the kernel on the launch stream) for
  gibbs   one GIBBS op (the gibbs-aug chain's program; the unrolled single-kind middle phase)
  zf      one ZF op (the generic middle phase, a computed per-coefficient factor)
  mask    one MASK op, one 35.7 MB mask shared by the channels
  maskc   one MASK op, a per-channel mask (4 x 35.7 MB)
  cmask   one CMASK op (--cmask), one 71.4 MB complex64 mask shared by the channels
  cmaskc  one CMASK op, a per-channel complex mask (4 x 71.4 MB)
at the C3 shape 2 x 4 x 240 x 240 x 155 (+5 pad; kernel k_kspace_half), and
  zf_ct   the ZF op at 2 x 4 x 240 x 90 x 60, whose spectrum rows (90 x 31 columns) are no multiple of 32:
          the one-tile-per-workgroup compiled kernel, whose middle phase is the unrolled ops_bfly.

One run (--child) is one process: warm-up, then --iters timed calls per program, interleaved, and the
median / min / max per program as one JSON line.  Without --child the script starts runs as fresh
child processes, `--runs` rounds of: the `--ab OTHER.so` library (e.g. the parent commit's build; with
`--ab-mask` it knows the MASK op and times the mask programs too), the in-tree library on the same
programs, the in-tree library with the mask programs (and with `--cmask` the complex ones) added.  It
stops at the first child that fails and prints the table of per-run medians: median of medians, min-max
spread, the comparison of the unchanged programs and the mask ratios.

A library older than the in-tree Python package lacks the entry points the package binds: `--ab-root DIR`
runs the other library's children on the package of that tree (DIR/medical-vision-textural-bias_amd).

Usage: python scripts/micro/mask_pass_b.py [--ab OTHER.so [--ab-mask] [--ab-root DIR]] [--cmask] [--runs 5] [--iters 30]
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

SHAPE, PAD = (2, 4, 240, 240, 155), 5
SHAPE_CT = (2, 4, 240, 90, 60)


def child(a) -> None:
    if a.root:   # the package that belongs to the library under test
        for p in (a.root, os.path.join(a.root, "medical-vision-textural-bias_amd")):
            sys.path.insert(0, os.path.abspath(p))
    import torch
    from texbias import kprog as K
    from texbias import runtime as rt
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    sp, hwd = SHAPE[2:], K.geometry(SHAPE[2:]).hwd
    data = {}
    for shape, pad in ((SHAPE, PAD), (SHAPE_CT, 0)):
        data[shape] = (torch.randn(shape, device=dev), torch.empty(shape[:-1] + (shape[-1] + pad,), device=dev), pad)
    progs = {"gibbs": (SHAPE, [K.gibbs_op(0.2, sp)]), "zf": (SHAPE, [K.zf_op(0.5, 7, hwd)]),
             "zf_ct": (SHAPE_CT, [K.zf_op(0.5, 7, K.geometry(SHAPE_CT[2:]).hwd)])}
    if a.mask:
        m1 = torch.rand(sp, device=dev)
        m4 = torch.rand((SHAPE[1],) + sp, device=dev)   # the ops hold raw addresses: m1, m4 live to the end
        progs["mask"] = (SHAPE, [K.mask_op(m1.data_ptr(), 1, hwd)])
        progs["maskc"] = (SHAPE, [K.mask_op(m4.data_ptr(), SHAPE[1], hwd)])
    if a.cmask:
        c1 = torch.polar(torch.rand(sp, device=dev), (torch.rand(sp, device=dev) * 2 - 1) * torch.pi)
        c4 = torch.polar(torch.rand((SHAPE[1],) + sp, device=dev),
                         (torch.rand((SHAPE[1],) + sp, device=dev) * 2 - 1) * torch.pi)
        progs["cmask"] = (SHAPE, [K.cmask_op(c1.data_ptr(), 1, hwd)])
        progs["cmaskc"] = (SHAPE, [K.cmask_op(c4.data_ptr(), SHAPE[1], hwd)])

    def call(shape, p):
        x, out, pad = data[shape]
        rt.kspace_filter(x, 3, [p] * shape[0], shape[1], out=out, pad=pad)

    for _ in range(a.warmup):
        for shape, p in progs.values():
            call(shape, p)
    torch.cuda.synchronize()
    rt.set_pass_timing(True)
    us = {k: [] for k in progs}
    kern = {}
    for _ in range(a.iters):
        for name, (shape, p) in progs.items():
            call(shape, p)
            ms, cnt, _, names = rt.pass_stats()   # synchronises on the call's events, then clears
            us[name].append(1e3 * ms[1] / max(cnt[1], 1))
            kern[name] = names[1]
    rt.set_pass_timing(False)
    res = {"lib": a.tag}
    for name, v in us.items():
        res[name] = {"kernel": kern[name], "median_us": round(statistics.median(v), 2),
                     "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
    print("RESULT " + json.dumps(res), flush=True)


def run_child(a, lib, tag, mask, cmask=False, root=None):
    env = dict(os.environ)
    if lib:
        env["TEXBIAS_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tag", tag, "--iters", str(a.iters),
           "--warmup", str(a.warmup)] + (["--mask"] if mask else []) + (["--cmask"] if cmask else []) + \
          (["--root", root] if root else [])
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"child ({tag}) exited with {p.returncode}: no further runs are started")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    print(line, flush=True)
    return json.loads(line[len("RESULT "):])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--mask", action="store_true", help="(child) also time the MASK programs")
    ap.add_argument("--cmask", action="store_true", help="also time the CMASK programs (in-tree library only)")
    ap.add_argument("--ab-mask", action="store_true", help="the --ab library knows the MASK op: compare it there too")
    ap.add_argument("--ab-root", default=None, help="the tree whose Python package goes with the --ab library")
    ap.add_argument("--root", default=None, help="(child) import texbias from this tree")
    ap.add_argument("--tag", default="tree")
    ap.add_argument("--ab", default=None, help="a second libtexbias.so to alternate with (no MASK programs)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    sets = {}
    kinds = ([(a.ab, "other", a.ab_mask, False)] if a.ab else []) + \
            [(None, "tree", a.ab_mask, False), (None, "tree+mask", True, a.cmask)]
    for _ in range(a.runs):
        for lib, tag, mask, cmask in kinds:
            r = run_child(a, lib, tag, mask, cmask, a.ab_root if lib else None)
            for name, v in r.items():
                if name != "lib":
                    sets.setdefault((tag, name), []).append(v["median_us"])
    print("| library | program | median of run medians (us) | min | max | spread |")
    print("|---|---|---|---|---|---|")
    for (tag, name), v in sets.items():
        print(f"| {tag} | {name} | {statistics.median(v):.1f} | {min(v):.1f} | {max(v):.1f} | {max(v) - min(v):.1f} |")
    med = {k: statistics.median(v) for k, v in sets.items()}
    spr = {k: max(v) - min(v) for k, v in sets.items()}
    if a.ab:
        for name in ("gibbs", "zf", "zf_ct") + (("mask", "maskc") if a.ab_mask else ()):
            d = med[("tree", name)] - med[("other", name)]
            lim = max(spr[("tree", name)], spr[("other", name)])
            print(f"{name}: tree - other = {d:+.1f} us, larger spread {lim:.1f} us -> "
                  f"{'within the spread' if abs(d) <= lim else 'faster, outside the spread' if d < 0 else 'SLOWER, outside the spread'}")
    base = med[("other", "zf")] if a.ab else med[("tree", "zf")]
    for name in ("mask", "maskc") + (("cmask", "cmaskc") if a.cmask else ()):
        print(f"{name} / zf ({'other' if a.ab else 'tree'} library): {med[('tree+mask', name)] / base:.3f}x")


if __name__ == "__main__":
    main()
