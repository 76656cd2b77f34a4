#!/usr/bin/env python3
"""What the trunk audit costs and what it reports, on one MI355X, in one command.

At BASELINE config c2 (512^2, K = 3, 8192 pixel rows + 2 patches of 96^2, fixed-seed trunks; a 'val' / 'train' iteration runs the
contextual VGG19[0:18] on 12 patches of which 6 carry a gradient):

  1. the census launches alone (npp_trunk16_census incl. its memset) on what a real forward of the contextual trunk stored, with
     and without the fp32 partner: device events around `--reps` passes over all stored layers, median of `--windows` such windows;
     the bytes scanned (the 16-byte units of the counted images' position range, border units included: the launch skips them
     without loading) and the GB/s, next to the HBM figures of MI355X_MICROARCH.md (8.0 TB/s spec, 6.29 TB/s measured float4 copy);
  2. an audited iteration against an unaudited one: three fits in ALTERNATED windows of one process -- unaudited twice (A, A': the
     A/A spread of the yardstick) and trunk_audit = 1 -- wall time per iteration with one synchronisation per window (an audit
     reads its records back, so the audited loop synchronises anyway);
  3. the reports of a `--fit_iters`-iteration fit audited every `--every` iterations: flags, per term the worst and the median
     dx_gap, per layer the worst share of flipped gates and the values at fp16's limits;
  4. switch off: the unaudited loop of THIS tree against a checkout of the parent commit (`--parent DIR`, built), each in fresh child
     processes run alternately (this, parent, parent, this, this, parent, ...; `--rounds` of each): per process the median window, then the range
     of the medians of one tree's processes (A/A) beside the difference between the trees.  Nothing new runs with the switch off, so the difference
     must lie inside the parent's own A/A spread.

Nothing here is a gate.

    python tools/trunk_audit_time.py [--windows 5] [--iters 100] [--warm 150] [--parent DIR] [--out profiles/trunk_audit_time.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the unaudited loop, for a child process of either tree: NPP_TIME_ROOT is the tree, argv = windows iters warm
CHILD = r"""
import json, os, sys, time
sys.path.insert(0, os.environ["NPP_TIME_ROOT"])
import numpy as np, torch
from npp_amd import synthetic as syn
from npp_amd.fit import CompletionFit
windows, iters, warm = (int(v) for v in sys.argv[1:4])
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
img, mask = syn.synthetic_image(512)
a, p, s = syn.synthetic_periodicity(512, 3)
f = CompletionFit(img, mask, a, p, syn.SEED0_FREQS, syn.init_params(3, seed=0), device=dev, N_rand=8192, shifts=s, seed=0, rng_mode="device")
for _ in range(warm):
    f.step_full()
ts = []
for _ in range(windows):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        f.step_full()
    torch.cuda.synchronize()
    ts.append((time.perf_counter() - t0) / iters * 1e3)
f.close()
print("RESULT " + json.dumps(ts))
"""


def fmt(ts):
    return f"{float(np.median(ts)):8.4f} ({min(ts):7.4f}..{max(ts):7.4f})"


def make(dev, audit, H=512, K=3):
    from npp_amd import synthetic as syn
    from npp_amd.fit import CompletionFit
    img, mask = syn.synthetic_image(H)
    angles, periods, shifts = syn.synthetic_periodicity(H, K)
    return CompletionFit(img, mask, angles, periods, syn.SEED0_FREQS, syn.init_params(K, seed=0), device=dev, N_rand=8192, shifts=shifts,
                         seed=0, rng_mode="device", trunk_audit=audit)


def census_time(lines, dev, windows, reps):
    import torch
    from npp_amd import ops
    from npp_amd._lib import TRUNK_CENSUS_WORDS
    from npp_amd.losses import ContextualLoss
    N, n, P = 12, 6, 96
    xy = torch.rand((N, 3, P, P), generator=torch.Generator().manual_seed(0)).to(dev)
    cx16 = ContextualLoss(use_vgg=True, device=dev).to(dev)
    cx32 = ContextualLoss(use_vgg=True, device=dev, trunk_precision="fp32").to(dev)
    sc, sh = cx16.input_norm()
    t16, t32 = cx16.hip_trunk, cx32.hip_trunk
    t16._forward(xy, sc, sh, n_keep=n)
    t32._forward(xy, sc, sh, n_keep=n)
    cen = t16.census(ref=t32)
    items = [(t16._x0[0], 16, 3, P, P, None)] + [(y, c, c, H, W, t32._acts[j]) for j, (y, c, H, W) in enumerate(t16._geom)]
    # 16-byte units of the scanned range: the chunks with a true channel x the counted images' padded positions
    scanned = sum(((c_real + 7) // 8) * n * (H + 2) * (W + 2) * 16 for _, _, c_real, H, W, _ in items)
    counted = sum(L["elements"] for L in cen.values()) * 2
    rec = torch.empty((len(items), TRUNK_CENSUS_WORDS), dtype=torch.int64, device=dev)
    for with_ref in (False, True):
        ts = []
        for _ in range(windows):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(reps):
                for i, (y, c, c_real, H, W, partner) in enumerate(items):
                    ops.trunk16_census(y, N, n, c, c_real, H, W, partner if with_ref else None, rec[i])
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) / reps * 1e3)
        med = float(np.median(ts))
        extra = counted * 2 if with_ref else 0                     # the partner's fp32 values of the counted elements
        lines.append(f"census of {len(items)} stored tensors ({n} of {N} patches of {P}^2, {'with' if with_ref else 'without'} the fp32 partner): "
                     f"{scanned / 1e6:.1f} MB of units scanned ({counted / 1e6:.1f} MB counted{f', + {extra / 1e6:.1f} MB of fp32 partner' if extra else ''}), "
                     f"{fmt(ts)} us for the {len(items)} launches ({med / len(items):.1f} us per memset + launch, the largest tensor "
                     f"{max(((cr + 7) // 8) * n * (H + 2) * (W + 2) * 16 for _, _, cr, H, W, _ in items) / 1e6:.1f} MB) = {(scanned + extra) / med / 1e3:.0f} GB/s "
                     f"(HBM: 8000 GB/s spec, 6290 GB/s measured float4 copy; {TRUNK_CENSUS_WORDS} record words per tensor)")


def audited_vs_not(lines, dev, windows, iters, warm):
    import torch
    fits = {"unaudited A": make(dev, 0), "unaudited A'": make(dev, 0), "audited": make(dev, 1)}
    try:
        for f in fits.values():
            for _ in range(warm):
                f.step_full()
        t = {k: [] for k in fits}
        for _ in range(windows):
            for k, f in fits.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(iters):
                    f.step_full()
                torch.cuda.synchronize()
                t[k].append((time.perf_counter() - t0) / iters * 1e3)
        for k in fits:
            lines.append(f"{k:13s} {fmt(t[k])} ms per iteration")
        ma, mb, mg = (float(np.median(t[k])) for k in fits)
        lines.append(f"A/A spread of the unaudited loop {abs(ma - mb):.4f} ms; an audit adds {mg - ma:+.4f} ms to its iteration "
                     f"(the exact-fp32 twins' forward and backward, the census launches, one export and two norms per layer, read-backs)")
    finally:
        for f in fits.values():
            f.close()


def fit_summary(lines, dev, fit_iters, every):
    f = make(dev, every)
    try:
        for _ in range(fit_iters):
            f.step_full()
        reps = list(f.trunk_audits)
    finally:
        f.close()
    lines.append(f"{fit_iters} iterations audited every {every}: {len(reps)} reports, {sum(bool(r['flags']) for r in reps)} flagged 'saturated' "
                 f"(iterations {[r['iteration'] for r in reps if r['flags']][:12]})")
    for term in ("contextual", "lpips", "style"):
        rs = [r["terms"][term] for r in reps if term in r["terms"]]
        if not rs:
            continue
        g = [t["dx_gap"] for t in rs]
        lines.append(f"  {term}: {len(rs)} audits, dx_gap worst {max(g):.3e}  median {float(np.median(g)):.3e}")
        for name in rs[0]["layers"]:
            Ls = [t["layers"][name] for t in rs if name in t["layers"]]
            share = [100.0 * L["gate_flips"] / max(L["elements"], 1) for L in Ls]
            fg = [L["feat_gap"] for L in Ls if L["feat_gap"] is not None]
            lines.append(f"    {name:8s} flipped gates worst {max(share):.3f} % median {float(np.median(share)):.3f} %, feat_gap worst "
                         f"{(max(fg) if fg else float('nan')):.3e}, at_max worst {max(L['at_max'] for L in Ls)}, nonfinite {max(L['nonfinite'] for L in Ls)}, "
                         f"subnormal median {int(np.median([L['subnormal'] for L in Ls]))} of {Ls[0]['elements']}")


def switch_off(lines, parent, windows, iters, warm, rounds=4):
    trees = {"this tree": ROOT, "parent": os.path.abspath(parent)}
    meds = {k: [] for k in trees}
    for r in range(rounds):
        # (the order within a pair alternates, so that neither tree always runs on the device the other has just left)
        for k, root in (list(trees.items())[::-1] if r % 2 else trees.items()):
            env = dict(os.environ, NPP_TIME_ROOT=root)
            p = subprocess.run([sys.executable, "-c", CHILD, str(windows), str(iters), str(warm)], env=env, cwd=root, capture_output=True,
                               text=True, timeout=600)
            res = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not res:
                lines.append(f"switch off: the child process of {k} failed ({p.returncode}): {p.stderr.strip()[-300:]}")
                return
            ts = json.loads(res[-1][7:])
            meds[k].append(float(np.median(ts)))
            lines.append(f"{k:10s} process {len(meds[k])}: {fmt(ts)} ms per iteration")
    aa = {k: max(v) - min(v) for k, v in meds.items()}                # (range of the processes' medians)
    diff = float(np.mean(meds["this tree"]) - np.mean(meds["parent"]))
    lines.append(f"switch off: A/A spread between processes: parent {aa['parent']:.4f} ms, this tree {aa['this tree']:.4f} ms; this tree - parent "
                 f"{diff:+.4f} ms ({'within' if abs(diff) <= aa['parent'] else 'outside'} the parent's A/A spread)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100, help="iterations per window")
    ap.add_argument("--warm", type=int, default=150, help="iterations before the first window")
    ap.add_argument("--reps", type=int, default=50, help="census passes per window")
    ap.add_argument("--fit_iters", type=int, default=2000, help="iterations of the audited fit of part 3 (the default length of a c2 fit)")
    ap.add_argument("--every", type=int, default=20)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (part 4; left out without it)")
    ap.add_argument("--rounds", type=int, default=4, help="child processes per tree in part 4 (the A/A spread is the range of their medians)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def progress(what):                                           # (the report itself is printed once, at the end)
        print(f"[trunk_audit_time] {what}", file=sys.stderr, flush=True)
    if args.parent:                                               # first: this process has not touched the GPU yet
        lines.append("== 4. switch off: the unaudited loop, this tree against the parent commit (child processes, alternated)")
        switch_off(lines, args.parent, args.windows, args.iters, args.warm, args.rounds)
        progress("part 4 done")
    sys.path.insert(0, ROOT)
    import torch
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lines.insert(0, f"trunk_audit_time: {torch.cuda.get_device_name(dev)}; c2 (512^2, K = 3, 8192 rows + 2 patches of 96^2); medians of "
                    f"{args.windows} windows (min..max)")
    lines.append(f"== 1. the census launches ({args.reps} passes over the stored tensors per window)")
    census_time(lines, dev, args.windows, args.reps)
    progress("part 1 done")
    lines.append(f"== 2. audited against unaudited iterations (alternated windows of {args.iters} iterations, {args.warm} before the first)")
    audited_vs_not(lines, dev, args.windows, args.iters, args.warm)
    progress("part 2 done")
    lines.append("== 3. what a fit's audits report (synthetic lattice)")
    fit_summary(lines, dev, args.fit_iters, args.every)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
