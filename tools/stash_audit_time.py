#!/usr/bin/env python3
"""What the stash audit costs and what it reports, on one MI355X, in one command.

At BASELINE config c2 (512^2, K = 3, 8192 pixel rows + 2 patches of 96^2 = 26 624 rows, fixed-seed trunks):

  1. the census launch alone (npp_stash8_census incl. its two memsets) on the workspace of a real iteration, W = 256 and 512: device
     events around `--reps` back-to-back launches, median of `--windows` such windows; the bytes it scans and the GB/s, next to the
     HBM figures of MI355X_MICROARCH.md (8.0 TB/s spec, 6.29 TB/s measured float4 copy);
  2. an audited iteration against an unaudited one: three fits in ALTERNATED windows of one process -- unaudited twice (A, A': the A/A
     spread of the yardstick) and stash_audit = 1 -- wall time per iteration with one synchronisation per window (an audit reads its
     record back, so the audited loop synchronises anyway);
  3. the reports of a `--fit_iters`-iteration fit audited every `--every` iterations: per tensor the worst and the median gradient gap,
     the codes at the formats' limits, the range of the tile scales, the iterations flagged "saturated";
  4. switch off: the unaudited loop of THIS tree against a checkout of the parent commit (`--parent DIR`, built), each in fresh child
     processes run alternately (this, parent, this, parent, ...): per process the median window, then the spread between the two
     processes of one tree (A/A) beside the difference between the trees.  Nothing new runs with the switch off, so the difference
     must lie inside the parent's own A/A spread.

Nothing here is a gate.

    python tools/stash_audit_time.py [--windows 5] [--iters 100] [--warm 150] [--parent DIR] [--out profiles/stash_audit_time.txt]
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
                         seed=0, rng_mode="device", stash_audit=audit)


def census_time(lines, dev, windows, reps):
    import torch
    from npp_amd import ops, synthetic as syn
    from npp_amd._lib import census_layout
    from npp_amd.model import NPPNet
    n, K, H = 8192 + 2 * 96 * 96, 3, 512
    bp = ops.pad_rows(n)
    for W in (256, 512):
        angles, periods, _ = syn.synthetic_periodicity(H, K)
        net = NPPNet(angles, periods, syn.SEED0_FREQS, (H, H), params=syn.init_params(K, seed=0, width=W), device=dev, width=W)
        rng = np.random.RandomState(0)
        c = np.zeros((bp, 2), np.int32)
        c[:n] = np.stack([rng.randint(0, H, n), rng.randint(0, H, n)], 1)
        net.zero_grad()
        net.forward_train(torch.from_numpy(c).to(dev))
        ws = net.workspace(bp)
        ws["dpred"].zero_()
        net.pixel_loss(bp, n, torch.from_numpy(rng.rand(n, 3).astype(np.float32)).to(dev))
        net.backward(bp)
        rec = ops.stash8_census(ws["actT"], ws["dzT"], bp, n, K, None, W)
        arrays, _ = ops.census_decode(rec.cpu().numpy(), K, W)
        # bytes the launch reads: every 16-byte piece with a counted byte -- whole arrays but for the padding rows
        scanned = sum((a["features"] + 15) // 16 * 16 for a in arrays.values()) * n
        ts = []
        for _ in range(windows):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(reps):
                ops.stash8_census(ws["actT"], ws["dzT"], bp, n, K, rec, W)
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) / reps * 1e3)
        med = float(np.median(ts))
        lines.append(f"census W = {W}: {len(arrays)} arrays, {n} rows, {scanned / 1e6:.1f} MB scanned, {fmt(ts)} us per launch "
                     f"= {scanned / med / 1e3:.0f} GB/s (HBM: 8000 GB/s spec, 6290 GB/s measured float4 copy; {census_layout(K, W)[2]} record words)")
        del net


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
                     f"(census, read-back, the 16-bit leg's three launches, {len(fits['audited'].net.layout)} x 2 norms)")
    finally:
        for f in fits.values():
            f.close()


def fit_summary(lines, dev, fit_iters, every):
    f = make(dev, every)
    try:
        for _ in range(fit_iters):
            f.step_full()
        reps = list(f.stash_audits)
    finally:
        f.close()
    lines.append(f"{fit_iters} iterations audited every {every}: {len(reps)} reports, {sum(bool(r['flags']) for r in reps)} flagged 'saturated' "
                 f"(iterations {[r['iteration'] for r in reps if r['flags']][:12]})")
    if not reps:
        return
    for name in reps[0]["grad_gap"]:
        g = [r["grad_gap"][name] for r in reps]
        lines.append(f"  gap {name:28s} worst {max(g):.3e}  median {float(np.median(g)):.3e}")
    for name in reps[0]["census"]:
        c = [r["census"][name] for r in reps]
        lines.append(f"  {name:7s} {c[0]['format']}: at_max worst {max(x['at_max'] for x in c)} of {c[0]['elements']} per audit, nonfinite "
                     f"{max(x['nonfinite'] for x in c)}, zero median {int(np.median([x['zero'] for x in c]))}, subnormal median "
                     f"{int(np.median([x['subnormal'] for x in c]))}")
    lo, hi = min(r["tile_scale"]["scale_min"] for r in reps), max(r["tile_scale"]["scale_max"] for r in reps)
    lines.append(f"  tile scales 2^{lo - 127}..2^{hi - 127}")


def switch_off(lines, parent, windows, iters, warm, rounds=2):
    trees = {"this tree": ROOT, "parent": os.path.abspath(parent)}
    meds = {k: [] for k in trees}
    for _ in range(rounds):
        for k, root in trees.items():
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
    aa = {k: max(v) - min(v) for k, v in meds.items()}
    diff = float(np.mean(meds["this tree"]) - np.mean(meds["parent"]))
    lines.append(f"switch off: A/A spread between processes: parent {aa['parent']:.4f} ms, this tree {aa['this tree']:.4f} ms; this tree - parent "
                 f"{diff:+.4f} ms ({'within' if abs(diff) <= aa['parent'] else 'outside'} the parent's A/A spread)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100, help="iterations per window")
    ap.add_argument("--warm", type=int, default=150, help="iterations before the first window")
    ap.add_argument("--reps", type=int, default=50, help="census launches per window")
    ap.add_argument("--fit_iters", type=int, default=2000, help="iterations of the audited fit of part 3 (the default length of a c2 fit)")
    ap.add_argument("--every", type=int, default=20)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (part 4; left out without it)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    if args.parent:                                               # first: this process has not touched the GPU yet
        lines.append("== 4. switch off: the unaudited loop, this tree against the parent commit (child processes, alternated)")
        switch_off(lines, args.parent, args.windows, args.iters, args.warm)
    sys.path.insert(0, ROOT)
    import torch
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lines.insert(0, f"stash_audit_time: {torch.cuda.get_device_name(dev)}; c2 (512^2, K = 3, 26 624 rows); medians of {args.windows} "
                    f"windows (min..max)")
    lines.append(f"== 1. the census launch ({args.reps} launches per window)")
    census_time(lines, dev, args.windows, args.reps)
    lines.append(f"== 2. audited against unaudited iterations (alternated windows of {args.iters} iterations, {args.warm} before the first)")
    audited_vs_not(lines, dev, args.windows, args.iters, args.warm)
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
