#!/usr/bin/env python3
"""What the exact-fp32 fit (precision="fp32") costs beside the default bf16 fit, on one MI355X.

At BASELINE config c2 (512^2 image, K = 3 proposals, W = 256, 8192 pixel rows + 2 patches per iteration) and at W = 512:
  * the three MLP launches of an iteration in both precisions on the SAME batch -- forward with stash, data-gradient chain, weight
    gradients -- plus the fp32 forward WITHOUT stash (the render kernel) on the same rows: what the stash stores cost;
  * the complete iteration (CompletionFit.step_full: sampler, forward, pixel + contextual (+ LPIPS) losses, backward, Adam) in both
    precisions.
Both precisions run on the same box in ALTERNATED windows (bf16, fp32, bf16, ...), every window timed with device events around
--reps back-to-back repetitions behind one warm-up repetition; reported: the median over the windows and (min..max).  The forward's
rate is the algorithmic work 2 ((K + 1) 462 W + 11 W^2 + 1.5 W) FLOP per row over its time, against the 157 TFLOP/s fp32 MFMA peak.
Nothing here is a gate.

    python tools/fp32_fit_time.py [--windows 5] [--reps 10] [--iters 30] [--out profiles/fp32_fit_time.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from npp_amd import ops, synthetic as syn  # noqa: E402
from npp_amd.fit import CompletionFit  # noqa: E402


def window(f, reps):
    """ms per repetition of f: device events around `reps` repetitions, one warm-up repetition first."""
    f()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def fmt(ts):
    return f"{float(np.median(ts)):9.3f} ({min(ts):8.3f}..{max(ts):8.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10, help="launches per window")
    ap.add_argument("--iters", type=int, default=30, help="complete iterations per window")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--K", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    H, K = args.size, args.K
    img, mask = syn.synthetic_image(H, seed=0)
    angles, periods, shifts = syn.synthetic_periodicity(H, K)
    lines = [f"fp32_fit_time: {H} x {H}, K = {K}, 8192 pixel rows + 2 patches; {torch.cuda.get_device_name(dev)}; ms, median of "
             f"{args.windows} alternated windows (min..max); launches: {args.reps} per window, iterations: {args.iters} per window"]
    for width in (256, 512):
        fits = {p: CompletionFit(img, mask, angles, periods, syn.SEED0_FREQS, syn.init_params(K, seed=0, width=width), device=dev,
                                 N_rand=8192, seed=0, shifts=shifts, rng_mode="fast", width=width, precision=p)
                for p in ("bf16", "fp32")}
        b = None
        while b is None:                              # one drawn batch (the same rows for both nets)
            b = fits["bf16"].sample_batch()
        coords, bp = b["coords"], b["bp"]
        for f in fits.values():                       # a complete state for the single launches: stash, dpred, gradients
            f.net.zero_grad()
            f.net.forward_train(coords)
            ws = f.net.workspace(bp)
            ws["dpred"].zero_()
            f.net.pixel_loss(bp, b["n_pix"], b["gt"])
            f.net.backward(bp)
        nb, nf = fits["bf16"].net, fits["fp32"].net
        wb, wf = nb.workspace(bp), nf.workspace(bp)
        out = torch.empty((bp, 3), dtype=torch.float32, device=dev)
        launches = {
            "bf16 forward + stash": lambda: nb.forward_train(coords),
            "fp32 forward + stash": lambda: nf.forward_train(coords),
            "fp32 forward, no stash": lambda: ops.mlp_fwd32(coords, nf.cfg, nf._w32_pack(), nf.params, out=out, out_act=1, width=width),
            "bf16 data gradients": lambda: ops.mlp_bwd(wb["dpred"], wb["pred"], K, nb.wb, nb.params, wb["actT"], wb["dzT"], width),
            "fp32 data gradients": lambda: ops.mlp_bwd32(wf["dpred"], wf["pred"], K, nf._w32b, nf.params, wf["actT"], wf["dzT"], width),
            "bf16 weight gradients": lambda: ops.mlp_wgrad(wb["dzT"], wb["actT"], bp, K, nb.ksplit, wb["gslabs"], width),
            "fp32 weight gradients": lambda: ops.mlp_wgrad32(wf["dzT"], wf["actT"], nf.cfg, bp, K, nf.ksplit, wf["gslabs"], width),
        }
        t = {k: [] for k in launches}
        it = {p: [] for p in fits}
        for _ in range(args.windows):
            for k, f in launches.items():             # (declared in alternating order)
                t[k].append(window(f, args.reps))
            for p, f in fits.items():
                it[p].append(window(f.step_full, args.iters))
        flop = 2.0 * ((K + 1) * 462 * width + 11 * width * width + 1.5 * width) * bp
        lines.append(f"-- W = {width}: {bp} rows per iteration ({b['n_pix']} pixel rows + patch rows, padded), wgrad split {nf.ksplit}; "
                     f"stash {sum(v.numel() * v.element_size() for kk, v in wf.items() if kk in ('actT', 'dzT')) / bp:.0f} B per row (fp32) "
                     f"against {sum(v.numel() * v.element_size() for kk, v in wb.items() if kk in ('actT', 'dzT')) / bp:.0f} (bf16 chain)")
        for k in launches:
            rate = f"   {flop / (float(np.median(t[k])) * 1e-3) / 1e12:6.1f} TFLOP/s" if "forward" in k else ""
            lines.append(f"{k:28s} {fmt(t[k])}{rate}")
        s, n = float(np.median(t["fp32 forward + stash"])), float(np.median(t["fp32 forward, no stash"]))
        lines.append(f"fp32 forward: stash costs {100 * (s / n - 1):+.1f} %; no-stash chain at {100 * flop / (n * 1e-3) / 157e12:.0f} % of the 157 TFLOP/s fp32 MFMA peak")
        for p in fits:
            lines.append(f"{'complete iteration, ' + p:28s} {fmt(it[p])}")
        lines.append(f"fp32 / bf16 complete iteration: {float(np.median(it['fp32'])) / float(np.median(it['bf16'])):.2f} x")
        for f in fits.values():
            f.close()
        del fits, launches
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
