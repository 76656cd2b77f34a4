#!/usr/bin/env python3
"""What the exact-fp32 trunks (trunk_precision="fp32": csrc/npp_conv32.hip) cost beside the default fp16 trunks, on one MI355X.

At the loop's shapes -- VGG19[0:18] on 12 x 3 x 96^2 (6 images carry a gradient) and VGG16 on 4 x 3 x 96^2 (2 carry one):
  * every convolution launch of the fp32 trunk on its own, forward and data gradient, with its rate: the algorithmic work
    2 * 9 * Cin * Cout * H * W FLOP per image over its time, against the 157 TFLOP/s fp32 MFMA peak;
  * the whole forward pass and the whole data-gradient pass of both trunks (HipTrunk32 / HipTrunk) on the same batch;
and the complete BASELINE c2 iteration (512^2, K = 3, 8192 pixel rows + 2 patches) in the four combinations of precision
(bf16 / fp32 MLP) and trunk_precision (fp16 / fp32).
Everything runs on the same box in ALTERNATED windows, every window timed with device events around --reps back-to-back repetitions
behind one warm-up repetition; reported: the median over the windows and (min..max).  Nothing here is a gate.

    python tools/trunk32_time.py [--windows 5] [--reps 10] [--iters 20] [--out profiles/trunk32_time.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from npp_amd import losses, ops, synthetic as syn  # noqa: E402
from npp_amd.fit import CompletionFit  # noqa: E402

PEAK = 157e12


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


def trunk_launches(t32, N, n, P, sc, sh, dev):
    """{label: (callable, FLOP)} for every convolution launch of HipTrunk32 at (N, 3, P, P) forward / (n, ...) data gradient."""
    out, H, cin = {}, P, 3
    x = torch.rand(N, 3, P, P, device=dev)
    for j, L in enumerate(t32.layers):
        if L["kind"] == "pool":
            H //= 2
            continue
        cout = L["cout"]
        xin = x if j == 0 else torch.rand(N, cin, H, H, device=dev)
        y = torch.empty(N, cout, H, H, device=dev)
        g = torch.randn(n, cout, H, H, device=dev)
        flop = 2.0 * 9 * cin * cout * H * H
        out[f"fwd   conv{j:<2d} {cin:3d}->{cout:3d} @{H:3d}^2 x{N:2d}"] = (
            lambda xin=xin, y=y, L=L, j=j: ops.conv32(xin, N, L["cout"], L["pf"], 0, y, bias=L["b"], in_norm=(sc, sh) if j == 0 else None),
            flop * N)
        if j == 0:
            dimg = torch.empty(N, 3, H, H, device=dev)
            out[f"dgrad conv{j:<2d} {cout:3d}->  3 @{H:3d}^2 x{n:2d}"] = (
                lambda g=g, dimg=dimg, L=L: ops.conv32(g, n, 3, L["pb"], 2, dimg, out_scale=sc), flop * n)
        else:
            dz = torch.empty(N, cin, H, H, device=dev)
            out[f"dgrad conv{j:<2d} {cout:3d}->{cin:3d} @{H:3d}^2 x{n:2d}"] = (
                lambda g=g, dz=dz, xin=xin, L=L: ops.conv32(g, n, L["cin"], L["pb"], 1, dz, gate=xin), flop * n)
        cin = cout
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10, help="launches / passes per window")
    ap.add_argument("--iters", type=int, default=20, help="complete iterations per window")
    ap.add_argument("--patch", type=int, default=96)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--K", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    P = args.patch
    lines = [f"trunk32_time: {torch.cuda.get_device_name(dev)}; ms, median of {args.windows} alternated windows (min..max); "
             f"{args.reps} launches / passes and {args.iters} iterations per window; rates against the {PEAK / 1e12:.0f} TFLOP/s fp32 MFMA peak"]
    cx, lp = losses.ContextualLoss, losses.LPIPS
    defs = [("VGG19[0:18]", losses._VGG19, (17,), 1234, 12, 6, cx.input_norm(cx)),
            ("VGG16", losses._VGG16, (3, 8, 15, 22, 29), 4321, 4, 2,
             ([2.0 / s for s in lp._SCALE], [(-1.0 - b) / s for b, s in zip(lp._SHIFT, lp._SCALE)]))]
    for name, cfg, taps, seed, N, n, (sc, sh) in defs:
        t32 = losses.HipTrunk32(cfg, taps, seed=seed, device=dev)
        t16 = losses.HipTrunk(cfg, taps, seed=seed, device=dev)
        x = torch.rand(N, 3, P, P, device=dev)
        launches = trunk_launches(t32, N, n, P, sc, sh, dev)
        gs = [torch.randn(n, *f.shape[1:], device=dev) for f in t32._forward(x, sc, sh, n_keep=n)]
        passes = {}
        for tag, t in (("fp32", t32), ("fp16", t16)):
            passes[f"{tag} trunk, whole forward pass"] = lambda t=t: t._forward(x, sc, sh, n_keep=n)
            passes[f"{tag} trunk, whole data-gradient pass"] = lambda t=t: t._backward(gs, n, sc, tuple(x.shape), zero_rest=False)
        tl, tp = {k: [] for k in launches}, {k: [] for k in passes}
        for _ in range(args.windows):
            for k, (f, _) in launches.items():
                tl[k].append(window(f, args.reps))
            for k, f in passes.items():                  # (forward before its data-gradient pass: the pass reads the stored outputs)
                tp[k].append(window(f, args.reps))
        lines.append(f"-- {name} on {N} x 3 x {P}^2, {n} images with a gradient")
        total = {"fwd": [0.0, 0.0], "dgrad": [0.0, 0.0]}
        for k, (_, flop) in launches.items():
            ms = float(np.median(tl[k]))
            total[k.split()[0]][0] += ms
            total[k.split()[0]][1] += flop
            lines.append(f"{k:36s} {fmt(tl[k])}   {flop / (ms * 1e-3) / 1e12:6.1f} TFLOP/s  {100 * flop / (ms * 1e-3) / PEAK:5.1f} %")
        for d, (ms, flop) in total.items():
            lines.append(f"{'sum of the ' + d + ' convolution launches':36s} {ms:9.3f}   {flop / (ms * 1e-3) / 1e12:6.1f} TFLOP/s  "
                         f"{100 * flop / (ms * 1e-3) / PEAK:5.1f} %")
        for k in passes:
            lines.append(f"{k:36s} {fmt(tp[k])}")
        for d in ("forward", "data-gradient"):
            a, b = (float(np.median(tp[f"{tag} trunk, whole {d} pass"])) for tag in ("fp32", "fp16"))
            lines.append(f"fp32 / fp16 whole {d} pass: {a / b:.1f} x")
    H, K = args.size, args.K
    img, mask = syn.synthetic_image(H, seed=0)
    angles, periods, shifts = syn.synthetic_periodicity(H, K)
    fits = {(p, tp_): CompletionFit(img, mask, angles, periods, syn.SEED0_FREQS, syn.init_params(K, seed=0), device=dev, N_rand=8192, seed=0,
                                    shifts=shifts, rng_mode="fast", precision=p, trunk_precision=tp_)
            for p in ("bf16", "fp32") for tp_ in ("fp16", "fp32")}
    it = {k: [] for k in fits}
    for _ in range(args.windows):
        for k, f in fits.items():
            it[k].append(window(f.step_full, args.iters))
    lines.append(f"-- complete c2 iteration ({H}^2, K = {K}, 8192 pixel rows + 2 patches of {fits['bf16', 'fp16'].patch_size}^2)")
    for (p, tp_), ts in it.items():
        lines.append(f"{'precision=' + p + ', trunk_precision=' + tp_:36s} {fmt(ts)}")
    base = float(np.median(it["bf16", "fp16"]))
    lines.append("against the default: " + ", ".join(f"{p}/{tp_} {float(np.median(ts)) / base:.2f} x" for (p, tp_), ts in it.items()))
    for f in fits.values():
        f.close()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
