#!/usr/bin/env python3
"""What LPIPS as a quality figure costs on one MI355X (npp_amd.metrics.LPIPSMetric, metrics.report(lpips=)) -- and, beside it, the
restatement in torch fp32 (tests/lpips_restatement.py) on the host of the same box, on the same images and the same fixed-seed trunks.

Images: the lattice pair of the tests (a noisy lattice and the same image with a rectangle of noise) at 256^2, 512^2 and 1024^2, a
centred rectangular hole as the unknown region; both nets.  Timed, on images that already lie on the device: LPIPSMetric.map,
LPIPSMetric.scalar and metrics.report with the metric (what train.py --eval_metrics --eval_lpips pays per test set), the report without
it for comparison, and per stage -- trunk, the five head launches, the composition, the reduction (three region launches, five tap
means, their copies to the host) -- between device events in passes of their own.  Method: every shape is warmed up once; then
--windows windows per form, the GPU's and the host's ALTERNATED (other people's work shares the host: a drift hits both), a GPU
window being --inner calls between two device synchronises under a host clock, a host window one call; the figure is the median of
the windows' per-call times, (min..max) beside it.

    python tools/lpips_metric_time.py [--windows 3] [--inner 5] [--sizes 256 512 1024] [--out profiles/lpips_metric_time.txt]
"""
import argparse
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lpips_restatement as LR  # noqa: E402
import metrics_restatement as MR  # noqa: E402
from npp_amd import metrics, ops, weights  # noqa: E402


def window(f, inner, gpu):
    if gpu:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        out = f()
    if gpu:
        torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) / inner * 1e3


def alternated(gpu_f, host_f, windows, inner):
    window(gpu_f, 1, True)                                           # warm-up of this shape
    tg, th, g, h = [], [], None, None
    for _ in range(windows):
        g, t = window(gpu_f, inner, True)
        tg.append(t)
        if host_f is not None:
            h, t = window(host_f, 1, False)
            th.append(t)
    return g, h, tg, th


def stages(m, a, b, regions, windows, inner):
    """Per-stage device time (ms per call, one list entry per window) of the metric's own sequence, between device events."""
    names = ("trunk", "head (5 launches)", "compose", "reduction (3 regions + 5 tap means)")
    out = {n: [] for n in names}
    for w in range(windows + 1):                                     # (window 0 warms up)
        acc = dict.fromkeys(names, 0.0)
        for _ in range(inner):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
            with torch.no_grad():
                x = torch.stack([a, b]).permute(0, 3, 1, 2).contiguous()
                ev[0].record()
                feats = m._features(x)
                ev[1].record()
                taps = [ops.lpips_tap_map(f0, f1, lin, m.layout) for (f0, f1), lin in zip(feats, m.lins)]
                ev[2].record()
                D = ops.lpips_compose(taps, a.shape[0], a.shape[1])
                ev[3].record()
                metrics._map_totals(D, regions)
                metrics._scalar(taps)
                ev[4].record()
            torch.cuda.synchronize()
            m._release()
            for k, n in enumerate(names):
                acc[n] += ev[k].elapsed_time(ev[k + 1])
        if w:
            for n in names:
                out[n].append(acc[n] / inner)
    return out


def fmt(ts):
    return f"{float(np.median(ts)):10.3f} ({min(ts):9.3f}..{max(ts):9.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5, help="GPU calls per window")
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    lines = [f"lpips_metric_time: median over {args.windows} windows per form, GPU and host windows alternated, a GPU window = {args.inner} "
             f"calls between device synchronises, a host window = 1 call of the torch fp32 restatement ({torch.get_num_threads()} threads); "
             f"one warm-up call per shape; fixed-seed random trunks (allow_random=True); {torch.cuda.get_device_name(dev)}; times in ms per "
             "call, (min..max)"]
    for net in ("vgg", "alex"):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m = metrics.LPIPSMetric(net, device=dev, allow_random=True)
        sd = LR.vgg_state_dict() if net == "vgg" else LR.alex_state_dict()
        lins = weights.lpips_lin(net)
        for n in args.sizes:
            a, b = LR.lattice_pair(n, n)
            mask = MR.mask("hole", (n, n))
            ad, bd, md = (torch.from_numpy(x).to(dev) for x in (a, b, mask))
            D, host, tm, th = alternated(lambda: m.map(ad, bd), lambda: LR.lpips(net, sd, lins, a, b, torch.float32), args.windows, args.inner)
            dist = LR.rel_l2(D.cpu().numpy(), host["map"])
            sc, _, ts, _ = alternated(lambda: m.scalar(ad, bd), None, args.windows, args.inner)
            rep, _, tr, _ = alternated(lambda: metrics.report(ad, bd, md, device=dev, lpips=m), None, args.windows, args.inner)
            _, _, tp, _ = alternated(lambda: metrics.report(ad, bd, md, device=dev), None, args.windows, args.inner)
            st = stages(m, ad, bd, [None, md, 1.0 - md], args.windows, args.inner)
            lines.append(f"-- {net} {n} x {n} (scalar {sc:.6f}, host {host['scalar']:.6f}; LPIPS known {rep['known']['lpips']:.6f}, unknown "
                         f"{rep['unknown']['lpips']:.6f}; rel-L2 of the GPU map against the host's fp32 map {dist:.2e})")
            lines.append(f"{'LPIPSMetric.map, images on the device':64s} {fmt(tm)}")
            lines.append(f"{'LPIPSMetric.scalar, images on the device':64s} {fmt(ts)}")
            lines.append(f"{'metrics.report with the metric (SSIM + 3 regions + LPIPS)':64s} {fmt(tr)}")
            lines.append(f"{'metrics.report without it':64s} {fmt(tp)}")
            lines.append(f"{'restatement in torch fp32 on the host (map + scalar)':64s} {fmt(th)}")
            for name, t in st.items():
                lines.append(f"{'  stage, device events: ' + name:64s} {fmt(t)}")
            lines.append(f"host / GPU: map {np.median(th) / np.median(tm):.0f}x; the trunk is "
                         f"{100 * np.median(st['trunk']) / sum(np.median(t) for t in st.values()):.0f} % of the stages' device time")
        del m
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
