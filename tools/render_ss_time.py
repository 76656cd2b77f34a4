#!/usr/bin/env python3
"""Supersampled renders: what averaging S x S samples inside the launch costs, (a) against the point-sampled launch that runs the
same number of chain rows and (b) against the two-step path it replaces (a dense render_grid, then the ordered block mean in torch).

In one process, alternated window by window (K = 3, W = 256 and 512, bf16 chain; the grid launch and the identity view with its
inside bytes):
  point_a  the point-sampled 2048^2 canvas (4 Mi chain rows)
  ss2      the 1024^2 canvas at supersample=2 (the same 4 Mi rows, a quarter of the stores)
  ss4      the 512^2 canvas at supersample=4 (the same rows, a sixteenth of the stores)
  two2     render_grid of the dense 2048^2 canvas at scale 2, origin -1/4, then the ordered 2 x 2 block mean in torch -> 1024^2
  two4     the same at scale 4, origin -3/8 and 4 x 4 blocks -> 512^2
  point_b  point_a again: point_b / point_a is the A/A spread every ratio is read against
Median of --windows windows of --reps launches each after warm-up; ss2 / ss4 equal two2 / two4 bit for bit (asserted).  The peak
device memory of each path beyond its result is read from torch's allocator.  Last, for a 4x minifying grid of a small K = 3 net, the
RMS distance of supersample 1, 2, 4 from supersample 8 (reported, not asserted).

    python tools/render_ss_time.py [--windows 7] [--reps 3] [--out profiles/render_ss_time.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import oracle  # noqa: E402
from npp_amd.model import NPPNet  # noqa: E402


def block_mean(dense, ss):
    """The ordered ss x ss block mean of a (ss H, ss W, 3) canvas: acc = 0, one add per sample a ss + b, one division."""
    H, W = dense.shape[0] // ss, dense.shape[1] // ss
    d = dense.view(H, ss, W, ss, 3)
    acc = torch.zeros((H, W, 3), dtype=torch.float32, device=dense.device)
    for a in range(ss):
        for b in range(ss):
            acc = acc + d[:, a, :, b]
    return acc / float(ss * ss)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--size", type=int, default=2048, help="side of the point-sampled canvas (a multiple of 4)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N, K = args.size, 3
    lines = [f"render_ss_time: {N}^2 chain rows per launch, K = {K}, bf16 chain, median of {args.windows} windows x {args.reps} launches, "
             f"{torch.cuda.get_device_name(dev)}"]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(f, reps):
        e0.record()
        for _ in range(reps):
            f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    def peak_extra(f):
        """Peak device memory of f() beyond what was allocated before it and beyond its result, in bytes."""
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        r = f()
        torch.cuda.synchronize()
        keep = sum(t.numel() * t.element_size() for t in (r if isinstance(r, tuple) else (r,)))
        return torch.cuda.max_memory_allocated(dev) - base - keep
    eye = np.eye(3)

    def origin(ss):
        return (1.0 / (2 * ss) - 0.5,) * 2
    for W in (256, 512):
        angles, periods, _ = oracle.synthetic_periodicity(N, K)
        net = NPPNet(angles, periods, oracle.SEED0_FREQS, (N, N), params=oracle.init_params(K, W=W, seed=0), device=dev, ksplit=1, width=W)
        two = {ss: (lambda ss=ss: block_mean(net.render_grid((N, N), origin=origin(ss), scale=float(ss)), ss)) for ss in (2, 4)}
        for kind in ("grid", "view"):
            if kind == "grid":
                def point():
                    return net.render_grid((N, N))

                def ssf(ss):
                    return lambda: net.render_grid((N // ss, N // ss), supersample=ss)
            else:
                def point():
                    return net.render_view((N, N), eye, return_inside=True)

                def ssf(ss):
                    return lambda: net.render_view((N // ss, N // ss), eye, return_inside=True, supersample=ss)
            cases = {"point_a": point, "ss2": ssf(2), "ss4": ssf(4), "two2": two[2], "two4": two[4], "point_b": point}
            for ss in (2, 4):
                got = cases[f"ss{ss}"]()
                got = got[0] if isinstance(got, tuple) else got
                assert torch.equal(got.view(torch.int32), two[ss]().view(torch.int32)), (W, kind, ss)
            mem = {k: peak_extra(f) for k, f in cases.items() if k != "point_b"}
            for f in cases.values():                                   # warm-up
                f()
            torch.cuda.synchronize()
            t = {k: [] for k in cases}
            for _ in range(args.windows):
                for k, f in cases.items():                             # alternated: point_a, ss2, ss4, two2, two4, point_b, point_a, ...
                    t[k].append(window(f, args.reps))
            med = {k: float(np.median(v)) for k, v in t.items()}
            for k in cases:
                lines.append(f"W={W:4d} {kind:4s} {k:7s} {med[k]:8.3f} ms  {N * N / (med[k] * 1e-3) / 1e6:8.1f} Mrows/s   "
                             f"(spread {min(t[k]):.3f}..{max(t[k]):.3f} ms)" +
                             (f"   peak extra memory {mem[k] / 2 ** 20:8.1f} MiB" if k in mem else ""))
            aa = med["point_b"] / med["point_a"]
            for ss in (2, 4):
                a, b = med[f"ss{ss}"] / med["point_a"], med[f"ss{ss}"] / med[f"two{ss}"]
                lines.append(f"W={W:4d} {kind:4s} (a) ss{ss} / point_a = {a:.4f}   A/A point_b / point_a = {aa:.4f}   -> "
                             f"{'inside' if abs(a - 1.0) <= abs(aa - 1.0) else 'OUTSIDE'} the A/A spread;   (b) ss{ss} / two{ss} = {b:.4f} "
                             f"({'ahead' if b < 1.0 else 'BEHIND'}; the two-step path is the grid's for both kinds)")
        del net, two, cases
        torch.cuda.empty_cache()
    # what the samples buy: a 4x minifying grid of the K = 3 net of the tests, every S against S = 8
    fit, canvas = (24, 40), (96, 160)
    angles, periods, _ = oracle.synthetic_periodicity(64, K)
    net = NPPNet(angles, periods, oracle.SEED0_FREQS, fit, params=oracle.init_params(K, W=256, seed=7 * K + 256), device=dev, ksplit=1, width=256)
    ref = net.render_grid(canvas, scale=0.25, supersample=8)
    for ss in (1, 2, 4):
        rms = float((net.render_grid(canvas, scale=0.25, supersample=ss) - ref).pow(2).mean().sqrt())
        lines.append(f"4x minifying grid ({canvas[0]} x {canvas[1]} canvas at scale 0.25 of a {fit[0]} x {fit[1]} fit, sigmoid output): "
                     f"RMS of supersample={ss} from supersample=8: {rms:.5f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
