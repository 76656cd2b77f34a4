#!/usr/bin/env python3
"""Rendering at any scale: what the grid launch costs against today's render.

In one process, alternated window by window on a 2048^2 canvas (K = 3, W = 256 and 512, bf16 chain):
  int32    NPPNet.render() on a materialised int32 coordinate grid (npp_mlp_fwd)
  grid1    NPPNet.render_grid() at scale 1, origin 0 (npp_mlp_fwd_grid: no coordinate buffer; the same pixels bit for bit)
  grid4x   NPPNet.render_grid() at scale 4 (the same number of rows, at 4x the density of a 512^2 region)
Median of --windows windows of --reps launches each after warm-up; rows/s and the fraction of the bf16 MFMA peak (2.5 PFLOP/s
dense) that the algorithmic MACs (oracle.mlp_macs_per_pixel) reach.  Then the end-to-end wall time of a chunked 4096^2
render_grid including the copy to the host.

    python tools/render_any_time.py [--windows 7] [--reps 5] [--out profiles/render_any_time.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import oracle  # noqa: E402
from npp_amd.model import NPPNet  # noqa: E402

PEAK_BF16 = 2.5e15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    S, K = args.size, 3
    lines = [f"render_any_time: {S}^2 canvas, K = {K}, bf16 chain, median of {args.windows} windows x {args.reps} launches, "
             f"{torch.cuda.get_device_name(dev)}"]
    yy, xx = torch.meshgrid(torch.arange(S, dtype=torch.int32), torch.arange(S, dtype=torch.int32), indexing="ij")
    grid = torch.stack([yy.reshape(-1), xx.reshape(-1)], 1).contiguous().to(dev)
    rows = S * S
    for W in (256, 512):
        angles, periods, _ = oracle.synthetic_periodicity(S, K)
        net = NPPNet(angles, periods, oracle.SEED0_FREQS, (S, S), params=oracle.init_params(K, W=W, seed=0), device=dev, ksplit=1, width=W)
        cases = {"int32": lambda: net.render(grid),
                 "grid1": lambda: net.render_grid((S, S)),
                 "grid4x": lambda: net.render_grid((S, S), scale=4.0)}
        assert torch.equal(cases["int32"]().reshape(S, S, 3), cases["grid1"]())
        for f in cases.values():                                       # warm-up
            f()
        torch.cuda.synchronize()
        t = {k: [] for k in cases}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(args.windows):
            for k, f in cases.items():                                 # alternated: int32, grid1, grid4x, int32, ...
                e0.record()
                for _ in range(args.reps):
                    f()
                e1.record()
                e1.synchronize()
                t[k].append(e0.elapsed_time(e1) / args.reps)
        macs = oracle.mlp_macs_per_pixel(K, W=W)[0]
        base = np.median(t["int32"])
        for k in cases:
            ms = float(np.median(t[k]))
            rps = rows / (ms * 1e-3)
            lines.append(f"W={W:4d} {k:7s} {ms:8.3f} ms  {rps / 1e6:8.1f} Mrows/s  {2 * macs * rps / PEAK_BF16 * 100:5.1f} % of bf16 peak  "
                         f"{base / ms:6.3f}x int32   (spread {min(t[k]):.3f}..{max(t[k]):.3f} ms)")
        # end to end: a chunked 4096^2 canvas at scale 2 including the device -> host copy
        big = 2 * S
        net.render_grid((big, big), scale=2.0).cpu()
        torch.cuda.synchronize()
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            img = net.render_grid((big, big), scale=2.0).cpu().numpy()
            walls.append(time.perf_counter() - t0)
        assert img.shape == (big, big, 3) and np.isfinite(img).all()
        lines.append(f"W={W:4d} end-to-end render_grid {big}^2 (scale 2, chunks of {1 << 22} rows) + copy to host: "
                     f"median {np.median(walls) * 1e3:.1f} ms ({big * big / np.median(walls) / 1e6:.1f} Mrows/s)")
        del net
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
