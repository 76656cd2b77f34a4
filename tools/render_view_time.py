#!/usr/bin/env python3
"""Perspective views: what the projective intake costs against the grid launch, and the image warp against its host twin.

In one process, alternated window by window on a 2048^2 canvas (K = 3, W = 256 and 512, bf16 chain):
  grid_a   NPPNet.render_grid() at scale 1, origin 0 (npp_mlp_fwd_grid)
  view     NPPNet.render_view() of the identity map with the inside bytes (npp_mlp_fwd_view: the same pixels bit for bit)
  grid_b   the grid launch again: grid_b / grid_a is the A/A spread the view ratio is read against
Median of --windows windows of --reps launches each after warm-up.  Then npp_warp_image_u8 (bilinear and nearest, 3 channels, a
projective map) at 512^2 and 2048^2 against npp_warp_image_u8_host, the kernel timed with events and the host twin with the wall clock.

    python tools/render_view_time.py [--windows 7] [--reps 5] [--out profiles/render_view_time.txt]
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
from npp_amd import view  # noqa: E402
from npp_amd.model import NPPNet  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    S, K = args.size, 3
    lines = [f"render_view_time: {S}^2 canvas, K = {K}, bf16 chain, median of {args.windows} windows x {args.reps} launches, "
             f"{torch.cuda.get_device_name(dev)}"]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(f, reps):
        e0.record()
        for _ in range(reps):
            f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps
    eye = np.eye(3)
    for W in (256, 512):
        angles, periods, _ = oracle.synthetic_periodicity(S, K)
        net = NPPNet(angles, periods, oracle.SEED0_FREQS, (S, S), params=oracle.init_params(K, W=W, seed=0), device=dev, ksplit=1, width=W)
        cases = {"grid_a": lambda: net.render_grid((S, S)),
                 "view": lambda: net.render_view((S, S), eye, return_inside=True),
                 "grid_b": lambda: net.render_grid((S, S))}
        img, inside = cases["view"]()
        assert torch.equal(img, cases["grid_a"]()) and bool((inside == 3).all())
        for f in cases.values():                                       # warm-up
            f()
        torch.cuda.synchronize()
        t = {k: [] for k in cases}
        for _ in range(args.windows):
            for k, f in cases.items():                                 # alternated: grid_a, view, grid_b, grid_a, ...
                t[k].append(window(f, args.reps))
        med = {k: float(np.median(v)) for k, v in t.items()}
        for k in cases:
            lines.append(f"W={W:4d} {k:7s} {med[k]:8.3f} ms  {S * S / (med[k] * 1e-3) / 1e6:8.1f} Mrows/s   "
                         f"(spread {min(t[k]):.3f}..{max(t[k]):.3f} ms)")
        aa, va = med["grid_b"] / med["grid_a"], med["view"] / med["grid_a"]
        inside_aa = abs(va - 1.0) <= abs(aa - 1.0)
        lines.append(f"W={W:4d} view / grid_a = {va:.4f}   A/A grid_b / grid_a = {aa:.4f}   -> the view ratio is "
                     f"{'inside' if inside_aa else 'OUTSIDE'} the A/A spread")
        del net
        torch.cuda.empty_cache()
    # the image warp: a 3-channel photograph under a projective map, kernel against host twin
    rng = np.random.RandomState(0)
    for n in (512, 2048):
        src = rng.randint(0, 256, (n, n, 3)).astype(np.uint8)
        M = np.array([[0.9, 0.05, 10.0], [-0.04, 0.95, 20.0], [2e-5, 1e-5, 1.0]])
        d_src = torch.from_numpy(src).to(dev)
        for mode in ("bilinear", "nearest"):
            got, gin = view.warp_image(d_src, M, (n, n), mode, device=dev)
            t0 = time.perf_counter()
            want, win = view.warp_image(src, M, (n, n), mode)
            host_ms = (time.perf_counter() - t0) * 1e3
            assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(gin.cpu().numpy(), win)
            ts = [window(lambda: view.warp_image(d_src, M, (n, n), mode, device=dev), args.reps) for _ in range(args.windows)]
            ms = float(np.median(ts))
            lines.append(f"warp_image {n:4d}^2 x 3 {mode:8s}: kernel {ms * 1e3:8.1f} us ({n * n / (ms * 1e-3) / 1e9:6.2f} Gpixel/s, with its "
                         f"allocations)   host twin {host_ms:8.1f} ms   {host_ms / ms:8.0f}x   equal bit for bit")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
