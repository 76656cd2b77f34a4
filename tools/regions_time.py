#!/usr/bin/env python3
"""What the connected-component work of the segmentation task costs on one MI355X (npp_amd.regions, csrc/npp_regions.hip) and, beside
it, the host path on the same inputs in the same run: `label`, `fill_holes`, `remove_small_objects`, the SLIC connectivity repair
(init_segment.enforce_connectivity) and the whole segment.segmentation_eval, at 256^2, 512^2 and 1024^2.

Inputs: synthetic -- a random mask at p = 0.59 (near the percolation threshold: large tortuous components), nested rings with
holes, and a blocky 4-valued label image with 25 % of its pixels displaced (the fragment structure SLIC leaves); not real SLIC output.
Every row: the GPU path and the host path alternate in windows of --inner calls, --windows windows each after one warm-up window;
a window is a host clock around work that ends in a device synchronise (the copies a call needs are inside it); the figure is the
median over the windows of the time per call, (min..max) beside it.  The results of the two paths are compared before they are timed.

    python tools/regions_time.py [--windows 5] [--inner 4] [--out profiles/regions_time.txt]
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
import regions_restatement as R  # noqa: E402
from npp_amd import init_segment as iseg, regions, segment  # noqa: E402


def alternate(f_gpu, f_host, windows, inner):
    """-> ((median, min, max) ms per call) for the GPU path and for the host path, windows alternated."""
    ts = {0: [], 1: []}
    for w in range(windows + 1):
        for k, f in enumerate((f_gpu, f_host)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                f()
            torch.cuda.synchronize()
            if w:
                ts[k].append((time.perf_counter() - t0) / inner * 1e3)
    return [(float(np.median(v)), min(v), max(v)) for v in (ts[0], ts[1])]


def eval_inputs(n):
    """A 'fitted' image and an 'input' that differ on discs, rings (holes to fill) and specks, over the whole frame."""
    yy, xx = np.mgrid[:n, :n]
    rs = np.random.RandomState(n)
    base = 0.25 + 0.1 * (np.sin(yy / 3.0) * np.cos(xx / 4.0))[..., None] + rs.uniform(0, 0.02, (n, n, 3))
    planted = np.zeros((n, n), bool)
    for cy, cx in rs.randint(40, n - 40, (n // 32, 2)):
        d2 = (yy - cy) ** 2 + (xx - cx) ** 2
        planted |= (d2 < 30 ** 2) & (d2 >= 12 ** 2)
    planted |= rs.rand(n, n) < 0.01
    return base.astype(np.float32), (base + 0.5 * planted[..., None]).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    from scipy import ndimage
    lines = [f"regions_time: GPU path (npp_amd.regions on {torch.cuda.get_device_name(dev)}) against the host path (SciPy / NumPy) in the same "
             f"run; windows of {args.inner} calls alternated, median of {args.windows} windows after one warm-up window, host clock around a "
             "device synchronise; ms per call (min..max); synthetic inputs, not real SLIC output"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        alex = segment.AlexFeatures(None, device=dev)
    lins = [np.full(c, 1.0 / c, np.float32) for c in (64, 192, 384, 256, 256)]
    for n in (256, 512, 1024):
        mask = np.random.RandomState(n).rand(n, n) < 0.59
        rings = R.rings(n, n) | (np.random.RandomState(n + 1).rand(n, n) < 0.3)
        labels = R.blocky(n, n, n)
        colour = R.colour_of((n, n))
        mask_t, rings_t = torch.from_numpy(mask).to(dev), torch.from_numpy(rings).to(dev)
        pred, blur = eval_inputs(n)
        ones = np.ones((n, n, 1), np.float32)
        ev = lambda how: segment.segmentation_eval(pred, blur, ones, ones, alex, lins, 0.15, 1e9, 1, final_mask=how)   # noqa: E731
        rows = [
            ("label, mask on the device / scipy.ndimage.label", lambda: regions.label(mask_t), lambda: ndimage.label(mask),
             lambda a, b: a[1] == b[1] and np.array_equal(a[0].cpu().numpy(), b[0])),
            ("label, NumPy in and out / scipy.ndimage.label", lambda: regions.label(mask, dev), lambda: ndimage.label(mask),
             lambda a, b: a[1] == b[1] and np.array_equal(a[0], b[0])),
            ("fill_holes, on the device / binary_fill_holes", lambda: regions.fill_holes(rings_t), lambda: ndimage.binary_fill_holes(rings),
             lambda a, b: np.array_equal(a.cpu().numpy(), b)),
            ("remove_small_objects(500), on the device / host", lambda: regions.remove_small_objects(mask_t, 500),
             lambda: segment.remove_small_objects(mask, 500), lambda a, b: np.array_equal(a.cpu().numpy(), b)),
            ("enforce_connectivity, cc_device / host", lambda: iseg.enforce_connectivity(labels, 200.0, colour, cc_device=dev),
             lambda: iseg.enforce_connectivity(labels, 200.0, colour), np.array_equal),
            ("segmentation_eval, final_mask gpu / host", lambda: ev("gpu"), lambda: ev("host"),
             lambda a, b: np.array_equal(a["non_period_mask_final"], b["non_period_mask_final"])),
        ]
        lines.append(f"-- {n} x {n} (mask: {regions.label(mask)[1]} components; label image: {regions.label(labels)[1]} fragments)")
        lines.append(f"{'':52s} {'GPU path':>34s} {'host path':>34s} {'host / GPU':>10s}")
        for what, f_gpu, f_host, same in rows:
            if not same(f_gpu(), f_host()):
                raise SystemExit(f"{what} at {n}: the two paths differ")
            g, h = alternate(f_gpu, f_host, args.windows, args.inner)
            lines.append(f"{what:52s} {g[0]:10.3f} ({g[1]:9.3f}..{g[2]:9.3f}) {h[0]:10.3f} ({h[1]:9.3f}..{h[2]:9.3f}) {h[0] / g[0]:9.1f}x")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
