#!/usr/bin/env python3
"""What the remapping task's blur detection costs, stage by stage, on one MI355X (npp_amd.blur) -- and, beside it, the host path
(io.get_blur_map: one batched LAPACK SVD per image row) on the same images and the same box.

Images: the g13b scene (tests/blur_restatement.py make_image: sharp half, blurred half, flat patch) at 256^2, 512^2 and 1024^2.
GPU stages: a host clock around work that ends in a device synchronise, one warm-up run discarded, median of --reps runs
(min..max beside it); the copies between host and device are inside the stage that needs them.  Host path: one run at 256^2 and
512^2; at 1024^2 one run with --host-1024, else four times the 512^2 time, marked as extrapolated.  Also written: the distance
of the GPU map from the two reference goldens (the figure the tests bound), and -- with --kernel-stats DIR -- the rows of the new
kernels from a kernel-trace run of this script's --profile-run mode:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/blur_time.py --profile-run
    python tools/blur_time.py [--reps 5] [--host-1024] [--kernel-stats DIR] [--out profiles/blur_time.txt]
"""
import argparse
import csv
import glob
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from blur_restatement import make_image  # noqa: E402
from npp_amd import blur, io as nio, ops  # noqa: E402

KERNELS = ("rgb_to_gray_u8_kernel", "blur_sv_share_kernel", "morph_row_kernel", "morph_col_kernel")


def timed(f, reps, warmup=1):
    out, ts = None, []
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append(time.perf_counter() - t0)
    return out, float(np.median(ts)) * 1e3, min(ts) * 1e3, max(ts) * 1e3


def kernel_stats(directory):
    """The new kernels' rows of rocprofv3's *kernel_stats.csv under `directory`."""
    rows = []
    for path in sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)):
        with open(path) as f:
            for r in csv.DictReader(f):
                if any(k in r.get("Name", "") for k in KERNELS):
                    rows.append(r)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-1024", action="store_true", help="run the host path at 1024^2 too (about a minute) instead of extrapolating")
    ap.add_argument("--profile-run", action="store_true", help="only run the GPU path twice at 1024^2 (to be traced by rocprofv3)")
    ap.add_argument("--kernel-stats", default=None, help="directory of a rocprofv3 --kernel-trace --stats --output-format csv run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.profile_run:
        img = make_image(1024, 1024)
        for _ in range(2):
            blur.get_blur_map(img, device=dev)
        torch.cuda.synchronize()
        return
    torch.set_num_threads(min(16, torch.get_num_threads()))
    lines = [f"blur_time: win_size 10, sv_num 3, thresh 50, 20 erosions + 40 dilations; GPU stages: median of {args.reps} runs after one "
             f"warm-up run, host clock around a device synchronise; host path: one run; {torch.cuda.get_device_name(dev)}; times in ms, (min..max)"]
    host512 = None
    for n in (256, 512, 1024):
        img = make_image(n, n)
        g = lambda f: timed(f, args.reps)                          # noqa: E731
        rows = []
        gray, *t = g(lambda: ops.rgb_to_gray_u8(torch.from_numpy(img).to(dev)))
        rows.append(("gray (with the copy to the device)", t))
        raw, *t = g(lambda: ops.blur_sv_share(gray, 3))
        rows.append(("singular-value share (kernel alone)", t))
        t_share = t[0]
        (bm, binary), *t = g(lambda: blur.finish(raw.cpu().numpy(), 50))
        rows.append(("copy to host + normalise + percentile + '>' (host)", t))
        clear, *t = g(lambda: blur.binary_dilation(blur.binary_erosion(binary, 20, dev), 40, dev).cpu())
        rows.append(("erode 20 + dilate 40 (with both copies)", t))
        t_morph = t[0]
        (bm2, clear2), *t = g(lambda: blur.get_blur_map(img, device=dev))
        rows.append(("blur.get_blur_map, whole call", t))
        t_gpu = t[0]
        if n < 1024 or args.host_1024:
            t0 = time.perf_counter()
            bm_h, clear_h = nio.get_blur_map(img)
            t_host, how = (time.perf_counter() - t0) * 1e3, "one run"
            if n == 512:
                host512 = t_host
            same = f"map differs from the host's by {np.abs(bm2 - bm_h).max():.2e}, {int((clear2 != clear_h).sum())} mask pixels differ"
        else:
            t_host, how, same = 4 * host512, "EXTRAPOLATED: 4 x the 512^2 run", "host path not run"
        lines.append(f"-- {n} x {n} (clear share {float((clear2 > 0).mean()):.3f}; {same})")
        for what, a in rows:
            lines.append(f"{what:56s} {a[0]:10.3f} ({a[1]:9.3f}..{a[2]:9.3f})")
        lines.append(f"{'io.get_blur_map on the host (' + how + ')':56s} {t_host:10.1f}")
        lines.append(f"host / GPU whole call: {t_host / t_gpu:.0f}x; host / share kernel: {t_host / t_share:.0f}x; "
                     f"morphology = {100 * t_morph / t_gpu:.0f} % of the whole GPU call")
    for name in ("g13_blur.npz", "g13b_blur_mask.npz"):
        gold = np.load(os.path.join(ROOT, "tests", "golden", name))
        bm, clear = blur.get_blur_map(gold["img"], device=dev)
        lines.append(f"{name}: GPU map distance from the reference's map {np.abs(bm - gold['blur_map']).max():.3e}, "
                     f"{int((clear != gold['clear']).sum())} mask pixels differ")
    if args.kernel_stats:
        rows = kernel_stats(args.kernel_stats)
        lines.append("-- rocprofv3 --kernel-trace --stats, two blur.get_blur_map calls at 1024^2 (--profile-run)")
        lines.append(f"{'kernel':40s} {'calls':>6s} {'total us':>12s} {'average us':>12s} {'min us':>12s} {'max us':>12s}")
        for r in rows:
            ns = lambda k: float(r[k]) / 1e3                       # noqa: E731
            lines.append(f"{r['Name'][:40]:40s} {r['Calls']:>6s} {ns('TotalDurationNs'):12.1f} {ns('AverageNs'):12.1f} {ns('MinNs'):12.1f} {ns('MaxNs'):12.1f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
