#!/usr/bin/env python3
"""What the quality report costs on one MI355X (npp_amd.metrics, npp_amd.evaluate) -- and, beside it, the float64 restatement's scipy
form (tests/metrics_restatement.py: scipy.ndimage.correlate1d, cropped) on the host of the same box, on the same images.

Images: the g13b scene (tests/blur_restatement.py make_image) at 256^2, 512^2 and 1024^2 as the ground truth, a blurred and noisy
copy of it as the prediction, a centred rectangular hole as the unknown region.  Timed: metrics.ssim_map and metrics.report on images
that already lie on the device (what train.py --eval_metrics pays per test set), and the whole `python -m npp_amd.evaluate` call in
process (PNG decoding, copies, the report, the JSON).  Method: every shape is warmed up once; then --windows windows per form, the
GPU's and the host's ALTERNATED (other people's work shares the host: a drift hits both), a GPU window being --inner calls between
two device synchronises under a host clock; the figure is the median of the windows' per-call times, (min..max) beside it.

    python tools/metrics_time.py [--windows 5] [--inner 20] [--out profiles/metrics_time.txt]
"""
import argparse
import contextlib
import io
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import metrics_restatement as R  # noqa: E402
from blur_restatement import make_image  # noqa: E402
from npp_amd import evaluate, io as nio, metrics  # noqa: E402


def scene(n):
    import scipy.ndimage as ndimage
    gt = make_image(n, n).astype(np.float64) / 255.0
    pred = np.clip(ndimage.gaussian_filter(gt, (1.0, 1.0, 0)) + np.random.RandomState(1).normal(0, 0.02, gt.shape), 0, 1)
    return pred.astype(np.float32), gt.astype(np.float32), R.mask("hole", (n, n))


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
    """-> (last GPU result, last host result, GPU per-call times, host per-call times), the two forms' windows taking turns."""
    window(gpu_f, 1, True)                                           # warm-up of this shape
    tg, th, g, h = [], [], None, None
    for _ in range(windows):
        g, t = window(gpu_f, inner, True)
        tg.append(t)
        if host_f is not None:
            h, t = window(host_f, 1, False)
            th.append(t)
    return g, h, tg, th


def fmt(ts):
    return f"{float(np.median(ts)):10.3f} ({min(ts):9.3f}..{max(ts):9.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20, help="GPU calls per window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    lines = [f"metrics_time: median over {args.windows} windows per form, GPU and host windows alternated, a GPU window = {args.inner} calls "
             f"between device synchronises, a host window = 1 call; one warm-up call per shape; {torch.cuda.get_device_name(dev)}; "
             "times in ms per call, (min..max)"]
    with tempfile.TemporaryDirectory() as tmp:
        for n in (256, 512, 1024):
            pred, gt, m = scene(n)
            pd, gd, md = (torch.from_numpy(x).to(dev) for x in (pred, gt, m))
            smap, smap_h, tg, th = alternated(lambda: metrics.ssim_map(pd, gd, device=dev), lambda: R.ssim_map_scipy(pred, gt), args.windows, args.inner)
            dist = float(np.abs(smap.cpu().numpy() - smap_h).max())
            rep, rep_h, rg, rh = alternated(lambda: metrics.report(pd, gd, md, device=dev), lambda: R.report(pred, gt, m, form=R.ssim_map_scipy),
                                            args.windows, args.inner)
            fig = max(abs(rep[r][k] - rep_h[r][k]) for r in rep for k in ("psnr", "ssim", "mae"))
            for name, img in (("pred.png", pred), ("gt.png", gt)):
                nio.imsave(os.path.join(tmp, name), img)
            nio.imsave(os.path.join(tmp, "mask.png"), np.repeat(m[..., None], 3, 2))
            argv = ["--pred", os.path.join(tmp, "pred.png"), "--gt", os.path.join(tmp, "gt.png"), "--mask", os.path.join(tmp, "mask.png"),
                    "--json", os.path.join(tmp, "report.json")]

            def whole():
                with contextlib.redirect_stdout(io.StringIO()):
                    return evaluate.main(argv)
            _, _, eg, _ = alternated(whole, None, args.windows, max(1, args.inner // 4))
            lines.append(f"-- {n} x {n} (SSIM all {rep['all']['ssim']:.4f}, unknown {rep['unknown']['ssim']:.4f}; PSNR unknown {rep['unknown']['psnr']:.2f} dB; "
                         f"GPU map differs from the host's by {dist:.2e}, the report's figures by {fig:.2e})")
            lines.append(f"{'metrics.ssim_map, images on the device':60s} {fmt(tg)}")
            lines.append(f"{'restatement ssim_map_scipy on the host':60s} {fmt(th)}")
            lines.append(f"{'metrics.report, images on the device (map + 3 regions)':60s} {fmt(rg)}")
            lines.append(f"{'restatement report (scipy form) on the host':60s} {fmt(rh)}")
            lines.append(f"{'evaluate.main, whole call (3 PNGs -> JSON file)':60s} {fmt(eg)}")
            lines.append(f"host / GPU: ssim_map {np.median(th) / np.median(tg):.0f}x, report {np.median(rh) / np.median(rg):.0f}x; "
                         f"the report's kernels are {100 * np.median(rg) / np.median(eg):.0f} % of the whole evaluate call")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
