#!/usr/bin/env python3
"""What the image work in front of the periodicity search costs, stage by stage, host path (NumPy / SciPy: cvlite.py,
search.find_mask_centroid) against GPU path (`--front_end gpu`: npp_amd.frontend), on one MI355X and the CPU beside it.

Shapes: the eight fixture masks of tests/golden/g15_masks.npz at their own sizes (the synthetic lattice image of the oracle under
the real hole) and the synthetic 512^2 and 1024^2 images with their centred hole.  Stages: gray + resizes + mask (proposal.im2act,
gray features; the GPU row includes the upload of image and mask), the edge count on 1 channel (gray) and on the 65 channels of
the AlexNet variant (64 conv1 maps of fixed-seed random filters + gray: proposal.act2edge), the distance transform, the far-point
selection behind it (host: find_mask_centroid minus its transform, a DIFFERENCE of medians; GPU: the kernels and the one read of
the record), the whole search.prepare_image and the whole per-image search.search_image (default 300-iteration candidate fits,
random ranking trunks, --rng_mode fast).  Method: per stage one warm-up of both paths, then --reps ALTERNATED windows (host, gpu,
host, gpu, ...) in this one process, a host clock around work that ends in a device synchronise; median (min..max) in ms.  Rows where
the GPU path is slower are marked, not dropped.

    python tools/search_front_time.py [--reps 5] [--shapes all|small] [--no-search] --out profiles/search_front_time.txt
"""
import argparse
import os
import sys
import tempfile
import time
import warnings

import numpy as np
import scipy.ndimage as ndimage
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle  # noqa: E402
from frontend_restatement import golden_masks  # noqa: E402
from npp_amd import NppError, frontend, io as nio, ops, proposal, search  # noqa: E402


def window(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def alternated(host, gpu, reps):
    """One warm-up of each, then reps alternated windows -> (host result, gpu result, host times, gpu times)."""
    rh, rg = host(), gpu()
    th, tg = [], []
    for _ in range(reps):
        rh, t = window(host)
        th.append(t)
        rg, t = window(gpu)
        tg.append(t)
    return rh, rg, th, tg


def row(what, th, tg):
    mh, mg = float(np.median(th)), float(np.median(tg))
    note = "" if mg <= mh else "   GPU PATH SLOWER"
    return (f"{what:44s} host {mh:9.3f} ({min(th):9.3f}..{max(th):9.3f})   gpu {mg:9.3f} ({min(tg):9.3f}..{max(tg):9.3f})   "
            f"host / gpu {mh / mg:7.2f}x{note}"), mh, mg


class Lines(list):
    """The report's lines, shown as they come."""
    def append(self, line):
        print(line, flush=True)
        super().append(line)

    def __iadd__(self, more):
        for line in more:
            self.append(line)
        return self


def scenes(which):
    out = []
    for name, m in golden_masks():
        H, W = m.shape
        img, _ = oracle.synthetic_image(H, W, noise=0.01)
        out.append((f"{H} x {W} ({name.split('/')[-1][:24]})", img, m.astype(np.float32)[..., None]))
    if which == "small":
        return out[3:4]
    for n in (512, 1024):
        img, mask = oracle.synthetic_image(n, noise=0.01)
        out.append((f"{n} x {n} (synthetic, centred hole)", img, mask))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="all", choices=["all", "small"])
    ap.add_argument("--no-search", action="store_true", help="skip the whole-image rows (prepare_image, search_image)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = ops.select_device("cuda:0")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    warnings.simplefilter("ignore")
    alex = proposal.AlexConv1(None, device=dev, allow_random=True)
    lines = Lines()
    lines += [f"search_front_time: host path against --front_end gpu, {args.reps} alternated windows per row after one warm-up of each, host "
             f"clock around a device synchronise, median (min..max) in ms; {torch.cuda.get_device_name(dev)}; {os.cpu_count()} host CPUs "
             f"visible, torch threads {torch.get_num_threads()}"]
    flags = ["--random-trunks", "--rng_mode", "fast", "--device", "cuda:0"]
    with tempfile.TemporaryDirectory() as tmp:
        for k, (title, img, mask) in enumerate(scenes(args.shapes)):
            H, W = mask.shape[:2]
            im8 = np.uint8(np.clip(img * mask, 0, 1) * 255)
            m8 = np.uint8(mask[..., 0])
            known = mask[..., 0].astype(np.float64)
            lines.append(f"-- {title}: map {H // 4} x {W // 4}, known share {known.mean():.3f}")
            (a_h, m_h), (a_g, m_g), th, tg = alternated(lambda: proposal.im2act(im8, m8, gray_only=True, device=dev),
                                                        lambda: proposal.im2act(im8, m8, gray_only=True, device=dev, front_end="gpu"), args.reps)
            lines.append(row("gray + resizes + mask (im2act, gray)", th, tg)[0] + ("" if torch.equal(a_h, a_g) else "   RESULTS DIFFER"))
            e_h, e_g, th, tg = alternated(lambda: proposal.act2edge(a_h[:-1], m_h), lambda: proposal.act2edge(a_h[:-1], m_h, front_end="gpu"),
                                          args.reps)
            lines.append(row("edge count, 1 channel (act2edge)", th, tg)[0] + ("" if np.array_equal(e_h.numpy(), e_g.cpu().numpy()) else "   RESULTS DIFFER"))
            a66, m66 = proposal.im2act(im8, m8, conv1=alex, device=dev)
            e_h, e_g, th, tg = alternated(lambda: proposal.act2edge(a66[:-1], m66), lambda: proposal.act2edge(a66[:-1], m66, front_end="gpu"),
                                          args.reps)
            lines.append(row("edge count, 65 channels (act2edge)", th, tg)[0] + ("" if np.array_equal(e_h.numpy(), e_g.cpu().numpy()) else "   RESULTS DIFFER"))
            known_d = torch.from_numpy(known).to(dev)
            d_h, d_g, th, tg = alternated(lambda: ndimage.distance_transform_edt(known), lambda: frontend.distance_sq(known_d), args.reps)
            same = np.array_equal(np.rint(d_h ** 2), d_g.cpu().numpy())
            r, edt_h, _ = row("distance transform", th, tg)
            lines.append(r + ("" if same else "   RESULTS DIFFER"))
            n_min = frontend.n_min(H, W)
            c_h, c_g, th, tg = alternated(lambda: search.find_mask_centroid(known), lambda: ops.far_points(d_g, 3, n_min).cpu().tolist(), args.reps)
            sel_h = [max(t - edt_h, 0.0) for t in th]
            lines.append(row("far-point selection (host: by difference)", sel_h, tg)[0])
            c_h, c_g, th, tg = alternated(lambda: search.find_mask_centroid(known), lambda: frontend.find_mask_centroid(known_d), args.reps)
            lines.append(row("pseudo-mask centroids (transform + selection)", th, tg)[0] +
                         ("   same centroids" if c_h == c_g else f"   centroids differ (tied distances): host {c_h[0]} gpu {c_g[0]}"))
            if args.no_search:
                continue
            src = nio.write_detected_dir(os.path.join(tmp, f"in{k}", "scene"), img, mask, np.ones_like(mask), [[0, 0]], [[1, 1]], [[[1, 0], [0, 1]]])
            pa = {fe: search.parse(["--datadir", src, "--outdir", os.path.join(tmp, f"out{k}"), "--front_end", fe] + flags) for fe in ("host", "gpu")}
            _, imgs, conv1, trunks = search._load(pa["host"])
            search._load(pa["gpu"])
            f32 = imgs[0].astype(np.float32)
            prep = lambda fe: search.prepare_image(f32, imgs[2], imgs[3], pa[fe], conv1, trunks)       # noqa: E731
            p_h, p_g, th, tg = alternated(lambda: prep("host"), lambda: prep("gpu"), args.reps)
            same = len(p_h[0]) == len(p_g[0]) and all(np.array_equal(x[1], y[1]) and x[2] == y[2] for x, y in zip(p_h[0], p_g[0]))
            lines.append(row("search.prepare_image, whole", th, tg)[0] + ("   same candidates" if same else "   CANDIDATES DIFFER"))
            full = lambda fe: search.search_image(f32, imgs[2], imgs[3], pa[fe], conv1, trunks)          # noqa: E731
            try:
                s_h, s_g, th, tg = alternated(lambda: full("host"), lambda: full("gpu"), max(2, args.reps // 2))
            except NppError as e:                                          # a size the ranking itself refuses, on either path
                lines.append(f"{'search.search_image, whole':44s} not run on either path: {e}")
                continue
            lines.append(row("search.search_image, whole (300-iteration fits)", th, tg)[0] +
                         ("   same ranking" if s_h["distances"] == s_g["distances"] else "   ranking distances differ (tied centroids or fit order)"))
    text = "\n".join(lines)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
