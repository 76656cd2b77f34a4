#!/usr/bin/env python3
"""What the initial coarse segmentation (npp_amd.init_segment) costs, stage by stage, on one MI355X -- and, beside each GPU stage,
the host time of the same stage in plain NumPy (tests/slic_restatement.py, at most 16 threads), which is the only alternative a
user of this build has.

Images: the tests' scene (rotated lattice + planted disc and block + invalid band) at 256^2, 512^2 and 676 x 494 (the largest
sample input of the reference).  GPU stages: a host clock around work that ends in a device synchronise, 2 warm-up runs discarded,
median of --reps runs (min..max beside it).  Host stages: median of --host-reps runs.

    python tools/init_seg_time.py [--reps 9] [--host-reps 3] [--out profiles/init_seg_time.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import slic_restatement as R  # noqa: E402
from npp_amd import init_segment as iseg, ops  # noqa: E402

SP_SIZE, SP_REGUL, NB_CLASSES = 20, 0.1, 3


def timed(f, reps, warmup, sync):
    out, ts = None, []
    for i in range(warmup + reps):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        if sync:
            torch.cuda.synchronize()
        if i >= warmup:
            ts.append(time.perf_counter() - t0)
    return out, float(np.median(ts)) * 1e3, min(ts) * 1e3, max(ts) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    lines = [f"init_seg_time: sp_size {SP_SIZE}, sp_regul {SP_REGUL}, {NB_CLASSES} classes, 10 SLIC rounds; GPU stages: median of {args.reps} runs "
             f"after 2 warm-up runs, host clock around a device synchronise; host stages: median of {args.host_reps} runs; "
             f"{torch.cuda.get_device_name(dev)}; times in ms, (min..max)"]
    m = (SP_SIZE * SP_REGUL) ** 1.5
    for name, n, crop in (("256x256", 256, None), ("512x512", 512, None), ("494x676", 676, 494)):
        img, valid = R.make_scene(n)[:2]
        if crop:
            img, valid = np.ascontiguousarray(img[:crop]), np.ascontiguousarray(valid[:crop])
        H, W = valid.shape
        g = lambda f: timed(f, args.reps, 2, True)                 # noqa: E731
        h = lambda f: timed(f, args.host_reps, 0, False)           # noqa: E731
        rows = []
        # -- per-pixel stages: GPU against the NumPy restatement
        t_img = torch.from_numpy(img).to(dev)
        lab, *t = g(lambda: ops.slic_prepare(t_img, float(img.min()), float(img.max()), m))
        lab_ref, *tr = h(lambda: R.prepare(img) / m)
        rows.append(("prepare (scale, blur, Lab)", t, tr))
        (raw, S), *t = g(lambda: iseg.slic_raw(img, valid, SP_SIZE, SP_REGUL, device=dev))
        (raw_ref, _), *tr = h(lambda: R.slic_raw(img, valid, SP_SIZE, SP_REGUL))
        rows.append(("SLIC: copies + prepare + 10 x (assign, update)", t, tr))
        sp, *t = h(lambda: iseg.enforce_connectivity(raw, 0.5 * S * S, img))
        rows.append(("connectivity repair (host in both)", t, t))
        (_, cen, feats), *t = g(lambda: iseg.superpixel_features(img, sp, device=dev))
        _, *tr = h(lambda: R.features(img, sp))
        rows.append((f"features of {sp.max()} superpixels (with copies)", t, tr))
        # -- per-superpixel stages: host in both
        Xs = iseg.standardise(feats)
        model, *t = h(lambda: iseg.fit_mixture(Xs, NB_CLASSES, 0))
        rows.append(("mixture: 9 restarts of EM (host in both)", t, t))
        proba = iseg.predict_proba(model, Xs)

        def cut():
            e = iseg.superpixel_edges(sp)
            return iseg.graph_cut(iseg.unary_cost(proba), e, iseg.edge_weights(e, Xs, cen), iseg.GC_REGUL)
        _, *t = h(cut)
        rows.append(("edges + alpha-expansion graph cut (host in both)", t, t))
        out, *t = g(lambda: iseg.initial_segmentation(img, valid, NB_CLASSES, SP_SIZE, SP_REGUL, 0, dev))
        host = sum(r[2][0] for r in rows[1:])               # (not run again: the host stages above are the whole of it)
        rows.append(("initial_segmentation, whole call (host: sum of stages)", t, (host, host, host)))
        lines.append(f"-- {name} (H {H}, W {W}; {int(valid.sum())} valid pixels, step S {S:.2f}, {int(raw.max())} centres, "
                     f"{int((raw != raw_ref).sum())} raw labels differ from the restatement's, periodic share {out['period_mask'].mean():.3f})")
        lines.append(f"{'stage':56s} {'this build':>28s} {'NumPy on the host':>30s}")
        for what, a, b in rows:
            lines.append(f"{what:56s} {a[0]:9.2f} ({a[1]:8.2f}..{a[2]:8.2f}) {b[0]:10.2f} ({b[1]:9.2f}..{b[2]:9.2f})")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
