#!/usr/bin/env python3
"""Adaptive supersampling of view renders: what the list indirection costs per chain row, and what a receding view gains.

In one process, alternated window by window (K = 3, W = 256 and 512, bf16 chain, a 2048^2 canvas):
  (a) uni{S}_a  the uniform view launches of the identity view at supersample = S, S = 1, 2, 4 (chunks of 4 Mi chain rows)
      list{S}   the listed launches holding ALL pixels of that canvas at the same S, in the same chunks: the same rows, each through
                the index list (the bits are the uniform launch's, asserted)
      uni{S}_b  uni{S}_a again: uni_b / uni_a is the A/A spread the ratio list / uni_a is read against
  (b) auto8     render_view(supersample=8) of a receding view for which `auto` is 8
      adaptive  render_view(supersample="adaptive") of it: class launch + compaction + listed launches
                (every pixel is the pixel of the uniform launch of its class; checked on the classes 8 and 0 here, which need no
                further uniform render)
      The matrix, its class shares and its chain-row ratio come from the host twin; the ratio must be at most 0.5 (a condition on
      the input, checked before the GPU is touched).
  (c) classes   the class launch alone
Median of --windows windows of --reps runs each after warm-up.

    python tools/render_adaptive_time.py [--windows 5] [--reps 1] [--out profiles/render_adaptive_time.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import oracle  # noqa: E402
from npp_amd import ops, view  # noqa: E402
from npp_amd.model import NPPNet  # noqa: E402

# d = 1 - 3 i / 8192 falls from 1 at the top canvas row to 0.2504 at row 2047: density 1 / d^1.5 from 1 to 7.98 (dyadic entries)
RECEDING = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-3.0 / 8192, 0.0, 1.0]])
CHUNK = 1 << 22


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--size", type=int, default=2048, help="side of the canvas")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    N, K = args.size, 3
    cls_host = view.supersample_classes(RECEDING, (N, N))
    shares, rows, ratio, top = view.class_rows(cls_host, auto=view.supersample_for(RECEDING, (N, N)))
    if top != 8 or not ratio <= 0.5:
        raise SystemExit(f"the receding view must have auto = 8 and a chain-row ratio <= 0.5 at this size: auto {top}, ratio {ratio:.3f}")
    dev = torch.device("cuda:0")
    lines = [f"render_adaptive_time: {N}^2 canvas, K = {K}, bf16 chain, median of {args.windows} windows x {args.reps} runs, "
             f"{torch.cuda.get_device_name(dev)}",
             "(b) receding view " + np.array2string(RECEDING.reshape(-1), separator=", ", max_line_width=200) + ": auto = 8; " +
             view.adaptive_note(cls_host, auto=8)]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(f, reps):
        e0.record()
        for _ in range(reps):
            f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps
    total = N * N
    eye = ops.view_arg(0, total, N, np.eye(3))
    every = torch.arange(total, dtype=torch.int64, device=dev)
    out = torch.empty((total, 3), dtype=torch.float32, device=dev)
    out2 = torch.empty((total, 3), dtype=torch.float32, device=dev)
    inside = torch.empty(total, dtype=torch.uint8, device=dev)
    inside2 = torch.empty(total, dtype=torch.uint8, device=dev)
    cls = torch.empty(total, dtype=torch.uint8, device=dev)
    for W in (256, 512):
        angles, periods, _ = oracle.synthetic_periodicity(N, K)
        net = NPPNet(angles, periods, oracle.SEED0_FREQS, (N, N), params=oracle.init_params(K, W=W, seed=0), device=dev, ksplit=1, width=W)
        kw = dict(precision="bf16", out_act=1, width=W)

        def uniform(ss, o=out, i=inside):
            chunk = CHUNK // (ss * ss)
            for s0 in range(0, total, chunk):
                ops.render(ops.view_arg(s0, chunk, N, np.eye(3)), net.cfg, net._wf_pack(), net.params, out=o[s0:s0 + chunk],
                           inside=i[s0:s0 + chunk], supersample=ss, **kw)

        def listed(ss, o=out2, i=inside2):
            chunk = CHUNK // (ss * ss)
            for s0 in range(0, total, chunk):
                ops.render(eye, net.cfg, net._wf_pack(), net.params, out=o, inside=i, supersample=ss, pixels=every[s0:s0 + chunk], **kw)
        cases = {}
        for ss in (1, 2, 4):
            out2.fill_(-1.0)
            inside2.fill_(9)
            uniform(ss)
            listed(ss)
            assert torch.equal(out.view(torch.int32), out2.view(torch.int32)) and torch.equal(inside, inside2), (W, ss)
            cases[f"uni{ss}_a"] = lambda ss=ss: uniform(ss)
            cases[f"list{ss}"] = lambda ss=ss: listed(ss)
            cases[f"uni{ss}_b"] = lambda ss=ss: uniform(ss)
        a8, i8 = net.render_view((N, N), RECEDING, supersample=8, return_inside=True)
        ad, iad, cad = net.render_view((N, N), RECEDING, supersample="adaptive", return_inside=True, return_classes=True)
        assert np.array_equal(cad.cpu().numpy(), cls_host) and torch.equal(iad, i8)
        sel = (cad == 8) | (cad == 0)
        assert torch.equal(ad.view(torch.int32)[sel], a8.view(torch.int32)[sel])
        del a8, i8, ad, iad, cad, sel
        cases["auto8"] = lambda: net.render_view((N, N), RECEDING, supersample=8, return_inside=True)
        cases["adaptive"] = lambda: net.render_view((N, N), RECEDING, supersample="adaptive", return_inside=True)
        cases["classes"] = lambda: ops.view_ss_classes(ops.view_arg(0, total, N, RECEDING), (N, N), cls, inside)
        for f in cases.values():                                   # warm-up
            f()
        torch.cuda.synchronize()
        t = {k: [] for k in cases}
        for _ in range(args.windows):
            for k, f in cases.items():                             # alternated
                t[k].append(window(f, args.reps))
        med = {k: float(np.median(v)) for k, v in t.items()}
        for k in cases:
            lines.append(f"W={W:4d} {k:8s} {med[k]:9.3f} ms   (spread {min(t[k]):.3f}..{max(t[k]):.3f} ms)")
        for ss in (1, 2, 4):
            a, aa = med[f"list{ss}"] / med[f"uni{ss}_a"], med[f"uni{ss}_b"] / med[f"uni{ss}_a"]
            lines.append(f"W={W:4d} (a) S={ss}: list / uni_a = {a:.4f}   A/A uni_b / uni_a = {aa:.4f}   -> "
                         f"{'inside' if abs(a - 1.0) <= abs(aa - 1.0) else 'OUTSIDE'} the A/A spread")
        r = med["adaptive"] / med["auto8"]
        lines.append(f"W={W:4d} (b) adaptive / auto8 = {r:.4f} at a chain-row ratio of {ratio:.4f}: adaptive is "
                     f"{'FASTER' if r < 1.0 else 'NOT faster'} than uniform auto on this view")
        lines.append(f"W={W:4d} (c) class launch alone: {med['classes']:.3f} ms for {total} pixels")
        del net, cases
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
