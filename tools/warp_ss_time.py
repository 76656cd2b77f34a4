#!/usr/bin/env python3
"""The antialiased image warp: what S x S samples per canvas pixel cost in the launch (npp_warp_image_u8_ss), and whether the
point launch (npp_warp_image_u8) kept its time.

A 3-channel 4096^2 source under a projective map onto a 512^2 and a 2048^2 canvas, bilinear, mean.  In one process, alternated
window by window per canvas:
  s1_a     npp_warp_image_u8_ss at ss = 1
  s2 s4 s8 ... at ss = 2, 4, 8; each is also given as a ratio to S^2 x the s1_a time of this run (1 = the samples cost what S^2
           point launches would)
  point    npp_warp_image_u8, the point launch
  s1_b     s1_a again: s1_b / s1_a is the A/A spread the ratios are read against
Every launch writes into buffers allocated before the windows (the times hold no allocation) and is timed with device events;
median of --windows windows after warm-up, each of as many launches as fill --window-ms (a point launch takes microseconds: a
window of a few launches would measure the enqueue).  Every S is first compared with the host twin byte for byte on
the 512^2 canvas, whose wall time is recorded.

With --parent-lib PATH (a libnpp_hip.so built from the commit before this entry point) the point launch is timed against that
library's: parent_a, new, parent_b alternated, both modes; the median of `new` must lie inside what the windows of parent_a and
parent_b span (the two medians' ratio is printed beside it).

    python tools/warp_ss_time.py [--windows 9] [--window-ms 100] [--parent-lib PATH] [--out profiles/warp_ss_time.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import npp_amd  # noqa: E402
from npp_amd import ops, view  # noqa: E402
from npp_amd._lib import SYMBOLS  # noqa: E402

SRC = 4096


def projective(n):
    """Most of the SRC^2 source on an n^2 canvas: SRC / n source pixels per canvas pixel, a little more towards one corner."""
    k = 0.9 * SRC / n
    return np.array([[k, 0.04 * k, 30.0], [-0.03 * k, k, 150.0], [0.04 / n, 0.02 / n, 1.0]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--window-ms", type=float, default=100.0, help="device time a window is filled to")
    ap.add_argument("--parent-lib", default=None, help="libnpp_hip.so of the parent commit, for the point launch's A/B")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    L = npp_amd.lib()
    lines = [f"warp_ss_time: {SRC}^2 x 3 source, projective map, bilinear, mean; median of {args.windows} windows of {args.window_ms:g} ms, "
             f"device events, {torch.cuda.get_device_name(dev)}"]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(f, reps):
        e0.record()
        for _ in range(reps):
            f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    def alternate(cases):
        reps = {}
        for k, f in cases.items():                                     # warm-up, and how many launches fill a window
            f()
            reps[k] = max(5, int(args.window_ms / max(window(f, 20), 1e-4)))
        t = {k: [] for k in cases}
        for _ in range(args.windows):
            for k, f in cases.items():
                t[k].append(window(f, reps[k]))
        return t, {k: float(np.median(v)) for k, v in t.items()}
    src = np.random.RandomState(0).randint(0, 256, (SRC, SRC, 3)).astype(np.uint8)
    d_src = torch.from_numpy(src).to(dev)

    def launcher(lib, n, mode, ss=None):
        """One launch of lib's point entry (ss None) or antialiased entry into buffers of its own."""
        out = torch.empty((n, n, 3), dtype=torch.uint8, device=dev)
        inside = torch.empty((n, n), dtype=torch.uint8, device=dev)
        m = (C.c_double * 9)(*projective(n).reshape(9))
        s, o, i, st = ops._p(d_src), ops._p(out), ops._p(inside), ops._stream()
        if ss is None:
            return lambda: ops.check(lib.npp_warp_image_u8(s, SRC, SRC, 3, n, n, m, mode, o, i, st), "npp_warp_image_u8")
        return lambda: ops.check(lib.npp_warp_image_u8_ss(s, SRC, SRC, 3, n, n, m, mode, ss, 0, o, i, st), "npp_warp_image_u8_ss")
    for n in (512, 2048):
        lo, hi = view.sampling_density(projective(n), (n, n))
        lines.append(f"canvas {n}^2: {lo:.2f} .. {hi:.2f} source pixels per canvas pixel")
        host_ms = {}
        if n == 512:
            for ss in view.SUPERSAMPLES:
                got, gin = view.warp_image(d_src, projective(n), (n, n), "bilinear", device=dev, supersample=ss)
                t0 = time.perf_counter()
                want, win = view.warp_image(src, projective(n), (n, n), "bilinear", supersample=ss)
                host_ms[ss] = (time.perf_counter() - t0) * 1e3
                assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(gin.cpu().numpy(), win), ss
        cases = {"s1_a": launcher(L, n, 1, 1), "s2": launcher(L, n, 1, 2), "s4": launcher(L, n, 1, 4), "s8": launcher(L, n, 1, 8),
                 "point": launcher(L, n, 1), "s1_b": launcher(L, n, 1, 1)}
        t, med = alternate(cases)
        for k, ss in (("s1_a", 1), ("s2", 2), ("s4", 4), ("s8", 8), ("point", 1), ("s1_b", 1)):
            lines.append(f"canvas {n:4d}^2 {k:5s} kernel {med[k] * 1e3:10.1f} us  (spread {min(t[k]) * 1e3:.1f}..{max(t[k]) * 1e3:.1f})   "
                         f"{n * n * ss * ss / (med[k] * 1e-3) / 1e9:7.2f} Gsample/s   / (S^2 x s1_a) = {med[k] / (ss * ss * med['s1_a']):.3f}" +
                         (f"   host twin {host_ms[ss]:9.1f} ms, equal byte for byte" if k in ("s1_a", "s2", "s4", "s8") and host_ms else ""))
        lines.append(f"canvas {n:4d}^2 A/A s1_b / s1_a = {med['s1_b'] / med['s1_a']:.4f}   point / s1_a = {med['point'] / med['s1_a']:.4f}")
    if args.parent_lib:
        P = C.CDLL(os.path.abspath(args.parent_lib))
        P.npp_warp_image_u8.restype, P.npp_warp_image_u8.argtypes = SYMBOLS["npp_warp_image_u8"]
        for n in (512, 2048):
            for mode, name in ((1, "bilinear"), (0, "nearest")):
                t, med = alternate({"parent_a": launcher(P, n, mode), "new": launcher(L, n, mode), "parent_b": launcher(P, n, mode)})
                aa, r = med["parent_b"] / med["parent_a"], med["new"] / med["parent_a"]
                lo, hi = min(t["parent_a"] + t["parent_b"]), max(t["parent_a"] + t["parent_b"])       # what the parent's own windows span
                verdict = "inside" if lo <= med["new"] <= hi else "OUTSIDE"
                lines.append(f"npp_warp_image_u8 {n:4d}^2 {name:8s}: parent_a {med['parent_a'] * 1e3:8.3f} us  new {med['new'] * 1e3:8.3f} us  "
                             f"parent_b {med['parent_b'] * 1e3:8.3f} us   new / parent_a = {r:.4f}   A/A parent_b / parent_a = {aa:.4f}   "
                             f"parent windows {lo * 1e3:.3f}..{hi * 1e3:.3f} us   -> new is {verdict} them")
    else:
        lines.append("npp_warp_image_u8 against the parent commit: not measured (no --parent-lib)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
