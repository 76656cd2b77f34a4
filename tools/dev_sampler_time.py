#!/usr/bin/env python3
"""What rng_mode="device" costs and saves beside the host draws, on one MI355X, in one command.

  * host CPU time of one draw_batch() (thread CPU time, one core) in "reference", "fast" and "device" mode at BASELINE config c2
    (512^2, K = 3, 8192 pixel rows + 2 patches) and at the 1024^2 remapping shape (the pixel population is the whole image); in
    device mode it is the host's share of the two launches: enqueue, the read of (source, k), the next decision's enqueue;
  * device time of the two launches (npp_dev_sampler_decide / npp_dev_sampler_pixels) for M = 1 and M = 8 images;
  * the complete iteration at c2 for one image: reference mode with its producer thread (prefetch = 8) against device mode, in
    ALTERNATED windows, with a second reference-mode fit in the same rotation: the A/A spread of the yardstick;
  * M = 8 stacked, end to end, in both modes, beside the device-only rate (StackedFit.step_from on a drawn batch).
Rows per iteration = N_rand + n_p P^2 per image.  Medians over the windows (min..max).  Nothing here is a gate.

    python tools/dev_sampler_time.py [--windows 5] [--iters 40] [--out profiles/dev_sampler_time.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from npp_amd import ops, synthetic as syn  # noqa: E402
from npp_amd.fit import CompletionFit  # noqa: E402
from npp_amd.stack import StackedFit  # noqa: E402


def fmt(ts):
    return f"{float(np.median(ts)):9.4f} ({min(ts):8.4f}..{max(ts):8.4f})"


def wall(fn, reps, dev):
    fn()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) / reps * 1e3


def events(fn, reps):
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def make(dev, H, K, mode, i=0, remap=False, **kw):
    img, mask = syn.synthetic_image(H, seed=i)
    angles, periods, shifts = syn.synthetic_periodicity(H, K)
    extra = dict(task="remapping", clear_mask=mask) if remap else {}
    return CompletionFit(img, mask, angles, periods, syn.SEED0_FREQS, syn.init_params(K, seed=i), device=dev, N_rand=8192, shifts=shifts,
                         seed=i, rng_mode=mode, **extra, **kw)


def host_draw_ms(f, n):
    """Thread CPU time and wall time of one draw_batch() (device mode: + the next decision's enqueue), ms."""
    def one():
        f.draw_batch()
        if f.rng_mode == "device":
            f.device_draws().launch_ahead()
    for _ in range(5):
        one()
    torch.cuda.synchronize(f.device)
    c0, w0 = time.thread_time(), time.perf_counter()
    for _ in range(n):
        one()
    c1, w1 = time.thread_time(), time.perf_counter()
    torch.cuda.synchronize(f.device)
    return (c1 - c0) / n * 1e3, (w1 - w0) / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=40, help="complete iterations per window")
    ap.add_argument("--draws", type=int, default=200)
    ap.add_argument("--M", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lines = [f"dev_sampler_time: {torch.cuda.get_device_name(dev)}; ms; medians of {args.windows} alternated windows (min..max), "
             f"{args.iters} iterations per window, {args.draws} draws per host figure"]
    lines.append("-- host time of one draw_batch(), thread CPU ms | wall ms")
    for name, H, K, remap in (("c2 512^2 K=3", 512, 3, False), ("remapping 1024^2 K=3", 1024, 3, True)):
        for mode in ("reference", "fast", "device"):
            f = make(dev, H, K, mode, remap=remap)
            cpu, w = host_draw_ms(f, args.draws)
            lines.append(f"{name:22s} {mode:10s} {cpu:8.4f} | {w:8.4f}")
            f.close()
            del f
    lines.append("-- device time of the two launches at c2 (device events, 50 launches per window)")
    for M in (1, args.M):
        fits = [make(dev, 512, 3, "device", i=i) for i in range(M)]
        from npp_amd.dev_sampler import DeviceDraws
        dd = DeviceDraws(fits, stream=torch.cuda.current_stream(dev))
        pix = torch.zeros((M, dd.n_pix), dtype=torch.int64, device=dev)
        ts = list(range(M))
        td = [events(lambda: ops.dev_sampler_decide(dd.imgs, M, ts, dd.n_p, dd.topk, dd.rec_dev[0]), 50) for _ in range(args.windows)]
        tp = [events(lambda: ops.dev_sampler_pixels(dd.imgs, M, ts, dd.n_pix, pix, dd.n_train_min), 50) for _ in range(args.windows)]
        lines.append(f"M = {M}: decision launch {fmt(td)}   pixel-row launch {fmt(tp)}   (back to back: includes the launch gap)")
        del dd, fits
    lines.append("-- complete iteration at c2, one image (step_full)")
    single = {"reference A (prefetch 8)": make(dev, 512, 3, "reference", prefetch=8),
              "reference A' (prefetch 8)": make(dev, 512, 3, "reference", prefetch=8),
              "device": make(dev, 512, 3, "device")}
    t = {k: [] for k in single}
    for f in single.values():
        for _ in range(10):
            f.step_full()
    for _ in range(args.windows):
        for k, f in single.items():
            t[k].append(wall(f.step_full, args.iters, dev))
    for k in single:
        lines.append(f"{k:28s} {fmt(t[k])}")
    ma, mb, md = (float(np.median(t[k])) for k in single)
    lines.append(f"A/A spread of the reference-mode loop {abs(ma - mb):.4f} ms; device - reference A {md - ma:+.4f} ms "
                 f"({'within' if abs(md - ma) <= abs(ma - mb) else 'outside'} the A/A spread)")
    for f in single.values():
        f.close()
    del single
    M = args.M
    lines.append(f"-- M = {M} stacked at c2")
    stacks = {mode: StackedFit([make(dev, 512, 3, mode, i=i) for i in range(M)]) for mode in ("reference", "device")}
    rows = M * (8192 + stacks["device"].n_p * stacks["device"].P ** 2)
    e2e = {k: [] for k in stacks}
    only = {k: [] for k in stacks}
    for st in stacks.values():
        for _ in range(6):
            st.step_full()
    for _ in range(args.windows):
        for k, st in stacks.items():
            e2e[k].append(wall(st.step_full, args.iters, dev))
    for k, st in stacks.items():
        for _ in range(args.windows):
            b = st.sample()
            only[k].append(wall(lambda: st.step_from(b), 10, dev))
    for k in stacks:
        me, mo = float(np.median(e2e[k])), float(np.median(only[k]))
        lines.append(f"{k:10s} end to end {fmt(e2e[k])} = {rows / me / 1e3:6.2f} M rows/s   device-only {fmt(only[k])} = {rows / mo / 1e3:6.2f} M rows/s"
                     f"   gap {100 * (me / mo - 1):+.1f} %")
    for st in stacks.values():
        st.close()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
