#!/usr/bin/env python3
"""What graph_iteration=True saves on the host and costs on the device, on one MI355X, in one command.

At BASELINE config c2 (512^2, K = 3, W = 256, 8192 pixel rows + 2 patches, fixed-seed trunks), with rng_mode="device" and with
the reference stream (prefetch = 8: the command line's default path), three fits per mode in ALTERNATED windows of one process:
the eager loop twice (A, A': the A/A spread of the yardstick) and the graph-mode loop.  Per window

  * host time per iteration: wall time of the step_full() calls of the window with no synchronisation inside it (it contains the
    host's waits where the loop throttles it: the pinned rings, the two sets of batch buffers), and beside it the CPU time of
    the calling thread;
  * device time per iteration: device events around the window (the window's iterations are all enqueued before the second
    event is waited for).

Then the same with the process confined to 2 cores (os.sched_setaffinity on every thread of itself): the host beside other load.  All loops run
under a torch.cuda.stream(...) of their own (a capture cannot begin on the default stream).  Medians over the windows
(min..max).  Nothing here is a gate; VERDICT.md expects <= 0.05 ms of host time against 0.255 ms.

    python tools/graph_iteration_time.py [--windows 5] [--iters 100] [--warm 200] [--out profiles/graph_iteration_time.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from npp_amd import synthetic as syn  # noqa: E402
from npp_amd.fit import CompletionFit  # noqa: E402


def fmt(ts):
    return f"{float(np.median(ts)):8.4f} ({min(ts):7.4f}..{max(ts):7.4f})"


def make(dev, mode, graph, H=512, K=3):
    img, mask = syn.synthetic_image(H)
    angles, periods, shifts = syn.synthetic_periodicity(H, K)
    return CompletionFit(img, mask, angles, periods, syn.SEED0_FREQS, syn.init_params(K, seed=0), device=dev, N_rand=8192, shifts=shifts,
                         seed=0, rng_mode=mode, prefetch=0 if mode == "device" else 8, graph_iteration=graph)


def confine(cores):
    """Every thread of this process (the loop, the sampler's producer, the runtime's own) onto `cores`."""
    for tid in os.listdir("/proc/self/task"):
        try:
            os.sched_setaffinity(int(tid), cores)
        except OSError:                                           # (a thread that ended meanwhile)
            pass


def window(f, iters, stream):
    """-> (host wall ms, device ms, CPU ms of the calling thread) per iteration of one window."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream.synchronize()
    a.record(stream)
    c0, t0 = time.thread_time(), time.perf_counter()
    for _ in range(iters):
        f.step_full()
    c1, t1 = time.thread_time(), time.perf_counter()
    b.record(stream)
    b.synchronize()
    return (t1 - t0) / iters * 1e3, a.elapsed_time(b) / iters, (c1 - c0) / iters * 1e3


def measure(fits, windows, iters, stream):
    host, devt, cpu = {k: [] for k in fits}, {k: [] for k in fits}, {k: [] for k in fits}
    for _ in range(windows):
        for k, f in fits.items():
            h, d, c = window(f, iters, stream)
            host[k].append(h)
            devt[k].append(d)
            cpu[k].append(c)
    return host, devt, cpu


def report(lines, title, fits, host, devt, cpu):
    lines.append(f"-- {title}")
    for k in fits:
        lines.append(f"{k:10s} host {fmt(host[k])}   device {fmt(devt[k])}   thread CPU {fmt(cpu[k])}")
    for name, t in (("host", host), ("device", devt), ("cpu", cpu)):
        ma, mb, mg = (float(np.median(t[k])) for k in fits)
        lines.append(f"{name:6s}: A/A spread of the eager loop {abs(ma - mb):.4f} ms; graph - eager A {mg - ma:+.4f} ms "
                     f"({'within' if abs(mg - ma) <= abs(ma - mb) else 'outside'} the A/A spread)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100, help="iterations per window")
    ap.add_argument("--warm", type=int, default=200, help="iterations before the first window (every key captured)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    stream = torch.cuda.Stream(dev)
    cores = sorted(os.sched_getaffinity(0))
    lines = [f"graph_iteration_time: {torch.cuda.get_device_name(dev)}; c2 (512^2, K = 3, W = 256); ms per iteration; medians of "
             f"{args.windows} alternated windows (min..max), {args.iters} iterations per window, {args.warm} before the first"]
    for mode in ("device", "reference"):
        fits = {"eager A": make(dev, mode, False), "eager A'": make(dev, mode, False), "graph": make(dev, mode, True)}
        stream.wait_stream(torch.cuda.default_stream(dev))
        try:
            with torch.cuda.stream(stream):
                for f in fits.values():
                    for _ in range(args.warm):
                        f.step_full()
                st = fits["graph"].graph_stats
                lines.append(f"== rng_mode {mode!r}{'' if mode == 'device' else ' with prefetch 8'}: after the warm-up {st['captured']} graphs "
                             f"captured, {st['replayed']} iterations replayed, {st['eager']} launch by launch")
                report(lines, f"{len(cores)} cores", fits, *measure(fits, args.windows, args.iters, stream))
                confine(set(cores[:2]))
                try:
                    report(lines, "confined to 2 cores", fits, *measure(fits, args.windows, args.iters, stream))
                finally:
                    confine(set(cores))
                st2 = fits["graph"].graph_stats
                lines.append(f"(graph-mode fit during the windows: {st2['replayed'] - st['replayed']} replayed, {st2['eager'] - st['eager']} launch by launch)")
        finally:
            stream.synchronize()
            for f in fits.values():
                f.close()
        del fits
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
