"""rng_mode="device": the sampler's decisions as GPU launches (include/npp_hip.h "rng_mode=device", csrc/npp_dev_sampler.hip).

What a host core draws per iteration in the other modes -- the patch source, the fake-patch centres, the lattice search for the
real patches (models/sampler.py:242-354) and the N_rand pixel rows (NPP_completion/train.py:172) -- comes from two launches on
the sampler stream that serve every image of a stack at once.  A draw is a pure function of (seed, draw index t, inputs): nothing
is carried between launches, so a pending decision can be dropped and launched again at no cost (a resumed or re-stacked fit).

The host reads two integers per image and draw, (source, k): the launch that decides draw t + 1 is enqueued when draw t is
materialised and its record is copied to pinned memory behind an event, so the read waits on work enqueued an iteration earlier.
"""
import ctypes as C

import numpy as np
import torch

from . import ops
from ._lib import DevImage, lib, check

SOURCES = ("val", "train", "same")


def make_image(sat, pool_val, pool_train, n_pool_val, n_pool_train, n_train, shifts_dydx, invalid_ratio, seed, H, W, P):
    """-> npp_dev_image.  sat / pool_val / pool_train: ADDRESSES (device memory for the launches, host memory for the twins) of the
    int32 summed-area table and the bounds-filtered (row, col) pools; shifts_dydx = ((dy, dx), (dy, dx))."""
    im = DevImage()
    im.sat, im.pool_val, im.pool_train = sat, pool_val, pool_train
    im.n_pool_val, im.n_pool_train, im.n_train = int(n_pool_val), int(n_pool_train), int(n_train)
    for i, v in enumerate(np.asarray(shifts_dydx, np.float64).reshape(4)):
        im.shifts[i] = float(v)
    im.invalid_ratio = float(invalid_ratio)
    im.seed_lo, im.seed_hi = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    im.H, im.W, im.P = int(H), int(W), int(P)
    return im


def parse_record(rec, topk):
    """One image's record (int32 words, host) -> the draw as GridPatchSampler.draw() returns it (source, k, n, cen, real_cen, weights) plus t."""
    src, k, n_p, t = (int(v) for v in rec[:4])
    if k < 0:
        raise ValueError("Cannot take a larger sample than population when 'replace=False' (rng_mode='device': the "
                         f"{SOURCES[src]!r} pool holds fewer than {n_p} patch centres)")
    nc = n_p * (1 + topk)
    cen = rec[4:4 + 2 * nc].reshape(nc, 2)
    w = rec[4 + 2 * nc:4 + 2 * nc + n_p * topk].view(np.float32)
    d = dict(source=SOURCES[src], k=k, n=n_p, t=t, cen=cen[:n_p].astype(np.int64))
    if SOURCES[src] == "same":
        d.update(real_cen=None, weights=w[:n_p].copy())
    elif k == 0:
        d.update(real_cen=None, weights=None)
    else:
        d.update(real_cen=cen[n_p:n_p + n_p * k].astype(np.float64), weights=w[:n_p * k].copy())
    return d


def _images_blob(images):
    return (DevImage * len(images))(*images)


def decide_host(images, ts, n_p, topk):
    """The decision launch's host twin (npp_dev_sampler_decide_host) -> (M, words) int32 records."""
    M = len(images)
    words = ops.dev_sampler_record_words(n_p, topk)
    rec = np.zeros((M, words), np.int32)
    ts = np.ascontiguousarray(ts, np.uint32)
    blob = _images_blob(images)
    check(lib().npp_dev_sampler_decide_host(C.cast(blob, C.c_void_p), M, ts.ctypes.data_as(C.c_void_p), int(n_p), int(topk),
                                            rec.ctypes.data_as(C.c_void_p), words), "npp_dev_sampler_decide_host")
    return rec


def pixels_host(images, ts, n_pix):
    """The pixel-row launch's host twin -> (M, n_pix) int64."""
    M = len(images)
    if any(n_pix > im.n_train for im in images):
        raise ValueError("Cannot take a larger sample than population when 'replace=False'")
    pix = np.zeros((M, n_pix), np.int64)
    ts = np.ascontiguousarray(ts, np.uint32)
    blob = _images_blob(images)
    check(lib().npp_dev_sampler_pixels_host(C.cast(blob, C.c_void_p), M, ts.ctypes.data_as(C.c_void_p), int(n_pix),
                                            pix.ctypes.data_as(C.c_void_p), n_pix), "npp_dev_sampler_pixels_host")
    return pix


def philox4x32_10(ctr, key):
    return ops.dev_philox4x32_10(ctr, key)


def perm_host(seed, t, stream, N, n):
    """Positions 0..n-1 of the keyed permutation of [0, N) (npp_dev_perm_host)."""
    if n > N:
        raise ValueError("Cannot take a larger sample than population when 'replace=False'")
    out = np.zeros(max(int(n), 1), np.int64)
    check(lib().npp_dev_perm_host(int(seed) & (2 ** 64 - 1), int(t), int(stream), int(N), int(n), out.ctypes.data_as(C.c_void_p)),
          "npp_dev_perm_host")
    return out[:n]


class ImageConsts:
    """The device-resident constants of one image for one patch size: int32 summed-area table, the two filtered pools, and the
    npp_dev_image that points at them."""

    def __init__(self, sat, pool_val, pool_train, n_train, shifts_dydx, invalid_ratio, seed, H, W, P, device):
        if int(sat.max()) >= 2 ** 31 or max(len(pool_val), len(pool_train), n_train) >= 2 ** 31:
            raise ValueError("rng_mode='device': images below 2^31 pixels")
        dev = torch.device(device)

        def up(a):                         # (an empty pool still needs an address: one zero row the launch never reads)
            a = np.ascontiguousarray(a, np.int32)
            return torch.from_numpy(a if a.size else np.zeros((1, 2), np.int32)).to(dev)
        self.sat, self.pool_val, self.pool_train = up(sat), up(pool_val), up(pool_train)
        self.image = make_image(self.sat.data_ptr(), self.pool_val.data_ptr(), self.pool_train.data_ptr(), len(pool_val), len(pool_train),
                                n_train, shifts_dydx, invalid_ratio, seed, H, W, P)


class DeviceDraws:
    """The two launches for the fits of one launch sequence (one CompletionFit, or the M of a StackedFit): per-image constants
    (rebuilt when a patch size changes), a small ring of device records with pinned copies, and at most ONE decision in flight --
    the one for the fits' next draw."""
    RING = 4

    def __init__(self, fits, stream=None):
        self.fits, self.M = list(fits), len(fits)
        f0 = self.fits[0]
        self.device = f0.device
        for f in self.fits:
            if f.rng_mode != "device" or f.patch_sampler is None:
                raise ValueError("DeviceDraws: rng_mode='device' fits with the patch losses (shifts=...) only")
            if (f.patch_num, f.topk, f.N_rand, f.device) != (f0.patch_num, f0.topk, f0.N_rand, f0.device):
                raise ValueError("DeviceDraws: the images of one launch share patch count, topk, N_rand and the device")
        if stream is None:
            stream = torch.cuda.Stream(self.device)
            stream.wait_stream(torch.cuda.current_stream(self.device))      # the constructors' uploads
        self.stream = stream
        self._cfg, self._pending, self._slot = None, None, 0
        self._build()

    def _config(self):
        return tuple((f.patch_size, f.patch_num, f.topk, f.invalid_ratio, f.seed) for f in self.fits)

    def _build(self):
        torch.cuda.synchronize(self.device)                  # (once per patch size: a ring slot may still be read)
        self.consts = []
        for f in self.fits:
            ps = f.patch_sampler
            self.consts.append(ImageConsts(ps.sat, ps.pool_val, ps.pool_train, f.i_train.shape[0], np.stack(ps.selected_shifts),
                                           f.invalid_ratio, f.seed, f.H, f.W, 2 * ps.patch_size_h_half, self.device))
        blob = _images_blob([c.image for c in self.consts])
        self.imgs = torch.from_numpy(np.frombuffer(bytes(blob), np.uint8).copy()).to(self.device)
        f0 = self.fits[0]
        self.n_p, self.topk, self.n_pix = f0.patch_num, f0.topk, f0.N_rand
        self.P = 2 * f0.patch_sampler.patch_size_h_half
        self.n_train_min = min(f.i_train.shape[0] for f in self.fits)
        words = ops.dev_sampler_record_words(self.n_p, self.topk)
        self.rec_dev = [torch.zeros((self.M, words), dtype=torch.int32, device=self.device) for _ in range(self.RING)]
        self.rec_pin = [torch.zeros((self.M, words), dtype=torch.int32).pin_memory() for _ in range(self.RING)]
        self._cfg, self._pending = self._config(), None

    def _ts(self):
        return [f._draw_iter & 0xFFFFFFFF for f in self.fits]

    def launch(self):
        """Enqueue the decision of every fit's NEXT draw (t = its draw index) on the sampler stream, with the pinned copy of the
        records and the event the read waits for."""
        if self._config() != self._cfg:
            self._build()
        ts = self._ts()
        slot = self._slot
        self._slot = (slot + 1) % self.RING
        with torch.cuda.stream(self.stream):
            ops.dev_sampler_decide(self.imgs, self.M, ts, self.n_p, self.topk, self.rec_dev[slot])
            self.rec_pin[slot].copy_(self.rec_dev[slot], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self._pending = (slot, ts, ev, self._cfg)

    def launch_ahead(self):
        """launch(), unless a patch-size decay is due before the next draw: a draw is never launched across a pending decay."""
        if not any(f.decay_due() for f in self.fits):
            self.launch()

    def take(self):
        """-> the M draws of the fits' next iteration (dicts as GridPatchSampler.draw() returns them, plus the device views the
        gather and the row assembly take), each fit's draw index advanced.  Launches the decision now when none is pending or the
        pending one no longer belongs to the fits' state (load_state_dict, a decay)."""
        p, self._pending = self._pending, None
        if p is None or p[1] != self._ts() or p[3] != self._config():
            self.launch()
            p, self._pending = self._pending, None
        slot, ts, ev, _ = p
        ev.synchronize()
        host, dev = self.rec_pin[slot].numpy(), self.rec_dev[slot]
        nc = self.n_p * (1 + self.topk)
        out = []
        for i, f in enumerate(self.fits):
            d = parse_record(host[i], self.topk)
            nk = 0 if d["real_cen"] is None else d["real_cen"].shape[0]
            d.update(P=self.P, device=True, slot=slot,
                     cen_dev=dev[i, 4:4 + 2 * nc].view(nc, 2)[:self.n_p + nk],
                     w_dev=None if d["weights"] is None else dev[i, 4 + 2 * nc:4 + 2 * nc + d["weights"].shape[0]].view(torch.float32))
            f._draw_iter += 1
            out.append(d)
        return out

    def pixels(self, draws, pix):
        """The pixel-row launch for the draws take() returned: pix (M, n_pix) int64, written in place on the current stream."""
        return ops.dev_sampler_pixels(self.imgs, self.M, [d["t"] & 0xFFFFFFFF for d in draws], self.n_pix, pix, self.n_train_min)
