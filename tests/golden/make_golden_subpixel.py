#!/usr/bin/env python3
"""g15: the reference's embedder and NPP_Net at NON-INTEGER positions, including negative ones and ones past the image border
(the network is a function of the plane; rendering a fit at sub-pixel density or beyond its canvas evaluates it there).

Same import recipe as make_golden.py (the reference's own modules, CPU, fp32).  K = 3, W = 256, snake, res = (211, 325) (the size
of the reference's first completion sample); parameters from oracle.init_params(3, W=256, seed=PARAM_SEED) loaded with
load_state_dict(strict=False) -- only their checksum is stored.  Coordinates: a 16 x 16 patch of a 2.5x canvas at origin
(-17.25, 40.5) (y = y0 + i / 2.5, x = x0 + j / 2.5 in fp32, as the grid launches form them) and 256 uniform points in
[-H, 2H) x [-W, 2W).

    python tests/golden/make_golden_subpixel.py       # writes tests/golden/g15_subpixel.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden import import_reference, _net, FREQ_SCALES, FREQ_OFFSETS, ANGLE_OFFSETS, OUT  # noqa: E402
import oracle  # noqa: E402

RES = (211, 325)
ANGLES = np.array([[80.54, 168.69], [80.54, 168.69], [33.3, 121.0]], np.float32)
PERIODS = np.array([[40.77, 36.48], [81.54, 72.96], [17.25, 23.5]], np.float32)
PARAM_SEED = 15
ORIGIN, SCALE, PATCH = (-17.25, 40.5), 2.5, 16


def coords():
    f32 = np.float32
    i, j = np.meshgrid(np.arange(PATCH), np.arange(PATCH), indexing="ij")
    y = f32(ORIGIN[0]) + i.reshape(-1).astype(f32) / f32(SCALE)
    x = f32(ORIGIN[1]) + j.reshape(-1).astype(f32) / f32(SCALE)
    H, W = RES
    rng = np.random.RandomState(15)
    u = np.stack([rng.uniform(-H, 2 * H, 256), rng.uniform(-W, 2 * W, 256)], 1).astype(f32)
    return np.concatenate([np.stack([y, x], 1).astype(f32), u], 0)


def param_checksum(P):
    return np.array([sum(float(np.asarray(v, np.float64).sum()) for v in P.values()),
                     sum(float(np.abs(np.asarray(v, np.float64)).sum()) for v in P.values())])


def g15_subpixel(R):
    torch.manual_seed(0)
    embedder, _ = R["emb"].get_embedder(10, 0, RES)
    freqs = np.array([float(fn.__defaults__[1]) for fn in embedder.embed_fns[1::2]], np.float32)
    c = coords()
    warps, embs = [], []
    for k in range(3):
        ep, d22 = R["emb"].get_embedder(10, 0, RES, selected_angles=torch.Tensor(ANGLES[k]), selected_periods=torch.Tensor(PERIODS[k]),
                                        freq_scales=FREQ_SCALES, freq_offsets=FREQ_OFFSETS, angle_offsets=ANGLE_OFFSETS)
        assert d22 == 22
        v = ep.embed(torch.from_numpy(c.copy()))
        warps.append(v.numpy())
        embs.append(embedder.embed(v).numpy())
    emb = np.concatenate(embs, 1)
    net = _net(R, 3, 256, 21)
    P = oracle.init_params(3, W=256, seed=PARAM_SEED)
    missing, unexpected = net.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()}, strict=False)
    assert not unexpected and all(m.startswith("alpha_linear") for m in missing), (missing, unexpected)
    with torch.no_grad():
        raw = net(None, torch.from_numpy(emb)).numpy()
    out = dict(coords=c, res=np.array(RES, np.int64), angles=ANGLES, periods=PERIODS, freqs=freqs, warp=np.stack(warps, 0),
               emb64=emb[:64].copy(), raw=raw, pred=torch.sigmoid(torch.from_numpy(raw)).numpy(),
               param_seed=np.int64(PARAM_SEED), param_checksum=param_checksum(P), origin=np.array(ORIGIN, np.float32),
               scale=np.float32(SCALE), patch=np.int64(PATCH))
    np.savez_compressed(os.path.join(OUT, "g15_subpixel.npz"), **out)


if __name__ == "__main__":
    g15_subpixel(import_reference())
    print("wrote", os.path.join(OUT, "g15_subpixel.npz"))
