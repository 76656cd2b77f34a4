"""Independent restatements for the tests of the search front end (npp_amd.frontend): the far-point walk of utils/miscs.py:53-96
with the tie rule the GPU path states (np.argsort(-dis, kind="stable"): largest distance first, ties by smallest row-major index),
whether a walk's result depends on that rule at all, the integer threshold n_min by plain search, the hysteresis fixed point of a
{0, weak, strong} map by labelling, and the fixture masks.  NumPy / SciPy only."""
import os

import numpy as np
import scipy.ndimage as ndimage

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_masks():
    """[(name, (H,W) uint8 0 / 1 mask, 1 = known)] of tests/golden/g15_masks.npz."""
    g = np.load(os.path.join(GOLDEN, "g15_masks.npz"))
    out = []
    for k, (shape, name) in enumerate(zip(g["shapes"], g["names"])):
        H, W = int(shape[0]), int(shape[1])
        out.append((str(name), np.unpackbits(g[f"bits_{k}"])[:H * W].reshape(H, W).astype(np.uint8)))
    return out


def n_min(H, W, threshold_ratio=0.3):
    """The smallest integer n with np.sqrt(n) >= min(H, W) * threshold_ratio, by counting up from zero."""
    thr = min(H, W) * threshold_ratio
    n = 0
    while not np.sqrt(n) >= thr:
        n += 1
    return n


def find_mask_centroid_stable(mask, topk=3, threshold_ratio=0.3):
    """search.find_mask_centroid with a stable sort -> (centroids [[h, w]], distances, unique): `unique` is True when, in every
    round, the accepted distance occurs once among the pixels eligible in that round (those far enough from all centroids accepted
    before) -- then no tie rule can change the result."""
    m = np.asarray(mask)
    H, W = m.shape
    dis = ndimage.distance_transform_edt(m).reshape(-1)
    order = np.argsort(-dis, kind="stable")
    thr = min(H, W) * threshold_ratio
    yy, xx = np.divmod(np.arange(H * W), W)
    eligible = np.ones(H * W, bool)
    cents, sel, unique = [], [], True
    for idx in order:
        if not eligible[idx]:
            continue
        unique = unique and int((eligible & (dis == dis[idx])).sum()) == 1
        h, w = int(idx // W), int(idx % W)
        cents.append([h, w])
        sel.append(float(dis[idx]))
        eligible &= np.sqrt((yy - h) ** 2 + (xx - w) ** 2) >= thr
        eligible[idx] = False                                              # (threshold 0: a pixel is still taken once)
        if len(cents) == topk:
            break
    return cents, sel, unique


def hysteresis(marks):
    """{0, 1 weak, 2 strong} -> bool: the pixels of the 8-connected components of (marks > 0) that hold a strong pixel."""
    marks = np.asarray(marks)
    lab, n = ndimage.label(marks > 0, structure=np.ones((3, 3), int))
    hit = np.zeros(n + 1, bool)
    hit[np.unique(lab[marks == 2])] = True
    hit[0] = False
    return hit[lab]


def spiral_marks(n=64):
    """An n x n map with a one-pixel-wide weak spiral (arms two pixels apart) whose only strong pixel is its inner end."""
    m = np.zeros((n, n), np.uint8)
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))
    y, x, d = 0, 0, 0
    m[0, 0] = 1
    length = 1
    while True:
        for turn in (0, 1):                                                # straight on while it can, else one turn to the right
            dy, dx = dirs[(d + turn) % 4]
            ny, nx, by, bx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if not (0 <= ny < n and 0 <= nx < n) or m[ny, nx]:
                continue
            if 0 <= by < n and 0 <= bx < n and m[by, bx]:                  # keep one free pixel between the arms
                continue
            d = (d + turn) % 4
            break
        else:
            break
        y, x = ny, nx
        m[y, x] = 1
        length += 1
    m[y, x] = 2
    return m, length
