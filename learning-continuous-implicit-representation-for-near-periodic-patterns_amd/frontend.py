"""The image work in front of the periodicity search on the GPU (`--front_end gpu`): the device twins of the host
functions the search runs before its candidate fits -- cvlite.py's OpenCV restatements (NPP_proposal/feature_searching.py:14-75,
utils/miscs.py:22-48) and search.find_mask_centroid / pseudo_mask_split (utils/miscs.py:53-96, loaders/loaders.py:34-54).  Every
function is named after its host twin, takes and returns device tensors and equals the twin bit for bit, with one stated
exception: the far-point walk orders the pixels by LARGEST DISTANCE FIRST, TIES BY SMALLEST ROW-MAJOR INDEX
(np.argsort(-dis, kind="stable")), where the host function keeps whatever order NumPy's default sort gives tied distances.  The
two agree wherever no accepted distance is tied; this path is the one that does not depend on the host's sort.

Kernels: csrc/npp_frontend.hip (include/npp_hip.h), through ops.py.  What crosses to the host: the hysteresis' "changed" flag per
batch of rounds, whether the mask has an unknown pixel, and the up to topk (index, d^2) pairs."""
import math

import numpy as np
import torch

from . import ops

_HYSTERESIS_ROUNDS = 8           # launches per look at the flags: rounds after the fixed point are no-ops, a look is a sync


def _dev_tensor(a, device=None):
    """A tensor as it is (moved to `device` if one is given), anything else uploaded from NumPy."""
    if isinstance(a, torch.Tensor):
        return a if device is None else a.to(ops.select_device(device))
    return torch.from_numpy(np.ascontiguousarray(a)).to(ops.select_device("cuda" if device is None else device))


def _chw(img_u8, name):
    """(h,w) | (C,h,w) uint8 -> ((C,h,w) contiguous, had a channel axis)."""
    if not isinstance(img_u8, torch.Tensor) or img_u8.dtype != torch.uint8 or img_u8.dim() not in (2, 3):
        raise TypeError(f"{name}: expected an (h, w) or (C, h, w) uint8 device tensor")
    return (img_u8[None] if img_u8.dim() == 2 else img_u8).contiguous(), img_u8.dim() == 3


def resize_nearest(img_u8, dsize):
    """cvlite.resize_nearest on an (H,W) uint8 device tensor; dsize = (w, h)."""
    return ops.resize_nearest_u8(img_u8.contiguous(), dsize)


def resize_linear_u8(img_u8, dsize):
    """cvlite.resize_linear_u8 on an (H,W) uint8 device tensor; dsize = (w, h)."""
    return ops.resize_linear_u8(img_u8.contiguous(), dsize)


def gaussian_blur3_u8(img_u8):
    """cvlite.gaussian_blur3_u8 on (h,w), or on every channel of (C,h,w) in one launch."""
    x, batched = _chw(img_u8, "img_u8")
    out = ops.gaussian_blur3_u8(x)
    return out if batched else out[0]


def normalize_to_uint8(act):
    """cvlite.normalize_to_uint8(act, channel_idx=(1, 2)) on a (C,h,w) fp32 device tensor."""
    return ops.normalize_u8(act.contiguous().float())


def _marks(img_chw, low, high):
    """Canny's {0, weak, strong} map after the hysteresis: rounds until one marks nothing (the fixed point is unique)."""
    marks = ops.canny_mark(img_chw, int(math.floor(low)), int(math.floor(high)))
    while int(ops.canny_hysteresis(marks, _HYSTERESIS_ROUNDS)[-1].item()):
        pass
    return marks


def canny_u8(img_u8, low, high):
    """cvlite.canny_u8 on (h,w), or on every channel of (C,h,w) in one launch sequence -> uint8 {0, 255}."""
    x, batched = _chw(img_u8, "img_u8")
    out = ops.canny_finish(_marks(x, low, high))
    return out if batched else out[0]


def _eroded(mask):
    """The mask eroded 4 times (utils/miscs.py:29; scipy's rule: ops.binary_morph) as (h,w) uint8 0 / 1."""
    return ops.binary_morph((mask != 0).to(torch.uint8).contiguous(), 4, False)


def canny_masked(img_u8, mask):
    """cvlite.canny_masked on single-channel images: blur 3 x 3, Canny(10, 100), edges outside the mask eroded 4 times removed.
    img (h,w) or (C,h,w) uint8, mask (h,w) -> uint8 {0, 255} (the host twin returns the same values as float64)."""
    x, batched = _chw(img_u8, "img_u8")
    out = ops.canny_finish(_marks(ops.gaussian_blur3_u8(x), 10, 100)) * _eroded(mask)[None]
    return out if batched else out[0]


def edge_count(activation, mask):
    """The loop of proposal.act2edge without a copy to the host: (C,h,w) fp32 activation, (h,w) mask -> (h,w) fp32, the number of
    channels whose normalised, blurred Canny(10, 100) map has an edge at the pixel, inside the mask eroded 4 times."""
    marks = _marks(ops.gaussian_blur3_u8(normalize_to_uint8(activation)), 10, 100)
    return ops.edge_count(marks, _eroded(mask))


def distance_sq(mask):
    """(H,W) device mask (non-zero = known) -> (H,W) int32: the exact squared Euclidean distance to the nearest zero pixel
    (== rint(scipy.ndimage.distance_transform_edt(mask) ** 2)).  A mask without a zero pixel has no distance: ValueError."""
    if not isinstance(mask, torch.Tensor) or mask.dim() != 2 or mask.numel() == 0:
        raise TypeError("mask: expected a non-empty (H, W) device tensor")
    if max(mask.shape) > ops.EDT_MAX_DIM:
        raise ValueError(f"mask: {tuple(mask.shape)} exceeds {ops.EDT_MAX_DIM} pixels per side")
    known = (mask != 0).to(torch.uint8).contiguous()
    if bool(known.all().item()):
        raise ValueError("distance_sq: the mask has no unknown pixel (no zero to measure the distance to)")
    return ops.edt_sq(known)


def n_min(H, W, threshold_ratio=0.3):
    """The host walk accepts a pixel when np.sqrt(n) >= min(H, W) * threshold_ratio for its integer squared distance n to every
    accepted one; sqrt is monotone, so that is n >= the smallest integer that passes -- computed here by the same float64 rule."""
    thr = min(int(H), int(W)) * threshold_ratio
    n = max(0, int(math.floor(thr * thr)) - 2)
    while np.sqrt(n) < thr:
        n += 1
    return min(n, 2 ** 31 - 1)


def find_mask_centroid(mask, topk=3, threshold_ratio=0.3, device=None):
    """search.find_mask_centroid with the stated tie rule: -> ([[h, w]], [distance]) of up to topk pixels, largest distance to the
    unknown region first, ties by smallest row-major index, pairwise >= threshold_ratio * min(H, W) apart."""
    if not 1 <= int(topk) <= ops.FAR_POINTS_MAX_TOPK:
        raise ValueError(f"topk: expected 1..{ops.FAR_POINTS_MAX_TOPK}, got {topk}")
    m = _dev_tensor(mask, device)
    H, W = m.shape
    rec = ops.far_points(distance_sq(m), int(topk), n_min(H, W, threshold_ratio)).cpu().tolist()
    pairs = [(rec[2 + 2 * k], rec[3 + 2 * k]) for k in range(rec[0])]
    return [[idx // W, idx % W] for idx, _ in pairs], [math.sqrt(d2) for _, d2 in pairs]


def pseudo_mask_split(mask, valid_mask, device=None):
    """search.pseudo_mask_split on the device: -> (pseudo (H,W,1) float64, i_train (n,2) int64, i_val (n,2) int64), the index
    lists in row-major order (torch.nonzero's, which is np.nonzero's)."""
    m = _dev_tensor(mask, device).to(torch.float64)
    m = m.reshape(m.shape[0], m.shape[1])
    v = _dev_tensor(valid_mask, device).to(torch.float64).reshape(m.shape)
    known = m * v
    cents, dist = find_mask_centroid(known)
    pseudo = torch.ones_like(m)
    for (h, w), d in zip(cents, dist):
        hw = int(d / np.sqrt(2) / 1.2)
        pseudo[max(h - hw, 0):h + hw, max(w - hw, 0):w + hw] = 0
    return pseudo[..., None], torch.nonzero(pseudo * known), torch.nonzero((1 - pseudo) * known)
