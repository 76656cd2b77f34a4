"""Helper of test_init_segment_cpu.py / test_gpu_init_segment.py (not a test file): the per-pixel steps of the initial coarse
segmentation (npp_amd.init_segment, csrc/npp_slic.hip) restated in plain float64 NumPy / SciPy, one function per kernel, written
from the algorithm's description (include/npp_hip.h "segmentation task") and the reference lines it cites -- not from the kernels.

The per-superpixel host steps (connectivity repair, mixture, graph cut, mask rule) ARE plain NumPy already and live in the package;
`slic` and `pipeline` below call them, so that "restatement pipeline" means: these per-pixel steps + the package's host steps.
Also here: the synthetic scene the purpose tests use.
"""
import numpy as np
import scipy.ndimage as ndi

from npp_amd import init_segment as iseg


# ---- the scene --------------------------------------------------------------------------------------------------------------
def make_scene(n=256):
    """A rotated two-sine lattice (periods 9 and 10.8 px: below the superpixel size, so that a superpixel averages whole periods)
    with two planted non-periodic regions and an invalid band.  -> img uint8 (n,n,3), valid bool, truth (periodic region) bool,
    disc bool, block bool."""
    y, x = np.mgrid[0:n, 0:n].astype(np.float64)
    th = np.deg2rad(20.0)
    u, v = x * np.cos(th) + y * np.sin(th), -x * np.sin(th) + y * np.cos(th)
    base = 0.5 + 0.2 * np.sin(2 * np.pi * u / 9.0) * np.sin(2 * np.pi * v / 10.8)
    img = np.stack([base, 0.9 * base + 0.05, 0.8 * base + 0.1], 2)
    img = img + np.random.RandomState(0).normal(0.0, 0.03, img.shape)
    rs = np.random.RandomState(1)
    disc = (y - 70) ** 2 + (x - 190) ** 2 < 38 ** 2
    block = (y > 200) & (x < 90)
    img[disc] = np.array([0.85, 0.2, 0.15]) + rs.uniform(-0.02, 0.02, (int(disc.sum()), 3))
    img[block] = np.array([0.1, 0.25, 0.7]) + rs.uniform(-0.02, 0.02, (int(block.sum()), 3))
    valid = np.ones((n, n), bool)
    valid[:, :12] = False
    img_u8 = np.uint8(np.rint(np.clip(img, 0.0, 1.0) * 255.0))
    return img_u8, valid, valid & ~disc & ~block, disc, block


def iou(a, b):
    a, b = np.asarray(a, bool), np.asarray(b, bool)
    return float((a & b).sum()) / float((a | b).sum())


# ---- prepare ------------------------------------------------------------------------------------------------------------------
def prepare(img_u8):
    """min-max scale -> Gaussian blur sigma 1 (reflect, truncate 4) -> sRGB to CIELAB (D65).  (3,H,W) float64 in Lab units,
    BEFORE the division by the compactness m."""
    a = img_u8.astype(np.float64)
    lo, hi = a.min(), a.max()
    a = (a - lo) / (hi - lo) if hi > lo else np.zeros_like(a)
    a = np.stack([ndi.gaussian_filter(a[..., c], 1.0, mode="reflect", truncate=4.0) for c in range(3)], 2)
    lin = np.where(a > 0.04045, ((a + 0.055) / 1.055) ** 2.4, a / 12.92)
    M = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
    xyz = lin @ M.T / np.array([0.95047, 1.0, 1.08883])
    f = np.where(xyz > 0.008856, np.cbrt(xyz), 7.787 * xyz + 16.0 / 116.0)
    return np.stack([116.0 * f[..., 1] - 16.0, 500.0 * (f[..., 0] - f[..., 1]), 200.0 * (f[..., 1] - f[..., 2])], 0)


# ---- assign -------------------------------------------------------------------------------------------------------------------
def _d2(lab_px, yx_px, centres, S):
    """(n, K) D2 = |Lab_p - Lab_k|^2 + |p - c_k|^2 / S^2 and the +-2S window test."""
    dy = centres[None, :, 0] - yx_px[:, None, 0]
    dx = centres[None, :, 1] - yx_px[:, None, 1]
    dc = ((lab_px[:, None, :] - centres[None, :, 2:]) ** 2).sum(2)
    return dc + (dy * dy + dx * dx) / (S * S), (np.abs(dy) <= 2 * S) & (np.abs(dx) <= 2 * S)


def assign(lab, mask, centres, S, rows_per_chunk=8):
    """lab (3,H,W) ALREADY divided by m, centres (K,5) (y, x, L, a, b).  -> labels (H,W) int32 (k + 1; 0 outside the mask) and the
    minimal D2 per pixel (inf outside the mask).  Candidates: the centres within +-2S on both axes; none: all centres."""
    H, W = mask.shape
    centres = np.asarray(centres, np.float64)
    labels = np.zeros((H, W), np.int32)
    dmin = np.full((H, W), np.inf)
    for y0 in range(0, H, rows_per_chunk):
        ys, xs = np.nonzero(mask[y0:y0 + rows_per_chunk])
        if len(ys) == 0:
            continue
        ys = ys + y0
        near = np.nonzero((centres[:, 0] >= y0 - 2 * S) & (centres[:, 0] <= y0 + rows_per_chunk - 1 + 2 * S))[0]
        yx = np.stack([ys, xs], 1).astype(np.float64)
        px = lab[:, ys, xs].T
        best = np.full(len(ys), -1)
        bd = np.full(len(ys), np.inf)
        if len(near):
            d2, win = _d2(px, yx, centres[near], S)
            d2 = np.where(win, d2, np.inf)
            j = d2.argmin(1)                                  # first minimum: lowest k on a tie
            bd = d2[np.arange(len(ys)), j]
            best = np.where(np.isfinite(bd), near[j], -1)
        lone = best < 0
        if lone.any():
            d2, _ = _d2(px[lone], yx[lone], centres, S)
            j = d2.argmin(1)
            best[lone], bd[lone] = j, d2[np.arange(len(j)), j]
        labels[ys, xs] = best + 1
        dmin[ys, xs] = bd
    return labels, dmin


def pixels_without_candidate(mask, centres, S):
    """How many mask pixels have no centre within +-2S on both axes (they take the nearest of all centres)."""
    ys, xs = np.nonzero(mask)
    c = np.asarray(centres, np.float64)
    win = (np.abs(c[None, :, 0] - ys[:, None]) <= 2 * S) & (np.abs(c[None, :, 1] - xs[:, None]) <= 2 * S)
    return int((~win.any(1)).sum())


def d2_of_labels(lab, centres, S, labels):
    """D2 of every labelled pixel to the centre its label names (inf where the label is 0)."""
    centres = np.asarray(centres, np.float64)
    out = np.full(labels.shape, np.inf)
    ys, xs = np.nonzero(labels > 0)
    c = centres[labels[ys, xs] - 1]
    out[ys, xs] = ((lab[:, ys, xs].T - c[:, 2:]) ** 2).sum(1) + ((c[:, 0] - ys) ** 2 + (c[:, 1] - xs) ** 2) / (S * S)
    return out


# ---- update -------------------------------------------------------------------------------------------------------------------
def update(lab, labels, centres):
    """Every centre -> the mean (y, x, L, a, b) of its members; no members: unchanged."""
    centres = np.array(centres, np.float64)
    K = len(centres)
    ys, xs = np.nonzero(labels > 0)
    k = labels[ys, xs] - 1
    n = np.bincount(k, minlength=K).astype(np.float64)
    cols = [ys, xs, lab[0, ys, xs], lab[1, ys, xs], lab[2, ys, xs]]
    has = n > 0
    for c, vals in enumerate(cols):
        s = np.bincount(k, weights=np.asarray(vals, np.float64), minlength=K)
        centres[has, c] = s[has] / n[has]
    return centres


# ---- features -----------------------------------------------------------------------------------------------------------------
def features(img_u8, labels):
    """-> count (N,), centroid (N,2), features (N,9): mean x 3, median x 3, meanGrad x 3 of the 0..255 values per superpixel 1..N
    (NaN for a label without pixels)."""
    N = int(labels.max())
    a = img_u8.astype(np.float64)
    count = np.bincount(labels.ravel(), minlength=N + 1)[1:]
    feats = np.full((N, 9), np.nan)
    cen = np.full((N, 2), np.nan)
    grad = np.stack([np.gradient(a[..., c])[0] + np.gradient(a[..., c])[1] for c in range(3)], 2)
    order = np.argsort(labels.ravel(), kind="stable")
    bounds = np.searchsorted(labels.ravel()[order], np.arange(1, N + 2))
    yy, xx = np.divmod(order, labels.shape[1])
    flat, gflat = a.reshape(-1, 3), grad.reshape(-1, 3)
    for k in range(N):
        m = order[bounds[k]:bounds[k + 1]]
        if len(m) == 0:
            continue
        cen[k] = yy[bounds[k]:bounds[k + 1]].mean(), xx[bounds[k]:bounds[k + 1]].mean()
        feats[k, 0:3] = flat[m].mean(0)
        feats[k, 3:6] = np.median(flat[m], axis=0)
        feats[k, 6:9] = gflat[m].mean(0)
    return count, cen, feats


# ---- the whole thing ------------------------------------------------------------------------------------------------------------
def start_centres(lab, mask, sp_size):
    """n_segments = int(H W / sp_size^2), S = sqrt(mask pixels / n_segments), centres at the grid points (S/2 + i S, S/2 + j S) whose
    pixel is in the mask, row-major, with that pixel's Lab.  -> S, centres (K,5)."""
    H, W = mask.shape
    S = np.sqrt(mask.sum() / int(H * W / sp_size ** 2))
    out = []
    for gy in np.arange(S / 2, H, S):
        for gx in np.arange(S / 2, W, S):
            if mask[int(gy), int(gx)]:
                out.append([gy, gx, *lab[:, int(gy), int(gx)]])
    return float(S), np.array(out, np.float64)


def slic_raw(img_u8, mask, sp_size, sp_regul, n_iter=10):
    """Ten assign / update rounds -> labels before the connectivity repair, and S."""
    lab = prepare(img_u8) / (sp_size * sp_regul) ** 1.5
    S, centres = start_centres(lab, mask, sp_size)
    labels = None
    for _ in range(n_iter):
        labels, _ = assign(lab, mask, centres, S)
        centres = update(lab, labels, centres)
    return labels, S


def slic(img_u8, mask, sp_size, sp_regul, n_iter=10):
    labels, S = slic_raw(img_u8, mask, sp_size, sp_regul, n_iter)
    return iseg.enforce_connectivity(labels, 0.5 * S * S, img_u8)


def pipeline(img_u8, valid, nb_classes=3, sp_size=20, sp_regul=0.1, seed=0):
    """init_segment.initial_segmentation with the per-pixel steps from this file."""
    sp = slic(img_u8, valid, sp_size, sp_regul)
    _, cen, feats = features(img_u8, sp)
    feats[np.isnan(feats)] = 0
    classes, proba = iseg.segment_superpixels(sp, feats, cen, nb_classes, seed)
    seg, period, non_period = iseg.masks_from_classes(sp, classes, valid)
    return dict(period_mask=period, non_period_mask=non_period, seg=seg, slic=sp, proba=proba)
