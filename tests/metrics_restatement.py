"""Float64 NumPy restatement of the quality figures (csrc/npp_metrics.hip, npp_amd.metrics), shared by test_metrics_cpu.py,
test_gpu_metrics.py and tools/metrics_time.py: the SSIM index map in two independent forms, the region figures made of it, and
the test images and masks.

SSIM (Wang, Bovik, Sheikh, Simoncelli 2004) with the usual constants: an 11 x 11 Gaussian window of sigma 1.5 normalised to sum 1
(the outer product of the normalised 1-D window), K1 = 0.01, K2 = 0.03, data range 1, population variances E[xy] - mu_x mu_y.  The
map holds one value per pixel whose whole window lies inside the image, the mean of its three channels' indices: (H - 10, W - 10),
entry (i, j) belongs to pixel (i + 5, j + 5).

* ssim_map_slices: the window, the five moments and the index written out with NumPy slicing (11 shifted slices per axis).
* ssim_map_scipy: scipy.ndimage.correlate1d along both axes with reflection, cropped by 5 -- the "filter, then crop" form; inside the
  crop no reflected pixel is ever read, so the two forms agree to roundoff."""
import math

import numpy as np

WIN, SIGMA, K1, K2 = 11, 1.5, 0.01, 0.03
R = WIN // 2
C1, C2 = (K1 * 1.0) ** 2, (K2 * 1.0) ** 2


def window():
    """The normalised 1-D Gaussian window (11 taps)."""
    g = np.array([math.exp(-((k - R) ** 2) / (2.0 * SIGMA * SIGMA)) for k in range(WIN)], np.float64)
    return g / g.sum()


def _index(mx, my, exx, eyy, exy):
    vx, vy, cxy = exx - mx * mx, eyy - my * my, exy - mx * my
    num = (2.0 * mx * my + C1) * (2.0 * cxy + C2)
    den = (mx * mx + my * my + C1) * (vx + vy + C2)
    return num / den


def _channel_mean(s):
    return (s[..., 0] + s[..., 1] + s[..., 2]) / 3.0


def ssim_map_slices(a, b):
    """(H,W,3) x 2 -> (H-10, W-10) float64, by explicit slicing: horizontal pass, vertical pass, index, channel mean."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    H, W = a.shape[:2]
    if H < WIN or W < WIN:
        raise ValueError(f"both sides must be at least {WIN}")
    g = window()

    def moment(f):
        h = np.zeros((H, W - 2 * R, 3))
        for k in range(WIN):
            h += g[k] * f[:, k:k + W - 2 * R]
        v = np.zeros((H - 2 * R, W - 2 * R, 3))
        for k in range(WIN):
            v += g[k] * h[k:k + H - 2 * R]
        return v
    return _channel_mean(_index(moment(a), moment(b), moment(a * a), moment(b * b), moment(a * b)))


def ssim_map_scipy(a, b):
    """The same map through scipy.ndimage.correlate1d with reflection, cropped by 5 on every side."""
    from scipy.ndimage import correlate1d
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    g = window()

    def moment(f):
        return correlate1d(correlate1d(f, g, axis=1, mode="reflect"), g, axis=0, mode="reflect")[R:-R, R:-R]
    return _channel_mean(_index(moment(a), moment(b), moment(a * a), moment(b * b), moment(a * b)))


def region_figures(a, b, weight, smap=None):
    """{"pixels", "psnr", "ssim", "mae"} of one (H,W) weight mask, as npp_amd.metrics defines them (None for an empty region, ssim None
    for a region without a pixel in rows 5 .. H-6, columns 5 .. W-6; the MSE under the PSNR floored at 1e-20)."""
    a, b, w = np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(weight, np.float64)
    if smap is None:
        smap = ssim_map_slices(a, b)
    d = a - b
    n = float(w.sum())
    if n <= 0:
        return {"pixels": 0, "psnr": None, "ssim": None, "mae": None}
    mse = float((w * (d * d).sum(-1)).sum()) / (3.0 * n)
    wi = w[R:-R, R:-R]
    ni = float(wi.sum())
    return {"pixels": int(n) if n == int(n) else n, "psnr": -10.0 * math.log10(max(mse, 1e-20)),
            "ssim": None if ni <= 0 else float((wi * smap).sum()) / ni, "mae": float((w * np.abs(d).sum(-1)).sum()) / (3.0 * n)}


def report(pred, gt, known_mask, valid_mask=None, form=ssim_map_slices):
    """npp_amd.metrics.report restated: all = valid, known = mask x valid, unknown = (1 - mask) x valid (form: which map)."""
    a, b = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    m = np.asarray(known_mask, np.float64).reshape(a.shape[:2])
    v = np.ones(a.shape[:2]) if valid_mask is None else np.asarray(valid_mask, np.float64).reshape(a.shape[:2])
    smap = form(a, b)
    return {"all": region_figures(a, b, v, smap), "known": region_figures(a, b, m * v, smap),
            "unknown": region_figures(a, b, (1.0 - m) * v, smap)}


# ---- test images and masks ----------------------------------------------------------------------------------------------------------
SHAPES = [(11, 11), (11, 40), (40, 11), (12, 37), (47, 33), (130, 70)]
CONTENTS = ["noise", "saturated", "flat", "ramp"]


def content(kind, shape, seed=0):
    """A pair of (H,W,3) float32 images in [0, 1]: uniform noise; saturated noise (values in {0, 1}); a flat image against itself
    plus 1e-3 (zero variances: the denominator is at its smallest, C2); a ramp against a slightly different ramp."""
    H, W = shape
    rs = np.random.RandomState(seed + 17 * H + W)
    if kind == "noise":
        a, b = rs.rand(H, W, 3), rs.rand(H, W, 3)
    elif kind == "saturated":
        a, b = (rs.rand(H, W, 3) < 0.5).astype(np.float64), (rs.rand(H, W, 3) < 0.5).astype(np.float64)
    elif kind == "flat":
        a = np.full((H, W, 3), 0.4)
        b = a + 1e-3
    elif kind == "ramp":
        y, x = np.mgrid[0:H, 0:W]
        r = (x + 2.0 * y) / (W + 2.0 * H)
        a = np.stack([r, 1.0 - r, 0.5 * r], -1)
        b = np.clip(a * 0.9 + 0.03 * np.sin(x / 3.0)[..., None] + 0.05, 0, 1)
    else:
        raise ValueError(kind)
    return a.astype(np.float32), b.astype(np.float32)


MASKS = ["hole", "irregular", "border_hole"]


def mask(kind, shape, seed=0):
    """(H,W) float32 known-masks (1 = known): a centred rectangular hole, an irregular mask thresholded from smoothed noise, a hole
    that touches the image border."""
    H, W = shape
    m = np.ones((H, W), np.float32)
    if kind == "hole":
        m[H // 3:2 * H // 3, W // 4:3 * W // 4] = 0
    elif kind == "irregular":
        from scipy.ndimage import gaussian_filter
        f = gaussian_filter(np.random.RandomState(seed + 5).rand(H, W), 2.0)
        m = (f > np.median(f)).astype(np.float32)
    elif kind == "border_hole":
        m[:H // 3, :W // 2] = 0
    else:
        raise ValueError(kind)
    return m
