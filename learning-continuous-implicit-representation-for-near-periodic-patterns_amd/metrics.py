"""How good a fitted or rendered image is against a ground truth, region by region: PSNR, SSIM and mean absolute error.

What runs where: the SSIM index map and the masked sums are HIP kernels (csrc/npp_metrics.hip, float64 throughout); the few hundred
per-block partial sums of a region are added on the host in float64, and the figures are formed from those totals there.

Conventions, the same on every entry:

* images are (H, W, 3) in [0, 1]: device or host tensors, NumPy arrays; uint8 images are 8-bit files, value / 255 (formed in float64,
  stored as float32: what the loaders of io.py give).  They end up as contiguous float32 tensors on `device`; a float32 tensor that
  already lies there is used in place.
* a region is an (H, W) or (H, W, 1) weight mask, 1 = member; bool is 0 / 1, uint8 is value / 255 like the mask PNGs of io.py.
  Fractional weights weigh (CompletionFit.psnr does the same).  None is the whole image.
* SSIM is Wang et al.'s index with the usual constants (11 x 11 Gaussian window of sigma 1.5, K1 = 0.01, K2 = 0.03, data range 1,
  population variances), evaluated only where the whole window lies inside the image -- so no border rule is involved, and inside
  that interior a "filter with reflection, crop 5" implementation gives the same numbers -- and averaged over the three channels per
  pixel: the map is (H - 10, W - 10), entry (i, j) belongs to pixel (i + 5, j + 5).  A region's SSIM is the weighted mean of the map
  over the region's pixels in rows 5 .. H - 6 and columns 5 .. W - 6.  H, W >= 11.
* PSNR is -10 log10(max(MSE, 1e-20)) with the MSE over the region's pixels and three channels (CompletionFit.psnr's definition, its
  floor included: identical images report 200 dB); MAE is the mean absolute error over the same numbers.

report() -> {"all": r, "known": r, "unknown": r} with r = {"pixels", "psnr", "ssim", "mae"}:

* all = valid_mask (the whole image without one), known = known_mask x valid_mask, unknown = (1 - known_mask) x valid_mask, so
  pixels(known) + pixels(unknown) = pixels(all);
* pixels is the sum of the region's weights (an int when it is whole);
* a region without pixels has pixels 0 and None for psnr, ssim and mae;
* a region with pixels but none where the SSIM map is defined (it lies wholly in the 5-pixel border) has ssim None and finite psnr
  and mae.

LPIPS of whole images is not reported: the plain LPIPS head of this package is pinned on patch-sized features only."""
import math

import numpy as np
import torch

from . import ops

BORDER = ops.SSIM_WIN // 2          # rows / columns at each image border without an SSIM value
PSNR_FLOOR = 1e-20                  # CompletionFit.psnr's floor under the MSE


def _image(a, dev, name):
    if not isinstance(a, torch.Tensor):
        a = torch.from_numpy(np.ascontiguousarray(a))
    if a.dtype == torch.uint8:
        a = (a.to(dev).to(torch.float64) / 255.0).to(torch.float32)
    if a.dim() != 3 or a.shape[2] != 3:
        raise ValueError(f"{name}: expected (H, W, 3), got {tuple(a.shape)}")
    return a.to(device=dev, dtype=torch.float32).contiguous()


def _region(m, dev, shape, name="region"):
    if m is None:
        return torch.ones(shape, dtype=torch.float32, device=dev)
    if not isinstance(m, torch.Tensor):
        m = torch.from_numpy(np.ascontiguousarray(m))
    if m.dtype == torch.uint8:
        m = (m.to(dev).to(torch.float64) / 255.0).to(torch.float32)
    if m.dim() == 3 and m.shape[2] == 1:
        m = m[..., 0]
    if tuple(m.shape) != tuple(shape):
        raise ValueError(f"{name}: expected {tuple(shape)} (or with a trailing 1), got {tuple(m.shape)}")
    return m.to(device=dev, dtype=torch.float32).contiguous()


def _pair(a, b, device):
    dev = ops.select_device(device)
    a, b = _image(a, dev, "a"), _image(b, dev, "b")
    if a.shape != b.shape:
        raise ValueError(f"images differ in size: {tuple(a.shape)} and {tuple(b.shape)}")
    return dev, a, b


def _totals(a, b, regions, smap):
    """The five totals (ops.region_sums) of every region: one launch per region, one copy for all, blocks added on the host."""
    parts = torch.stack([ops.region_sums(a, b, w, smap) for w in regions])
    return parts.cpu().numpy().sum(axis=1)


def _psnr(t):
    return None if t[0] <= 0 else -10.0 * math.log10(max(float(t[1]) / (3.0 * float(t[0])), PSNR_FLOOR))


def _mae(t):
    return None if t[0] <= 0 else float(t[2]) / (3.0 * float(t[0]))


def _ssim(t):
    return None if t[3] <= 0 else float(t[4]) / float(t[3])


def ssim_map(a, b, device="cuda:0"):
    """The SSIM index map of two images as a float64 tensor (H - 10, W - 10) on `device` (module docstring)."""
    _, a, b = _pair(a, b, device)
    return ops.ssim_map(a, b)


def ssim(a, b, region=None, device="cuda:0"):
    """Mean SSIM over the region's pixels that have a map value (the whole map without a region); None when there is none."""
    dev, a, b = _pair(a, b, device)
    return _ssim(_totals(a, b, [_region(region, dev, a.shape[:2])], ops.ssim_map(a, b))[0])


def psnr(a, b, region=None, device="cuda:0"):
    """-10 log10 of the mean squared error over the region's pixels and three channels, floored at 1e-20; None for an empty region."""
    dev, a, b = _pair(a, b, device)
    return _psnr(_totals(a, b, [_region(region, dev, a.shape[:2])], None)[0])


def mae(a, b, region=None, device="cuda:0"):
    """Mean absolute error over the region's pixels and three channels; None for an empty region."""
    dev, a, b = _pair(a, b, device)
    return _mae(_totals(a, b, [_region(region, dev, a.shape[:2])], None)[0])


def report(pred, gt, known_mask, valid_mask=None, device="cuda:0"):
    """{"all" | "known" | "unknown": {"pixels", "psnr", "ssim", "mae"}} of `pred` against `gt` (module docstring: all = valid,
    known = mask x valid, unknown = (1 - mask) x valid; an empty region gives pixels 0 and None figures; a region wholly inside the
    5-pixel border gives ssim None).  Plain Python numbers: the dict goes through json.dumps as it is."""
    dev, a, b = _pair(pred, gt, device)
    hw = a.shape[:2]
    m, v = _region(known_mask, dev, hw, "known_mask"), _region(valid_mask, dev, hw, "valid_mask")
    totals = _totals(a, b, [v, m * v, (1.0 - m) * v], ops.ssim_map(a, b))
    out = {}
    for name, t in zip(("all", "known", "unknown"), totals):
        n = float(t[0])
        out[name] = {"pixels": int(n) if n == int(n) else n, "psnr": _psnr(t), "ssim": _ssim(t), "mae": _mae(t)}
    return out


def quantised(pred, known_mask, valid_mask=None):
    """A rendered (H, W, 3) device image as io.dump_testset writes it to pred_rgb_img.png -- pred m v + pred (1 - m) v in float64, clipped
    to [0, 1], rounded to 8 bits -- and read back by io._imread_rgb, without leaving the device: the figures of this image are the
    figures of the file."""
    p = pred.to(torch.float64)
    m = _region(known_mask, p.device, p.shape[:2], "known_mask").to(torch.float64)[..., None]
    v = _region(valid_mask, p.device, p.shape[:2], "valid_mask").to(torch.float64)[..., None]
    q = torch.round((p * m * v + p * (1.0 - m) * v).clamp(0.0, 1.0) * 255.0)
    return (q / 255.0).to(torch.float32)
