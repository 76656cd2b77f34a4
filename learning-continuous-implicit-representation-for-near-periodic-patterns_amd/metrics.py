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

LPIPS (LPIPSMetric; report(..., lpips=metric)) is the reference's own definition, externel_lib/lpips/lpips.py:92-133 with
use_robust=False, normalize=True, and comes as TWO numbers that must not be mixed up:

* per tap k with features a, b (C, h, w) of the two images: d_k(p) = sum_c lin_k[c] (a_c(p) / (|a(p)| + 1e-10) - b_c(p) / (|b(p)| +
  1e-10))^2;
* the distance map (spatial=True) D = sum_k upsample(d_k -> (H, W)), bilinear with align_corners=False; a REGION's LPIPS is the
  weighted mean of D over the region's pixels.  The trunk sees the whole images as they are given -- nothing is masked out before
  it -- only the mean is restricted to the region;
* the scalar LPIPS (spatial=False) sum_k mean_p d_k(p) is the number papers quote for a whole image.  It is NOT the mean of D:
  bilinear upsampling does not keep a map's mean.  report() gives it once, as "lpips_image".

The nets: "vgg" is VGG16 with taps relu1_2 .. relu5_3 on the exact-fp32 trunk (losses.HipTrunk32, any H x W), "alex" is
segment.AlexFeatures; the scaling layer and the 2x - 1 are folded as losses.LPIPS / segment.lpips_alex_spatial fold them.  The trunk
is the only fp32 stage: head, composition and sums are float64 kernels with fixed summation orders (csrc/npp_lpips_map.hip), so two
runs give identical bits.  The pretrained trunks are the user's (weights.resolve finds vgg16-*.pth / alexnet-*.pth); the lin layers ship
with the package.  A figure from random trunks means nothing, so the metric refuses to be built without a state dict unless asked by
name (allow_random=True).

With lpips=metric every region of report() gains "lpips" (None for a region without pixels) and the report gains "lpips_image":
{"net", "scalar"}; with lpips=None the report is what it was before the key existed, bit for bit."""
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


def _map_totals(dmap, regions):
    """(sum w, sum w map) of a float64 map under every region (None: all ones): one launch per region, one copy, blocks added on the host."""
    parts = torch.stack([ops.map_region_sums(dmap, w) for w in regions])
    return parts.cpu().numpy().sum(axis=1)


def _mean(t):
    return None if t[0] <= 0 else float(t[1]) / float(t[0])


def _scalar(taps):
    """sum_k mean_p d_k(p) (spatial=False): every tap's mean from its own fixed-order sums, the taps added in tap order."""
    total = 0.0
    for d in taps:
        total += _mean(_map_totals(d, [None])[0])
    return total


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


def report(pred, gt, known_mask, valid_mask=None, device="cuda:0", lpips=None):
    """{"all" | "known" | "unknown": {"pixels", "psnr", "ssim", "mae"}} of `pred` against `gt` (module docstring: all = valid,
    known = mask x valid, unknown = (1 - mask) x valid; an empty region gives pixels 0 and None figures; a region wholly inside the
    5-pixel border gives ssim None).  lpips: an LPIPSMetric on the same device -- every region gains "lpips", the region mean of the
    distance map, and the report "lpips_image": {"net", "scalar"}, from one pass of the trunk.  Plain Python numbers: the dict goes
    through json.dumps as it is."""
    dev, a, b = _pair(pred, gt, device)
    hw = a.shape[:2]
    m, v = _region(known_mask, dev, hw, "known_mask"), _region(valid_mask, dev, hw, "valid_mask")
    regions = [v, m * v, (1.0 - m) * v]
    totals = _totals(a, b, regions, ops.ssim_map(a, b))
    out = {}
    for name, t in zip(("all", "known", "unknown"), totals):
        n = float(t[0])
        out[name] = {"pixels": int(n) if n == int(n) else n, "psnr": _psnr(t), "ssim": _ssim(t), "mae": _mae(t)}
    if lpips is not None:
        if lpips.device != dev:
            raise ValueError(f"lpips: the metric lives on {lpips.device}, the report runs on {dev}")
        taps, dmap = lpips._maps(a, b)
        for name, t in zip(("all", "known", "unknown"), _map_totals(dmap, regions)):
            out[name]["lpips"] = _mean(t)
        out["lpips_image"] = {"net": lpips.net, "scalar": _scalar(taps)}
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


# ---- LPIPS of whole images -------------------------------------------------------------------------------------------------------
_VGG_TAPS = (3, 8, 15, 22, 29)                      # relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 of torchvision's vgg16.features
_LPIPS_SHIFT, _LPIPS_SCALE = (-0.030, -0.088, -0.188), (0.458, 0.448, 0.450)     # lpips.py:136-143 ScalingLayer
# Smallest side at which every tap still has a position.  vgg: four 2 x 2 / 2 pools in front of relu5_3, n -> n // 2 each, so
# n // 16 >= 1.  alex: conv1 (11, stride 4, pad 2) gives (n - 7) // 4 + 1, the two MaxPool(3, 2) give (n - 3) // 2 + 1 each and need n >= 3:
# the last pool's input must be >= 3, so the first pool's >= 7, so (n - 7) // 4 >= 6, n >= 31 (31 -> 7 -> 3 -> 1).
LPIPS_MIN_SIDE = {"vgg": 16, "alex": 31}
_CHECKPOINT = {"vgg": "vgg16-*.pth (torchvision's vgg16 state_dict)", "alex": "alexnet-owt-*.pth (torchvision's alexnet state_dict)"}


def _build_trunk(net, state_dict, dev):
    """The feature extractor of one net on `dev`: losses.HipTrunk32 over VGG16 (instances of one state dict share their packed
    weights, as every trunk of losses.py does) or segment.AlexFeatures.  Their own fixed-seed warnings are replaced by the metric's."""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if net == "vgg":
            from . import losses
            return losses.HipTrunk32(losses._VGG16, taps=_VGG_TAPS, state_dict=state_dict, seed=4321, device=dev)
        from . import segment
        return segment.AlexFeatures(state_dict, device=dev)


class LPIPSMetric:
    """LPIPS of two whole images (module docstring): LPIPS(net, spatial=True / False).forward(a, b, use_robust=False, normalize=True) of
    the reference on (H, W, 3) images in [0, 1].

    net: "vgg" (H, W >= 16: four 2 x 2 pools lie in front of relu5_3) or "alex" (H, W >= 31: conv1 of stride 4 and two 3 x 3 / 2 pools,
    31 -> 7 -> 3 -> 1); a smaller image would leave a tap without a position and is refused.  trunk_state_dict: torchvision's vgg16 /
    alexnet state dict; without one the constructor raises ValueError naming the checkpoint, unless allow_random=True: then fixed-seed
    random trunks are built and one warning says that the figures mean nothing.  lin_weights: the five lin vectors, None:
    weights.lpips_lin(net), the packaged LPIPS v0.1 layers.

    map(a, b) -> D, float64 (H, W) on the device; taps(a, b) -> [d_k]; scalar(a, b) -> sum_k mean d_k (the whole-image number);
    region(a, b, region=None) -> weighted mean of D (None for a region without pixels).  The trunk's per-shape activation buffers are
    released when a call returns: a directory run meets many sizes, and a 1024^2 pass holds more than 1 GB of them."""

    def __init__(self, net="vgg", trunk_state_dict=None, lin_weights=None, device="cuda:0", allow_random=False):
        if net not in LPIPS_MIN_SIDE:
            raise ValueError(f"net: 'vgg' or 'alex', got {net!r}")
        if trunk_state_dict is None:
            if not allow_random:
                raise ValueError(f"LPIPSMetric(net={net!r}): no trunk_state_dict -- load {_CHECKPOINT[net]} and pass it; LPIPS from random "
                                 "trunks is meaningless and is computed only with allow_random=True")
            import warnings
            warnings.warn(f"npp_amd.metrics: LPIPS({net}) runs on fixed-seed RANDOM trunks (allow_random=True): its figures are not LPIPS "
                          f"distances; pass {_CHECKPOINT[net]}", stacklevel=2)
        self.net = net
        self.device = ops.select_device(device)
        if lin_weights is None:
            from . import weights
            lin_weights = weights.lpips_lin(net)
        self.lins = [torch.as_tensor(np.asarray(w, np.float32).reshape(-1)).contiguous().to(self.device) for w in lin_weights]
        if len(self.lins) != 5:
            raise ValueError(f"lin_weights: five vectors, got {len(self.lins)}")
        self.trunk = _build_trunk(net, trunk_state_dict, self.device)
        self.layout = "nchw" if net == "vgg" else "nhwc"
        # the 2x - 1 of normalize=True and the scaling layer as one affine map of the image, x * scale + shift per channel
        self._in_scale = [2.0 / s for s in _LPIPS_SCALE]
        self._in_shift = [(-1.0 - sh) / s for sh, s in zip(_LPIPS_SHIFT, _LPIPS_SCALE)]

    def _check_size(self, H, W):
        need = LPIPS_MIN_SIDE[self.net]
        if H < need or W < need:
            raise ValueError(f"LPIPS({self.net}): H={H} W={W}: both must be at least {need} (a smaller image leaves the deepest tap "
                             "without a position)")

    def _features(self, x):
        """(2, 3, H, W) fp32 in [0, 1] -> per tap the features of image 0 and image 1, each contiguous in self.layout."""
        if self.net == "vgg":
            feats = self.trunk._forward(x, self._in_scale, self._in_shift)
        else:
            sh = torch.tensor(_LPIPS_SHIFT, device=x.device).view(1, 3, 1, 1)
            sc = torch.tensor(_LPIPS_SCALE, device=x.device).view(1, 3, 1, 1)
            feats = self.trunk.features_nhwc((((2 * x - 1) - sh) / sc).contiguous())      # segment.lpips_alex_spatial's folding
        return [(f[0], f[1]) for f in feats]

    def _release(self):
        """Drop what the trunk keeps per input shape (HipTrunk32._buf and its list of the last pass's activations)."""
        buf = getattr(self.trunk, "_buf", None)
        if buf is not None:
            buf.clear()
        if hasattr(self.trunk, "_acts"):
            self.trunk._acts = []

    def _maps(self, a, b):
        """Device images (H, W, 3) fp32 -> ([d_k], D): one pass of the trunk over both images, five head launches, one composition."""
        H, W = int(a.shape[0]), int(a.shape[1])
        self._check_size(H, W)
        ops.check_current(self.device)
        try:
            with torch.no_grad():
                x = torch.stack([a, b]).permute(0, 3, 1, 2).contiguous()
                taps = [ops.lpips_tap_map(f0, f1, lin, self.layout) for (f0, f1), lin in zip(self._features(x), self.lins)]
                return taps, ops.lpips_compose(taps, H, W)
        finally:
            self._release()

    def _pair(self, a, b):
        dev, a, b = _pair(a, b, self.device)
        return a, b

    def taps(self, a, b):
        """The five taps' distance maps d_k, float64 (h_k, w_k) device tensors."""
        return self._maps(*self._pair(a, b))[0]

    def map(self, a, b):
        """The distance map D of LPIPS(spatial=True), a float64 (H, W) device tensor."""
        return self._maps(*self._pair(a, b))[1]

    def scalar(self, a, b):
        """LPIPS(spatial=False): sum_k mean_p d_k(p), the number quoted for a whole image (not the mean of map())."""
        return _scalar(self._maps(*self._pair(a, b))[0])

    def region(self, a, b, region=None):
        """The weighted mean of the distance map over a region (None: the whole image); None for a region without pixels."""
        a, b = self._pair(a, b)
        w = None if region is None else _region(region, self.device, a.shape[:2])
        return _mean(_map_totals(self._maps(a, b)[1], [w])[0])
