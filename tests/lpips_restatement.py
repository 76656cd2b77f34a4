"""Torch restatement, on the CPU, of LPIPS of whole images (npp_amd.metrics.LPIPSMetric, csrc/npp_lpips_map.hip), shared by
test_lpips_metric_cpu.py, test_gpu_lpips_metric.py and tools/lpips_metric_time.py.  Test infrastructure only: the product package
runs none of it.

The definition is the reference's externel_lib/lpips/lpips.py:92-133 with use_robust=False, normalize=True, written once and
parametrised by dtype (float32: the reference's own arithmetic; float64: the yardstick of the GPU tests):

* trunk: VGG16 taps relu1_2 .. relu5_3 through comparators.TorchTrunk(_VGG16, taps, seed) -- the layers and weights HipTrunk32 packs
  -- or an AlexNet `features` stack as in tests/golden/make_golden_segment.py, both from a state dict or a seed;
* head (`head`): unit-normalise over the channels with the 1e-10 in the denominator, squared difference, the 1 x 1 lin convolution;
* distance map: F.interpolate(bilinear, align_corners=False) of every tap's map to the image, summed in tap order;
* region mean: weighted mean of the distance map; scalar: sum over the taps of the tap's plain mean."""
import numpy as np
import torch
import torch.nn.functional as F

VGG_TAPS = (3, 8, 15, 22, 29)
VGG_RANDOM_SEED = 4321                       # the fixed seed of LPIPSMetric("vgg", allow_random=True) (losses.LPIPS's own)
ALEX_RANDOM_SEED = 99                        # segment.AlexFeatures' fixed seed
SHIFT, SCALE = (-0.030, -0.088, -0.188), (0.458, 0.448, 0.450)
ALEX = [(0, 64, 3, 11, 4, 2), (3, 192, 64, 5, 1, 2), (6, 384, 192, 3, 1, 1), (8, 256, 384, 3, 1, 1), (10, 256, 256, 3, 1, 1)]
ALEX_POOL_BEFORE = (3, 6)
CHNS = {"vgg": [64, 128, 256, 512, 512], "alex": [64, 192, 384, 256, 256]}


# ---- trunks ------------------------------------------------------------------------------------------------------------------------
def vgg_state_dict(seed=VGG_RANDOM_SEED):
    """The fixed-seed VGG16 of losses._Trunk as a state dict ('<idx>.weight' / '<idx>.bias': what `vgg.features` saves)."""
    import warnings
    from comparators import TorchTrunk
    from npp_amd.losses import _VGG16
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t = TorchTrunk(_VGG16, VGG_TAPS, seed=seed)
    return {k: v.detach().clone() for k, v in t.features.state_dict().items()}


def alex_state_dict(seed=ALEX_RANDOM_SEED, biases=False):
    """An AlexNet `features` state dict drawn from torch.Generator().manual_seed(seed).  biases=False: segment.AlexFeatures' own
    fixed-seed init (weights only, zero biases); True: the stack of tests/golden/make_golden_segment.py (bias = randn * 0.05 drawn
    after each weight)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for idx, co, ci, k, _, _ in ALEX:
        sd[f"features.{idx}.weight"] = torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5
        sd[f"features.{idx}.bias"] = torch.randn(co, generator=g) * 0.05 if biases else torch.zeros(co)
    return sd


def vgg_features(sd, x):
    """[relu1_2 .. relu5_3] of x (N, 3, H, W), in x's dtype."""
    import warnings
    from comparators import TorchTrunk
    from npp_amd.losses import _VGG16
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t = TorchTrunk(_VGG16, VGG_TAPS, state_dict=sd).to(x.dtype)
    with torch.no_grad():
        return t(x)


def alex_features(sd, x):
    """[relu1 .. relu5] of x (N, 3, H, W), in x's dtype (pretrained_networks.py:56-94 on torchvision's layer list)."""
    outs = []
    with torch.no_grad():
        for idx, _, _, _, st, pd in ALEX:
            if idx in ALEX_POOL_BEFORE:
                x = F.max_pool2d(x, 3, 2)
            x = F.relu(F.conv2d(x, sd[f"features.{idx}.weight"].to(x.dtype), sd[f"features.{idx}.bias"].to(x.dtype), stride=st, padding=pd))
            outs.append(x)
    return outs


# ---- the head, written once ---------------------------------------------------------------------------------------------------------
def normalize_tensor(f, eps=1e-10):
    return f / (torch.sqrt(torch.sum(f ** 2, dim=1, keepdim=True)) + eps)


def head(feats0, feats1, lins, HW):
    """Per-tap features (1, C, h, w) of the two images (any float dtype, the lins are cast to it) -> ([d_k (h, w)], D (H, W), scalar)."""
    taps, ups, scalar = [], [], None
    for f0, f1, lin in zip(feats0, feats1, lins):
        diff = (normalize_tensor(f0) - normalize_tensor(f1)) ** 2
        d = F.conv2d(diff, torch.as_tensor(np.asarray(lin)).to(diff.dtype).view(1, -1, 1, 1))
        taps.append(d[0, 0])
        ups.append(F.interpolate(d, size=tuple(HW), mode="bilinear", align_corners=False))
        m = d.mean([2, 3], keepdim=True)
        scalar = m if scalar is None else scalar + m
    D = ups[0].clone()
    for u in ups[1:]:
        D = D + u
    return taps, D[0, 0], float(scalar)


def preprocess(img, dtype):
    """(H, W, 3) in [0, 1] -> the trunk's input (1, 3, H, W): 2x - 1, then the scaling layer (lpips.py:93-99, :136-143)."""
    x = torch.as_tensor(np.asarray(img)).to(dtype).permute(2, 0, 1)[None]
    x = 2 * x - 1
    return (x - torch.tensor(SHIFT, dtype=dtype).view(1, 3, 1, 1)) / torch.tensor(SCALE, dtype=dtype).view(1, 3, 1, 1)


def lpips(net, sd, lins, a, b, dtype=torch.float64):
    """The whole metric on two (H, W, 3) images -> dict(taps=[(h, w) arrays], map=(H, W) array, scalar=float), computed in `dtype`."""
    feats = vgg_features if net == "vgg" else alex_features
    f0, f1 = feats(sd, preprocess(a, dtype)), feats(sd, preprocess(b, dtype))
    taps, D, scalar = head(f0, f1, lins, np.asarray(a).shape[:2])
    return {"taps": [t.numpy() for t in taps], "map": D.numpy(), "scalar": scalar}


def head_on_features(feats0, feats1, lins, HW):
    """The float64 head on given fp32 features [(C, h, w) arrays] (the fp32 values are exact inputs) -> like lpips()."""
    f0 = [torch.as_tensor(np.asarray(f)).double()[None] for f in feats0]
    f1 = [torch.as_tensor(np.asarray(f)).double()[None] for f in feats1]
    taps, D, scalar = head(f0, f1, [np.asarray(l, np.float64) for l in lins], HW)
    return {"taps": [t.numpy() for t in taps], "map": D.numpy(), "scalar": scalar}


def region_mean(dmap, weight=None):
    """Weighted mean of a map over a region (None: all pixels); None for a region without pixels."""
    d = np.asarray(dmap, np.float64)
    w = np.ones_like(d) if weight is None else np.asarray(weight, np.float64).reshape(d.shape)
    n = float(w.sum())
    return None if n <= 0 else float((w * d).sum()) / n


def rel_l2(x, ref):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(x - ref) / max(np.linalg.norm(ref), 1e-300))


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def lattice_pair(H, W, seed=3):
    """An RGB image pair (H, W, 3) float32 in [0, 1]: a noisy two-frequency lattice, and the same image with a rectangle of uniform
    noise that the pattern does not explain (the inputs of tests/golden/make_golden_segment.py, in colour and at any size)."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    base = torch.stack([0.5 + 0.35 * torch.cos(2 * np.pi * xx / 16) * torch.cos(2 * np.pi * yy / 20),
                        0.5 + 0.30 * torch.sin(2 * np.pi * (xx + yy) / 12),
                        0.5 + 0.25 * torch.cos(2 * np.pi * yy / 9)], -1)
    a = (base + 0.02 * torch.randn(H, W, 3, generator=g)).clamp(0, 1)
    b = a.clone()
    y0, y1, x0, x1 = H // 3, (3 * H) // 4, W // 4, (3 * W) // 4
    b[y0:y1, x0:x1] = torch.rand(y1 - y0, x1 - x0, 3, generator=g)
    return a.numpy(), b.numpy()


def sparse_features(shape, seed, zero_share=0.3, dead_positions=2):
    """Random fp32 features (C, h, w) >= 0 with exact zeros at `zero_share` of the entries and a few all-zero positions (the + 1e-10
    branch of the normalisation)."""
    rs = np.random.RandomState(seed)
    f = rs.rand(*shape).astype(np.float32) * 3.0
    f[rs.rand(*shape) < zero_share] = 0.0
    C, h, w = shape
    for _ in range(min(dead_positions, h * w - 1)):
        f[:, rs.randint(h), rs.randint(w)] = 0.0
    return f
