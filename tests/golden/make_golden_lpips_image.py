#!/usr/bin/env python3
"""g16_lpips_image.npz: LPIPS of whole RGB images from the REFERENCE's own LPIPS.forward (externel_lib/lpips/lpips.py:92-133,
use_robust=False, normalize=True), once with spatial=True, retPerLayer=True (the distance map) and once with spatial=False (the
scalar), for net='vgg' on a 40 x 52 pair and net='alex' on an 80 x 67 pair.  torchvision's pretrained trunks are not available
offline: behind obj.net stand the fixed-seed VGG16 of comparators.TorchTrunk and the AlexNet-`features`-shaped stack
of make_golden_segment.py; the `lin` layers carry the vendored weights/v0.1/{vgg,alex}.pth; everything after the trunk is the
reference's code.  lpips.py:126-128 sums the per-layer maps IN PLACE into res[0], so the taps are recorded where the reference
hands them to its upsample(), before that sum.  Runs only where the reference tree exists (make_golden.REF); the committed .npz is what the tests read.

    python tests/golden/make_golden_lpips_image.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden import import_reference, OUT, REF          # noqa: E402
from make_golden_segment import alex_weights                # noqa: E402
import lpips_restatement as LR                              # noqa: E402  (inputs and the VGG stand-in's construction only)

VGG_SEED, ALEX_SEED = 20251, 20252
CASES = {"vgg": (40, 52, [64, 128, 256, 512, 512]), "alex": (80, 67, [64, 192, 384, 256, 256])}


def reference_lpips(LL, net, chns, trunk):
    obj = LL.LPIPS.__new__(LL.LPIPS)
    torch.nn.Module.__init__(obj)
    obj.pnet_type, obj.pnet_tune, obj.pnet_rand, obj.spatial, obj.lpips, obj.version = net, False, False, True, True, "0.1"
    obj.scaling_layer = LL.ScalingLayer()
    obj.chns, obj.L = chns, 5
    obj.adaptive_perceps = []
    obj.lins = torch.nn.ModuleList([LL.NetLinLayer(c, use_dropout=True) for c in chns])
    for i, l in enumerate(obj.lins):
        setattr(obj, f"lin{i}", l)
    obj.load_state_dict(torch.load(os.path.join(REF, f"externel_lib/lpips/weights/v0.1/{net}.pth"), map_location="cpu"), strict=False)
    obj.eval()
    obj.net = trunk
    return obj


def main():
    import_reference()
    import lpips.lpips as LL
    F = torch.nn.functional
    from comparators import TorchTrunk
    from npp_amd.losses import _VGG16
    vgg = TorchTrunk(_VGG16, LR.VGG_TAPS, seed=VGG_SEED)
    W = alex_weights(ALEX_SEED)

    class Alex:                                                  # pretrained_networks.py:56-94 on torchvision's layer list
        def forward(self, x):
            outs = []
            x = F.relu(F.conv2d(x, W[0][0], W[0][1], stride=4, padding=2)); outs.append(x)
            x = F.relu(F.conv2d(F.max_pool2d(x, 3, 2), W[1][0], W[1][1], padding=2)); outs.append(x)
            x = F.relu(F.conv2d(F.max_pool2d(x, 3, 2), W[2][0], W[2][1], padding=1)); outs.append(x)
            x = F.relu(F.conv2d(x, W[3][0], W[3][1], padding=1)); outs.append(x)
            x = F.relu(F.conv2d(x, W[4][0], W[4][1], padding=1)); outs.append(x)
            return outs

    seen = []
    G = LL.LPIPS.forward.__globals__                             # (the module the class was defined in, whatever name it was imported under)
    upsample = G["upsample"]

    def recording_upsample(in_tens, out_HW=(64, 64)):            # the tap's own map, before lpips.py:126-128 adds into res[0]
        seen.append(in_tens.detach().clone())
        return upsample(in_tens, out_HW=out_HW)
    G["upsample"] = recording_upsample
    out = {"vgg_seed": np.int64(VGG_SEED), "alex_seed": np.int64(ALEX_SEED)}
    for net, (H, Wd, chns) in CASES.items():
        a, b = LR.lattice_pair(H, Wd, seed=3 if net == "vgg" else 4)
        a, b = (np.round(a * 255) / 255).astype(np.float32), (np.round(b * 255) / 255).astype(np.float32)     # 8-bit images
        obj = reference_lpips(LL, net, chns, vgg if net == "vgg" else Alex())
        in0, in1 = torch.from_numpy(a).permute(2, 0, 1)[None], torch.from_numpy(b).permute(2, 0, 1)[None]
        del seen[:]
        with torch.no_grad():
            obj.spatial = True
            val, _ = obj.forward(in0, in1, False, retPerLayer=True, normalize=True)
            obj.spatial = False
            scalar = obj.forward(in0, in1, False, normalize=True)
        assert len(seen) == 5 and tuple(val.shape) == (1, 1, H, Wd) and tuple(scalar.shape) == (1, 1, 1, 1)
        out.update({f"{net}_in0": a, f"{net}_in1": b, f"{net}_val": val[0, 0].numpy(), f"{net}_scalar": scalar.reshape(()).numpy()})
        for k in range(5):
            out[f"{net}_tap{k}"] = seen[k][0, 0].numpy()
            out[f"{net}_lin{k}"] = obj.lins[k].model[1].weight.detach().numpy().reshape(-1)
    np.savez_compressed(os.path.join(OUT, "g16_lpips_image.npz"), **out)
    print({k: (v.shape if hasattr(v, "shape") else v) for k, v in out.items()})
    print("vgg scalar", float(out["vgg_scalar"]), "mean of map", float(out["vgg_val"].mean()),
          "| alex scalar", float(out["alex_scalar"]), "mean of map", float(out["alex_val"].mean()))


if __name__ == "__main__":
    main()
