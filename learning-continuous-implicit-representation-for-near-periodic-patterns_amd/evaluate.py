"""Quality report of an image against a ground truth, as one JSON object (npp_amd.metrics.report: PSNR, SSIM and mean absolute error
over the regions all / known / unknown).

    python -m npp_amd.evaluate --pred out.png --gt gt_img.png [--mask unknown_mask.png] [--valid valid_mask.png] [--json report.json]
    python -m npp_amd.evaluate --results results/completion_top3/<name> --datadir data/completion/detected/<name> [--json report.json]

The mask files are those of a detected directory and are read like io.py's loaders read them: gray / 255, WHITE = KNOWN in
`unknown_mask.png` (the file config.odgt calls fpath_mask; loaders.py:99-103 multiplies it with the valid mask) and white = valid in
`valid_mask.png`.  Without --mask everything is known, without --valid everything valid.  The second form takes the newest
testset_<iter>/pred_rgb_img.png of a fit's result directory and the ground truth and masks of the detected directory it was fitted
on (io.load_npp_completion with one proposal); its output then carries the iteration and equals the metrics.json that
`python -m npp_amd.train --eval_metrics` left in that result directory.

LPIPS is off by default; `--lpips vgg` (or `alex`) adds it (npp_amd.metrics.LPIPSMetric, the reference's
externel_lib/lpips/lpips.py:92-133 with use_robust=False, normalize=True): every region gains "lpips", the mean over the region's
pixels of the distance map D = sum_k upsample(d_k) (spatial=True) -- the trunk sees the whole images, only the mean is restricted to
the region -- and the report gains "lpips_image": {"net", "scalar"}, the scalar form sum_k mean d_k (spatial=False) that papers quote
for a whole image.  The two are different numbers: bilinear upsampling does not keep a map's mean.  The pretrained trunk is the
user's: --vgg16 / --alexnet PATH, or the places torchvision's pretrained=True leaves vgg16-*.pth / alexnet-owt-*.pth
(npp_amd.weights); the lin layers ship with the package (--lpips_lin PATH reads a user's lpips weights file instead).
--random-trunks runs on fixed-seed random trunks, as in npp_amd.search: for tests and synthetic runs, the figures then mean nothing.
Without --lpips the output text is what it was before the flag existed."""
import argparse
import json
import os
import re


def parse(argv=None):
    ap = argparse.ArgumentParser(description="PSNR / SSIM / MAE of an image against a ground truth, region by region, as JSON")
    ap.add_argument("--pred", default=None, help="the image to judge (PNG)")
    ap.add_argument("--gt", default=None, help="the ground truth (PNG of the same size)")
    ap.add_argument("--mask", default=None, help="unknown_mask.png of a detected directory: white = known (io.load_npp_completion)")
    ap.add_argument("--valid", default=None, help="valid_mask.png of a detected directory: white = valid")
    ap.add_argument("--results", default=None, help="a fit's result directory (holds testset_<iter>/): judge its newest test-set dump ...")
    ap.add_argument("--datadir", default=None, help="... against the ground truth and masks of this detected directory")
    ap.add_argument("--json", default=None, help="also write the report to this file")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--lpips", default=None, choices=["vgg", "alex"],
                    help="also report LPIPS on this net: per region the mean of the distance map, per image the scalar form (off by default)")
    ap.add_argument("--vgg16", default=None, help="torchvision vgg16 state_dict (.pth): the trunk of --lpips vgg")
    ap.add_argument("--alexnet", default=None, help="torchvision alexnet state_dict (.pth): the trunk of --lpips alex")
    ap.add_argument("--lpips_lin", default=None, help="lpips weights/v0.1/<net>.pth (the five 1x1 lin layers; default: the packaged copy)")
    ap.add_argument("--random-trunks", action="store_true",
                    help="run --lpips WITHOUT the pretrained trunk (fixed-seed random weights: tests and synthetic runs only -- the "
                         "figures are then not LPIPS distances)")
    args = ap.parse_args(argv)
    files, dirs = args.pred is not None or args.gt is not None, args.results is not None or args.datadir is not None
    if files == dirs or (files and (args.pred is None or args.gt is None)) or (dirs and (args.results is None or args.datadir is None)):
        ap.error("give either --pred and --gt (with optional --mask / --valid) or --results and --datadir")
    if dirs and (args.mask is not None or args.valid is not None):
        ap.error("--results / --datadir take the masks of the detected directory; --mask / --valid belong to --pred / --gt")
    return args


def newest_testset(results):
    """(iteration, directory) of the newest testset_<iter> dump under a result directory."""
    found = sorted((int(m.group(1)), e) for e in os.listdir(results) for m in [re.fullmatch(r"testset_(\d+)", e)] if m)
    if not found:
        raise SystemExit(f"{results}: no testset_<iter> directory")
    return found[-1][0], os.path.join(results, found[-1][1])


def dumps(rep):
    """The one serialisation of a report (evaluate's output and train's metrics.json are compared as text)."""
    return json.dumps(rep, sort_keys=True)


def lpips_metric(net, args, lin_path, device):
    """The LPIPSMetric of --lpips / --eval_lpips `net` from parsed flags (vgg16 / alexnet / random_trunks): the checkpoint is found
    like every other (weights.resolve: SystemExit naming it when it is missing and --random-trunks is not given) and read once per
    process (weights.load_state_dict), so the metric shares the packed weights of every trunk built from the same file."""
    from . import metrics, weights
    name = {"vgg": "vgg16", "alex": "alexnet"}[net]
    lacking = weights.resolve(args, [name], args.random_trunks)
    return metrics.LPIPSMetric(net, trunk_state_dict=weights.load_state_dict(getattr(args, name)), lin_weights=weights.lpips_lin(net, lin_path),
                               device=device, allow_random=bool(lacking))


def evaluate(args):
    from . import io as nio
    from . import metrics
    lp = None if args.lpips is None else lpips_metric(args.lpips, args, args.lpips_lin, args.device)
    if args.results is not None:
        it, tdir = newest_testset(args.results)
        d = nio.load_npp_completion(args.datadir, 1)
        pred, gt, mask, valid = nio._imread_rgb(os.path.join(tdir, "pred_rgb_img.png")), d["img"], d["mask"], d["valid_mask"]
        extra = {"iteration": it}
    else:
        pred, gt = nio._imread_rgb(args.pred), nio._imread_rgb(args.gt)
        valid = None if args.valid is None else nio._imread_gray(args.valid)
        mask = None if args.mask is None else nio._imread_gray(args.mask)
        if mask is not None and valid is not None:
            mask = mask * valid                                       # loaders.py:103
        extra = {}
    if mask is None:
        import numpy as np
        mask = np.ones(pred.shape[:2], np.float32)
    rep = metrics.report(pred.astype("float32"), gt.astype("float32"), mask.astype("float32"),
                         None if valid is None else valid.astype("float32"), device=args.device, **({} if lp is None else {"lpips": lp}))
    rep.update(extra)
    return rep


def main(argv=None):
    args = parse(argv)
    rep = evaluate(args)
    text = dumps(rep)
    print(text)
    if args.json:
        with open(args.json, "w") as f:
            f.write(text + "\n")
    return rep


if __name__ == "__main__":
    main()
