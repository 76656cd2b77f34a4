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

LPIPS of whole images is deliberately not reported: the pretrained trunks are not part of this package, and its plain LPIPS head is
pinned on patch-sized features only."""
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


def evaluate(args):
    from . import io as nio
    from . import metrics
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
                         None if valid is None else valid.astype("float32"), device=args.device)
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
