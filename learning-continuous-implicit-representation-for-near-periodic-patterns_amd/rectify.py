"""Rectify a photograph of a planar pattern into the input folder `search` and `train` read.

    python -m npp_amd.rectify --photo P.png --quad y0 x0 y1 x1 y2 x2 y3 x3 --size H W
           [--mask photo_mask.png] --outdir data/completion/input/<name> [--supersample 1|2|4|8|auto] [--device cuda:0|cpu]

--quad: the corners (row col) of the pattern's rectangle in the photograph, in the order top-left, top-right, bottom-right,
bottom-left; the corner pixel centres of the H x W canvas land on them.  Written: gt_img.png (bilinear), valid_mask.png (the part of
the canvas the photograph covers), unknown_mask.png (--mask, a photo-frame mask with white = known, warped with nearest; all white
without it), masked_img.png (image x mask x valid) and view.json (sizes, quad and both 3 x 3 maps: `python -m npp_amd.render --view`
puts a fit back into the photograph).  The warp is npp_warp_image_u8 (float64 positions, bit for bit the same on the device and with
--device cpu, which runs the library's host twin and touches no GPU).

--supersample S (1, 2, 4, 8 or auto; default 1: point sampling) reduces every canvas pixel from S x S samples spread over its
footprint (npp_warp_image_u8_ss): gt_img.png is the mean of the bilinear samples that lie in the photograph, unknown_mask.png the
DARKEST nearest sample (a canvas pixel is known only if every counted sample of it reads known, so a hole's rim does not leak into
the training pixels), valid_mask.png white where the pixel centre lies in the photograph and a sample counts.  auto: the smallest S
that brings the largest sampling density down to view.MINIFY_WARN photo pixels per sample (view.supersample_for).  A photograph
several times the canvas's size wants it: point sampling turns a fine regular texture into moire of another period."""
import argparse
import os
import sys

import numpy as np


def parse(argv=None):
    ap = argparse.ArgumentParser(prog="python -m npp_amd.rectify", description=__doc__.split("\n")[0])
    ap.add_argument("--photo", required=True, help="the photograph (PNG)")
    ap.add_argument("--quad", type=float, nargs=8, required=True, metavar="YX",
                    help="y0 x0 y1 x1 y2 x2 y3 x3: top-left, top-right, bottom-right, bottom-left corner of the pattern's rectangle")
    ap.add_argument("--size", type=int, nargs=2, required=True, metavar=("H", "W"), help="size of the rectified canvas")
    ap.add_argument("--mask", default=None, help="photo-frame mask (PNG, white = known); default: everything known")
    ap.add_argument("--outdir", required=True, help="folder to write (must not exist or be empty)")
    ap.add_argument("--supersample", default=None, metavar="S",
                    help="S x S samples per canvas pixel, reduced in the launch: 1, 2, 4, 8 or auto (default 1: point sampling)")
    ap.add_argument("--device", default="cuda:0", help="cuda:N, or cpu for the library's host twin")
    args = ap.parse_args(argv)
    args.supersample_given = args.supersample is not None        # the closing line names S only when the flag was given
    if args.supersample != "auto":
        if args.supersample not in (None, "1", "2", "4", "8"):
            ap.error(f"--supersample {args.supersample}: must be 1, 2, 4, 8 or auto")
        args.supersample = int(args.supersample or 1)
    return args, ap


def main(argv=None):
    """-> the folder written.  Every argument is checked before a device is touched."""
    args, ap = parse(argv)
    from . import view
    if min(args.size) < 2:
        ap.error(f"--size {args.size}: both sides must be >= 2")
    if not np.isfinite(args.quad).all():
        ap.error(f"--quad {args.quad}: must be finite")
    if args.device != "cpu" and not args.device.startswith("cuda"):
        ap.error(f"--device {args.device}: cuda:N or cpu")
    for flag, path in (("--photo", args.photo), ("--mask", args.mask)):
        if path is not None and not os.path.isfile(path):
            ap.error(f"{flag} {path}: no such file")
    if os.path.exists(args.outdir) and (not os.path.isdir(args.outdir) or view.exists_nonempty(args.outdir)):
        ap.error(f"--outdir {args.outdir}: exists and is not empty")
    quad = np.asarray(args.quad, np.float64).reshape(4, 2)
    size = tuple(args.size)
    try:
        r2p, p2r = view.quad_to_rect(quad, size)
    except ValueError as e:
        ap.error(f"--quad {args.quad}: {e}")
    photo = view.imread_u8(args.photo)
    mask = view.imread_u8(args.mask, gray=True) if args.mask else None
    if mask is not None and mask.shape != photo.shape[:2]:
        ap.error(f"--mask {args.mask}: {mask.shape[0]} x {mask.shape[1]}, the photograph is {photo.shape[0]} x {photo.shape[1]}")
    ss = view.supersample_for(r2p, size) if args.supersample == "auto" else args.supersample
    print(view.density_report(r2p, size, "sampling density of the rectified canvas in the photograph", ss))

    host = lambda a: a if isinstance(a, np.ndarray) else a.cpu().numpy()      # noqa: E731
    gt, valid = (host(a) for a in view.warp_image(photo, r2p, size, "bilinear", device=args.device, supersample=ss))
    if mask is None:
        known = np.full(size, 255, np.uint8)
    else:
        known = host(view.warp_image(mask, r2p, size, "nearest", device=args.device, supersample=ss,
                                     reduce="min" if ss > 1 else "mean")[0])        # S = 1: the point launch, as without the flag
    keep = (known >= 128) & (valid != 0)
    masked = gt * keep[..., None].astype(np.uint8)

    from PIL import Image
    os.makedirs(args.outdir, exist_ok=True)
    for name, arr in (("gt_img.png", gt), ("valid_mask.png", valid), ("unknown_mask.png", known), ("masked_img.png", masked)):
        Image.fromarray(arr).save(os.path.join(args.outdir, name))
    view.write(os.path.join(args.outdir, "view.json"), photo.shape[:2], size, quad, r2p, p2r)
    print(f"rectified {photo.shape[0]} x {photo.shape[1]} -> {size[0]} x {size[1]} ({int((valid != 0).sum())} of {size[0] * size[1]} "
          f"canvas pixels covered)" + (f", {ss} x {ss} samples per canvas pixel" + (" (auto)" if args.supersample == "auto" else "")
                                       if args.supersample_given else "") + f" -> {args.outdir}")
    return args.outdir


if __name__ == "__main__":
    main(sys.argv[1:])
