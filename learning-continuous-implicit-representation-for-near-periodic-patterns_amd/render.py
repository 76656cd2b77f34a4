"""Render a saved NPP-Net (train.py --save_model -> model.npz) on any canvas: a denser grid than the image it was fitted to, a window
that reaches past the image border (the periodic warps carry the pattern on), or both.

    python -m npp_amd.render --model results/completion_top3/<name>/model.npz --out big.png --scale 2
    python -m npp_amd.render --model M.npz --out ext.png --origin -256 -256 --size 723 837

Canvas pixel (i, j) is the network at (y0 + i / sy, x0 + j / sx) of the fit's pixel frame (NPPNet.render_grid).  --size defaults to
ceil(H sy) x ceil(W sx): the fit's own canvas at that density.  The PNG is written with the conversion of the test-set dumps
(io.imsave: clip to [0, 1], round to 8 bit); --npy keeps the float32 values.

    python -m npp_amd.render --model M.npz --view view.json --out O.png [--into P.png] [--mask photo_mask.png] [--beyond]

With --view (the view.json `python -m npp_amd.rectify` wrote) the canvas is the photograph's frame and the network is evaluated
directly at the photograph's pixel positions mapped through photo_to_rect (NPPNet.render_view): no rendered image is resampled.
--into P.png writes the photograph with the render in place of its pixels inside the fit's rectangle (--beyond: wherever the plane
is in view; --mask: only where that photo-frame mask is black, i.e. unknown); every other pixel keeps the photograph's bytes.

    python -m npp_amd.render --model M.npz --out thumb.png --scale 0.25 --supersample auto

--supersample S (1, 2, 4, 8 or auto; default 1) renders every canvas pixel as the mean of S x S samples spread over its footprint,
averaged inside the render launch: antialiasing for a canvas that is coarser than the fit (a --scale below 1, the far end of a
--view).  auto takes the smallest S that brings the coarsest spot down to view.MINIFY_WARN fit pixels per sample, at most 8.
adaptive applies that rule per canvas pixel of a --view (NPPNet.render_view supersample="adaptive": every pixel is the pixel of the
uniform render at its own S, and the near field of a receding plane stops paying for the far end); the closing line names each
class's share and the chain rows against auto.  Without --view a grid has one density, and adaptive is auto."""
import argparse
import math
import os
import sys


def parse(argv=None):
    ap = argparse.ArgumentParser(prog="python -m npp_amd.render", description=__doc__.split("\n")[0])
    ap.add_argument("--model", required=True, help="model file written by `python -m npp_amd.train --save_model`")
    ap.add_argument("--out", required=True, help="output image (PNG)")
    ap.add_argument("--scale", type=float, nargs="+", default=None, metavar="S",
                    help="canvas pixels per fit pixel: one value, or SY SX (default 1)")
    ap.add_argument("--origin", type=float, nargs=2, default=None, metavar=("Y0", "X0"),
                    help="fit-frame position of canvas pixel (0, 0) (default 0 0)")
    ap.add_argument("--size", type=int, nargs=2, default=None, metavar=("H", "W"), help="canvas size (default ceil(H sy) x ceil(W sx))")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"], help="bf16: the fused chain of the fit; fp32: the exact chain")
    ap.add_argument("--npy", default=None, help="also write the (H, W, 3) float32 canvas as .npy")
    ap.add_argument("--chunk_rows", type=int, default=1 << 22, help="canvas pixels per launch (times S^2 samples: chain rows per launch)")
    ap.add_argument("--supersample", default=None, metavar="S",
                    help="S x S samples per canvas pixel, averaged in the launch: 1, 2, 4, 8, auto or adaptive (per pixel of a --view; "
                         "default 1: point sampling)")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--view", default=None, help="view.json of `python -m npp_amd.rectify`: render in the photograph's frame")
    ap.add_argument("--into", default=None, help="with --view: the photograph (PNG) to put the render into")
    ap.add_argument("--mask", default=None, help="with --into: photo-frame mask (PNG, white = known); replace only where it is black")
    ap.add_argument("--beyond", action="store_true", help="with --into: also replace pixels past the fit's border, wherever the plane is in view")
    args = ap.parse_args(argv)
    if args.view is not None:
        for flag, v in (("--scale", args.scale), ("--origin", args.origin), ("--size", args.size)):
            if v is not None:
                ap.error(f"{flag} cannot be combined with --view: the canvas and the map come from the view file")
        if (args.mask is not None or args.beyond) and args.into is None:
            ap.error("--mask / --beyond need --into")
    elif args.into is not None or args.mask is not None or args.beyond:
        ap.error("--into / --mask / --beyond need --view")
    args.scale = [1.0] if args.scale is None else args.scale
    args.origin = [0.0, 0.0] if args.origin is None else args.origin
    if len(args.scale) not in (1, 2):
        ap.error("--scale takes one value S or two values SY SX")
    sy, sx = (args.scale * 2)[:2]
    if not all(math.isfinite(s) and s > 0 for s in (sy, sx)):
        ap.error(f"--scale {args.scale}: must be finite and > 0")
    if not all(math.isfinite(o) for o in args.origin):
        ap.error(f"--origin {args.origin}: must be finite")
    if args.size is not None and min(args.size) < 1:
        ap.error(f"--size {args.size}: both sides must be >= 1")
    if args.chunk_rows < 1:
        ap.error(f"--chunk_rows {args.chunk_rows}: must be >= 1")
    args.scale = (sy, sx)
    args.supersample_given = args.supersample is not None        # the closing line names S only when the flag was given
    if args.supersample not in ("auto", "adaptive"):
        if args.supersample not in (None, "1", "2", "4", "8"):
            ap.error(f"--supersample {args.supersample}: must be 1, 2, 4, 8 or auto, or adaptive (a class per pixel of a --view)")
        args.supersample = int(args.supersample or 1)
    return args, ap


def auto_supersample(scale):
    """--supersample auto of a grid render: view.supersample_for's rule on the fit pixels per canvas pixel, max(1 / sy, 1 / sx)."""
    from . import view
    return view.supersample_for_density(max(1.0 / scale[0], 1.0 / scale[1]))


def main(argv=None):
    """-> the rendered canvas, (H, W, 3) float32 NumPy.  Every argument and the model file are checked before the GPU is touched."""
    args, ap = parse(argv)
    from . import modelfile
    if not os.path.isfile(args.model):
        ap.error(f"--model {args.model}: no such file")
    try:
        d = modelfile.read(args.model)
    except ValueError as e:
        ap.error(f"--model: {e}")
    sy, sx = args.scale
    H, W = d["res"]
    size = tuple(args.size) if args.size is not None else (math.ceil(H * sy), math.ceil(W * sx))
    out_dir = os.path.dirname(os.path.abspath(args.out))
    if not os.path.isdir(out_dir):
        ap.error(f"--out {args.out}: directory {out_dir} does not exist")

    if args.view is not None:
        return _main_view(args, ap, (H, W))
    from . import io as nio
    from .model import NPPNet
    net = NPPNet.load(args.model, device=args.device)
    ss = auto_supersample((sy, sx)) if args.supersample in ("auto", "adaptive") else args.supersample
    img = net.render_grid(size, origin=tuple(args.origin), scale=(sy, sx), precision=args.precision, chunk_rows=args.chunk_rows,
                          supersample=ss)
    img = img.cpu().numpy()
    nio.imsave(args.out, img)               # what dump_testset writes as pred_rgb_img.png (a tanh output is clipped there too)
    if args.npy:
        import numpy as np
        np.save(args.npy, img)
    print(f"rendered {size[0]} x {size[1]} ({args.precision}) at scale ({sy:g}, {sx:g}), origin ({args.origin[0]:g}, {args.origin[1]:g}) "
          f"of a {H} x {W} fit" + _ss_note(args, ss) + f" -> {args.out}")
    return img


def _ss_note(args, ss):
    """What the closing line says about supersampling: nothing unless the flag was given."""
    if not args.supersample_given:
        return ""
    how = {"auto": " (auto)", "adaptive": " (adaptive: a grid has one density, so this is auto)"}.get(args.supersample, "")
    return f", {ss} x {ss} samples per pixel" + how


def _main_view(args, ap, res):
    """--view: the render in the photograph's frame (NPPNet.render_view under photo_to_rect), alone or put into the photograph."""
    import numpy as np
    from . import view
    try:
        v = view.read(args.view)
    except ValueError as e:
        ap.error(f"--view: {e}")
    if tuple(v["rect_size"]) != tuple(res):
        ap.error(f"--view {args.view}: rectified size {v['rect_size']} is not the fit's {tuple(res)}")
    for flag, path in (("--into", args.into), ("--mask", args.mask)):
        if path is not None and not os.path.isfile(path):
            ap.error(f"{flag} {path}: no such file")
    size = v["photo_size"]
    photo = view.imread_u8(args.into) if args.into else None
    mask = view.imread_u8(args.mask, gray=True) if args.mask else None
    for flag, a in (("--into", photo), ("--mask", mask)):
        if a is not None and tuple(a.shape[:2]) != tuple(size):
            ap.error(f"{flag}: {a.shape[0]} x {a.shape[1]}, the view's photograph is {size[0]} x {size[1]}")
    adaptive = args.supersample == "adaptive"
    ss = view.supersample_for(v["photo_to_rect"], size) if args.supersample == "auto" else args.supersample
    print(view.density_report(v["photo_to_rect"], size, "sampling density of the photograph on the fit's plane", ss))

    from . import io as nio
    from .model import NPPNet
    net = NPPNet.load(args.model, device=args.device)
    img, inside, *classes = net.render_view(size, v["photo_to_rect"], precision=args.precision, chunk_rows=args.chunk_rows,
                                            return_inside=True, supersample=ss, return_classes=adaptive)
    if photo is not None:
        from PIL import Image
        Image.fromarray(view.composite(photo, img, inside, mask=mask, beyond=args.beyond).cpu().numpy()).save(args.out)
    img = img.cpu().numpy()
    if photo is None:
        nio.imsave(args.out, img)
    if args.npy:
        np.save(args.npy, img)
    n_in, n_fit = int((inside != 0).sum()), int((inside == 3).sum())
    print(f"rendered {size[0]} x {size[1]} ({args.precision}) under {args.view}: {n_in} pixels in view, {n_fit} inside the "
          f"{res[0]} x {res[1]} fit" + (", " + view.adaptive_note(classes[0].cpu().numpy(), auto=view.supersample_for(v["photo_to_rect"], size))
                                        if adaptive else _ss_note(args, ss)) + (f", put into {args.into}" if args.into else "") + f" -> {args.out}")
    return img


if __name__ == "__main__":
    main(sys.argv[1:])
