#!/usr/bin/env python3
"""Golden G15 masks: the known-pixel masks of the reference's eight sample inputs (data/*/input/*/unknown_mask.png times
valid_mask.png, non-zero = known, as search.pseudo_mask_split multiplies them) -- real hole shapes for the distance transform and the
far-point selection of the periodicity search's front end.  Data only: the script reads those PNGs and nothing else.  Stored as
np.packbits rows (`bits_<k>`) with `shapes` (8, 2) and `names`.
    python tests/golden/make_golden_masks.py"""
import glob
import os

import numpy as np
from PIL import Image

REF, OUT = os.environ.get("NPP_REFERENCE", "/root/reference"), os.path.dirname(os.path.abspath(__file__))


def main():
    dirs = sorted(os.path.dirname(p) for p in glob.glob(os.path.join(REF, "data", "*", "input", "*", "unknown_mask.png")))
    rd = lambda d, f: np.asarray(Image.open(os.path.join(d, f)).convert("L"), dtype=np.float64) / 255.0   # noqa: E731  (io._imread_gray)
    out, shapes, names = {}, [], []
    for k, d in enumerate(dirs):
        known = (rd(d, "unknown_mask.png") * rd(d, "valid_mask.png")) != 0
        out[f"bits_{k}"] = np.packbits(known.reshape(-1))
        shapes.append(known.shape)
        names.append("/".join(d.split(os.sep)[-3:]))
        print(names[-1], known.shape, "known share", known.mean())
    np.savez_compressed(os.path.join(OUT, "g15_masks.npz"), shapes=np.asarray(shapes, np.int64), names=np.asarray(names), **out)


if __name__ == "__main__":
    main()
