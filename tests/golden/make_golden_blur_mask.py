#!/usr/bin/env python3
"""Golden G13b: NPP_remapping/blur_detection.py:13-60 get_blur_map on an image whose CLEAR MASK is not trivial (g13_blur.npz is
72 x 88: 20 erosions delete every blob there, so its mask is all ones and cannot test the morphology).  150 x 230: a sharp left
half, a Gaussian-blurred right half and a flat patch (rank-1 windows, the map's maximum).  The pixel count is even on purpose:
with an odd count the 50th percentile is itself a data value and no pixel has a margin to it.  Same recipe as
make_golden_blur.py: cv2 is not installed, so the reference's function definition is ast-executed from the reference file with a
stand-in `cv2` (OpenCV's documented 14-bit fixed-point RGB2GRAY) and `np.float` mapped to float.
    python tests/golden/make_golden_blur_mask.py"""
import ast
import os
import sys
import types

import numpy as np
import scipy.ndimage as ndimage

REF, OUT = os.environ.get("NPP_REFERENCE", "/root/reference"), os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
from blur_restatement import make_image  # noqa: E402  (the scene's recipe, shared with the tests and tools/blur_time.py)


def main():
    cv2 = types.SimpleNamespace(COLOR_RGB2GRAY=7,
                                cvtColor=lambda img, code: ((img.astype(np.int64) * np.array([4899, 9617, 1868])).sum(-1) + 8192 >> 14).astype(np.uint8))
    npx = types.ModuleType("np")
    npx.__dict__.update(np.__dict__)
    npx.float = float
    ns = {"cv2": cv2, "np": npx, "ndimage": ndimage}
    tree = ast.parse(open(os.path.join(REF, "NPP_remapping/blur_detection.py")).read())
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name == "get_blur_map":
            exec(compile(ast.Module([node], []), "blur_detection.py", "exec"), ns)
    img = make_image()
    thresh = 50
    bm, clear = ns["get_blur_map"](img, thresh=thresh)
    np.savez_compressed(os.path.join(OUT, "g13b_blur_mask.npz"), img=img, blur_map=bm, clear=clear, thresh=np.int64(thresh))
    margin = np.abs(bm - np.percentile(bm, thresh)).min()
    print(bm.shape, "clear share", clear.mean() / 255, "map max at flat patch", bm[40, 50], "margin to the threshold", margin)


if __name__ == "__main__":
    main()
