"""NumPy restatement of the supersampling class rule (include/npp_hip.h "adaptive supersampling"), in the operation order the header
states: the inside byte of the pixel centre by the fp32 view rule (view_restatement.view_coords), then d, t and the thresholds as
one float64 NumPy operation each -- NumPy never contracts, so each is rounded separately.  The tests compare the library's host
twin and kernel with this byte for byte."""
import numpy as np

import view_restatement as R

# The test view: every entry is dyadic.  On the 37 x 53 canvas all five classes occur, every class that can end in a ragged tile
# does (327 % 64, 465 % 16, 291 % 4 are not 0), 7 pixels have d exactly 0, 25 canvas rows change class inside the row and no pixel
# lies within 0.5 % of a threshold.
ADAPT_VIEW = np.array([[0.875, 0.0625, -3.0], [-0.03125, 1.125, 2.0], [-0.03125, -0.00390625, 1.015625]])
ADAPT_COUNTS = {0: 387, 1: 327, 2: 465, 4: 291, 8: 491}
# a power-of-two affine view of scale 1/4: density 4 everywhere, class 4
QUARTER = R.affine(0.25, 0.25, -3.0, 5.5)
# the whole canvas behind the horizon: d = -1 - i / 8 < 0 everywhere
BEHIND = np.array([[3.0, 0.5, 12.0], [0.25, 4.0, -9.0], [-0.125, 0.0, -1.0]])


def abs_det(M):
    """adet of the rule: |det| of the matrix stored as fp32, in float64, in the written order."""
    a, b, c, d1, e, f, g, h, k = (np.float64(v) for v in np.asarray(M, np.float64).reshape(9).astype(np.float32))
    return np.abs((a * (e * k - f * h) - b * (d1 * k - f * g)) + c * (d1 * h - e * g))


def classes(M, size, res, start=0, n=None):
    """-> (classes (n,) uint8 in {0, 1, 2, 4, 8}, inside (n,) uint8, margin (n,) float64) of canvas pixels [start, start + n): margin
    is the smallest relative distance |adet / (c t) - 1| to a threshold c t of a pixel in view (inf elsewhere)."""
    Hc, Wc = size
    n = Hc * Wc - start if n is None else n
    _, inside = R.view_coords(M, size, res, start, n)
    m = np.asarray(M, np.float64).reshape(9).astype(np.float32).astype(np.float64)
    p = np.arange(start, start + n, dtype=np.int64)
    i, j = (p // Wc).astype(np.float64), (p % Wc).astype(np.float64)
    d = np.abs((m[6] * i + m[7] * j) + m[8])
    t = (d * d) * d
    adet = abs_det(M)
    cls = np.full(n, 8, np.uint8)
    for S in (4, 2, 1):
        cls[adet <= (2.25 * S * S) * t] = S
    cls[inside == 0] = 0
    with np.errstate(divide="ignore", invalid="ignore"):
        margin = np.min([np.abs(adet / ((2.25 * S * S) * t) - 1.0) for S in (1, 2, 4)], 0)
    return cls, inside, np.where(inside != 0, margin, np.inf)
