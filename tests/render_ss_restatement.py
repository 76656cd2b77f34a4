"""NumPy restatement of the supersampling rule (include/npp_hip.h "supersampled launches"), in the style of view_restatement.py:
every product, sum and quotient is one NumPy operation on fp32 arrays, so each is rounded separately.  The tests compare the
library's host twins and kernels with these bit for bit."""
import numpy as np

import view_restatement as R

F = np.float32
SS = (1, 2, 4, 8)

# a slanted horizon that cuts through pixels: d = (-i / 8 + j / 128) + 57 / 64 (dyadic numbers, exact in fp32)
SS_HORIZON = np.array([[3.0, 0.5, 12.0], [0.25, 4.0, -9.0], [-0.125, 0.0078125, 0.890625]])
# the grid of the render_at comparison
GRID_SCALE, GRID_ORIGIN = (0.75, 1.3), (-3.5, 17.25)


def offsets(ss):
    """off[a] = (2 a + 1) / (2 ss) - 0.5, a = 0 .. ss - 1, fp32 (every value exact)."""
    a = np.arange(ss, dtype=np.float32)
    return (F(2) * a + F(1)) / F(2 * ss) - F(0.5)


def canvas_positions(width, ss, start, n):
    """(fi, fj) fp32 of the n ss^2 chain rows of a launch on canvas pixels [start, start + n): row r is sample r % ss^2 = a ss + b of
    pixel start + r // ss^2, at (i + off[a], j + off[b])."""
    r = np.arange(n * ss * ss, dtype=np.int64)
    p, s = start + r // (ss * ss), r % (ss * ss)
    off = offsets(ss)
    fi = (p // width).astype(np.float32) + off[s // ss]
    fj = (p % width).astype(np.float32) + off[s % ss]
    assert fi.dtype == fj.dtype == np.float32
    return fi, fj


def grid_samples(size, origin, scale, ss, start=0, n=None):
    """(n ss^2, 2) fp32 [y, x]: y = y0 + fi / sy, x = x0 + fj / sx (a quotient, then a separate add)."""
    Hc, Wc = size
    n = Hc * Wc - start if n is None else n
    fi, fj = canvas_positions(Wc, ss, start, n)
    y = F(origin[0]) + fi / F(scale[0])
    x = F(origin[1]) + fj / F(scale[1])
    return np.stack([y, x], 1).astype(np.float32)


def view_samples(M, size, res, ss, start=0, n=None):
    """-> (yx (n ss^2, 2) fp32, counts (n ss^2,) bool, inside (n,) uint8): the sample positions under the view ((0, 0) where a sample is
    not in view), which samples count, and the byte a launch writes per pixel: the point launch's byte of the pixel centre, 0 where no
    sample counts."""
    Hc, Wc = size
    n = Hc * Wc - start if n is None else n
    m = np.asarray(M, np.float64).reshape(9).astype(np.float32)
    fi, fj = canvas_positions(Wc, ss, start, n)
    d, y, x = R._position(m, fi, fj)
    assert d.dtype == y.dtype == x.dtype == np.float32
    counts = (d > 0) & np.isfinite(y) & np.isfinite(x)
    yx = np.stack([np.where(counts, y, F(0)), np.where(counts, x, F(0))], 1).astype(np.float32)
    _, centre = R.view_coords(M, size, res, start, n)
    inside = np.where(counts.reshape(n, ss * ss).any(1), centre, 0).astype(np.uint8)
    return yx, counts, inside


def average(o, counts_mask=None):
    """o (n, ss^2, C) fp32 sample values, counts_mask (n, ss^2) bool or None (all count) -> (mean (n, C) fp32, count (n,)): acc = +0,
    one rounded fp32 add per counting sample in order, then a quotient by the count (0 / 0 where none counts: the caller stores 0)."""
    o = np.asarray(o, np.float32)
    n, s2, C = o.shape
    mask = np.ones((n, s2), bool) if counts_mask is None else np.asarray(counts_mask, bool).reshape(n, s2)
    acc = np.zeros((n, C), np.float32)
    for s in range(s2):
        acc = np.where(mask[:, s, None], acc + o[:, s], acc)
        assert acc.dtype == np.float32
    count = mask.sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = acc / count.astype(np.float32)[:, None]
    return mean.astype(np.float32), count


def pixel_colours(o, counts_mask, inside):
    """What a view launch stores: average(), and exactly +0 where the centre's inside byte is 0 or no sample counts."""
    mean, count = average(o, counts_mask)
    return np.where(((np.asarray(inside) != 0) & (count > 0))[:, None], mean, F(0)).astype(np.float32)
