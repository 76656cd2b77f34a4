"""NumPy restatement of the view rule (include/npp_hip.h npp_view, npp_warp_image_u8), written in the operation order the header
states: every product and sum is one NumPy operation on arrays of ONE dtype (fp32 for the render rule, float64 for the warp), so each
is rounded separately -- NumPy never contracts.  The tests compare the library's host twins and kernels with these bit for bit."""
import numpy as np


def _position(m, i, j):
    """d, y, x of canvas pixels (i, j) under the nine numbers m; m, i, j share one floating dtype."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d = (m[6] * i + m[7] * j) + m[8]
        y = ((m[0] * i + m[1] * j) + m[2]) / d
        x = ((m[3] * i + m[4] * j) + m[5]) / d
    return d, y, x


def view_coords(M, size, res, start=0, n=None):
    """The render rule in fp32 -> (yx (n, 2) float32, inside (n,) uint8) of canvas pixels [start, start + n) of a size = (H', W')
    canvas against the fit size res = (H, W): inside 0 not in view (the position is then (0, 0)), 1 in view, 3 in view and
    -0.5 <= y < H - 0.5, -0.5 <= x < W - 0.5."""
    Hc, Wc = size
    n = Hc * Wc - start if n is None else n
    p = np.arange(start, start + n, dtype=np.int64)
    m = np.asarray(M, np.float64).reshape(9).astype(np.float32)
    d, y, x = _position(m, (p // Wc).astype(np.float32), (p % Wc).astype(np.float32))
    assert d.dtype == y.dtype == x.dtype == np.float32
    view = (d > 0) & np.isfinite(y) & np.isfinite(x)
    half = np.float32(0.5)
    rect = (y >= -half) & (y < np.float32(res[0]) - half) & (x >= -half) & (x < np.float32(res[1]) - half)
    inside = np.where(view, np.where(rect, 3, 1), 0).astype(np.uint8)
    yx = np.stack([np.where(view, y, np.float32(0)), np.where(view, x, np.float32(0))], 1).astype(np.float32)
    return yx, inside


def warp_image(src, M, size, mode):
    """The warp in float64 -> (out (Ho, Wo[, C]) uint8, inside (Ho, Wo) uint8 in {0, 255}); mode 'nearest' or 'bilinear'."""
    src = np.asarray(src, np.uint8)
    a = src.reshape(src.shape[0], src.shape[1], -1)
    Hs, Ws, C = a.shape
    Ho, Wo = size
    m = np.asarray(M, np.float64).reshape(9)
    i, j = np.meshgrid(np.arange(Ho, dtype=np.float64), np.arange(Wo, dtype=np.float64), indexing="ij")
    d, y, x = _position(m, i, j)
    ok = (d > 0) & np.isfinite(y) & np.isfinite(x)
    if mode == "nearest":
        with np.errstate(invalid="ignore"):
            iy, ix = np.floor(y + 0.5), np.floor(x + 0.5)
            ok = ok & (iy >= 0) & (iy < Hs) & (ix >= 0) & (ix < Ws)
        iy, ix = np.where(ok, iy, 0).astype(np.int64), np.where(ok, ix, 0).astype(np.int64)
        out = a[iy, ix]
    else:
        with np.errstate(invalid="ignore"):
            ok = ok & (y >= 0) & (y <= Hs - 1) & (x >= 0) & (x <= Ws - 1)
        y, x = np.where(ok, y, 0.0), np.where(ok, x, 0.0)
        y0f, x0f = np.floor(y), np.floor(x)
        y0, x0 = y0f.astype(np.int64), x0f.astype(np.int64)
        y1, x1 = np.minimum(y0 + 1, Hs - 1), np.minimum(x0 + 1, Ws - 1)
        fy, fx = (y - y0f)[..., None], (x - x0f)[..., None]
        a00, a01, a10, a11 = (a[r, c].astype(np.float64) for r, c in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)))
        v = ((1 - fy) * ((1 - fx) * a00 + fx * a01)) + (fy * ((1 - fx) * a10 + fx * a11))
        out = np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)
    out = np.where(ok[..., None], out, 0).astype(np.uint8)
    return out.reshape((Ho, Wo) + src.shape[2:]), np.where(ok, 255, 0).astype(np.uint8)


# ---- the views the CPU and GPU tests share ------------------------------------------------------------------------------------------
CANVAS = (37, 53)


def affine(sy, sx, y0, x0):
    """The grid launch at origin (y0, x0), scale (sy, sx) as a view; exact for power-of-two scales."""
    return np.array([[1.0 / sy, 0.0, y0], [0.0, 1.0 / sx, x0], [0.0, 0.0, 1.0]])


# (sy, sx, y0, x0): every power of two of the issue, origins that are negative, fractional, past the border and -0.0
POW2_VIEWS = [(1, 1, 0.0, 0.0), (2, 2, -0.0, -0.0), (0.25, 0.5, -3.0, 5.5), (4, 8, 17.25, -40.0), (0.5, 0.25, -0.0, 100.0),
              (8, 1, 3.0, -0.0)]

# a general affine view (rotation, shear, scale) and a projective one over the canvas
AFFINE = np.array([[0.83, -0.31, 4.2], [0.27, 1.12, -6.5], [0.0, 0.0, 1.0]])
PROJECTIVE = np.array([[1.9, 0.22, -7.5], [-0.15, 2.3, 11.0], [0.0031, 0.0017, 1.0]])
# the horizon crosses the canvas: d = 1 - i / 8 is exactly 0 on canvas row 8 (dyadic numbers: exact in fp32 and float64), d < 0 below it
HORIZON = np.array([[3.0, 0.5, 12.0], [0.25, 4.0, -9.0], [-0.125, 0.0, 1.0]])

# the warp cases: source 23 x 31, canvas 40 x 29
WARP_SRC, WARP_CANVAS = (23, 31), (40, 29)
WARP_MAPS = {
    "identity": np.eye(3),
    "shift": np.array([[1.0, 0, -4], [0, 1.0, 6], [0, 0, 1]]),                                  # integer translation
    "affine": np.array([[0.52, 0.11, 1.3], [-0.07, 0.93, 2.9], [0, 0, 1.0]]),
    "projective": np.array([[0.9, 0.2, -5.0], [-0.1, 1.4, -3.0], [0.004, 0.006, 1.0]]),          # leaves the source on two sides
    "horizon": np.array([[0.6, 0.1, 2.0], [0.05, 0.9, 1.0], [-0.0625, 0.0, 1.0]]),              # d = 0 on canvas row 16
}


def warp_source(C, seed=0):
    """A seeded (23, 31, C) uint8 image ((23, 31) for C = 1)."""
    a = np.random.RandomState(seed).randint(0, 256, WARP_SRC + (C,)).astype(np.uint8)
    return a[..., 0] if C == 1 else a
