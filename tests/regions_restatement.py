"""Helper of test_regions_cpu.py / test_gpu_regions.py (not a test): the case generators and the yardstick of the connected-component
entries (include/npp_hip.h npp_cc_*).  The yardstick is scipy.ndimage.label with its default cross structure -- for an image of
several values, each distinct value labelled separately and the union renumbered in raster order of first appearance (label's own
numbering of one mask is already that order) -- and direct NumPy statements of the statistics.  Nothing here comes from the kernels."""
import numpy as np
import scipy.ndimage as ndi

SHAPES = [(1, 1), (1, 70), (70, 1), (2, 2), (17, 33), (64, 64), (65, 63), (97, 130), (211, 325)]     # every border of a 16 / 32 tile


# ---- the yardstick --------------------------------------------------------------------------------------------------------------
def raster_renumber(ids, inside):
    """ids (H,W), distinct per component where `inside` -> 1..C in raster order of first appearance, 0 outside; C."""
    out = np.zeros(ids.shape, np.int32)
    if not inside.any():
        return out, 0
    values, first = np.unique(ids[inside], return_index=True)
    remap = np.zeros(int(values.max()) + 1, np.int64)
    remap[values[np.argsort(first, kind="stable")]] = np.arange(1, len(values) + 1)
    out[inside] = remap[ids[inside]]
    return out, len(values)


def label(x):
    """The 4-connected components of equal non-zero values of x -> (numbered (H,W) int32, C)."""
    x = np.asarray(x)
    if x.dtype == bool:
        x = x.astype(np.int32)
    ids = np.zeros(x.shape, np.int64)
    base = 0
    for v in np.unique(x[x != 0]):
        lab, n = ndi.label(x == v)
        ids[lab > 0] = lab[lab > 0] + base
        base += n
    return raster_renumber(ids, x != 0)


def stats(numbered, C, values=None):
    """sizes (C,), sums (C,nch), border (C,), boxes (C,4) of the components 1..C, stated directly."""
    H, W = numbered.shape
    flat = numbered.ravel()
    sizes = np.bincount(flat, minlength=C + 1)[1:].astype(np.int64)
    nch = 0 if values is None else values.shape[2]
    sums = np.zeros((C, nch), np.int64)
    for k in range(nch):
        sums[:, k] = np.rint(np.bincount(flat, weights=values[..., k].ravel().astype(np.float64), minlength=C + 1)[1:]).astype(np.int64)
    edge = np.zeros((H, W), bool)
    edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
    border = np.zeros(C, np.uint8)
    border[np.unique(numbered[edge & (numbered > 0)]) - 1] = 1
    boxes = np.zeros((C, 4), np.int32)
    for c, sl in enumerate(ndi.find_objects(numbered, max_label=C)):
        boxes[c] = (sl[0].start, sl[1].start, sl[0].stop - 1, sl[1].stop - 1)
    return sizes, sums, border, boxes


# ---- the contents ---------------------------------------------------------------------------------------------------------------
def serpentine(H, W):
    """Every second row set, joined alternately at the right and the left end: ONE component whose chain is ~H W / 2 long."""
    m = np.zeros((H, W), bool)
    m[0::2] = True
    for k, y in enumerate(range(1, H - 1, 2)):
        m[y, W - 1 if k % 2 == 0 else 0] = True
    return m


def spiral(H, W):
    """A square spiral: an arm one pixel wide walked inwards from (0, 0), turning right whenever the cell ahead is taken or the one
    behind it is (so that a one-pixel gap stays between the laps)."""
    m = np.zeros((H, W), bool)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = True
    inb = lambda i, j: 0 <= i < H and 0 <= j < W                                         # noqa: E731
    while True:
        for _ in range(4):
            ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if inb(ny, nx) and not m[ny, nx] and not (inb(ay, ax) and m[ay, ax]):
                y, x = ny, nx
                m[y, x] = True
                break
            dy, dx = dx, -dy
        else:
            return m


def comb(H, W):
    """A spine along the last row, a tooth on every second column."""
    m = np.zeros((H, W), bool)
    m[1:, 0::2] = True
    m[H - 1] = True
    return m


def rings(H, W):
    """Nested rings by Chebyshev distance to the border: rings 0, 2, 4, .. set -- holes inside objects inside holes."""
    y, x = np.mgrid[0:H, 0:W]
    d = np.minimum(np.minimum(y, H - 1 - y), np.minimum(x, W - 1 - x))
    return (d // 2) % 2 == 0


def frame_island(H, W):
    m = np.zeros((H, W), bool)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    m[H // 2 - H // 8:H // 2 + H // 8 + 1, W // 2 - W // 8:W // 2 + W // 8 + 1] = True
    if H >= 9 and W >= 9:
        m[H // 2, W // 2] = False                                                        # a hole in the island where it has room
    return m


def blocky(H, W, seed):
    """A blocky 4-valued image (values 0..3, 0 = outside) with 25 % of its pixels displaced: the fragment structure SLIC leaves."""
    rs = np.random.RandomState(seed)
    coarse = rs.randint(0, 4, ((H + 10) // 11 + 1, (W + 12) // 13 + 1))
    img = np.kron(coarse, np.ones((11, 13), np.int64))[:H, :W]
    k = rs.rand(H, W) < 0.25
    yy, xx = np.mgrid[0:H, 0:W]
    sy = np.clip(yy + rs.randint(-3, 4, (H, W)), 0, H - 1)
    sx = np.clip(xx + rs.randint(-3, 4, (H, W)), 0, W - 1)
    img = np.where(k, img[sy, sx], img)
    return img.astype(np.int32)


def contents(H, W):
    """name -> (H,W) image: bool masks and one int32 image of several values."""
    y, x = np.mgrid[0:H, 0:W]
    out = {"zeros": np.zeros((H, W), bool), "ones": np.ones((H, W), bool), "checker": (y + x) % 2 == 0, "rows": y % 2 == 0,
           "cols": x % 2 == 0, "serpentine": serpentine(H, W), "spiral": spiral(H, W), "comb": comb(H, W), "rings": rings(H, W),
           "frame": frame_island(H, W)}
    for p in (0.3, 0.5, 0.59, 0.8):                         # 0.59: near the site-percolation threshold, large tortuous components
        out[f"random{p}"] = np.random.RandomState(int(p * 100) + H * 1000 + W).rand(H, W) < p
    out["blocky"] = blocky(H, W, H * 7 + W)
    return out


def cases():
    """[(id, image)] over SHAPES x contents."""
    return [(f"{H}x{W}-{name}", img) for H, W in SHAPES for name, img in contents(H, W).items()]


def colour_of(shape, seed=5):
    return np.random.RandomState(seed).randint(0, 256, tuple(shape) + (3,)).astype(np.uint8)


def planted_pair(H=60, W=90):
    """A mask with one component of exactly 499 pixels beside one of exactly 500 (and a speck of 3)."""
    m = np.zeros((H, W), bool)
    m[2:22, 2:27] = True          # 20 x 25 = 500
    m[2:22, 30:55] = True         # 500 ...
    m[21, 54] = False             # ... - 1 = 499
    m[40, 40:43] = True
    return m
