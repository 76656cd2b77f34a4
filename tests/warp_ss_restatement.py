"""NumPy restatement of the antialiased warp (include/npp_hip.h npp_warp_image_u8_ss), in the style of view_restatement.py: every
product, sum and quotient is one NumPy operation on float64 arrays, so each is rounded separately, and the samples of a pixel are
added in a loop over s.  The tests compare the library's host twin and kernel with it bit for bit."""
import numpy as np

from view_restatement import _position, WARP_MAPS, WARP_SRC, WARP_CANVAS, warp_source  # noqa: F401  (the cases the tests share)

SS = (1, 2, 4, 8)
REDUCES = ("mean", "min")


def offsets(ss):
    """off[a] = (2 a + 1) / (2 ss) - 0.5, a = 0 .. ss - 1, float64 (every value exact)."""
    a = np.arange(ss, dtype=np.float64)
    return (2.0 * a + 1.0) / np.float64(2 * ss) - 0.5


def sample(a, m, fi, fj, mode):
    """The source (Hs, Ws, C) uint8 at the canvas positions (fi, fj) (float64 arrays) under the nine numbers m -> (v (..., C) float64,
    counts (...) bool): the value before rounding -- the tapped byte, or the blend in the written order -- and whether the position
    lies in the source by the mode's test.  A position that does not count computes on source pixel (0, 0)."""
    Hs, Ws, _ = a.shape
    d, y, x = _position(m, fi, fj)
    ok = (d > 0) & np.isfinite(y) & np.isfinite(x)
    if mode == "nearest":
        with np.errstate(invalid="ignore"):
            iy, ix = np.floor(y + 0.5), np.floor(x + 0.5)
            ok = ok & (iy >= 0) & (iy < Hs) & (ix >= 0) & (ix < Ws)
        iy, ix = np.where(ok, iy, 0).astype(np.int64), np.where(ok, ix, 0).astype(np.int64)
        v = a[iy, ix].astype(np.float64)
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
    assert v.dtype == np.float64
    return v, ok


def sample_counts(src, M, size, mode, ss):
    """-> (counts (Ho, Wo, ss^2) bool, centre (Ho, Wo) bool): which samples of every canvas pixel count, and whether its centre does."""
    src = np.asarray(src, np.uint8)
    a = src.reshape(src.shape[0], src.shape[1], -1)
    Ho, Wo = size
    m = np.asarray(M, np.float64).reshape(9)
    i, j = np.meshgrid(np.arange(Ho, dtype=np.float64), np.arange(Wo, dtype=np.float64), indexing="ij")
    off = offsets(ss)
    counts = np.stack([sample(a, m, i + off[s // ss], j + off[s % ss], mode)[1] for s in range(ss * ss)], -1)
    return counts, sample(a, m, i, j, mode)[1]


def warp_image_ss(src, M, size, mode, ss, reduce="mean"):
    """-> (out (Ho, Wo[, C]) uint8, inside (Ho, Wo) uint8 in {0, 255}); mode 'nearest' or 'bilinear', reduce 'mean' or 'min'."""
    src = np.asarray(src, np.uint8)
    a = src.reshape(src.shape[0], src.shape[1], -1)
    C = a.shape[2]
    Ho, Wo = size
    m = np.asarray(M, np.float64).reshape(9)
    i, j = np.meshgrid(np.arange(Ho, dtype=np.float64), np.arange(Wo, dtype=np.float64), indexing="ij")
    off = offsets(ss)
    acc = np.zeros((Ho, Wo, C), np.float64)                       # mean: the ordered sum; min: the smallest value so far
    cnt = np.zeros((Ho, Wo), np.int64)
    for s in range(ss * ss):
        v, counts = sample(a, m, i + off[s // ss], j + off[s % ss], mode)
        if reduce == "mean":
            acc = np.where(counts[..., None], acc + v, acc)
        else:
            acc = np.where(counts[..., None] & ((cnt == 0)[..., None] | (v < acc)), v, acc)
        cnt = cnt + counts
        assert acc.dtype == np.float64
    if reduce == "mean":
        acc = acc / np.maximum(cnt, 1).astype(np.float64)[..., None]              # one IEEE quotient
    ok = sample(a, m, i, j, mode)[1] & (cnt > 0)                   # the centre is in the source and a sample counts
    out = np.clip(np.floor(acc + 0.5), 0, 255).astype(np.uint8)
    out = np.where(ok[..., None], out, 0).astype(np.uint8)
    return out.reshape((Ho, Wo) + src.shape[2:]), np.where(ok, 255, 0).astype(np.uint8)


# ---- cases the CPU and GPU tests share, with results that follow without the restatement ------------------------------------------------
def _block_map(S):
    """Canvas (i, j), sample (a, b) -> the integer source position (S i + a, S j + b): off[a] S + (S - 1) / 2 = a."""
    return np.array([[S, 0, (S - 1) / 2], [0, S, (S - 1) / 2], [0, 0, 1.0]])


def block_mean_case(S, seed=5):
    """-> (src (5 S, 7 S, 3), map, canvas (5, 7), the exact mean bytes (2 sum + S^2) // (2 S^2) of every S x S block)."""
    src = np.random.RandomState(seed + S).randint(0, 256, (5 * S, 7 * S, 3)).astype(np.uint8)
    sums = src.astype(np.int64).reshape(5, S, 7, S, 3).sum((1, 3))
    return src, _block_map(S), (5, 7), ((2 * sums + S * S) // (2 * S * S)).astype(np.uint8)


def block_min_case(S, seed=9):
    """A 0 / 255 source with one 0 per S x S block -> (src (5 S, 7 S), map, canvas, the mean byte floor(255 (S^2 - 1) / S^2 + 0.5))."""
    rng = np.random.RandomState(seed + S)
    src = np.full((5, S, 7, S), 255, np.uint8)
    for i in range(5):
        for j in range(7):
            src[i, rng.randint(S), j, rng.randint(S)] = 0
    return src.reshape(5 * S, 7 * S), _block_map(S), (5, 7), int(np.floor(255.0 * (S * S - 1) / (S * S) + 0.5))


def stripe_case():
    """64 x 64, odd columns 255 and even columns 0; every fourth pixel from (2, 2): -> (src, map, canvas 12 x 12)."""
    src = np.zeros((64, 64), np.uint8)
    src[:, 1::2] = 255
    return src, np.array([[4.0, 0, 2], [0, 4.0, 2], [0, 0, 1]]), (12, 12)


# the rectify command: most of a 128 x 160 photograph on a 24 x 30 canvas (it minifies about 5 x)
RECTIFY_QUAD = [2.0, 5.5, 7.5, 150.25, 118.0, 140.0, 110.5, 12.0]


def rectify_inputs(tmp_path):
    """A seeded 128 x 160 photograph and a mask with a hole -> (photo, mask, the command's arguments up to --outdir / --device)."""
    from PIL import Image
    rng = np.random.RandomState(21)
    photo = rng.randint(0, 256, (128, 160, 3)).astype(np.uint8)
    mask = np.full((128, 160), 255, np.uint8)
    mask[40:75, 50:97] = 0
    Image.fromarray(photo).save(tmp_path / "photo.png")
    Image.fromarray(mask).save(tmp_path / "mask.png")
    argv = ["--photo", str(tmp_path / "photo.png"), "--quad", *map(str, RECTIFY_QUAD), "--size", "24", "30", "--mask", str(tmp_path / "mask.png")]
    return photo, mask, argv
