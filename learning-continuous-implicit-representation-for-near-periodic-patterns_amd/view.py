"""Perspective views: the 3 x 3 map between a photograph and the rectified canvas a pattern is fitted on (DESIGN.md "Perspective
views").

A view is a row-major 3 x 3 matrix M that takes a canvas pixel (row i, col j) to a position (y, x) of a target frame, integer
positions at pixel centres:

    d = (m6 i + m7 j) + m8,   y = ((m0 i + m1 j) + m2) / d,   x = ((m3 i + m4 j) + m5) / d

in exactly this operation order, every product and sum rounded separately.  The host part below (fitting, inverting, the view.json
file) is float64 NumPy; the image warp (npp_warp_image_u8, float64) and the projective render (NPPNet.render_view, fp32) evaluate
the rule in the library, on the device or by its host twins."""
import json
import os

import numpy as np

MINIFY_WARN = 1.5      # target pixels per canvas pixel above which point sampling visibly aliases (sampling_density)


def _points(p, name):
    a = np.asarray(p, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] < 4:
        raise ValueError(f"{name}: expected (N >= 4, 2) points [row, col], got shape {a.shape}")
    if not np.isfinite(a).all():
        raise ValueError(f"{name}: points must be finite")
    return a


def _normalizer(p):
    """Hartley's conditioning: the similarity that moves the centroid to 0 and the mean distance to sqrt(2)."""
    c = p.mean(0)
    s = np.sqrt(((p - c) ** 2).sum(1)).mean()
    if not s > 0:
        raise ValueError("degenerate correspondences: all points coincide")
    k = np.sqrt(2.0) / s
    return np.array([[k, 0, -k * c[0]], [0, k, -k * c[1]], [0, 0, 1.0]])


def homography_from_points(src_yx, dst_yx):
    """The map M with M(src) = dst for N >= 4 correspondences, (row, col) -> (y, x), by least squares (the direct linear transform on
    conditioned points), normalised so that m8 = 1.  ValueError names the condition when the points do not determine a map: fewer
    than four, repeated, or three of four collinear."""
    s, d = _points(src_yx, "src_yx"), _points(dst_yx, "dst_yx")
    if s.shape != d.shape:
        raise ValueError(f"src_yx {s.shape} and dst_yx {d.shape} must pair up")
    Ts, Td = _normalizer(s), _normalizer(d)
    sn = s @ Ts[:2, :2].T + Ts[:2, 2]
    dn = d @ Td[:2, :2].T + Td[:2, 2]
    A = np.zeros((2 * len(s), 9))
    for k, ((i, j), (y, x)) in enumerate(zip(sn, dn)):
        A[2 * k] = [i, j, 1, 0, 0, 0, -y * i, -y * j, -y]
        A[2 * k + 1] = [0, 0, 0, i, j, 1, -x * i, -x * j, -x]
    _, sv, vt = np.linalg.svd(A)
    if sv[7] <= 1e-10 * sv[0]:
        raise ValueError("degenerate correspondences: collinear or repeated points do not determine a homography "
                         f"(rank of the design matrix < 8, singular values {sv[0]:.3g} .. {sv[7]:.3g})")
    M = np.linalg.inv(Td) @ vt[8].reshape(3, 3) @ Ts
    if not abs(M[2, 2]) > 1e-12 * np.abs(M).max():
        raise ValueError("degenerate correspondences: the source origin maps to infinity (m8 = 0), the map cannot be normalised")
    M = M / M[2, 2]
    back = apply(M, s)
    if not np.isfinite(back).all() or np.linalg.matrix_rank(M) < 3:
        raise ValueError("degenerate correspondences: collinear points give a singular homography")
    return M


def check_matrix(M):
    """M as a (3, 3) float64 array; ValueError for a wrong shape, a non-finite entry (in float64 or once stored as float32) or a
    singular matrix."""
    m = np.asarray(M, dtype=np.float64)
    if m.size != 9:
        raise ValueError(f"M: expected a 3 x 3 matrix, got shape {m.shape}")
    m = m.reshape(3, 3)
    with np.errstate(over="ignore"):
        if not (np.isfinite(m).all() and np.isfinite(m.astype(np.float32)).all()):
            raise ValueError("M: non-finite matrix entry")
    if np.linalg.det(m) == 0.0 or not np.linalg.cond(m) < 1e15:
        raise ValueError("M: singular matrix")
    return m


def invert(M):
    """The inverse map, scaled by a POSITIVE factor so that |m8| = 1 where m8 != 0 (a positive factor keeps the sign of d, which
    decides what is in view).  ValueError when M is singular."""
    inv = np.linalg.inv(check_matrix(M))
    k = abs(inv[2, 2])
    return inv / k if k > 1e-300 else inv


def apply(M, pts_ij):
    """The positions (N, 2) [y, x] of the points (N, 2) [row, col] under M, float64, in the operation order of the module docstring."""
    m = np.asarray(M, dtype=np.float64).reshape(-1)
    p = np.asarray(pts_ij, dtype=np.float64).reshape(-1, 2)
    i, j = p[:, 0], p[:, 1]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d = (m[6] * i + m[7] * j) + m[8]
        return np.stack([((m[0] * i + m[1] * j) + m[2]) / d, ((m[3] * i + m[4] * j) + m[5]) / d], 1)


def _size(size):
    H, W = (int(s) for s in size)
    if H < 1 or W < 1:
        raise ValueError(f"size {tuple(size)}: both sides must be >= 1")
    return H, W


def quad_to_rect(quad_yx, size):
    """quad_yx: the four corners (row, col) of the pattern's rectangle in the photograph, in the order top-left, top-right,
    bottom-right, bottom-left; size = (H, W) of the rectified canvas, whose corner PIXEL CENTRES land on them.  ->
    (rect_to_photo, photo_to_rect), both (row, col) -> (y, x)."""
    q = np.asarray(quad_yx, dtype=np.float64).reshape(-1, 2)
    if q.shape[0] != 4:
        raise ValueError(f"quad_yx: expected four corners, got {q.shape[0]}")
    H, W = _size(size)
    if H < 2 or W < 2:
        raise ValueError(f"size {tuple(size)}: a rectified canvas needs at least 2 x 2 pixels")
    rect = np.array([[0, 0], [0, W - 1], [H - 1, W - 1], [H - 1, 0]], np.float64)
    r2p = homography_from_points(rect, q)
    return r2p, invert(r2p)


def sampling_density(M, size):
    """(smallest, largest) sqrt|det J| of the map over the size = (H, W) canvas: target pixels per canvas pixel (1 = the target's own
    density, 2 = every second target pixel is skipped in each direction: point sampling aliases).  For a homography det J =
    det M / d^3; evaluated on a 3 x 3 lattice of the canvas (corners, edge midpoints, centre), the extremes of a monotone |d|.  A
    lattice point that is not in view (d <= 0) counts as infinite."""
    m = check_matrix(M)
    H, W = _size(size)
    i, j = np.meshgrid(np.array([0.0, (H - 1) / 2, H - 1]), np.array([0.0, (W - 1) / 2, W - 1]), indexing="ij")
    d = (m[2, 0] * i + m[2, 1] * j) + m[2, 2]
    with np.errstate(divide="ignore"):
        dens = np.where(d > 0, np.sqrt(abs(np.linalg.det(m)) / np.abs(d) ** 3), np.inf)
    return float(dens.min()), float(dens.max())


SUPERSAMPLES = (1, 2, 4, 8)      # samples per canvas pixel and direction the render launches take (NPPNet.render_view supersample=)


def supersample_for_density(density):
    """The smallest S in SUPERSAMPLES whose S x S samples per canvas pixel bring `density` target pixels per canvas pixel down to
    density / S <= MINIFY_WARN per sample; the largest S where none does (an infinite density included)."""
    for S in SUPERSAMPLES:
        if density / S <= MINIFY_WARN:
            return S
    return SUPERSAMPLES[-1]


def supersample_for(M, size):
    """supersample_for_density of the largest sampling_density of the view over the size = (H, W) canvas: what
    `python -m npp_amd.render --view ... --supersample auto` renders with."""
    return supersample_for_density(sampling_density(M, size)[1])


def supersample_classes(M, size, res=(1, 1)):
    """The (H', W') uint8 map of render_view(supersample="adaptive"): per pixel of the size = (H', W') canvas 0 where it is not in
    view, else supersample_for_density of sqrt|det J| at the pixel centre -- the exact rule of include/npp_hip.h "adaptive
    supersampling" on M stored as float32, by the library's host twin (the device launch gives the same bytes).  res = (H, W) of the
    fit: it does not enter the classes (only inside byte 3, which this does not return)."""
    from . import ops
    Hc, Wc = _size(size)
    return ops.view_ss_classes_host(ops.view_arg(0, Hc * Wc, Wc, check_matrix(M)), res)[0].reshape(Hc, Wc)


def class_rows(classes, auto=None):
    """Of a class map -> (shares, rows, ratio, top): {S: share of the in-view pixels with class S}, the chain rows of the adaptive
    render, their ratio to the rows of the uniform render of the whole canvas at S = top, and top itself: `auto`, or by default the
    largest class present (1 for a canvas with nothing in view)."""
    c = np.asarray(classes).reshape(-1)
    counts = {S: int((c == S).sum()) for S in SUPERSAMPLES}
    n_in = sum(counts.values())
    top = auto if auto is not None else max([S for S in SUPERSAMPLES if counts[S]], default=1)
    rows = sum(S * S * k for S, k in counts.items())
    return {S: (counts[S] / n_in if n_in else 0.0) for S in SUPERSAMPLES}, rows, rows / (c.size * top * top), top


def adaptive_note(classes, auto=None):
    """What the commands say about an adaptive render: each class's share of the in-view pixels and the chain rows against uniform."""
    shares, rows, ratio, top = class_rows(classes, auto)
    return ("adaptive samples per pixel: " + ", ".join(f"{S} x {S} on {100 * shares[S]:.1f} %" for S in SUPERSAMPLES) +
            f" of the pixels in view; {rows} chain rows, {ratio:.3f} of uniform {top} x {top}")


def density_report(M, size, what, supersample=1):
    """One line for the commands: the density range, with a warning when the view minifies by more than MINIFY_WARN per sample
    (supersample = S: S x S samples per canvas pixel, named in the line when S > 1; "adaptive": each class's share of the in-view
    pixels and the chain rows against uniform `auto`, from supersample_classes)."""
    lo, hi = sampling_density(M, size)
    line = f"{what}: {lo:.3f} .. {hi:.3f} target pixels per canvas pixel"
    if isinstance(supersample, str) and supersample == "adaptive":
        return line + "; " + adaptive_note(supersample_classes(M, size), auto=supersample_for(M, size))
    if supersample == 1:
        if hi > MINIFY_WARN:
            line += f"  WARNING: minifies by more than {MINIFY_WARN} -- point sampling aliases there (no antialiasing)"
        return line
    line += f", {supersample} x {supersample} samples per canvas pixel ({lo / supersample:.3f} .. {hi / supersample:.3f} per sample)"
    if hi / supersample > MINIFY_WARN:
        line += f"  WARNING: still minifies by more than {MINIFY_WARN} per sample -- it aliases there"
    return line


# ---- view.json: settings only ------------------------------------------------------------------------------------------------------
def write(path, photo_size, rect_size, quad_yx, rect_to_photo, photo_to_rect):
    """view.json: photo size, rectified size, the quad, and both matrices as nine numbers each."""
    doc = {"photo_size": [int(s) for s in photo_size], "rect_size": [int(s) for s in rect_size],
           "quad_yx": np.asarray(quad_yx, np.float64).reshape(4, 2).tolist(),
           "rect_to_photo": check_matrix(rect_to_photo).reshape(-1).tolist(),
           "photo_to_rect": check_matrix(photo_to_rect).reshape(-1).tolist()}
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return path


def read(path):
    """-> dict(photo_size (H, W), rect_size (H, W), quad_yx (4, 2), rect_to_photo (3, 3), photo_to_rect (3, 3)); ValueError for a
    file that is not a view.json."""
    try:
        with open(path) as f:
            doc = json.load(f)
        out = {"photo_size": _size(doc["photo_size"]), "rect_size": _size(doc["rect_size"]),
               "quad_yx": np.asarray(doc["quad_yx"], np.float64).reshape(4, 2),
               "rect_to_photo": check_matrix(doc["rect_to_photo"]), "photo_to_rect": check_matrix(doc["photo_to_rect"])}
    except (OSError, KeyError, TypeError, json.JSONDecodeError) as e:
        raise ValueError(f"{path}: not a view.json ({type(e).__name__}: {e})") from e
    except ValueError as e:
        raise ValueError(f"{path}: not a view.json ({e})") from e
    return out


# ---- the library's side ------------------------------------------------------------------------------------------------------------
def _is_cpu(device):
    return device is None or str(device) == "cpu"


def canvas_coords(M, size, res=(1, 1), start=0, n=None, device="cpu", return_inside=False):
    """The fp32 fit-frame positions (n, 2) [y, x] a view launch forms for canvas pixels [start, start + n) of the size = (H', W')
    canvas (M stored as float32; (0, 0) for a pixel not in view), by the library's host twin -- so NPPNet.render_at(canvas_coords(...))
    is render_view(...) bit for bit on the pixels in view.  return_inside: also the bytes 0 / 1 / 3 against the fit size res = (H, W).
    device: "cpu" (NumPy arrays) or a torch device (the host result, copied there)."""
    from . import ops
    Hc, Wc = _size(size)
    n = Hc * Wc - int(start) if n is None else int(n)
    yx, inside = ops.view_coords_host(ops.view_arg(start, n, Wc, check_matrix(M)), res)
    if not _is_cpu(device):
        import torch
        yx, inside = torch.from_numpy(yx).to(device), torch.from_numpy(inside).to(device)
    return (yx, inside) if return_inside else yx


def warp_image(img_u8, M, size, mode="bilinear", device=None, supersample=1, reduce="mean"):
    """The size = (Ho, Wo) canvas whose pixel (i, j) reads the (Hs, Ws[, C <= 4]) uint8 image at M(i, j) (float64; 'bilinear' or
    'nearest': include/npp_hip.h npp_warp_image_u8), and its (Ho, Wo) coverage mask, 255 where the position lies in the image.
    supersample = S in SUPERSAMPLES: every canvas pixel is reduced from S x S samples spread over its footprint, of which those in
    the image count -- reduce 'mean' (their ordered float64 mean: antialiasing) or 'min' (the darkest: a mask stays black where any
    sample is black) -- and the mask is 255 where the pixel centre lies in the image and a sample counts (npp_warp_image_u8_ss).
    The defaults are the point warp.  device None / "cpu": NumPy arrays through the library's host twin; otherwise device tensors
    in and out.  ValueError by the argument's name, before a device is touched."""
    from . import ops
    ops.check_warp(mode, supersample, reduce)
    if _is_cpu(device):
        return ops.warp_image_u8_host(np.asarray(img_u8), check_matrix(M), size, mode, supersample, reduce)
    import torch
    dev = ops.select_device(device)
    t = img_u8 if isinstance(img_u8, torch.Tensor) else torch.from_numpy(np.array(img_u8))
    t = t.to(device=dev, dtype=torch.uint8).contiguous()
    return ops.warp_image_u8(t, check_matrix(M), size, mode, supersample, reduce)


def composite(photo_u8, render, inside, mask=None, beyond=False):
    """Put a render_view canvas into the photograph it was rendered for: photo_u8 (H, W, 3) uint8, render (H, W, 3) float in [0, 1],
    inside (H, W) the render's bytes.  Pixels with inside == 3 (inside != 0 with beyond: the pattern carried past the fit's border)
    are replaced by the render's 8-bit conversion (io.imsave: clip to [0, 1], times 255, round half to even); with mask (H, W) uint8
    in the photo's frame, white = known, only where the mask is black (< 128: unknown).  Every other pixel keeps the photograph's
    bytes.  Torch on the render's device -> (H, W, 3) uint8 tensor there."""
    import torch
    render = torch.as_tensor(render)
    dev = render.device

    def on_dev(a):                                   # arrays decoded from a PNG are read-only: copy before torch sees them
        return a.to(dev) if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a)).to(dev)
    photo, inside = on_dev(photo_u8), on_dev(inside)
    if photo.dtype != torch.uint8 or photo.dim() != 3 or photo.shape[2] != 3:
        raise ValueError(f"photo_u8: expected (H, W, 3) uint8, got {tuple(photo.shape)} {photo.dtype}")
    if tuple(render.shape) != tuple(photo.shape) or tuple(inside.shape) != tuple(photo.shape[:2]):
        raise ValueError(f"render {tuple(render.shape)} / inside {tuple(inside.shape)} do not match the photograph {tuple(photo.shape)}")
    sel = (inside != 0) if beyond else (inside == 3)
    if mask is not None:
        m = on_dev(mask)
        if tuple(m.shape) != tuple(photo.shape[:2]):
            raise ValueError(f"mask {tuple(m.shape)} does not match the photograph {tuple(photo.shape[:2])}")
        sel = sel & (m < 128)
    r8 = torch.round(render.to(torch.float64).clamp(0.0, 1.0) * 255.0).to(torch.uint8)
    return torch.where(sel[..., None], r8, photo)


def imread_u8(path, gray=False):
    """A PNG as uint8: (H, W, 3) RGB, or (H, W) with gray."""
    from PIL import Image
    return np.asarray(Image.open(path).convert("L" if gray else "RGB"), dtype=np.uint8)


def exists_nonempty(path):
    return os.path.isdir(path) and len(os.listdir(path)) > 0
