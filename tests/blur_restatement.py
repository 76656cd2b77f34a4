"""Host restatements shared by test_gpu_blur.py and test_blur_cpu.py: the 20 x 20 windows of the padded image through the
reference's own index map (blur_detection.py:15-30, as io.get_blur_map builds them), the share formula of :38-41 on LAPACK's
singular values in a chosen precision, the test images (the g13b scene's recipe, the window kinds that can go wrong), and a NumPy
restatement of the kernel's own Jacobi loop (same pair ordering, same tolerance), which is what the sweep cap of
csrc/npp_blur.hip rests on."""
import numpy as np

WS = 10


def windows(gray, ws=WS):
    """(H,W) -> (H,W,2ws,2ws) view: the block new_img[i:i+2ws, j:j+2ws] of every pixel."""
    gray = np.asarray(gray, np.float64)
    H, W = gray.shape

    def mirror(n):
        idx = np.arange(n + 2 * ws)
        return np.where(idx < ws, ws - idx, np.where(idx > n + ws - 1, 2 * n - idx, idx - ws))       # (negative: NumPy wraps)
    new_img = gray[mirror(H)[:, None], mirror(W)[None, :]]
    return np.lib.stride_tricks.sliding_window_view(new_img, (2 * ws, 2 * ws))[:H, :W]


def singular_values(gray, dtype):
    """LAPACK singular values of every window, computed in `dtype` -> (H,W,20) of that dtype."""
    win = windows(gray)
    return np.stack([np.linalg.svd(win[i].astype(dtype), compute_uv=False) for i in range(win.shape[0])])


def share(sv, sv_num):
    """blur_detection.py:39-41 in the precision of `sv`."""
    return sv[..., :sv_num].sum(-1) / (sv.sum(-1) + sv.dtype.type(1e-6))


def normalise(raw):
    raw = np.asarray(raw, np.float64)
    return (raw - raw.min()) / (raw.max() - raw.min())


def make_image(H=150, W=230):
    """The g13b scene (tests/golden/make_golden_blur_mask.py writes its golden; tools/blur_time.py scales it up): a sharp left
    half, a Gaussian-blurred right half and a flat patch."""
    import scipy.ndimage as ndimage
    rs = np.random.RandomState(0)
    y, x = np.mgrid[0:H, 0:W]
    base = 0.5 + 0.25 * np.sin(2 * np.pi * x / 9.0) + 0.2 * np.sin(2 * np.pi * (y + 0.3 * x) / 7.0)
    img = np.stack([base, base * 0.9 + 0.05, 1 - base], -1) + rs.normal(0, 0.03, (H, W, 3))
    bl = ndimage.gaussian_filter(img, (3, 3, 0))
    img[:, W // 2:] = bl[:, W // 2:]     # right half blurred
    img[H * 2 // 15:H * 2 // 5, W * 3 // 23:W * 7 // 23] = 0.6     # a flat patch ([20:60, 30:70] at 150 x 230): rank-1 windows
    return (np.clip(img, 0, 1) * 255).astype(np.uint8)


CONTENTS = ["zero", "constant", "checkerboard", "rank3", "saturated", "ramp"]


def content(kind, shape, seed=0):
    """(H,W) uint8 gray images whose windows are the hard ones: all zero, rank 1, rank 2, exactly rank 3, saturated noise, a ramp."""
    H, W = shape
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W]
    if kind == "zero":
        a = np.zeros(shape)
    elif kind == "constant":
        a = np.full(shape, 137)
    elif kind == "checkerboard":
        a = 30 + 190 * ((y + x) % 2)
    elif kind == "rank3":
        a = rs.randint(0, 6, (H, 3)) @ rs.randint(0, 6, (3, W)) * 3
    elif kind == "saturated":
        a = np.rint(np.clip(rs.normal(128, 200, shape), 0, 255))
    elif kind == "ramp":
        a = np.floor(255.0 * (1.3 * y + 0.9 * x) / (1.3 * (H - 1) + 0.9 * (W - 1)))
    elif kind == "uniform":
        a = rs.randint(0, 256, shape)
    else:
        raise KeyError(kind)
    assert a.min() >= 0 and a.max() <= 255
    return a.astype(np.uint8)


def jacobi_singular_values(blocks, tol=1e-9, max_sweeps=16):
    """The loop of blur_sv_share_kernel on (N,20,20) blocks in float64: one-sided Jacobi, round-robin ordering (in step s column 19
    meets column s, column c meets (2s - c) mod 19), a pair rotated while |a_p . a_q| > tol |a_p| |a_q|, a block done after a sweep
    without a rotation.  -> (singular values (N,20), unsorted; sweeps used per block, the confirming one included; blocks still
    rotating in the last sweep)."""
    A = np.array(blocks, np.float64)
    N, n = A.shape[0], A.shape[2]
    used, active = np.zeros(N, int), np.ones(N, bool)
    rotated = np.zeros(N, bool)
    c = np.arange(n)
    for sweep in range(max_sweeps):
        rotated = np.zeros(N, bool)
        for s in range(n - 1):
            partner = np.where(c == n - 1, s, np.where(c == s, n - 1, (2 * s - c) % (n - 1)))
            lo = c[c < partner]
            hi = partner[lo]
            ap, aq = A[:, :, lo], A[:, :, hi]
            al, be, ga = (ap * ap).sum(1), (aq * aq).sum(1), (ap * aq).sum(1)
            rot = (ga * ga > tol * tol * (al * be)) & (np.abs(ga) > 1e-18)
            zeta = (be - al) / (2 * np.where(rot, ga, 1.0))
            t = np.where(zeta >= 0, 1.0, -1.0) / (np.abs(zeta) + np.sqrt(1 + zeta * zeta))
            cs = np.where(rot, 1 / np.sqrt(1 + t * t), 1.0)
            sn = np.where(rot, cs * t, 0.0)
            A[:, :, lo] = cs[:, None, :] * ap - sn[:, None, :] * aq
            A[:, :, hi] = sn[:, None, :] * ap + cs[:, None, :] * aq
            rotated |= rot.any(1)
        used[active] = sweep + 1
        active &= rotated
        if not rotated.any():
            break
    return np.sqrt((A * A).sum(1)), used, rotated
