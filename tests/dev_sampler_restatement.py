"""NumPy restatement of the rng_mode="device" draws, written from their definition (include/npp_hip.h "rng_mode=device",
DESIGN 6e), not from the kernels: Philox4x32-10, the patch source, the cycle-walking Feistel permutation, the lattice half of
GridPatchSampler.draw() and the pixel rows.  The CPU tests compare the library's host twins with it, the GPU tests the launches."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
U32 = np.uint64(0xFFFFFFFF)
SOURCES = ("val", "train", "same")


def philox4x32_10(ctr, key):
    """ctr: 4 arrays (or ints) of 32-bit words, key: 2 ints -> 4 uint64 arrays holding 32-bit words."""
    c = [np.asarray(v, np.uint64) & U32 for v in np.broadcast_arrays(*[np.asarray(v, np.uint64) for v in ctr])]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & U32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & U32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def key_of(seed):
    return int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF


def uniform(seed, t):
    """The source draw: word 0 of counter (0, 0, t, 0) times 2^-32, as a double."""
    return float(philox4x32_10((0, 0, t, 0), key_of(seed))[0]) * 2.0 ** -32


def source_of(u):
    if u < 0.5:
        return "val"
    if 0.5 < u < 0.8:
        return "train"
    return "same"


def perm(N, n, t, stream, seed):
    """Positions 0..n-1 of the keyed permutation of [0, N) -> int64 (n,); t an array of T draw indices -> (T, n)."""
    N, n = int(N), int(n)
    if n > N:
        raise ValueError("Cannot take a larger sample than population when 'replace=False'")
    bits = max(int(N - 1).bit_length(), 2)
    bits += bits & 1
    b = np.uint64(bits // 2)
    mask = np.uint64((1 << (bits // 2)) - 1)
    key = key_of(seed)
    tt = np.asarray(t, np.uint64)
    shape = tt.shape + (n,)
    x = np.broadcast_to(np.arange(n, dtype=np.uint64), shape).reshape(-1).copy()
    tt = np.broadcast_to(tt[..., None], shape).reshape(-1)
    todo = np.ones(x.shape[0], bool)
    while todo.any():
        v, tv = x[todo], tt[todo]
        L, R = v >> b, v & mask
        for r in range(8):
            F = philox4x32_10((R, r, tv, stream), key)[0] & mask
            L, R = R, L ^ F
        v = (L << b) | R
        x[todo] = v
        todo[todo] = v >= np.uint64(N)
    return x.astype(np.int64).reshape(shape)


def summed_area(mask_hw):
    known = (np.asarray(mask_hw) >= 0.5).astype(np.int64)
    sat = np.zeros((known.shape[0] + 1, known.shape[1] + 1), np.int64)
    sat[1:, 1:] = known.cumsum(0).cumsum(1)
    return sat


def filtered(pool, H, W, P):
    pool = np.asarray(pool, np.int64)
    h = P // 2
    ok = (pool[:, 0] > h) & (pool[:, 0] < H - (h + 1)) & (pool[:, 1] > h) & (pool[:, 1] < W - (h + 1))
    return pool[ok]


def draw(sat, pool_val, pool_train, shifts_dydx, H, W, P, n_p, topk, invalid_ratio, seed, t):
    """One decision: dict(source, k, cen (n_p, 2) int64, real (n_p k, 2) int32 | None, weights float32 | None).  pool_*: the
    bounds-filtered pools; shifts_dydx: ((dy, dx), (dy, dx))."""
    src = source_of(uniform(seed, t))
    pool = pool_val if src == "val" else pool_train
    cen = pool[perm(pool.shape[0], n_p, t, 1, seed)]
    out = dict(source=src, cen=cen, t=t)
    if src == "same":
        out.update(k=1, real=None, weights=np.ones(n_p, np.float32))
        return out
    s0, s1 = (np.asarray(s, np.float64) for s in shifts_dydx)
    idx = np.arange(400)
    a, b = (idx // 20 - 10).astype(np.float64), (idx % 20 - 10).astype(np.float64)
    dist0 = np.abs(a) + np.abs(b)
    dist0[dist0 == 0] = 10000.0
    per_patch, kmin = [], topk
    for p in range(n_p):
        y = (np.float64(cen[p, 0]) + a * s0[0]) + b * s1[0]
        x = (np.float64(cen[p, 1]) + a * s0[1]) + b * s1[1]
        ok = (y > 0) & (y < H - 1) & (x > 0) & (x < W - 1)
        ry, rx = np.rint(y).astype(np.int64), np.rint(x).astype(np.int64)
        y0, y1 = np.clip(ry - P // 2, 0, H), np.clip(ry + P // 2, 0, H)
        x0, x1 = np.clip(rx - P // 2, 0, W), np.clip(rx + P // 2, 0, W)
        unknown = P * P - (sat[y1, x1] - sat[y0, x1] - sat[y1, x0] + sat[y0, x0])
        ok &= ~(unknown.astype(np.float64) > np.float64(P * P) * np.float64(invalid_ratio))
        kmin = min(kmin, int(ok.sum()) - 1)
        if kmin <= 0:
            out.update(k=0, real=None, weights=None)
            return out
        order = sorted(np.nonzero(ok)[0], key=lambda i: (dist0[i], i))[:kmin]          # stable: distance, then candidate index
        inv = [1.0 / dist0[i] for i in order]
        total = 0.0
        for v in inv:                                                                   # summed in candidate order
            total += v
        per_patch.append((np.stack([ry[order], rx[order]], 1).astype(np.int32),
                          np.array([v / total for v in inv], np.float64).astype(np.float32)))
    out.update(k=kmin, real=np.concatenate([c[:kmin] for c, _ in per_patch], 0),
               weights=np.concatenate([w[:kmin] for _, w in per_patch]))
    return out


def centres_i32(d):
    """(n_p (1 + k), 2) int32: fake, then real -- the order of GridPatchSampler.centres_i32."""
    c = d["cen"].astype(np.int32)
    return c if d["real"] is None else np.concatenate([c, d["real"]], 0)


def pixels(n_train, n_pix, seed, t):
    return perm(n_train, n_pix, t, 2, seed)


# ---- the shared test inputs ---------------------------------------------------------------------------------------------
SHIFTS_DXDY = ((16.0, 2.5), (-2.0, 13.5))          # (dx, dy) as selected_shifts[0] holds them; the sampler flips to (dy, dx)
PIXEL_CASES = ((1, 1), (64, 64), (4097, 64), (245000, 8192))


def case_image(H=72, W=104, holes=((20, 44, 30, 52), (44, 60, 30, 40)), rs_seed=5, P=16):
    """Mask: ones, zeros at the holes, then RandomState(rs_seed).uniform < 0.05 set to 0; the image from the same RandomState
    after that.  -> dict(img, mask, known, unknown (the pools, np.nonzero order), sat, pool_train, pool_val (filtered), ...)."""
    mask = np.ones((H, W), np.float32)
    for y0, y1, x0, x1 in holes:
        mask[y0:y1, x0:x1] = 0
    rs = np.random.RandomState(rs_seed)
    mask[rs.uniform(size=(H, W)) < 0.05] = 0
    img = rs.uniform(size=(H, W, 3)).astype(np.float32)
    known, unknown = np.stack(np.nonzero(mask), 1), np.stack(np.nonzero(1 - mask), 1)
    return dict(img=img, mask=mask, H=H, W=W, P=P, known=known, unknown=unknown, sat=summed_area(mask),
                pool_train=filtered(known, H, W, P), pool_val=filtered(unknown, H, W, P),
                shifts_dydx=tuple((dy, dx) for dx, dy in SHIFTS_DXDY))


def case_draws(c, n_p, topk, invalid_ratio, seed, ts):
    return [draw(c["sat"], c["pool_val"], c["pool_train"], c["shifts_dydx"], c["H"], c["W"], c["P"], n_p, topk, invalid_ratio, seed, t)
            for t in ts]
