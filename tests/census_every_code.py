"""The inputs of the census-core tests (csrc/npp_census.h), CPU and GPU: buffers whose COUNTED elements hold every code of their
format -- e4m3 and e5m2 in a stash workspace, fp16 in a flat trunk tensor -- at the smallest shapes that still take every path of the
kernels.  Built from the NumPy restatements of the two layouts, not from the library."""
import numpy as np

import stash_census_restatement as RS
import trunk_census_restatement as RT

# stash: K = 1, width 256, 65 real rows in two 64-row tiles -- the first tile's 16-byte pieces are counted whole, the second tile
# has one real row: each of its pieces is counted byte by byte (one of its two rows), and so are the embedding's and dz_rgb's
STASH = dict(K=1, W=256, Bp=128, n_rows=65)
# trunk: 2 x 16 x 32 x 64 = 65 536 counted elements, every fp16 code once (16 true channels: two chunks, no padded channel)
TRUNK = (2, 2, 16, 16, 32, 64)                  # (N_total, n, C, c_real, H, W)


def stash_buffers(sizes):
    """sizes: ops.train_workspace(K, Bp, 1, W).  -> (act, dz) uint8: the counted bytes of every array run through all 256 byte
    values (stride 37, coprime to 256: neighbours differ in every field), everything else is poison (0x7F: e4m3 NaN, 0x7B: e5m2's
    largest finite code)."""
    K, W, Bp, n_rows = (STASH[k] for k in ("K", "W", "Bp", "n_rows"))
    act, dz = np.full(sizes[1], 0x7F, np.uint8), np.full(sizes[2], 0x7B, np.uint8)
    n_wg = Bp // 64
    tab, act_ks, dz_ks = RS.table(K, W)
    for i, (name, side, ks0, nks, kind) in enumerate(tab):
        pos = RS.positions(ks0, nks, kind, n_wg, n_rows)
        buf, base = (act, act_ks * n_wg * 2048) if side == "act" else (dz, 0)
        buf[pos + base] = (np.arange(pos.size) * 37 + 11 * i) % 256
        assert name == "dz_rgb" or len(np.unique(buf[pos + base])) == 256
    sc = dz[dz_ks * n_wg * 1024:][:4 * n_wg].view(np.int32)
    sc[:] = [0x7B7B7B00 | 120, 0x7B7B7B00 | 131]                       # the E8M0 bytes of the two tiles' scales
    return act, dz


def trunk_tensor(seed=3):
    """-> (flat uint16 codes, ref32 (N_total, c_real, H, W) fp32): every fp16 code exactly once over the counted elements in a seeded
    order, every uncounted code 0x7BFF or a NaN; the partner agrees in sign with the fp16 value except on every third element."""
    N_total, n, C, c_real, H, W = TRUNK
    rng = np.random.RandomState(seed)
    flat = np.where(rng.rand(C // 8, RT.nposp(N_total, H, W), 8) < 0.5, 0x7BFF, 0x7E00).astype(np.uint16)
    codes = rng.permutation(65536).astype(np.uint16).reshape(n, c_real, H, W)
    flat[RT.index(*TRUNK)] = codes
    with np.errstate(invalid="ignore"):
        on16 = codes.view(np.float16) > 0
    mag = rng.rand(n, c_real, H, W).astype(np.float32) + 0.5
    ref = np.where(on16, mag, -mag).astype(np.float32)
    flip = (np.arange(codes.size).reshape(codes.shape) % 3) == 0
    ref[flip] = -ref[flip]
    return flat, ref
