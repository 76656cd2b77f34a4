"""NumPy restatement of the trunk census (include/npp_hip.h "trunk audit"), written from the description of the
"flat padded" layout in csrc/npp_conv.hip's header -- not from the kernel or its host twin:

  an activation (N, C, H, W) is stored as [C/8 chunks][NPOSP positions][8 channels] fp16; the position axis enumerates all images
  with a one-pixel border each, pos = GUARD + n (H+2)(W+2) + y (W+2) + x (interior y in 1..H, x in 1..W), GUARD = 1024 units on
  both ends and the image positions rounded up to a multiple of 512; element j of chunk c8 is the true channel
  32 (c8 >> 2) + 16 ((c8 >> 1) & 1) + 8 (j >> 2) + 4 (c8 & 1) + (j & 3).

The census counts the interior positions of images < n and the channels < c_real, and nothing else."""
import numpy as np

GUARD, ROUND = 1024, 512
FIELDS = ("elements", "zero", "subnormal", "at_max", "nonfinite")
CASES = [(3, 2, 16, 3, 5, 7), (2, 2, 64, 64, 8, 8), (1, 1, 128, 128, 1, 3)]       # (N_total, n, C, c_real, H, W)
# codes every planted tensor carries: +-0, the smallest / largest subnormal of both signs, +-65504, +-infinity, NaNs of both signs,
# +-1, the smallest normal, a negative subnormal-adjacent normal
SPECIAL = [0x0000, 0x8000, 0x0001, 0x83FF, 0x03FF, 0x8001, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x7E00, 0xFE01, 0x7C01, 0x3C00, 0xBC00,
           0x0400, 0x8400, 0x7BFE, 0xFBFE]


def nposp(N, H, W):
    s = N * (H + 2) * (W + 2)
    return (s + ROUND - 1) // ROUND * ROUND + 2 * GUARD


def chan(c8, j):
    return 32 * (c8 >> 2) + 16 * ((c8 >> 1) & 1) + 8 * (j >> 2) + 4 * (c8 & 1) + (j & 3)


def index(N_total, n, C, c_real, H, W):
    """(chunk, position, element) index arrays of shape (n, c_real, H, W): where the layout keeps logical element (img, ch, y, x)."""
    where = {chan(c8, j): (c8, j) for c8 in range(C // 8) for j in range(8)}
    assert sorted(where) == list(range(C))
    img, ch, y, x = np.meshgrid(np.arange(n), np.arange(c_real), np.arange(H), np.arange(W), indexing="ij")
    c8 = np.array([where[c][0] for c in range(c_real)])[ch]
    j = np.array([where[c][1] for c in range(c_real)])[ch]
    pos = GUARD + img * (H + 2) * (W + 2) + (y + 1) * (W + 2) + (x + 1)
    return c8, pos, j


def census(flat, N_total, n, C, c_real, H, W, ref32=None):
    """flat: uint16 codes (C/8, nposp, 8) -> the decoded census, counted on the gathered (n, c_real, H, W) codes."""
    flat = np.asarray(flat, np.uint16).reshape(C // 8, nposp(N_total, H, W), 8)
    codes = flat[index(N_total, n, C, c_real, H, W)]
    a = (codes & 0x7FFF).astype(np.int64)
    e = a >> 10
    fin = e != 31
    out = {"format": "fp16", "elements": int(codes.size), "zero": int((a == 0).sum()), "subnormal": int(((e == 0) & (a != 0)).sum()),
           "at_max": int((a == 0x7BFF).sum()), "nonfinite": int((~fin).sum()),
           "exp_hist": [int(((e == b) & fin).sum()) for b in range(32)], "gate_on": 0, "gate_flips": 0}
    if ref32 is not None:
        with np.errstate(invalid="ignore"):
            on16 = codes.view(np.float16) > 0                          # (NaN > 0 is False, +infinity > 0 is True)
        on32 = np.asarray(ref32, np.float32)[:n] > 0
        out["gate_on"], out["gate_flips"] = int(on16.sum()), int((on16 != on32).sum())
    return out


def planted(case, seed):
    """One planted tensor of a case -> (flat uint16 codes, ref32 (N_total, c_real, H, W) fp32, counted: bool mask of flat).
    Counted elements: uniformly random codes (every class of a large tensor) with SPECIAL planted over the leading ones; the
    partner agrees in sign with the fp16 value except where a disagreement is planted -- every third element, and fp16 +0 against a
    positive fp32 value.  EVERY uncounted code -- guards, borders, the tail, padded channels, images >= n -- is 0x7BFF or a NaN."""
    N_total, n, C, c_real, H, W = case
    rng = np.random.RandomState(seed)
    flat = np.where(rng.rand(C // 8, nposp(N_total, H, W), 8) < 0.5, 0x7BFF, 0x7E00).astype(np.uint16)
    codes = rng.randint(0, 65536, (n, c_real, H, W)).astype(np.uint16)
    k = min(len(SPECIAL), codes.size)
    codes.reshape(-1)[:k] = SPECIAL[:k]
    idx = index(N_total, n, C, c_real, H, W)
    flat[idx] = codes
    counted = np.zeros(flat.shape, bool)
    counted[idx] = True
    with np.errstate(invalid="ignore"):
        on16 = codes.view(np.float16) > 0
    mag = rng.rand(n, c_real, H, W).astype(np.float32) + 0.5
    ref = np.where(on16, mag, -mag).astype(np.float32)
    flip = (np.arange(codes.size).reshape(codes.shape) % 3) == 0
    ref[flip] = -ref[flip]
    ref[codes == 0x0000] = 0.25                                        # fp16 +0 (gate closed) against a positive fp32 value: a flip
    ref_all = rng.randn(N_total, c_real, H, W).astype(np.float32)       # images >= n of the partner: never read
    ref_all[:n] = ref
    return flat, ref_all, counted
