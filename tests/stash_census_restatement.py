"""NumPy restatement of the stash census (include/npp_hip.h "stash audit"), written from the layout's description -- the comments
of csrc/npp_layout.h ("W8-format", "embedding slot order", the k-step offsets) and the header's definition of the counters -- not
a call into the library.  The yardstick of tests/test_stash_audit_cpu.py and of the GPU tests' "NumPy decode of the bytes".

W8-format: a unit is 8 bytes = features 16 ks + perm16(hh, 0..7) of one row; an array of NKS k-steps takes NKS KiB per 64-row tile:
[tile][ks pair][group of 8 rows][line of 256 B], line = [ks & 1][hh][row & 7][8 B].  Array base = k-step offset * tiles * 1 KiB.
actF: a 16-bit region of (total k-steps) * tiles * 2 KiB comes first, then the 8-bit arrays.  dzF: the arrays, then one int32 per tile."""
import numpy as np

FIELDS = ("elements", "zero", "subnormal", "at_max", "nonfinite")
EMB_KS, E = 30, 462


def emb_real(ks, hh, j):
    """Whether slot (k-step, lane half, element) of an embedding array is one of the 462 reference columns (-> its column, or -1)."""
    if ks < 28:
        t = 8 * ks + j
        return -1 if t >= 220 else (1 + 2 * (t // 22) + hh) * 22 + t % 22
    if ks == 28:
        return 8 * hh + j
    return 16 + j if (hh == 0 and j < 6) else -1


def table(K, W):
    """[(name, side 'act' | 'dz', k-step offset, k-steps, kind 'all' | 'emb' | 'rgb')] of the arrays a K-proposal, width-W net writes,
    and the total k-steps of the two sides."""
    A = W // 16
    multi = K > 1
    t = [(f"a{l}", "act", l * A, A, "all") for l in range(8)] + [("f1", "act", 8 * A, A, "all")]
    if multi:
        t += [("a_s", "act", 9 * A, A, "all"), ("f2", "act", 10 * A, A, "all")]
    t += [("a_p", "act", 11 * A, A // 2, "all")]
    emb0 = 11 * A + A // 2
    t += [(f"emb{p}", "act", emb0 + EMB_KS * p, EMB_KS, "emb") for p in range(K)]
    t += [(f"dz{l}", "dz", l * A, A, "all") for l in range(8)] + [("dz_f1", "dz", 8 * A, A, "all")]
    if multi:
        t += [("dz_s", "dz", 9 * A, A, "all"), ("dz_f2", "dz", 10 * A, A, "all")]
    t += [("dz_p", "dz", 11 * A, A // 2, "all"), ("dz_rgb", "dz", 11 * A + A // 2, 2, "rgb")]
    return t, emb0 + EMB_KS * K, 11 * A + A // 2 + 2


def positions(ks0, nks, kind, n_wg, n_rows):
    """Byte offsets (from the side's 8-bit base) of every counted element of one array: rows < n_rows, real features."""
    row = np.arange(n_rows, dtype=np.int64)[:, None, None, None]
    ks = np.arange(nks, dtype=np.int64)[None, :, None, None]
    hh = np.arange(2, dtype=np.int64)[None, None, :, None]
    j = np.arange(8, dtype=np.int64)[None, None, None, :]
    wg, r64 = row // 64, row % 64
    off = (ks0 * n_wg * 1024 + ((wg * (nks // 2) + ks // 2) * 8 + (r64 >> 3)) * 256 + (ks & 1) * 128 + hh * 64 + (r64 & 7) * 8 + j)
    if kind == "all":
        real = np.ones((1, nks, 2, 8), bool)
    elif kind == "emb":
        real = np.array([[[emb_real(k, h, e) >= 0 for e in range(8)] for h in range(2)] for k in range(nks)])[None]
    else:                                   # dz_rgb: dL/draw of the three colours in elements 0..2 of the first unit
        real = np.zeros((1, nks, 2, 8), bool)
        real[0, 0, 0, :3] = True
    return off[np.broadcast_to(real, off.shape)]


def count(codes, fmt):
    """The header's counters over a vector of bytes: fmt 'e4m3' (3 mantissa bits, largest finite 0x7E, NaN 0x7F) or 'e5m2'
    (2 mantissa bits, largest finite 0x7B, 0x7C.. infinity / NaN)."""
    c = codes.astype(np.int64) & 0x7F
    mbits, top, nf = (3, 0x7E, 0x7F) if fmt == "e4m3" else (2, 0x7B, 0x7C)
    finite = c < nf
    ex = c >> mbits
    hist = np.bincount(ex[finite], minlength=32)[:32]
    return {"elements": int(c.size), "zero": int((c == 0).sum()), "subnormal": int(((ex == 0) & (c != 0)).sum()),
            "at_max": int((c == top).sum()), "nonfinite": int((~finite).sum()), "exp_hist": [int(v) for v in hist]}


def census(act, dz, Bp, n_rows, K, W):
    """-> ({name: counters + 'format'}, {'tiles', 'scale_min', 'scale_max'}, boolean masks of the counted bytes of act / dz)."""
    n_wg = Bp // 64
    tab, act_ks, dz_ks = table(K, W)
    act8 = act_ks * n_wg * 2048
    out, used = {}, {"act": np.zeros(act.size, bool), "dz": np.zeros(dz.size, bool)}
    for name, side, ks0, nks, kind in tab:
        pos = positions(ks0, nks, kind, n_wg, n_rows) + (act8 if side == "act" else 0)
        buf = act if side == "act" else dz
        fmt = "e4m3" if side == "act" else "e5m2"
        assert not used[side][pos].any()
        used[side][pos] = True
        out[name] = dict(count(buf[pos], fmt), format=fmt)
    tiles = (n_rows + 63) // 64
    sbase = dz_ks * n_wg * 1024
    sc = dz[sbase:sbase + 4 * n_wg].view(np.int32)[:tiles] & 255
    used["dz"][sbase:sbase + 4 * tiles] = True
    return out, {"tiles": int(tiles), "scale_min": int(sc.min()), "scale_max": int(sc.max())}, used["act"], used["dz"]
