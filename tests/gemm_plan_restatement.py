"""Plain-Python restatement of the launcher of the fp32 dense-layer GEMM (csrc/npp_linear.hip, gemm_prepare) and the case table of
the exact sweep (tests/test_gemm_plan_cpu.py checks the table, tests/test_gpu_dense_gemm.py runs it).  No torch, no HIP.

gemm_plan() says which path a call takes: how many k ranges the contraction is split into and how they meet, and whether each
operand's runs of 4 are fetched as one 16-byte load or as four clamped 4-byte loads.  One plan_* function per extern "C" entry point
maps the layer arguments to gemm_plan()'s inputs the way the wrapper fills GemmArgs.  The fills (512 workgroups for one problem, 640
for a batched launch) are the library's defaults; NPP_GEMM_BATCH_FILL changes the second one, so users of the plan skip when it is set.

The case table describes every case of the sweep by layer shape and buffer layout only (Lay: where a matrix sits inside a flat,
sentinel-filled buffer whose start is 16-byte aligned), and lists next to it the path the case is there for (`path`), written down from
the launcher's rules by hand -- the tests assert that the restated plan of the case agrees with it before anything is launched."""
import os
from collections import namedtuple

FILL_SINGLE, FILL_BATCHED = 512, 640
GUARD = 8                                   # sentinel floats in front of and behind every matrix (a multiple of 4: alignment is `off`'s)


def fill_overridden():
    return "NPP_GEMM_BATCH_FILL" in os.environ


# one GEMM operand as the vector-load test sees it: element stride along its contiguous index, along the other index, between the
# batches, the extent along the contiguous index, and the address of its first element modulo 16
Operand = namedtuple("Operand", "cont other batch extent addr16")
Plan = namedtuple("Plan", "form M N K nb splits kchunk vec_a vec_b grid mode scalar_a scalar_b")


def scalar_causes(op, nb):
    """Why an operand is NOT fetched with 16-byte loads (empty: it is)."""
    why = []
    if op.cont != 1:
        why.append("strided")
    if op.other % 4:
        why.append("ld")
    if op.extent % 4:
        why.append("extent")
    if op.addr16 % 16:
        why.append("pointer")
    if nb > 1 and op.batch % 4:
        why.append("batch")
    return tuple(why)


def gemm_plan(M, N, K, nb, a_kc, b_kc, A, B, ldc, scb=0, act=0, Z=False, dact=False, accumulate=False, batch_split=False,
              two_pass=False):
    """gemm_prepare: nb is GemmArgs.nbatch (0 or 1: one problem).  Returns a Plan; mode is 'none', 'atomic' (float atomicAdd into a
    cleared or accumulated C) or 'two_pass' (partial tiles in a slab, added in range order by a second launch)."""
    nb = nb if nb > 1 else 1
    gx, gy = (N + 63) // 64, (M + 63) // 64
    tiles = gx * gy * nb
    dense_out = scb == M * N
    splits = 1
    if (act == 0 and not Z and not dact and ldc == N and tiles < 128 * nb and K >= 256
            and (nb == 1 or (batch_split and (accumulate or dense_out)))):
        fill = FILL_BATCHED if nb > 1 else FILL_SINGLE
        splits = min(32, (K + 63) // 64, max(1, (fill + tiles - 1) // tiles))
    kchunk = ((K + splits - 1) // splits + 31) // 32 * 32
    splits = (K + kchunk - 1) // kchunk
    ca, cb = scalar_causes(A, nb), scalar_causes(B, nb)
    mode = "none" if splits == 1 else ("two_pass" if two_pass else "atomic")
    return Plan(("KC" if a_kc else "MC") + "/" + ("KC" if b_kc else "NC"), M, N, K, nb, splits, kchunk, not ca, not cb,
                (gx, gy, splits * nb), mode, ca, cb)


def det_scratch_bytes(plan):
    """npp_gram_fwd_det_scratch_bytes: tickets, partial tiles, bias partials of the ordered split, + 64."""
    gx, gy, _ = plan.grid
    tiles = gx * gy
    return 4 * (plan.nb * tiles + plan.nb * tiles * plan.splits * 4096 + plan.nb * gy * plan.splits * 64) + 64


def splits_from_det_scratch_bytes(nbytes, N, C):
    g = (C + 63) // 64
    per_split = N * g * g * 4096 + N * g * 64
    rest = (nbytes - 64) // 4 - N * g * g
    assert (nbytes - 64) % 4 == 0 and rest % per_split == 0, (nbytes, N, C)
    return rest // per_split


# ---- the extern "C" wrappers ---------------------------------------------------------------------------------------------------
def plan_linear_fwd(B, cin, cout, act, ldx, ldy, has_z, x16, w16, nb=0, sxb=0, swb=0, syb=0):
    return gemm_plan(B, cout, cin, nb, True, True, Operand(1, ldx, sxb, cin, x16), Operand(1, cin, swb, cin, w16), ldy, syb, act=act,
                     Z=has_z)


def plan_linear_bwd_data(B, cin, cout, in_used, lddz, lddx, accumulate, dz16, w16, nb=0, sdzb=0, swb=0, sdxb=0, dact=False):
    return gemm_plan(B, in_used, cout, nb, True, False, Operand(1, lddz, sdzb, cout, dz16), Operand(1, cin, swb, in_used, w16), lddx, sdxb,
                     dact=dact, accumulate=accumulate)


def plan_linear_bwd_weight(B, cin, cout, lddz, ldx, accumulate, dz16, x16, nb=0, sdzb=0, sxb=0, sdwb=0):
    """nb >= 1: npp_linear_bwd_weight_batched (accumulates, may split per batch)."""
    batched = nb >= 1
    return gemm_plan(cout, cin, B, nb, False, False, Operand(1, lddz, sdzb, cout, dz16), Operand(1, ldx, sxb, cin, x16), cin, sdwb,
                     accumulate=True if batched else accumulate, batch_split=batched)


def plan_linear_bwd_weight_strided(B, cin, cout, dz_sr, dz_so, sdzb, x_sr, x_si, sxb, nb, lddw, sdwb, dz16, x16):
    a_kc, b_kc = dz_sr == 1, x_sr == 1
    A = Operand(dz_sr, dz_so, sdzb, B, dz16) if a_kc else Operand(dz_so, dz_sr, sdzb, cout, dz16)
    Bo = Operand(x_sr, x_si, sxb, B, x16) if b_kc else Operand(x_si, x_sr, sxb, cin, x16)
    return gemm_plan(cout, cin, B, nb, a_kc, b_kc, A, Bo, lddw, sdwb, accumulate=True, batch_split=True)


def plan_gram_fwd(N, C, hw, f16=0, det=False):
    f = Operand(1, hw, C * hw, hw, f16)
    return gemm_plan(C, C, hw, N, True, True, f, f, C, C * C, batch_split=True, two_pass=det)


def plan_gram_bwd(N, C, hw, dg16=0, f16=0):
    """Two launches: dG F, then (accumulating) dG^T F -- one problem per launch when N == 1."""
    F = Operand(1, hw, C * hw, hw, f16)
    first = gemm_plan(C, hw, C, N, True, False, Operand(1, C, C * C, C, dg16), F, hw, C * hw)
    second = gemm_plan(C, hw, C, N, False, False, Operand(1, C, C * C, C, dg16), F, hw, C * hw, accumulate=True)
    return first, second


# ---- where a matrix sits -------------------------------------------------------------------------------------------------------
class Lay:
    """A (rows, cols) matrix, or nb of them, inside a flat buffer: element (b, r, c) at GUARD + off + b * sb + r * ld + c.  The buffer
    starts 16-byte aligned, so the first element's address modulo 16 is 4 * off modulo 16."""

    def __init__(self, rows, cols, ld=None, off=0, nb=None, sb=None):
        self.rows, self.cols, self.ld, self.off, self.nb = rows, cols, cols if ld is None else ld, off, nb
        self.sb = (rows * self.ld if sb is None else sb) if nb is not None else 0
        assert self.ld >= cols

    @property
    def start(self):
        return GUARD + self.off

    @property
    def addr16(self):
        return (4 * self.off) % 16

    @property
    def shape(self):
        return (self.rows, self.cols) if self.nb is None else (self.nb, self.rows, self.cols)

    @property
    def strides(self):
        return (self.ld, 1) if self.nb is None else (self.sb, self.ld, 1)

    @property
    def size(self):
        last = ((self.nb or 1) - 1) * self.sb + (self.rows - 1) * self.ld + self.cols
        return GUARD + self.off + max(last, self.rows * self.ld) + GUARD


def block(rows, cols, blk, nb=None):
    """dense and aligned, or a column block at float offset 1 of a buffer 4 wider (the leading dimension keeps cols' residue mod 4)."""
    return Lay(rows, cols, cols + 4, 1, nb) if blk else Lay(rows, cols, nb=nb)


def _m4(n):
    return n % 4 == 0


# ---- the case table ------------------------------------------------------------------------------------------------------------
FWD_SHAPES = [(1, 1, 1), (3, 5, 2), (63, 31, 63), (64, 32, 64), (65, 33, 65), (130, 100, 70)]
FWD_SPLIT = {(33, 300, 128): 5, (33, 256, 128): 4, (33, 255, 128): 1, (5, 2052, 64): 22}      # k ranges (255 < 256: the limit's other side)
WGRAD_SHAPES = {(1, 1, 1): 1, (31, 5, 3): 1, (257, 20, 64): 5, (300, 65, 63): 5, (2048, 64, 64): 32, (2100, 33, 1): 22}
BWD_SPLIT = {(70, 64, 512): 8, (10, 128, 2050): 22}
STRIDED_SHAPES = {(32, 5, 3): 1, (288, 106, 32): 5, (2048, 64, 64): 32,
                  (31, 5, 3): 1}       # (added for the coverage check: feature-major operands whose rows are no whole runs of 4)
GRAM_SHAPES = [(1, 1, 1), (2, 3, 5), (1, 64, 256), (2, 64, 300), (3, 65, 257), (1, 128, 2050)]
GRAM_BWD_SHAPES = {(1, 256, 36): 4, (1, 512, 9): 8, (2, 256, 36): 1, (3, 65, 70): 1}
BATCH_SHAPES = [(3, 5, 2), (64, 32, 64), (65, 33, 65), (130, 100, 70)]
BATCH_WGRAD_SHAPES = [(31, 5, 3), (64, 32, 64), (257, 20, 64), (300, 65, 63), (2048, 64, 64)]


def fwd_cases():
    out = []
    for (B, cin, cout) in FWD_SHAPES:
        for act in (0, 1, 2):
            for z in (False, True):
                for bias in (False, True):
                    for xblk in (False, True):
                        for yblk in (False, True):
                            out.append(dict(fam="fwd", B=B, cin=cin, cout=cout, act=act, z=z, bias=bias, xblk=xblk, yblk=yblk,
                                            path=dict(splits=1, vec_a=not xblk and _m4(cin), vec_b=_m4(cin))))
    for (B, cin, cout), s in FWD_SPLIT.items():
        for xblk in (False, True):
            for ywide in (False, True):                       # the same values through a wider y: one range
                out.append(dict(fam="fwd", B=B, cin=cin, cout=cout, act=0, z=False, bias=True, xblk=xblk, yblk=False, ywide=ywide,
                                path=dict(splits=1 if ywide else s, vec_a=not xblk and _m4(cin), vec_b=_m4(cin))))
    return out


def fwd_lays(c):
    y = Lay(c["B"], c["cout"], c["cout"] + 3, 0) if c.get("ywide") else block(c["B"], c["cout"], c["yblk"])
    return dict(x=block(c["B"], c["cin"], c["xblk"]), w=Lay(c["cout"], c["cin"]), y=y, z=block(c["B"], c["cout"], not c["yblk"]))


def fwd_plan(c):
    L = fwd_lays(c)
    return plan_linear_fwd(c["B"], c["cin"], c["cout"], c["act"], L["x"].ld, L["y"].ld, c["z"], L["x"].addr16, L["w"].addr16)


def bwd_data_cases():
    out = []
    for (B, cin, cout) in FWD_SHAPES:
        for used in sorted({u for u in (cin, cin - 3, 4 * (cin // 8)) if u >= 1}):
            for wcol in (0, 1, 4):
                for acc in (False, True):
                    out.append(dict(fam="bwd_data", B=B, cin=cin, cout=cout, used=used, wcol=wcol, acc=acc,
                                    path=dict(splits=1, vec_a=_m4(cout), vec_b=wcol != 1 and _m4(cin) and _m4(used))))
    for (B, cin, cout), s in BWD_SPLIT.items():
        for wcol in (0, 1):
            for acc in (False, True):
                out.append(dict(fam="bwd_data", B=B, cin=cin, cout=cout, used=cin, wcol=wcol, acc=acc, dense_dx=True,
                                path=dict(splits=s, vec_a=_m4(cout), vec_b=wcol == 0)))
    return out


def bwd_data_lays(c):
    """w: `cin` columns from column wcol of a matrix 8 wider (the entry point's `in` is that matrix's width)."""
    dxblk = not c.get("dense_dx") and c["wcol"] != 0
    return dict(dz=Lay(c["B"], c["cout"]), w=Lay(c["cout"], c["cin"], c["cin"] + 8, c["wcol"]), dx=block(c["B"], c["used"], dxblk))


def bwd_data_plan(c):
    L = bwd_data_lays(c)
    return plan_linear_bwd_data(c["B"], L["w"].ld, c["cout"], c["used"], L["dz"].ld, L["dx"].ld, c["acc"], L["dz"].addr16, L["w"].addr16)


def bwd_weight_cases():
    out = []
    for (B, cin, cout), s in WGRAD_SHAPES.items():
        for db in (False, True):
            for acc in (False, True):
                for dzblk in (False, True):
                    for xblk in (False, True):
                        out.append(dict(fam="bwd_weight", B=B, cin=cin, cout=cout, db=db, acc=acc, dzblk=dzblk, xblk=xblk,
                                        path=dict(splits=s, vec_a=not dzblk and _m4(cout), vec_b=not xblk and _m4(cin))))
    return out


def bwd_weight_lays(c):
    return dict(dz=block(c["B"], c["cout"], c["dzblk"]), x=block(c["B"], c["cin"], c["xblk"]), dw=Lay(c["cout"], c["cin"]),
                db=Lay(1, c["cout"]))


def bwd_weight_plan(c):
    L = bwd_weight_lays(c)
    return plan_linear_bwd_weight(c["B"], c["cin"], c["cout"], L["dz"].ld, L["x"].ld, c["acc"], L["dz"].addr16, L["x"].addr16)


def blob_row(cin, cout, odd):
    """Row length of a parameter blob [w (out x in) | b (out) | pad]: the next multiple of 4 above the parameters, + 1 when odd."""
    n = (cout * cin + cout + 4) // 4 * 4
    return n + 1 if odd else n


def batched_cases():
    """dact: 0 none, 2 / 3 / 4 the derivative folded into the data gradient (zy values of the issue's table)."""
    out = []
    for (B, cin, cout) in BATCH_SHAPES:
        for nb in (1, 2, 5):
            for odd in (False, True):
                for shared in (False, True):
                    for act in (0, 2):
                        out.append(dict(fam="fwd_b", nb=nb, B=B, cin=cin, cout=cout, odd=odd, shared=shared, act=act, z=act == 2,
                                        path=dict(splits=1, vec_a=_m4(cin), vec_b=_m4(cin) and (nb == 1 or not odd))))
                for used in sorted({cin, max(1, cin - 3)}):
                    for acc, dact in ((False, 0), (True, 0), (False, 2), (False, 3), (False, 4)):
                        out.append(dict(fam="bwd_data_b", nb=nb, B=B, cin=cin, cout=cout, odd=odd, used=used, acc=acc, dact=dact,
                                        path=dict(splits=1, vec_a=_m4(cout), vec_b=_m4(cin) and _m4(used) and (nb == 1 or not odd))))
    for (B, cin, cout) in BATCH_WGRAD_SHAPES:
        for nb in (1, 2, 5):
            for where in ("dense", "blob4", "blobodd"):
                s = WGRAD_SHAPES.get((B, cin, cout), 1)
                if nb > 1 and s > 1:                     # 640 / (nb tiles) ranges, never more than B / 64
                    s = {(257, 20, 64): 5, (300, 65, 63): 5, (2048, 64, 64): {2: 32, 5: 32}[nb]}[(B, cin, cout)]
                out.append(dict(fam="bwd_weight_b", nb=nb, B=B, cin=cin, cout=cout, where=where,
                                path=dict(splits=s, vec_a=_m4(cout), vec_b=_m4(cin))))
    return out


def batched_lays(c):
    nb, B, cin, cout = c["nb"], c["B"], c["cin"], c["cout"]
    if c["fam"] == "bwd_weight_b":
        row = cout * cin + cout if c["where"] == "dense" else blob_row(cin, cout, c["where"] == "blobodd")
        if c["where"] == "dense":                        # dw (nb, out, in) and db (nb, out) back to back, each in its own buffer
            dw, db = Lay(cout, cin, nb=nb), Lay(1, cout, nb=nb)
        else:
            dw, db = Lay(cout, cin, nb=nb, sb=row), Lay(1, cout, off=cout * cin, nb=nb, sb=row)
        return dict(dz=Lay(B, cout, nb=nb), x=Lay(B, cin, nb=nb), dw=dw, db=db)
    row = blob_row(cin, cout, c["odd"])
    w, b = Lay(cout, cin, nb=nb, sb=row), Lay(1, cout, off=cout * cin, nb=nb, sb=row)
    if c["fam"] == "fwd_b":
        return dict(x=Lay(B, cin, nb=nb, sb=0 if c["shared"] else None), w=w, b=b, y=Lay(B, cout, cout + 3, 1, nb=nb),
                    z=Lay(B, cout, nb=nb))
    return dict(dz=Lay(B, cout, nb=nb), w=w, b=b, dx=Lay(B, c["used"], nb=nb), zy=Lay(B, c["used"], c["used"] + 1, 0, nb=nb))


def batched_plan(c):
    L = batched_lays(c)
    nb, B, cin, cout = c["nb"], c["B"], c["cin"], c["cout"]
    if c["fam"] == "fwd_b":
        return plan_linear_fwd(B, cin, cout, c["act"], L["x"].ld, L["y"].ld, c["z"], L["x"].addr16, L["w"].addr16, nb, L["x"].sb,
                               L["w"].sb, L["y"].sb)
    if c["fam"] == "bwd_data_b":
        return plan_linear_bwd_data(B, cin, cout, c["used"], L["dz"].ld, L["dx"].ld, c["acc"], L["dz"].addr16, L["w"].addr16, nb,
                                    L["dz"].sb, L["w"].sb, L["dx"].sb, dact=c["dact"] != 0)
    return plan_linear_bwd_weight(B, cin, cout, L["dz"].ld, L["x"].ld, True, L["dz"].addr16, L["x"].addr16, nb, L["dz"].sb, L["x"].sb,
                                  L["dw"].sb)


def strided_cases():
    out = []
    for (B, cin, cout), s in STRIDED_SHAPES.items():
        for fm_dz in (False, True):
            for fm_x in (False, True):
                for wide_dw in (False, True):
                    for nb in (1, 3):
                        # x always has 3 more features than the layer reads; the 16-byte loads need whole aligned runs along the
                        # operand's contiguous index: the rows B when feature-major, the features when row-major
                        va = _m4(B) if fm_dz else _m4(cout)
                        vb = _m4(B) if fm_x else (_m4(cin) and _m4(cin + 3))
                        out.append(dict(fam="strided", nb=nb, B=B, cin=cin, cout=cout, fm_dz=fm_dz, fm_x=fm_x, wide_dw=wide_dw,
                                        path=dict(splits=1 if wide_dw else s, vec_a=va, vec_b=vb)))
    return out


def strided_lays(c):
    nb, B, cin, cout = c["nb"], c["B"], c["cin"], c["cout"]
    xw = cin + 3
    return dict(dz=Lay(cout, B, nb=nb) if c["fm_dz"] else Lay(B, cout, nb=nb), x=Lay(xw, B, nb=nb) if c["fm_x"] else Lay(B, xw, nb=nb),
                dw=Lay(cout, cin, cin + 2 if c["wide_dw"] else cin, nb=nb), db=Lay(1, cout, nb=nb))


def strided_plan(c):
    L = strided_lays(c)
    dz_sr, dz_so = (1, L["dz"].ld) if c["fm_dz"] else (L["dz"].ld, 1)
    x_sr, x_si = (1, L["x"].ld) if c["fm_x"] else (L["x"].ld, 1)
    return plan_linear_bwd_weight_strided(c["B"], c["cin"], c["cout"], dz_sr, dz_so, L["dz"].sb, x_sr, x_si, L["x"].sb, c["nb"],
                                          L["dw"].ld, L["dw"].sb, L["dz"].addr16, L["x"].addr16)


def gram_cases():
    out = []
    for (N, C, hw) in GRAM_SHAPES:
        s = {(1, 64, 256): 4, (2, 64, 300): 5, (3, 65, 257): 5, (1, 128, 2050): 22}.get((N, C, hw), 1)
        for det in (False, True):
            out.append(dict(fam="gram_fwd", N=N, C=C, hw=hw, det=det,
                            path=dict(splits=s, vec_a=_m4(hw), vec_b=_m4(hw), mode="none" if s == 1 else ("two_pass" if det else "atomic"))))
    for (N, C, hw), s in GRAM_BWD_SHAPES.items():
        out.append(dict(fam="gram_bwd", N=N, C=C, hw=hw, path=dict(splits=s, vec_a=_m4(C), vec_b=_m4(hw))))
    return out


def gram_plans(c):
    if c["fam"] == "gram_fwd":
        return (plan_gram_fwd(c["N"], c["C"], c["hw"], det=c["det"]),)
    return plan_gram_bwd(c["N"], c["C"], c["hw"])


def case_plans(c):
    fam = c["fam"]
    if fam == "fwd":
        return (fwd_plan(c),)
    if fam == "bwd_data":
        return (bwd_data_plan(c),)
    if fam == "bwd_weight":
        return (bwd_weight_plan(c),)
    if fam in ("fwd_b", "bwd_data_b", "bwd_weight_b"):
        return (batched_plan(c),)
    if fam == "strided":
        return (strided_plan(c),)
    return gram_plans(c)


def all_cases():
    return fwd_cases() + bwd_data_cases() + bwd_weight_cases() + batched_cases() + strided_cases() + gram_cases()


def name(c):
    return " ".join(f"{k}={v}" for k, v in c.items() if k != "path")


def path_mismatch(c, plans):
    """What of the case's listed path its plans do not show ('' when they agree).  Every plan of a case (npp_gram_bwd has two) has the
    listed range count and B-operand load; vec_a is the first launch's."""
    want, bad = c["path"], []
    for i, p in enumerate(plans):
        for key in ("splits", "vec_b", "mode") + (("vec_a",) if i == 0 else ()):
            if key in want and getattr(p, key) != want[key]:
                bad.append(f"launch {i}: {key} is {getattr(p, key)}, listed {want[key]}")
    return "; ".join(bad)


# ---- value ranges of the exact sweep ---------------------------------------------------------------------------------------------
OPERAND_MAX, PRIOR_MAX = 3, 8


def headroom(c, plan):
    """Largest magnitude any partial or final sum of the case can reach, in units of the finest grid its values sit on: operands are
    integers in [-3, 3], biases and prior contents integers in [-8, 8]; a launch repeated into its own output (the batched weight
    gradient, the second launch of npp_gram_bwd) finds one earlier result there.  The folded activation derivatives are multiples of
    1/4 (sigmoid y (1 - y) at y in {0, 1/2, 1}; tanh 1 - y^2 at |y| in {0, 1/2, 1}), so those products live on a grid of 1/4."""
    total = OPERAND_MAX * OPERAND_MAX * plan.K * 2 + PRIOR_MAX + PRIOR_MAX
    if c["fam"] == "gram_bwd":
        total *= 2                                        # (dG + dG^T) has entries up to 6
    if c.get("dact"):
        total *= 4
    return total
