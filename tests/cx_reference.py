"""Float64 reference, case table and defect catalogue for the contextual-loss core (csrc/npp_cx.hip).

TEST INFRASTRUCTURE ONLY: imported by tests/test_cx_forms_cpu.py (the tests of the tests, no GPU) and by
tests/test_gpu_cx_forms.py (the kernels against float64).  No HIP kernel takes part in anything here.

Reference.  `cx_ref` is oracle.npp_torch_oracle.cx_loss_t with autograd in float64, `cx_ref32` the same call in float32 on the CPU;
`d32(case)` is the distance between the two (relative on the loss, relative L2 on dL/dx): the noise scale of ONE float32 evaluation
of this formula on the case's own inputs.  The GPU test allows K_LOSS * d32 on the loss and K_GRAD * d32 on the gradient.

Case table.  `CASES` lists the smallest shapes at which each launch sequence of `cx_launch` can still go wrong; `dispatch` restates
the predicates of `cx_launch` (and of cx_sim_kernel's body choice) in Python, so that the CPU test can assert what each case hits.

Seeds and mixes.  Each case's seed was searched (a = b = 0.7, the project's recipe, everywhere) until the float64 reference ALONE
showed stable arg-min / arg-max: no row whose two smallest D are within 1e-5 relative, no column whose two largest cx are, and
no entry of raw within 1e-6 of a clamp edge on the cases below hw = 2047 and C = 864.  On the large cases 10 to 100 such entries
exist at every seed; tests/test_cx_forms_cpu.py measures what they carry instead (`conditioning`).

Defects.  `cx_loss_staged` restates cx_loss_t stage by stage (bit-identical without a defect, asserted by the CPU test) with one
switch per named defect of `DEFECTS`; `defect_effect` gives the distance a defect moves loss and gradient in float64.  To check the
detection claim by hand: `defect_effect(case_by_name("fast_one_tile"), "no_min_path")` against `bounds(case)`.
"""
import dataclasses
import functools

import numpy as np
import torch

from oracle.npp_torch_oracle import cx_loss_t

# ---- the bounds of the GPU test ------------------------------------------------------------------------------------------------
# bound = K * d32(case), separately on the loss and on the gradient.  K = the smallest power of two at or above 4 x the worst
# (kernel error / d32) measured on an MI355X over the whole table; the measured ratios are in tests/test_gpu_cx_forms.py.
# With these K the catalogue's weakest separations are (tests/test_cx_forms_cpu.py prints all): the dropped last column 18 bounds
# on the loss of a value-only call (fast_hw2048: one column of 2048) and 120 with a gradient, the dropped clamp gate 156 bounds
# (gen_hw2047), everything else above 3000.
K_LOSS = 32              # worst ratio on the loss 4.72 (groups_gen_hw63)
K_GRAD = 8               # worst ratio on the gradient 1.75 (gen_hw2)
LOSS_CAP = 1e-5          # K * d32 must stay at or below these on every case (asserted on the CPU)
GRAD_CAP = 1e-4
# The loss is ONE float32 word: no float32 evaluation can be expected closer to the float64 value than the rounding of that word,
# up to 2^-24 relative.  Where the CPU's float32 loss lands closer than that by luck (seen: 4e-10), the distance says nothing about
# the noise scale, and d32 of the loss is taken as 2^-24.
LOSS_D32_FLOOR = 2.0 ** -24
DETECT_FACTOR = 10.0     # a defect counts as detected when it moves loss or gradient by this many bounds

# ---- cx_launch's predicates, restated ------------------------------------------------------------------------------------------
K_LDS_DEFAULT = 48 * 1024      # kLdsDefault
CX_MAX_COLS = 32               # kCxMaxCols: columns per lane in registers, hw <= 64 * 32
CX_ROW_WAVES = 16              # kCxRowWaves: rows (= waves) per block of cx_rows_fwd32_kernel
BIG_Q = 4                      # kBigQ


def big_fwd_fits(N, C, hw):
    """The value-only big form's arrays (tiled matrix, re-tiled operands, row-sum quarters) inside the 2 N hw^2 floats of D + cx."""
    t = (hw + 127) // 128
    return N * (t * t * 16384 + 2 * t * C * 128 + hw * BIG_Q) <= 2 * N * hw * hw


def rows_lds_bytes(hw):
    return CX_ROW_WAVES * hw * 4


def dispatch(N, C, hw, grad, weight):
    """What cx_launch does with (N, C, hw, d_dfx != null, d_weight != null): the launch sequence (`form`) and the kernel-internal
    paths the shape takes."""
    big = hw > 64 * CX_MAX_COLS
    fast = not big and hw % 32 == 0                    # selects the backward contraction (cx_dx32s_kernel) and loss_in_rows, nothing else
    loss_in_rows = fast and grad and not weight
    raised_lds = not big and rows_lds_bytes(hw) > K_LDS_DEFAULT      # every non-big form takes cx_rows_fwd32_kernel
    fits = big_fwd_fits(N, C, hw)
    if fast:
        form = "fast"
    elif big and not grad and fits:
        form = "big-value"
    elif big and not grad:
        form = "big-value-no-fit"
    elif big:
        form = "big-gradient"
    else:
        form = "generic"
    vec = hw % 4 == 0
    uses_sim = form != "big-value"                     # cx_sim_kernel (64 x 64 tiles); the big-value form has its own contraction
    bodies = set()
    if uses_sim:
        if vec and hw >= 64:
            bodies.add("FULL")                         # tile (0, 0) lies wholly inside the map (C % 32 == 0 always)
        if not vec or hw % 64:
            bodies.add("non-FULL")                     # scalar loads, or a last tile that is partial
    chunks = C // 32
    # the row minima: by atomicMin in cx_sim_kernel where cx_rows_fwd_big_kernel reads them (CxWs::sim_atomic_min), in the row pass's
    # registers on every smaller map, in cx_sim_big_kernel on the value-only big form
    return dict(form=form, big=big, fast=fast, loss_in_rows=loss_in_rows, raised_lds=raised_lds, big_fwd_fits=fits,
                sim_atomic_min=big and uses_sim,
                loads="vector" if vec else "scalar", sim_bodies=bodies,
                chunks="one" if chunks == 1 else ("odd" if chunks % 2 else "even"))


# ---- the case table ------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    form: str                  # the form the case is meant to hit WITH a gradient ("big" cases: see value_form)
    shape: tuple               # (N, C, h, w)
    pins: str
    seed: int = 0
    a: float = 0.7             # x = relu(a y + b randn)
    b: float = 0.7
    band_width: float = 0.5
    weighted: bool = False
    groups: tuple = None       # ((x0, nk), ...) of a grouped case
    value_form: str = None     # the form of the value-only call where it differs from `form`
    modes: tuple = ("grad", "value")

    @property
    def hw(self):
        return self.shape[2] * self.shape[3]


# group g of a grouped case: y scaled by 1 + 0.5 g' and offset by 0.3 g' (g' = index among the active groups, modulo 3: further
# out the offset swamps the noise, x and y coincide and the loss goes to 0, where a RELATIVE distance means little)
def group_stats(k):
    return 1.0 + 0.5 * (k % 3), 0.3 * (k % 3)


GROUPS_7 = ((0, 2), (2, 0), (2, 1), (3, 4))          # X = 7, M = 4: an idle group in the middle that shares its x0 with the next
GROUPS_16 = tuple((i, 1) for i in range(16))         # M = NPP_MAX_STACK groups of one sample each

CASES = (
    Case("fast_one_tile", "fast", (2, 32, 8, 8), "one tile, one chunk, FULL body", seed=0),
    Case("fast_hw32_c96", "fast", (3, 96, 4, 8), "hw = 32 < tile, odd chunk count (pair loop + single tail)", seed=1),
    Case("fast_hw96_c128", "fast", (2, 128, 8, 12), "hw = 96: second tile partial (non-FULL body), even chunk count > 2", seed=0),
    Case("fast_9_blocks", "fast", (9, 32, 8, 8), "9 logical blocks on a grid of 16: xcd_block remap, surplus-block exit", seed=0),
    Case("fast_hw768", "fast", (1, 64, 24, 32), "hw = 768: largest row under the default LDS limit", seed=7),
    Case("fast_hw800", "fast", (1, 32, 25, 32), "hw = 800: smallest row over it (raised-limit launch)", seed=1),
    Case("fast_hw2048", "fast", (1, 32, 32, 64), "hw = 2048: largest fast row, all kCxMaxCols register columns in use", seed=5),
    Case("gen_hw2", "generic", (1, 32, 1, 2), "hw = 2: far below one tile; scalar loads", seed=0),
    Case("gen_hw63", "generic", (2, 64, 7, 9), "hw = 63: one column short of a tile; scalar loads", seed=0),
    Case("gen_hw65", "generic", (1, 32, 5, 13), "hw = 65: one column into the second tile; scalar loads", seed=0),
    Case("gen_hw120", "generic", (2, 64, 10, 12), "hw = 120: generic with vector loads (added: the issue's generic shapes are all scalar)",
         seed=2),
    Case("gen_hw2047", "generic", (1, 32, 23, 89), "hw = 2047: largest small form, odd; raised-limit launch of the row pass (131 008 B of LDS)",
         seed=3),
    Case("big_hw2049", "big-gradient", (1, 32, 3, 683),
         "hw = 2049: second column chunk holds a single column; scalar loads; value only: 17 tiles of 128, one-column last tile, t8 = 3",
         seed=11, value_form="big-value"),
    Case("big_hw2112", "big-gradient", (1, 32, 33, 64), "hw = 2112: a multiple of 32, yet not the fast form; value only: 17 full tiles",
         seed=6, value_form="big-value"),
    Case("big_nofit_c864", "big-gradient", (1, 864, 3, 683),
         "C = 864: smallest C at hw = 2049 for which big_fwd_fits is false -> value-only call falls back to cx_sim_kernel + cx_rows_fwd_big_kernel",
         seed=1, value_form="big-value-no-fit"),
    # variations
    Case("fast_bw0.1", "fast", (2, 32, 8, 8), "band width 0.1", seed=0, band_width=0.1),
    Case("fast_bw1.0", "fast", (2, 32, 8, 8), "band width 1.0", seed=0, band_width=1.0),
    Case("gen_bw0.1", "generic", (2, 64, 7, 9), "band width 0.1", seed=0, band_width=0.1),
    Case("gen_bw1.0", "generic", (2, 64, 7, 9), "band width 1.0", seed=0, band_width=1.0),
    Case("fast_weighted", "fast", (2, 32, 8, 8), "weights: loss_in_rows off, cx_loss_kernel after cx_rows_fwd32_kernel", seed=0, weighted=True),
    Case("gen_weighted", "generic", (2, 64, 7, 9), "weights on the generic form (cx_loss_kernel after cx_rows_fwd32_kernel, as every generic case)",
         seed=0, weighted=True),
    Case("big_weighted", "big-gradient", (2, 32, 3, 683), "weights on the big forms (N = 2: two different weights)", seed=9, weighted=True,
         value_form="big-value"),
)

# grouped cases (ops.cx_fwd_bwd_groups / cx_fwd_bwd_flat; gradient only: the grouped entry points always want one)
GROUP_CASES = (
    Case("groups_fast_hw64", "fast", (7, 32, 8, 8), "4 groups, one idle, on the fast form", seed=0, groups=GROUPS_7, modes=("grad",)),
    Case("groups_gen_hw63", "generic", (7, 32, 7, 9), "4 groups, one idle, on the generic form", seed=0, groups=GROUPS_7, modes=("grad",)),
    Case("groups_16_singles", "fast", (16, 32, 4, 8), "M = NPP_MAX_STACK groups of one sample each", seed=0, groups=GROUPS_16,
         modes=("grad",)),
)
ALL_CASES = CASES + GROUP_CASES


def case_by_name(name):
    return next(c for c in ALL_CASES if c.name == name)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(x, y, weight or None) float32 NumPy: y = relu(randn) [* scale + offset per group], x = relu(a y + b randn)."""
    rng = np.random.RandomState(1000 + case.seed)
    y = np.maximum(rng.randn(*case.shape), 0)
    if case.groups is not None:
        k = 0
        for x0, nk in case.groups:
            if nk > 0:
                s, o = group_stats(k)
                y[x0:x0 + nk] = y[x0:x0 + nk] * s + o
                k += 1
    x = np.maximum(case.a * y + case.b * rng.randn(*case.shape), 0)
    wt = (0.5 + rng.rand(case.shape[0])).astype(np.float32) if case.weighted else None
    x, y = x.astype(np.float32), y.astype(np.float32)
    for arr in (x, y):
        arr.setflags(write=False)
    return x, y, wt


# ---- the staged restatement with its defect switches ---------------------------------------------------------------------------
DEFECTS = {
    "drop_last_col": "the last column of the last column tile left out of the column maxima (its maximum stays at the cleared 0)",
    "no_min_path": "the row minimum's own gradient path (corr / dm^2 in cx_rows_bwd_kernel) dropped",
    "no_clamp_gate": "the clamp gate dropped: d raw passes where raw is outside (0, 1)",
    "n_over_batch": "1 / N taken over the batch instead of the group",
    "mu_over_batch": "the channel mean taken over the batch instead of the group",
    "weight_ignored": "the weight ignored (taken as 1)",
    "scale_twice": "the scale applied twice",
    "chunk_twice": "the last 32-channel chunk counted twice in the squared norms",
}
GRADIENT_ONLY = ("no_min_path", "no_clamp_gate")     # these leave the forward value alone: invisible to a value-only call


def cx_loss_staged(x, y, band_width=0.5, weight=None, defect=None, mu=None, n_div=None, probe=None):
    """cx_loss_t stage by stage.  mu / n_div: the channel mean and the sample count of the loss mean when they are NOT the ones of
    (x, y) themselves (defects of the grouped form).  probe: dict that receives the intermediates."""
    F = torch.nn.functional
    N, C = x.shape[:2]
    if mu is None:
        mu = y.mean(dim=(0, 2, 3), keepdim=True)
    xc, yc = x - mu, y - mu
    if defect == "chunk_twice":
        def norm2(v):
            ss = (v * v).sum(dim=1, keepdim=True) + (v[:, C - 32:] * v[:, C - 32:]).sum(dim=1, keepdim=True)
            return v / ss.sqrt().clamp_min(1e-12)
        xn, yn = norm2(xc), norm2(yc)
    else:
        xn, yn = F.normalize(xc, p=2, dim=1), F.normalize(yc, p=2, dim=1)
    raw = torch.bmm(xn.reshape(N, C, -1).transpose(1, 2), yn.reshape(N, C, -1))
    cl = torch.clamp(raw, min=0, max=1)
    if defect == "no_clamp_gate":
        cl = raw + (cl - raw).detach()
    dist = 1 - cl
    dmin, _ = torch.min(dist, dim=2, keepdim=True)
    if defect == "no_min_path":
        dmin = dmin.detach()
    w = torch.exp((1 - dist / (dmin + 1e-5)) / band_width)
    cx = w / torch.sum(w, dim=2, keepdim=True)
    cmax = torch.max(cx, dim=1)[0]
    if defect == "drop_last_col":
        cmax = torch.cat([cmax[:, :-1], torch.zeros_like(cmax[:, -1:])], dim=1)
    cxn = torch.mean(cmax, dim=1)
    if probe is not None:
        probe.update(raw=raw, cl=cl, dist=dist, cx=cx)
    if weight is not None:
        if defect == "weight_ignored":
            weight = torch.ones_like(weight)
        return torch.sum(-torch.log(cxn * weight + 1e-5))
    if n_div is None:
        return torch.mean(-torch.log(cxn + 1e-5))
    return torch.sum(-torch.log(cxn + 1e-5)) / n_div


def _evaluate(x, y, band_width, weight, scale, groups, dtype, defect=None):
    """-> (losses float64 (M,) or (1,), dL/dx float64 NumPy).  defect None: oracle.npp_torch_oracle.cx_loss_t itself."""
    xt = torch.tensor(np.asarray(x)).to(dtype).clone().requires_grad_(True)
    yt = torch.tensor(np.asarray(y)).to(dtype)
    wt = None if weight is None else torch.tensor(np.asarray(weight)).to(dtype)
    if defect == "scale_twice":
        scale = scale * scale
    fn = cx_loss_t if defect is None else functools.partial(cx_loss_staged, defect=defect)
    if groups is None:
        terms = [fn(xt, yt, band_width, wt) * scale]
    else:
        assert wt is None
        n_all = sum(nk for _, nk in groups)
        lo, hi = min(x0 for x0, nk in groups if nk), max(x0 + nk for x0, nk in groups if nk)
        terms = []
        for x0, nk in groups:
            if nk == 0:
                terms.append(None)
                continue
            kw = {}
            if defect == "n_over_batch":
                kw["n_div"] = n_all
            if defect == "mu_over_batch":
                kw["mu"] = yt[lo:hi].mean(dim=(0, 2, 3), keepdim=True)
            terms.append(fn(xt[x0:x0 + nk], yt[x0:x0 + nk], band_width, None, **kw) * scale)
    total = sum(t for t in terms if t is not None)
    total.backward()
    losses = np.array([0.0 if t is None else float(t.detach().double()) for t in terms], np.float64)
    return losses, xt.grad.double().numpy()


def cx_ref(x, y, band_width, weight=None, scale=1.0, groups=None):
    """The loss (one per group when groups = [(x0, nk), ...] is given; 0 for an idle group) and dL/dx, float64.  Every group with
    nk > 0 is an independent cx_loss_t over samples x0 .. x0 + nk: its own channel mean, its own 1 / nk."""
    return _evaluate(x, y, band_width, weight, scale, groups, torch.float64)


def cx_ref32(x, y, band_width, weight=None, scale=1.0, groups=None):
    """The same call evaluated in float32 on the CPU."""
    return _evaluate(x, y, band_width, weight, scale, groups, torch.float32)


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def loss_dist(a, b):
    """Largest relative distance of the losses a from b (idle groups, b == 0, must be 0 in a as well)."""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    live = b != 0
    assert np.all(a[~live] == 0)
    return float(np.max(np.abs(a[live] - b[live]) / np.abs(b[live])))


@functools.lru_cache(maxsize=None)
def reference(case):
    """(losses, dL/dx) of the case in float64 at scale 1; computed once, shared, read-only."""
    x, y, wt = inputs(case)
    losses, dx = cx_ref(x, y, case.band_width, wt, 1.0, case.groups)
    losses.setflags(write=False)
    dx.setflags(write=False)
    return losses, dx


@functools.lru_cache(maxsize=None)
def d32(case):
    """(relative distance on the loss, relative L2 on the gradient) of cx_ref32 from cx_ref on the case's inputs."""
    x, y, wt = inputs(case)
    l32, dx32 = cx_ref32(x, y, case.band_width, wt, 1.0, case.groups)
    l64, dx64 = reference(case)
    return max(loss_dist(l32, l64), LOSS_D32_FLOOR), rel_l2(dx32, dx64)


def bounds(case):
    """The GPU test's bounds for the case: (relative on the loss, relative L2 on the gradient)."""
    dl, dg = d32(case)
    return K_LOSS * dl, K_GRAD * dg


def applicable_defects(case, scale=1.0):
    out = ["drop_last_col", "no_min_path", "no_clamp_gate", "chunk_twice"]
    if case.groups is not None:
        out += ["n_over_batch", "mu_over_batch"]
    if case.weighted:
        out.append("weight_ignored")
    if scale != 1.0:
        out.append("scale_twice")
    return out


def defect_effect(case, defect, scale=1.0):
    """How far the defect moves the float64 result: (relative on the loss, relative L2 on the gradient)."""
    x, y, wt = inputs(case)
    l64, dx64 = reference(case)
    ld, dxd = _evaluate(x, y, case.band_width, wt, scale, case.groups, torch.float64, defect=defect)
    return loss_dist(ld, l64 * scale), rel_l2(dxd, dx64 * scale)


# ---- conditioning: is a float64 comparison fair on this case? ----------------------------------------------------------------
def conditioning(case):
    """From the float64 reference alone:
      row_gap   smallest relative gap between the two smallest D of a row     (arg-min stable in fp32 when well above 1e-7)
      col_gap   smallest relative gap between the two largest cx of a column  (arg-max stable)
      n_edge    raw entries within 1e-6 of a clamp edge (0 or 1)
      edge_grad relative L2 of the part of dL/dx that those entries carry (or would carry with their gate open): what flipping
                the gate of ALL of them moves the gradient by."""
    x, y, wt = inputs(case)
    xt = torch.tensor(x).double().requires_grad_(True)
    yt = torch.tensor(y).double()
    wtt = None if wt is None else torch.tensor(wt).double()
    groups = case.groups if case.groups is not None else ((0, case.shape[0]),)
    row_gap = col_gap = np.inf
    n_edge = 0
    moved = torch.zeros_like(xt)
    for x0, nk in groups:
        if nk == 0:
            continue
        p = {}
        loss = cx_loss_staged(xt[x0:x0 + nk], yt[x0:x0 + nk], case.band_width, wtt, defect="no_clamp_gate", probe=p)
        (g,) = torch.autograd.grad(loss, p["cl"], retain_graph=True)        # dL/d clamp(raw): what an open gate passes
        raw = p["raw"].detach()
        near = (raw.abs() < 1e-6) | ((raw - 1).abs() < 1e-6)
        n_edge += int(near.sum())
        if near.any():
            moved = moved + torch.autograd.grad(p["raw"], xt, grad_outputs=g * near)[0]
        if case.hw > 1:
            d2 = torch.topk(p["dist"].detach(), 2, dim=2, largest=False)[0]
            row_gap = min(row_gap, float(((d2[..., 1] - d2[..., 0]) / d2[..., 1].clamp_min(1e-300)).min()))
            c2 = torch.topk(p["cx"].detach(), 2, dim=1, largest=True)[0]
            col_gap = min(col_gap, float(((c2[:, 0] - c2[:, 1]) / c2[:, 0]).min()))
    _, dx = reference(case)
    return dict(row_gap=row_gap, col_gap=col_gap, n_edge=n_edge,
                edge_grad=float(np.linalg.norm(moved.numpy()) / np.linalg.norm(dx)))
