"""The case table of the exact sweep over the 16-bit trunk convolutions (csrc/npp_conv.hip, csrc/npp_conv_pair.hip), its operand
generators and its float64 reference.  tests/test_conv_plan_cpu.py checks the table on the host (listed forms against
npp_conv3x3_plan, coverage, exactness conditions); tests/test_gpu_conv_exact.py runs it on the GPU.  Both import THIS module, so both
see the same arrays.

Why integers: every operand is a small integer that fp16 / bf16 hold exactly, every partial sum is an integer below 2^24 and every
stored result an integer the 16-bit format holds (|v| <= 2048 in fp16, <= 256 in bf16).  Then every summation order, split, fold and
fused pair must give the SAME BITS as a float64 convolution: the assertion is equality, and a ReLU gate cannot flip.

A case:
  entry   "conv" (npp_conv3x3 / _pf), "pool" (npp_conv3x3_pool), "dgrad_pool" (npp_conv3x3_dgrad_pool)
  mode    0 forward, 1 gated data gradient, 2 linear data gradient (the launch's mode argument)
  N, n    N_total and n_run;  H, W, cin, cout: the LAUNCH's geometry and channels (a data gradient's cin is the convolution's Cout)
  tune    the npp_tune settings (conv_win, conv_wink, conv_wstat) the form is listed under
  form    (family, ct, pt, s, npt, wstat) as npp_conv3x3_plan reports it
  seed    of the operand generator; the value sets and densities follow from entry / mode / channels (recipe())
  options tap = (ctap, scale or None, y_null), image (3-channel image layer through trunk_image_in and the in_natural pack),
          addend (dgrad_pool), next_pack (run a second time with d_next_pack and require equal bits; never on a weight-stationary
          launch, which drops the request)."""
import functools

import numpy as np
import torch

GUARD, POS_ROUND = 1024, 512          # csrc/npp_trunk_layout.h
SENTINEL = 0x5A5A                     # 16-bit fill of an output buffer before the launch: fp16 203.25 / bf16 1.5e16, never a result
TAP_SENTINEL = -7777.25               # fp32 fill of a tap buffer: not an integer (times a power of two >= 1/4)
F16_MAX_INT, BF16_MAX_INT = 2048, 256
MODES = ("fwd", "dgrad_mask", "dgrad_lin", "fwd_pool", "dgrad_pool")      # ConvMode of csrc/npp_conv.hip
TILE_FORMS = ((2, 2, 1), (2, 2, 4), (2, 1, 4), (1, 1, 4), (1, 1, 8), (2, 1, 1), (1, 1, 1))


# ---- layout -----------------------------------------------------------------------------------------------------------------------
def conv_chan(c8, j):
    """true channel of element j of chunk c8 (csrc/npp_trunk_layout.h)"""
    return 32 * (c8 >> 2) + 16 * ((c8 >> 1) & 1) + 8 * (j >> 2) + 4 * (c8 & 1) + (j & 3)


def npos_round(N, H, W):
    return (N * (H + 2) * (W + 2) + POS_ROUND - 1) // POS_ROUND * POS_ROUND


def nposp(N, H, W):
    return npos_round(N, H, W) + 2 * GUARD


def run_range(n_run, H, W):
    """positions a launch computes: n_run images rounded up to 512 (n_run = N_total: the tensor's whole rounded position axis)"""
    return npos_round(n_run, H, W)


def kernel_mode(c):
    return {"conv": c["mode"], "pool": 3, "dgrad_pool": 4}[c["entry"]]


def fold_of(c):
    return {"conv": 0, "pool": 1, "dgrad_pool": 2}[c["entry"]]


def name(c):
    t = c["tune"]
    return (f"{c['entry']}{c['mode']}-{c['N']}.{c['n']}x{c['H']}x{c['W']}-{c['cin']}to{c['cout']}-"
            f"w{t['conv_win']}k{t['conv_wink']}s{t['conv_wstat']}" + ("-img" if c.get("image") else "") +
            ("-add" if c.get("addend") else "") + ("-tap" + "".join(str(int(bool(v))) for v in c["tap"][1:]) + str(c["tap"][0]) if c.get("tap") else ""))


def written_positions(N, H, W, upto, interior_only, n_lim=None):
    """bool (npos_round(N, H, W),) over the position axis without its guards: the positions of the (N, ., H, W) geometry a launch
    writes -- p < upto (and image < n_lim), all of them or the interior ones only.  -> (written, interior)"""
    S = (H + 2) * (W + 2)
    p = np.arange(npos_round(N, H, W))
    r = p % S
    y, x = r // (W + 2), r % (W + 2)
    interior = (p < N * S) & (y >= 1) & (y <= H) & (x >= 1) & (x <= W)
    w = p < upto
    if n_lim is not None:
        w &= (p // S) < n_lim
    return (w & interior) if interior_only else w, interior


def to_bits(vals, f16):
    """float array -> the uint16 codes of its fp16 / bf16 values (-0 becomes +0: the kernels never store -0 from integer sums)"""
    t = torch.from_numpy(np.ascontiguousarray(vals, dtype=np.float32) + 0.0).to(torch.float16 if f16 else torch.bfloat16)
    return t.view(torch.int16).numpy().view(np.uint16)


def flat_expect(vals, N, C, H, W, written, f16, base=None):
    """The whole flat buffer [C/8][nposp][8] as uint16 codes: SENTINEL everywhere (or the codes of `base`), and at the positions
    `written` (written_positions) the values of vals (N, C, H, W) with a zero border and a zero tail behind the last image."""
    S, nr = (H + 2) * (W + 2), npos_round(N, H, W)
    pad = np.zeros((N, C, H + 2, W + 2), np.float32)
    pad[:, :, 1:-1, 1:-1] = vals
    flat = np.zeros((C, nr), np.uint16)
    flat[:, :N * S] = to_bits(pad, f16).transpose(1, 0, 2, 3).reshape(C, N * S)
    chunks = C // 8
    idx = np.array([[conv_chan(c8, j) for j in range(8)] for c8 in range(chunks)])
    per = flat[idx].transpose(0, 2, 1)                                          # (chunks, nr, 8)
    buf = np.full((chunks, nr + 2 * GUARD, 8), SENTINEL, np.uint16) if base is None else base.copy()
    core = buf[:, GUARD:GUARD + nr, :]
    core[:, written, :] = per[:, written, :]
    return buf


# ---- operand recipes ----------------------------------------------------------------------------------------------------------------
def recipe(c):
    """Value sets and densities of a case's operands.  Forward: activations in {0..3}, weights in {-2..2}, integer bias; the worst
    case (512 -> 512) reaches |sum| = 867 < 2048.  Gradients: values in {-1, 0, 1}, gradient density 3/16 from 256 channels on and
    1/2 below, weights nonzero with probability 3/4: at most 81 at 512 -> 512 (limit 256).  ReLU masks / pre-pool activations hold
    zeros and (masks) negative values."""
    if kernel_mode(c) in (0, 3):
        return dict(seed=c["seed"], x=(0, 1, 2, 3), w=(-2, -1, 0, 1, 2), bias=(-4, 4))
    return dict(seed=c["seed"], g=(-1, 0, 1), g_density=3 / 16 if c["cin"] >= 256 else 1 / 2, w=(-1, 0, 1), w_density=3 / 4,
                mask=(-1, 0, 1, 2, 1, 2, 3, 1), xpre=(0, 0, 1, 2, 1, 2, 3, 1), addend=(-2, 2))


def _sparse_pm1(rng, shape, density):
    return (rng.randint(0, 2, shape) * 2 - 1) * (rng.rand(*shape) < density)


IMG_SCALE, IMG_SHIFT = (0.5, 1.0, 2.0), (1.0, 0.0, -1.0)        # trunk_image_in: powers of two, integer shifts
GRAD_SCALE = (0.5, 2.0, 4.0)                                    # tap_scale of the image gradient


@functools.lru_cache(maxsize=4)                   # (a case is used by one test at a time; the large ones hold ~300 MB)
def _operands(index):
    c = CASES[index]
    r = recipe(c)
    rng = np.random.RandomState(r["seed"])
    N, H, W, cin, cout = c["N"], c["H"], c["W"], c["cin"], c["cout"]
    km = kernel_mode(c)
    o = {}
    if km in (0, 3):
        creal = 3 if c.get("image") else cin
        o["x"] = rng.choice(r["x"], (N, creal, H, W)).astype(np.float32)
        o["w"] = rng.choice(r["w"], (cout, creal, 3, 3)).astype(np.float32)
        o["bias"] = rng.randint(r["bias"][0], r["bias"][1] + 1, cout).astype(np.float32)
        if c.get("image"):       # the fp32 image whose x * scale + shift is o["x"] exactly
            s, b = np.array(IMG_SCALE, np.float32)[None, :, None, None], np.array(IMG_SHIFT, np.float32)[None, :, None, None]
            o["img"] = (o["x"] - b) / s
    else:
        creal = 3 if c.get("image") else cout                 # channels of the convolution's INPUT = the launch's output
        o["g"] = _sparse_pm1(rng, (N, cin, H, W), r["g_density"]).astype(np.float32)
        o["w"] = _sparse_pm1(rng, (cin, creal, 3, 3), r["w_density"]).astype(np.float32)     # torch Conv2d weight (Cout, Cin, 3, 3) of the layer
        if km == 1:
            o["mask"] = rng.choice(r["mask"], (N, cout, H, W)).astype(np.float32)
        if km == 4:
            o["xpre"] = rng.choice(r["xpre"], (N, cout, 2 * H, 2 * W)).astype(np.float32)
            if c.get("addend"):
                o["addend"] = rng.randint(r["addend"][0], r["addend"][1] + 1, (N, cout, 2 * H, 2 * W)).astype(np.float32)
    return o


def operands(c):
    """fp32 NumPy arrays of the case (the last few are cached; treat as read-only)"""
    return _operands(c["index"])


@functools.lru_cache(maxsize=4)
def _reference(index):
    c = CASES[index]
    o = operands(c)
    km = kernel_mode(c)
    F = torch.nn.functional
    t = lambda a: torch.from_numpy(a).to(torch.float64)
    r = {}
    if km in (0, 3):
        pre = F.conv2d(t(o["x"]), t(o["w"]), t(o["bias"]), padding=1)
        r["pre"] = pre.numpy()
        r["absmax_sum"] = float(F.conv2d(t(o["x"]).abs(), t(o["w"]).abs(), t(o["bias"]).abs(), padding=1).max())
        y = torch.relu(pre)
        r["y"] = y.numpy()
        if km == 3:
            r["pool"] = F.max_pool2d(y, 2, 2).numpy()
    else:
        d = F.conv_transpose2d(t(o["g"]), t(o["w"]), padding=1)
        r["absmax_sum"] = float(F.conv_transpose2d(t(o["g"]).abs(), t(o["w"]).abs(), padding=1).max())
        r["d"] = d.numpy()
        if km == 1:
            r["y"] = torch.where(t(o["mask"]) > 0, d, torch.zeros_like(d)).numpy()
        elif km == 2:
            r["y"] = r["d"]
        else:
            xp = t(o["xpre"]).requires_grad_(True)
            (F.max_pool2d(xp, 2, 2) * d).sum().backward()                         # torch routes to the first maximum in scan order
            g = xp.grad if "addend" not in o else xp.grad + t(o["addend"])
            r["routed"] = g.detach().numpy()                                       # before the pre-pool ReLU gate
            r["dz"] = torch.where(xp.detach() > 0, g, torch.zeros_like(g)).numpy()
    return r


def reference(c):
    """float64 reference (the last few are cached; read-only): forward pre / y (/ pool); gradients d (the convolution's result) and y or dz"""
    return _reference(c["index"])


# ---- the table ----------------------------------------------------------------------------------------------------------------------
def tune_of(win, wink, wstat):
    return dict(conv_win=win, conv_wink=wink, conv_wstat=wstat)


def _c(entry, mode, N, n, H, W, cin, cout, tune, form, seed, **opt):
    c = dict(entry=entry, mode=mode, N=N, n=n, H=H, W=W, cin=cin, cout=cout, tune=tune_of(*tune), form=form, seed=seed)
    c.update(opt)
    return c


CASES = []
CASES_BY_NAME = {}


def all_cases():
    return CASES


def _register(cases):
    for c in cases:
        assert name(c) not in CASES_BY_NAME, name(c)
        CASES_BY_NAME[name(c)] = c
        c["index"] = len(CASES)                   # key of the operand / reference caches
        CASES.append(c)


def _five_modes(N, n, H, W, cin, cout, tune, form, seed, pool_hw=None, **opt):
    """one shape in the five modes of conv3x3_kernel (the forward + pool fold needs even H, W: pool_hw replaces an odd shape, and the
    fold's two-row tiles count positions differently -- both keep the listed form)"""
    ph, pw = pool_hw or (H, W)
    return [_c("conv", 0, N, n, H, W, cin, cout, tune, form, seed, **opt),
            _c("conv", 1, N, n, H, W, cin, cout, tune, form, seed + 1),
            _c("conv", 2, N, n, H, W, cin, cout, tune, form, seed + 2),
            _c("pool", 0, N, n, ph, pw, cin, cout, tune, form, seed + 3),
            _c("dgrad_pool", 2, N, n, H, W, cin, cout, tune, form, seed + 4, addend=seed % 20 == 0)]


# Shapes: the smallest the plan query gives for each (form, mode) -- `python tests/conv_cases.py` prints that search -- varied so that
# odd H, W % 16 != 0, n_run < N_total and Cout = 48 / 96 occur; (14, 30) images have exactly 512 padded positions.
T000, WIN2, WINK2, WSTAT = (0, 0, 0), (2, 0, 0), (0, 2, 0), (0, 0, 1)
SC = GRAD_SCALE
_register(
    # ---- conv3x3_kernel<1, 1, 1>: one channel step or an odd number of them, one 32-channel tile
    _five_modes(1, 1, 2, 2, 16, 16, T000, ("tile", 1, 1, 1, 0, 0), 100) +
    [_c("conv", 1, 2, 1, 9, 13, 32, 32, T000, ("tile", 1, 1, 1, 0, 0), 110),
     _c("conv", 0, 2, 2, 5, 7, 16, 96, T000, ("tile", 1, 1, 1, 0, 0), 111, tap=(40, None, False)),             # odd cot_n: no 2-tile form
     _c("conv", 2, 2, 2, 7, 20, 64, 16, T000, ("tile", 1, 1, 1, 0, 0), 112, image=True, tap=(3, SC, False)),    # the image gradient
     _c("conv", 2, 2, 1, 9, 13, 32, 16, T000, ("tile", 1, 1, 1, 0, 0), 113, image=True, tap=(3, SC, True)),
     _c("dgrad_pool", 2, 2, 2, 3, 18, 32, 32, T000, ("tile", 1, 1, 1, 0, 0), 114)] +
    # ---- <2, 1, 1>: the image layer's pick (CI == 1) and 16 -> 48
    _five_modes(1, 1, 2, 2, 16, 48, T000, ("tile", 2, 1, 1, 0, 0), 120, tap=(3, (0.25, 2.0, 8.0), False)) +
    [_c("conv", 0, 2, 2, 9, 13, 16, 64, T000, ("tile", 2, 1, 1, 0, 0), 130, image=True, tap=(64, None, True)),
     _c("conv", 0, 3, 2, 10, 14, 16, 64, T000, ("tile", 2, 1, 1, 0, 0), 131, image=True, next_pack=True),
     _c("pool", 0, 2, 1, 6, 14, 16, 48, T000, ("tile", 2, 1, 1, 0, 0), 132, tap=(20, None, False)),
     _c("pool", 0, 1, 1, 4, 18, 16, 64, T000, ("tile", 2, 1, 1, 0, 0), 133),
     _c("dgrad_pool", 2, 2, 1, 5, 14, 16, 48, T000, ("tile", 2, 1, 1, 0, 0), 134, addend=True)] +
    # ---- <1, 1, 8>: eight channel steps, too few positions for anything wider
    _five_modes(1, 1, 14, 30, 128, 32, T000, ("tile", 1, 1, 8, 0, 0), 140) +
    [_c("pool", 0, 1, 1, 4, 16, 128, 32, T000, ("tile", 1, 1, 8, 0, 0), 150, next_pack=True),
     _c("dgrad_pool", 2, 1, 1, 3, 16, 128, 32, T000, ("tile", 1, 1, 8, 0, 0), 151, addend=True, next_pack=True),
     _c("pool", 0, 1, 1, 2, 2, 128, 256, WSTAT, ("tile", 1, 1, 8, 0, 1), 152)] +
    # ---- <1, 1, 4>: 64 -> 96 on 1536 positions (odd cot_n), 64 -> 16 on 3584
    _five_modes(4, 3, 14, 30, 64, 96, T000, ("tile", 1, 1, 4, 0, 0), 160, tap=(96, None, False)) +
    [_c("conv", 1, 3, 3, 31, 33, 64, 16, T000, ("tile", 1, 1, 4, 0, 0), 170, next_pack=True),
     _c("conv", 2, 3, 3, 31, 33, 64, 16, T000, ("tile", 1, 1, 4, 0, 0), 171, image=True, tap=(3, SC, False))] +
    # ---- <2, 1, 4>: 64 -> 512 on 1024 positions
    _five_modes(1, 1, 21, 22, 64, 512, T000, ("tile", 2, 1, 4, 0, 0), 180, pool_hw=(24, 22)) +
    [_c("conv", 0, 3, 3, 44, 44, 64, 48, T000, ("tile", 2, 1, 4, 0, 0), 190, tap=(3, (0.5, 1.0, 2.0), True))] +
    # ---- <2, 2, 4>: 64 -> 512 on 2048 positions
    _five_modes(1, 1, 40, 46, 64, 512, T000, ("tile", 2, 2, 4, 0, 0), 200) +
    # ---- <2, 2, 1>: 32 -> 512 on 8192 positions
    _five_modes(2, 2, 62, 62, 32, 512, T000, ("tile", 2, 2, 1, 0, 0), 210) +
    # ---- weight-stationary block numbering, and the same launches one image later (the activations outweigh half the pack)
    [_c("conv", 0, 5, 4, 14, 30, 16, 512, WSTAT, ("tile", 2, 1, 1, 0, 1), 220),
     _c("conv", 0, 5, 5, 14, 30, 16, 512, WSTAT, ("tile", 2, 1, 1, 0, 0), 221),
     _c("conv", 1, 3, 2, 14, 30, 64, 256, WSTAT, ("tile", 1, 1, 4, 0, 1), 222),
     _c("conv", 1, 3, 3, 14, 30, 64, 256, WSTAT, ("tile", 1, 1, 4, 0, 0), 223),
     _c("conv", 2, 1, 1, 21, 22, 64, 512, WSTAT, ("tile", 2, 1, 4, 0, 1), 224),
     _c("dgrad_pool", 2, 1, 1, 2, 2, 64, 256, WSTAT, ("tile", 1, 1, 4, 0, 1), 225, addend=True),
     _c("conv", 0, 1, 1, 40, 46, 64, 512, WSTAT, ("tile", 2, 2, 4, 0, 1), 226)] +
    # ---- conv3x3_win_kernel
    [_c("conv", m, 1, 1, 2, 2, 16, 48, WIN2, ("win", 2, 8, 1, 0, 0), 230 + m) for m in range(3)] +
    [_c("conv", 0, 3, 2, 9, 13, 32, 64, WIN2, ("win", 2, 8, 1, 0, 0), 240, tap=(33, None, False), next_pack=True),
     _c("conv", 1, 2, 2, 15, 17, 128, 64, WIN2, ("win", 2, 8, 1, 0, 0), 241),
     _c("conv", 2, 2, 1, 14, 30, 64, 64, WIN2, ("win", 2, 8, 1, 0, 0), 242)] +
    # ---- conv3x3_wink_kernel, one and two position tiles per wave
    [_c("conv", m, 1, 1, 2, 2, 32, 48, WINK2, ("wink", 2, 4, 2, 1, 0), 250 + m) for m in range(3)] +
    [_c("conv", 0, 2, 1, 9, 13, 64, 64, WINK2, ("wink", 2, 4, 2, 1, 0), 260, tap=(3, (0.5, 1.0, 2.0), False), next_pack=True),
     _c("conv", 1, 2, 2, 15, 17, 128, 64, WINK2, ("wink", 2, 4, 2, 1, 0), 261)] +
    [_c("conv", m, 4, 3, 44, 44, 32, 512, WINK2, ("wink", 2, 8, 2, 2, 0), 270 + m) for m in range(3)])


# ---- the fused pair launches (csrc/npp_conv_pair.hip) ----------------------------------------------------------------------------------
# forward: (cin, cmid, cout, H, W, N_total, n_run, seed); n_keep and the tap are swept by the GPU test.  The intermediate activation
# lives in LDS as fp16 and the pair's data gradient keeps its gated intermediate gradient as bf16: both must be exact integers too.
PAIR_FWD = [(16, 64, 64, H, W, 3, 2, 300 + i) for i, (H, W) in enumerate([(2, 2), (16, 16), (18, 34), (6, 50)])] + \
           [(64, 128, 128, H, W, 3, 2, 310 + i) for i, (H, W) in enumerate([(2, 2), (8, 16), (10, 18), (22, 6)])]
PAIR_DGRAD = [(H, W, 3, 2, 320 + i) for i, (H, W) in enumerate([(1, 1), (16, 16), (17, 33), (5, 40)])]       # (H, W, N_total, n_run, seed)
PATCH = dict(n_p=1, k=2, P=18, seed=330, scale=(0.5, 1.0, 2.0), shift=(1.0, 0.0, -1.0))


@functools.lru_cache(maxsize=None)
def pair_fwd_operands(case):
    """first block: a 3-channel integer image (through trunk_image_in) and weights in {-1, 0, 1}; second block: activations in
    {0..3}, conv a's weights nonzero with probability 1/4; conv b's weights nonzero with probability 1/4 (first) / 1/8 (second)"""
    cin, cmid, cout, H, W, N, n, seed = case
    rng = np.random.RandomState(seed)
    first = cin == 16
    o = dict(x=rng.randint(0, 4, (N, 3 if first else cin, H, W)).astype(np.float32),
             wa=_sparse_pm1(rng, (cmid, 3 if first else cin, 3, 3), 1.0 if first else 0.25).astype(np.float32),
             ba=rng.randint(-2, 3, cmid).astype(np.float32),
             wb=_sparse_pm1(rng, (cout, cmid, 3, 3), 0.25 if first else 0.125).astype(np.float32),
             bb=rng.randint(-4, 5, cout).astype(np.float32))
    if first:
        s, b = np.array(IMG_SCALE, np.float32)[None, :, None, None], np.array(IMG_SHIFT, np.float32)[None, :, None, None]
        o["img"] = (o["x"] - b) / s
    return o


def pair_fwd_reference_of(x, o):
    F = torch.nn.functional
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.float64)
    pa = F.conv2d(t(x), t(o["wa"]), t(o["ba"]), padding=1)
    ya = torch.relu(pa)
    pb = F.conv2d(ya, t(o["wb"]), t(o["bb"]), padding=1)
    yb = torch.relu(pb)
    bound = F.conv2d(F.conv2d(t(x).abs(), t(o["wa"]).abs(), t(o["ba"]).abs(), padding=1), t(o["wb"]).abs(), t(o["bb"]).abs(), padding=1)
    return dict(pre_a=pa.numpy(), ya=ya.numpy(), pre_b=pb.numpy(), yb=yb.numpy(), pool=F.max_pool2d(yb, 2, 2).numpy(), absmax_sum=float(bound.max()))


@functools.lru_cache(maxsize=None)
def pair_fwd_reference(case):
    o = pair_fwd_operands(case)
    return pair_fwd_reference_of(o["x"], o)


@functools.lru_cache(maxsize=None)
def pair_dgrad_operands(case):
    H, W, N, n, seed = case
    rng = np.random.RandomState(seed)
    return dict(dz=_sparse_pm1(rng, (N, 64, H, W), 0.5).astype(np.float32), wb=_sparse_pm1(rng, (64, 64, 3, 3), 0.75).astype(np.float32),
                ya=rng.choice((-1, 0, 1, 2, 1, 2, 3, 1), (N, 64, H, W)).astype(np.float32),
                wa=_sparse_pm1(rng, (64, 3, 3, 3), 0.75).astype(np.float32))


@functools.lru_cache(maxsize=None)
def pair_dgrad_reference(case):
    """conv b's data gradient -> gate by y_a > 0 -> conv a's data gradient -> times GRAD_SCALE[c]"""
    o = pair_dgrad_operands(case)
    F = torch.nn.functional
    t = lambda a: torch.from_numpy(a).to(torch.float64)
    d = F.conv_transpose2d(t(o["dz"]), t(o["wb"]), padding=1)
    mid = torch.where(t(o["ya"]) > 0, d, torch.zeros_like(d))
    img = F.conv_transpose2d(mid, t(o["wa"]), padding=1)
    bound = F.conv_transpose2d(F.conv_transpose2d(t(o["dz"]).abs(), t(o["wb"]).abs(), padding=1), t(o["wa"]).abs(), padding=1)
    return dict(mid=mid.numpy(), dimg=(img * torch.tensor(GRAD_SCALE, dtype=torch.float64)[None, :, None, None]).numpy(),
                absmax_sum=float(bound.max()) * max(GRAD_SCALE))


@functools.lru_cache(maxsize=None)
def patch_operands():
    """prediction rows and crops b / scale[c] with integer b, 0 / 1 masks of npp_conv_pair_fwd_patch, and the batch [x | y] they compose
    (NPP_completion/train.py:230-236: u = fake fm + pred (1 - fm), x = u rm, y = real rm), times scale plus shift"""
    n_p, k, P, rng = PATCH["n_p"], PATCH["k"], PATCH["P"], np.random.RandomState(PATCH["seed"])
    sc = np.array(PATCH["scale"], np.float32)               # values b / scale[c], b in {0..3}: the composed input b + shift[c] is an integer
    o = dict(pred=rng.randint(0, 4, (n_p * P * P, 3)).astype(np.float32) / sc[None, :],
             fake=rng.randint(0, 4, (n_p, 3, P, P)).astype(np.float32) / sc[None, :, None, None],
             fmask=rng.randint(0, 2, (n_p, 1, P, P)).astype(np.float32),
             real=rng.randint(0, 4, (n_p * k, 3, P, P)).astype(np.float32) / sc[None, :, None, None],
             rmask=rng.randint(0, 2, (n_p * k, 1, P, P)).astype(np.float32))
    pw = pair_fwd_operands((16, 64, 64, P, P, 2 * n_p * k, 2 * n_p * k, PATCH["seed"] + 1))
    o.update({key: pw[key] for key in ("wa", "ba", "wb", "bb")})
    return o


def patch_composed(o, comp):
    n_p, k, P = PATCH["n_p"], PATCH["k"], PATCH["P"]
    pv = o["pred"].reshape(n_p, P, P, 3).transpose(0, 3, 1, 2)
    u = o["fake"] * o["fmask"] + pv * (1 - o["fmask"]) if comp else pv
    x = np.repeat(u, k, axis=0) * o["rmask"]
    v = np.concatenate([x, o["real"] * o["rmask"]], 0)
    return v * np.array(PATCH["scale"], np.float32)[None, :, None, None] + np.array(PATCH["shift"], np.float32)[None, :, None, None]


if __name__ == "__main__":        # the search the table was drawn from: the cheapest shape of each (form, mode) within 8192 positions
    import itertools
    from npp_amd import ops
    from npp_amd._lib import NppError
    best = {}
    shapes = [(N, n, H, W) for N in (1, 2, 3, 4) for n in range(1, N + 1) for H in (2, 3, 5, 9, 14, 21, 30, 31, 40, 44, 62)
              for W in (2, 13, 14, 16, 18, 22, 30, 33, 46, 62) if run_range(n, H, W) <= 8192]
    for win, wink, wstat in itertools.product((0, 2), (0, 2), (0, 1)):
        for k, v in tune_of(win, wink, wstat).items():
            ops.tune(k, v)
        for (N, n, H, W), cin, cout, (mode, fold) in itertools.product(shapes, (16, 32, 64, 128, 512), (16, 32, 48, 96, 256, 512),
                                                                      ((0, 0), (1, 0), (2, 0), (0, 1), (2, 2))):
            try:
                p = ops.conv3x3_plan(N, n, H, W, cin, cout, mode, fold)
            except NppError:
                continue
            key = (p["family"], p["ct"], p["pt"], p["s"], p["npt"], p["wstat"], MODES[mode if not fold else 2 + fold])
            cost = run_range(n, H, W) * cin * cout
            if key not in best or cost < best[key][0]:
                best[key] = (cost, (N, n, H, W, cin, cout), (win, wink, wstat))
    for k in sorted(best):
        print(k, best[k][1:])
