"""Kernels that keep scratch between launches, driven at CHANGING problem shapes.

The deterministic paths keep state in device memory between launches: arrival counters that the last block re-arms, fixed-point
accumulators that the last arriver clears, partial-sum slabs, a block count left for the next launch.  The Python side caches that
scratch under keys that hold less than the full problem shape (stream only, or (device, C, stream), or a byte size), so one scratch
meets many shapes.  Every other test of these ops calls a given scratch at ONE shape; a kernel whose leftover state is only valid
for the shape that left it passes all of them (lpips_plain_kernel did: its counter sat at scratch[gridDim.x]).

One helper, `_sequence`, drives every case: a list of shapes A, B, A, C, A (B larger, C smaller than A: the grid grows, shrinks and
returns to a shape already seen), seeded inputs per step, the op on the project's cached / persistent scratch, and per step
  (a) the result against a plain float64 restatement of the operation's formula on the CPU (no HIP kernel takes part), and
  (b) bit equality with the same call on a freshly allocated scratch (zeroed; NaN-filled where the scratch is documented as needing
      no initial content) -- stale state shows here even where its effect would hide inside a tolerance.
Each case computes the op's block count from the formula in its launcher and the helper refuses a sequence in which consecutive
steps do not differ in it, so a sequence that stops changing the grid fails instead of passing vacuously.

Bounds of (a) are the ones the suite's existing test of the same op uses against its reference (named at each case).  Where an op
has none (robust_elem, light_wgrad), the bound is 4 x the distance of the SAME formula in float32 on the CPU from the float64 value,
on the test's own inputs, with a floor of 1e-6 relative: the kernels sum in block order, torch in its own."""
import math

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import npp_amd
    npp_amd.lib()          # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


# ---- the driver --------------------------------------------------------------------------------------------------------------
def _sequence(shapes, blocks, make, run, check, size=None, same_shape=False, unordered=None):
    """shapes: A, B, A, C, A (+ optional further steps).  blocks(shape): the op's block count(s), which must differ between
    consecutive steps.  make(shape, step) -> inputs; run(inputs, fresh) -> tuple of result tensors, fresh = on a newly allocated
    scratch instead of the cached one; check(inputs, got, step): assertion (a).  size(shape): B > A > C is asserted when given.
    same_shape: for a scratch whose contract is re-use at ONE shape -- the steps then differ in their data only.
    unordered: {output index: bound(inputs)} for a word that the op itself documents as a float sum in arrival order (no bits are
    promised for it in ANY two runs): |cached - fresh| <= bound takes the place of bit equality there, and only there."""
    counts = [blocks(s) for s in shapes]
    if same_shape:
        assert len(set(shapes)) == 1 and len(shapes) >= 3
    else:
        assert len(shapes) >= 5 and shapes[0] == shapes[2] == shapes[4] and shapes[1] != shapes[0] != shapes[3], shapes
        if size is not None:
            assert size(shapes[1]) > size(shapes[0]) > size(shapes[3]), shapes
        for a, b in zip(counts, counts[1:]):
            assert a != b, f"consecutive steps launch the same grid: {counts}"
    for step, shape in enumerate(shapes):
        inp = make(shape, step)
        got = run(inp, False)
        twin = run(inp, True)
        torch.cuda.synchronize()
        assert len(got) == len(twin)
        for k, (g, t) in enumerate(zip(got, twin)):
            if unordered and k in unordered:
                assert float((g - t).abs().max()) <= unordered[k](inp), f"step {step} shape {shape}: output {k}: {g} against {t} on a fresh scratch"
                continue
            assert torch.equal(g, t), f"step {step} shape {shape} (blocks {counts[step]}): output {k} differs from the fresh-scratch run"
        check(inp, got, step)


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _np(t):
    return t.detach().cpu().numpy()


def _measured_bound(v32, v64):
    """4 x the distance of the float32 CPU evaluation from the float64 one (relative L2), floor 1e-6."""
    return max(4.0 * rel_l2(_np(v32), _np(v64)), 1e-6)


def _nan_bytes(n, dev):
    return torch.full((int(n),), 255, dtype=torch.uint8, device=dev)          # 0xFF bytes: NaN as fp32, 4294967295 as a counter


# ---- float64 restatements ----------------------------------------------------------------------------------------------------
def _plain_head(f0, f1, lin):
    """lpips.py:99-133 with use_robust=False: normalize_tensor (eps 1e-10), squared difference, lin 1x1 conv, spatial mean, summed
    over the batch (tests/test_gpu_parity.py _lpips_plain_head_torch, in the dtype of its arguments)."""
    n0 = f0 / (f0.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    n1 = f1 / (f1.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    return ((n0 - n1).pow(2) * lin[None, :, None, None]).sum(1).mean((1, 2)).sum()


def _adaptive_nll(x, lat_alpha, lat_scale):
    """robust_loss_pytorch AdaptiveLossFunction.lossfun, elementwise, in the dtype of x (oracle.adaptive_params / robust_nll /
    _log_partition restated in torch so that autograd gives every gradient): alpha = sigmoid(l) (1.999 - 0.001) + 0.001, scale =
    (1 - 1e-5) softplus(l + log(e - 1)) + 1e-5, rho = beta / alpha ((x^2 / (c^2 beta) + 1)^(alpha / 2) - 1) with beta = |alpha - 2|,
    nll = rho + log c + log Z(alpha), log Z from the cubic Hermite spline table of the package (resources/partition_spline.npz).
    The last axis of x runs over the latents."""
    dt = x.dtype
    xs, vals, tans = oracle.load_partition_spline()
    vals, tans = torch.from_numpy(vals.astype(np.float64)).to(dt), torch.from_numpy(tans.astype(np.float64)).to(dt)
    alpha = torch.sigmoid(lat_alpha) * (1.999 - 0.001) + 0.001
    scale = (1.0 - 1e-5) * torch.nn.functional.softplus(lat_scale + math.log(math.expm1(1.0))) + 1e-5
    beta = (alpha - 2.0).abs().clamp_min(float(np.finfo(np.float32).eps))
    rho = (beta / alpha) * (((x / scale) ** 2 / beta + 1.0) ** (0.5 * alpha) - 1.0)
    xq = ((2.25 * alpha - 4.5) / ((alpha - 2.0).abs() + 0.25) + alpha + 2.0) * float(xs)
    n = vals.shape[0]
    lo = xq.detach().floor().clamp(0, n - 2).long()
    t = xq - lo.to(dt)
    assert bool(((t >= 0) & (t <= 1)).all())                  # alpha in (0.001, 1.999): inside the table
    t2, t3 = t * t, t * t * t
    h01 = -2.0 * t3 + 3.0 * t2
    h11 = t3 - t2
    logz = vals[lo] * (1.0 - h01) + vals[lo + 1] * h01 + tans[lo] * (h11 - t2 + t) + tans[lo + 1] * h11
    return rho + torch.log(scale) + logz


def _lpips_head(f0, f1, lin, lat, scale):
    """One tap of LPIPS.forward as ops.lpips_layer scales it: (scale / N) sum_n mean_pos sum_c lin_c term_c, term = the adaptive NLL
    of the normalised difference (lat = [latent_alpha (C) | latent_scale (C)]) or, lat None, its square."""
    N, Cc = f0.shape[:2]
    n0 = f0 / (f0.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    n1 = f1 / (f1.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    d = (n0 - n1).permute(0, 2, 3, 1)
    term = d.pow(2) if lat is None else _adaptive_nll(d, lat[:Cc], lat[Cc:])
    return (scale / N) * (term * lin).sum(-1).mean((1, 2)).sum()


def _pixel_loss(pred, gt, lat, weight):
    """img2mse(pred, gt, 'robust_loss_adaptive') (mse_calculator.py:13-27, no mask): weight x mean of the adaptive NLL over (N, 3)."""
    return weight * _adaptive_nll(pred - gt, lat[:3], lat[3:]).mean()


def _robust_elem(a, b, lat, coef):
    """ops.robust_elem: sum_n coef_n sum_j nll(a - b)[n][j] with latents per element j."""
    D = a.shape[1]
    return (coef[:, None] * _adaptive_nll(a - b, lat[:D], lat[D:])).sum()


def _cx_loss(x, y, band_width=0.5):
    """contextual_loss(x, y, band_width, loss_type='cosine') (functional.py:9-63), oracle.cx_loss_t: dtype-generic torch."""
    from oracle.npp_torch_oracle import cx_loss_t
    return cx_loss_t(x, y, band_width)


def _snake(z):
    return z + torch.sin(z) ** 2                               # activations.py:29-35, a = 1


# ---- case 1: ops.lpips_plain_layer on one scratch ---------------------------------------------------------------------------
def _plain_grid(shape):
    N, h, w = shape
    return min(256, (N * h * w + 15) // 16)                    # lpips_plain_go: one block per 16 positions, capped at 256


# per C: A, B, A, C, A.  Grids: 16 / 256 (capped, 512 groups) / 1 -- 3 (tail group, h != w) / 256 exactly / 1 (tail) -- 8 (tail,
# h != w) / 256 (capped, 300 groups) / 1
_PLAIN_SEQ = {64: [(1, 16, 16), (2, 64, 64), (1, 16, 16), (1, 4, 4), (1, 16, 16)],
              256: [(1, 5, 7), (1, 64, 64), (1, 5, 7), (1, 3, 3), (1, 5, 7)],
              512: [(2, 6, 10), (3, 40, 40), (2, 6, 10), (1, 2, 8), (2, 6, 10)]}


@pytest.mark.parametrize("C", [64, 256, 512])
def test_plain_lpips_head_on_one_scratch_at_changing_shapes(dev, C):
    """ops.lpips_plain_layer(..., scratch=ws), the deterministic head that LPIPS.plain launches, on ONE scratch: value against float64
    (rtol 3e-5, the bound of test_lpips_plain_vs_reference), bits against a fresh zeroed scratch, and the scratch-less atomic form
    against float64 within the same bound.  Grids of 1, a few, exactly 256 and capped at 256; tail groups (N h w not a multiple of
    16) and h != w included."""
    from npp_amd import ops
    shapes = _PLAIN_SEQ[C]
    every = [s for seq in _PLAIN_SEQ.values() for s in seq]
    npos = lambda s: s[0] * s[1] * s[2]                          # noqa: E731
    assert {1, 256} <= {_plain_grid(s) for s in shapes} and any(1 < _plain_grid(s) < 256 for s in shapes)
    assert any(npos(s) == 16 * 256 for s in every) and any(npos(s) > 16 * 256 for s in every)          # exactly the cap, and beyond it
    assert any(npos(s) % 16 for s in every) and any(s[1] != s[2] for s in every)                       # a tail group, h != w
    ws = torch.zeros(ops.LPIPS_PLAIN_SCRATCH, dtype=torch.float32, device=dev)

    def make(shape, step):
        N, h, w = shape
        g = torch.Generator().manual_seed(1000 * C + step)
        return dict(f0=torch.rand(N, C, h, w, generator=g), f1=torch.rand(N, C, h, w, generator=g), lin=torch.rand(C, generator=g) * 0.1)

    def run(inp, fresh):
        out = torch.zeros(1, device=dev)
        s = torch.zeros(ops.LPIPS_PLAIN_SCRATCH, dtype=torch.float32, device=dev) if fresh else ws
        ops.lpips_plain_layer(inp["f0"].to(dev), inp["f1"].to(dev), inp["lin"].to(dev), 1.5, out, scratch=s)
        return (out,)

    def check(inp, got, step):
        ref = 1.5 * float(_plain_head(inp["f0"].double(), inp["f1"].double(), inp["lin"].double()))
        atomic = torch.zeros(1, device=dev)
        ops.lpips_plain_layer(inp["f0"].to(dev), inp["f1"].to(dev), inp["lin"].to(dev), 1.5, atomic)
        print(f"plain C={C} step {step} {tuple(inp['f0'].shape)}: det {got[0].item():.9g} atomic {atomic.item():.9g} fp64 {ref:.9g}")
        np.testing.assert_allclose(got[0].item(), ref, rtol=3e-5)
        np.testing.assert_allclose(atomic.item(), ref, rtol=3e-5)
    _sequence(shapes, _plain_grid, make, run, check, size=lambda s: s[0] * s[1] * s[2])


# ---- case 2: LPIPS.plain on one instance ------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2])
def test_lpips_plain_score_on_one_instance_at_changing_image_sizes(dev, N):
    """LPIPS.plain (the candidate score, ops.DETERMINISTIC default) on ONE instance at 64^2, 128^2, 64^2, 96 x 160, 64^2: the per-tap
    scratches are cached per stream only.  The first and every later 64^2 score are the same bits (same inputs); every score has the
    bits of a fresh zeroed scratch, agrees with the atomic form (ops.DETERMINISTIC = False) and with the float64 head formula on the
    trunk's own features (hip_trunk._forward's taps fetched to the host: the trunk is not under test), rtol 3e-5 (the bound of
    test_lpips_plain_vs_reference).
    Before the counter moved to a fixed slot, the third call lost the terms of taps 1..4: the 128^2 call had left float bits where
    the 64^2 grids keep their counters.  Tap 0 launches 256 blocks at every size here (capped); the precondition is on taps 1..4."""
    from npp_amd import ops
    from npp_amd.losses import LPIPS
    m = LPIPS(device=dev)
    sizes = [(64, 64), (128, 128), (64, 64), (96, 160), (64, 64)]
    grids = lambda s: tuple(min(256, (N * (s[0] >> k) * (s[1] >> k) + 15) // 16) for k in range(1, 5))      # noqa: E731
    for a, b in zip(sizes, sizes[1:]):
        assert all(x != y for x, y in zip(grids(a), grids(b))), (grids(a), grids(b))
    seen = {}
    feats = []
    real_forward = m.hip_trunk._forward

    def spy(*a, **k):
        out = real_forward(*a, **k)
        feats[:] = [f.detach().cpu().double() for f in out]
        return out
    m.hip_trunk._forward = spy

    def make(shape, step):
        g = torch.Generator().manual_seed(7 * shape[0] + shape[1] + 100 * N)            # per SHAPE: the 64^2 steps repeat their inputs
        return dict(a=torch.rand(N, 3, *shape, generator=g).to(dev), b=torch.rand(N, 3, *shape, generator=g).to(dev), shape=shape)

    def run(inp, fresh):
        keep = dict(m._plain_ws) if hasattr(m, "_plain_ws") else None
        if fresh and keep is not None:
            m._plain_ws.clear()                                  # LPIPS.plain allocates a zeroed scratch for the stream
        try:
            out = m.plain(inp["a"], inp["b"]).clone()
        finally:
            if fresh and keep is not None:
                m._plain_ws.clear()
                m._plain_ws.update(keep)
        return (out,)

    def check(inp, got, step):
        v = got[0].item()                                        # (feats: the taps of the last call, these inputs)
        ref = sum(float(_plain_head(f[:N], f[N:], lin.detach().cpu().double())) for f, lin in zip(feats, m.lins))
        ops.DETERMINISTIC = False
        try:
            atomic = m.plain(inp["a"], inp["b"]).item()
        finally:
            ops.DETERMINISTIC = True
        first = seen.setdefault(inp["shape"], v)
        print(f"LPIPS.plain N={N} step {step} {inp['shape']}: det {v:.9g} first-at-this-size {first:.9g} atomic {atomic:.9g} fp64 {ref:.9g}")
        assert v == first, f"step {step}: {v!r} != {first!r}, the first score at {inp['shape']}"
        np.testing.assert_allclose(v, atomic, rtol=3e-5)
        np.testing.assert_allclose(v, ref, rtol=3e-5)
    assert ops.DETERMINISTIC
    _sequence(sizes, grids, make, run, check)


# ---- case 3: ops.lpips_layer / ops.lpips_layers ------------------------------------------------------------------------------
def _lp_blocks(N, C, hw):
    """T.nb of lp_fill (csrc/npp_lpips.hip): groups of 4 positions for small deep taps, else 16; at most 192 blocks, evenly loaded."""
    nh = N * hw
    pl = 4 if (nh <= 2048 and C % 64 == 0) else 16
    groups = (nh + pl - 1) // pl
    per = (groups + 191) // 192
    return (groups + per - 1) // per


def _lp_check(tag, loss, df0, dlat, f0, f1, lin, lat, scale):
    """loss / df0 / dlatent of one tap against float64 autograd.  Bounds: plain head rtol 2e-5 on the value and 2e-5 relative L2 on
    the gradient (test_lpips_plain_head_with_gradient); adaptive head 5e-5 / 2e-3 relative L2 / rtol 1e-2 atol 2e-6 (d alpha) / rtol
    2e-3 atol 2e-7 (d scale) (test_lpips_head_golden)."""
    Cc = f0.shape[1]
    x = f0.double().requires_grad_(True)
    l64 = None if lat is None else lat.double().requires_grad_(True)
    ref = _lpips_head(x, f1.double(), lin.double(), l64, scale)
    ref.backward()
    e_df = rel_l2(_np(df0), _np(x.grad))
    print(f"{tag}: loss {loss:.9g} fp64 {ref.item():.9g} df0 relL2 {e_df:.3g}")
    if lat is None:
        np.testing.assert_allclose(loss, ref.item(), rtol=2e-5)
        assert e_df < 2e-5, e_df
        return
    np.testing.assert_allclose(loss, ref.item(), rtol=5e-5)
    assert e_df < 2e-3, e_df
    np.testing.assert_allclose(_np(dlat)[:Cc], _np(l64.grad)[:Cc], rtol=1e-2, atol=2e-6)
    np.testing.assert_allclose(_np(dlat)[Cc:], _np(l64.grad)[Cc:], rtol=2e-3, atol=2e-7)


@pytest.mark.parametrize("side", [False, True], ids=["default_stream", "side_stream"])
@pytest.mark.parametrize("robust", [True, False], ids=["adaptive", "plain"])
def test_lpips_layer_workspace_at_changing_shapes(dev, robust, side):
    """ops.lpips_layer: the workspace (2 C + 1 fixed-point accumulators + the arrival counter, cleared by the last arriver) is cached
    per (device, C, stream): C = 64 and the stream stay, N and h w change (72 / 150 / 4 blocks, both position-group widths).  Loss,
    df0 and dlatent against float64 autograd; bits against freshly zeroed workspaces (ops._lp_ws emptied for the twin run, then put
    back).  Once on the default stream and once on a side stream, whose workspace is its own."""
    from npp_amd import ops
    C = 64
    shapes = [(2, 12, 12), (3, 40, 40), (2, 12, 12), (1, 4, 4), (2, 12, 12)]
    spline, n_knots, xs = ops.load_spline(dev)
    stream = torch.cuda.Stream(device=dev) if side else torch.cuda.current_stream(dev)
    assert ops.DETERMINISTIC

    def make(shape, step):
        N, h, w = shape
        g = torch.Generator().manual_seed(31 * step + 5)
        return dict(f0=torch.rand(N, C, h, w, generator=g), f1=torch.rand(N, C, h, w, generator=g), lin=torch.rand(C, generator=g) * 0.1,
                    lat=torch.cat([torch.randn(C, generator=g) * 0.5, torch.randn(C, generator=g) * 0.3]) if robust else None)

    def run(inp, fresh):
        keep = dict(ops._lp_ws)
        if fresh:
            ops._lp_ws.clear()
        try:
            with torch.cuda.stream(stream):
                f0, f1, lin = inp["f0"].to(dev), inp["f1"].to(dev), inp["lin"].to(dev)
                lat = inp["lat"].to(dev) if robust else None
                loss, df0 = torch.zeros(1, device=dev), torch.empty_like(f0)
                dlat = torch.zeros_like(lat) if robust else None
                ops.lpips_layer(f0, f1, lin, lat, spline, n_knots, xs, 0.7, loss, df0, dlat)
                assert (f0.device, C, ops._stream().value) in ops._lp_ws
            stream.synchronize()
        finally:
            if fresh:
                ops._lp_ws.clear()
                ops._lp_ws.update(keep)
        return (loss, df0) + ((dlat,) if robust else ())

    def check(inp, got, step):
        _lp_check(f"lpips_layer {'adaptive' if robust else 'plain'} step {step} {tuple(inp['f0'].shape)}", got[0].item(), got[1],
                  got[2] if robust else None, inp["f0"], inp["f1"], inp["lin"], inp["lat"], 0.7)
    _sequence(shapes, lambda s: _lp_blocks(s[0], C, s[1] * s[2]), make, run, check, size=lambda s: s[0] * s[1] * s[2])


_CHNS = (64, 128, 256, 512, 512)


@pytest.mark.parametrize("side", [False, True], ids=["default_stream", "side_stream"])
@pytest.mark.parametrize("robust", [True, False], ids=["adaptive", "plain"])
def test_lpips_layers_workspaces_at_changing_shapes(dev, robust, side):
    """ops.lpips_layers (five VGG16-shaped taps in one launch, a workspace per (device, C, stream, tap)): N and the image size change,
    every tap's block count with them; per tap df0 and dlatent and the loss word against float64 autograd, bits of every df0 and
    dlatent against fresh workspaces.
    The loss WORD of this launch is the one output without promised bits: each tap's last block adds its (order-independent,
    fixed-point) term to it with a float atomicAdd, so the five terms meet in arrival order ("the REPORTED loss
    word ... in arrival order ... no gradient reads it"; test_lpips_heads_in_one_launch_equal_the_five_launches allows 1e-6 for the
    same reason).  Two orders of five float additions differ by at most 2 x 4 roundings of half an ulp of a partial sum, and no
    partial sum exceeds sum_k |term_k|: the cached and the fresh run may differ by 8 x 2^-24 x sum_k |term_k| (terms from the
    float64 restatement), about a part in 2e6 -- a term lost to stale state is a million times that."""
    from npp_amd import ops
    shapes = [(2, 32), (3, 48), (2, 32), (1, 16), (2, 32)]                     # (N, side of tap 0); tap k is side >> k
    spline, n_knots, xs = ops.load_spline(dev)
    stream = torch.cuda.Stream(device=dev) if side else torch.cuda.current_stream(dev)

    def blocks(s):
        return tuple(_lp_blocks(s[0], c, (s[1] >> k) ** 2) for k, c in enumerate(_CHNS))
    for a, b in zip(shapes, shapes[1:]):
        assert all(x != y for x, y in zip(blocks(a), blocks(b))), (blocks(a), blocks(b))       # EVERY tap's grid changes

    def make(shape, step):
        N, h = shape
        g = torch.Generator().manual_seed(77 * step + 3)
        r = lambda c, k: torch.rand(N, c, h >> k, h >> k, generator=g)       # noqa: E731
        return dict(f0=[r(c, k) for k, c in enumerate(_CHNS)], f1=[r(c, k) for k, c in enumerate(_CHNS)],
                    lin=[torch.rand(c, generator=g) * 0.1 for c in _CHNS],
                    lat=[torch.cat([torch.randn(c, generator=g) * 0.5, torch.randn(c, generator=g) * 0.3]) for c in _CHNS] if robust else None)

    def run(inp, fresh):
        keep = dict(ops._lp_ws)
        if fresh:
            ops._lp_ws.clear()
        try:
            with torch.cuda.stream(stream):
                f0, f1, lin = ([t.to(dev) for t in inp[k]] for k in ("f0", "f1", "lin"))
                lat = [t.to(dev) for t in inp["lat"]] if robust else None
                loss, df0 = torch.zeros(1, device=dev), [torch.empty_like(t) for t in f0]
                dlat = [torch.zeros_like(t) for t in lat] if robust else None
                ops.lpips_layers(f0, f1, lin, lat, spline, n_knots, xs, 0.7, loss, df0, dlat)
            stream.synchronize()
        finally:
            if fresh:
                ops._lp_ws.clear()
                ops._lp_ws.update(keep)
        return (loss,) + tuple(df0) + (tuple(dlat) if robust else ())

    def check(inp, got, step):
        total = 0.0
        for k in range(5):
            x = inp["f0"][k].double().requires_grad_(True)
            l64 = inp["lat"][k].double().requires_grad_(True) if robust else None
            ref = _lpips_head(x, inp["f1"][k].double(), inp["lin"][k].double(), l64, 0.7)
            ref.backward()
            total += ref.item()
            e = rel_l2(_np(got[1 + k]), _np(x.grad))
            print(f"lpips_layers {'adaptive' if robust else 'plain'} step {step} tap {k}: df0 relL2 {e:.3g}")
            assert e < (2e-3 if robust else 2e-5), (k, e)
            if robust:
                c = _CHNS[k]
                np.testing.assert_allclose(_np(got[6 + k])[:c], _np(l64.grad)[:c], rtol=1e-2, atol=2e-6)
                np.testing.assert_allclose(_np(got[6 + k])[c:], _np(l64.grad)[c:], rtol=2e-3, atol=2e-7)
        print(f"lpips_layers step {step}: loss {got[0].item():.9g} fp64 {total:.9g}")
        np.testing.assert_allclose(got[0].item(), total, rtol=5e-5 if robust else 2e-5)
    def word_bound(inp):
        terms = [_lpips_head(inp["f0"][k].double(), inp["f1"][k].double(), inp["lin"][k].double(), inp["lat"][k].double() if robust else None, 0.7)
                 for k in range(5)]
        return 8.0 * 2.0 ** -24 * sum(abs(float(t)) for t in terms)
    _sequence(shapes, blocks, make, run, check, size=lambda s: s[0] * s[1] * s[1], unordered={0: word_bound})


# ---- case 4: ops.robust_elem -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4096, 1000])
def test_robust_elem_workspace_at_changing_sample_counts(dev, D):
    """ops.robust_elem: the workspace (per-block partial loss sums + the arrival ticket, which the launcher clears) is cached per
    (device, D, stream); D stays, N = 2, 4, 2, 1, 2.  Its grid is ceil(D / 256) blocks whatever N is (one thread per element walks the
    N samples), so with the cache key holding D no sequence can change the grid on one workspace: the precondition here is on N, the
    part of the shape the key does not hold, and the (constant) block count is asserted to be what the launcher documents.
    Loss, d loss / d a and the latent gradients against float64 autograd; bits against a NaN-filled workspace (documented as needing
    no initial content).
    Bound (no earlier test compares this op with a reference at op level): 4 x the relative L2 distance of the float32 CPU evaluation
    of the same formula from the float64 one on the step's inputs, floor 1e-6.  Measured on these inputs (CPU, the ten steps of the
    two parameters): loss 6e-9 .. 8e-8 and d a 1e-7 -> the floor, 1e-6; latent gradients 5e-5 .. 9e-5 (float32 autograd through the
    spline and the power loses that much to cancellation) -> 2e-4 .. 3.5e-4."""
    from npp_amd import ops
    from npp_amd._lib import lib
    spline, n_knots, xs = ops.load_spline(dev)
    nbytes = int(lib().npp_robust_elem_workspace_bytes(D))
    blocks = (D + 255) // 256
    assert nbytes == 4 * (blocks + 16)                           # [blocks] partial sums + the ticket: the documented layout
    shapes = [2, 4, 2, 1, 2]

    def make(N, step):
        g = torch.Generator().manual_seed(13 * step + D)
        return dict(a=torch.randn(N, D, generator=g) * 0.5, b=torch.randn(N, D, generator=g) * 0.5,
                    lat=torch.cat([torch.randn(D, generator=g) * 0.5, torch.randn(D, generator=g) * 0.3]),
                    coef=(0.5 + torch.rand(N, generator=g)) / (N * D))

    def run(inp, fresh):
        key = (dev, D, ops._stream().value)
        keep = ops._re_ws.get(key)
        if fresh:
            ops._re_ws[key] = _nan_bytes(nbytes, dev)
        try:
            loss, dlat = torch.zeros(1, device=dev), torch.zeros(2 * D, device=dev)
            dd = ops.robust_elem(inp["a"].to(dev), inp["b"].to(dev), inp["lat"].to(dev), spline, n_knots, xs, inp["coef"].tolist(), loss, True, dlat)
            assert key in ops._re_ws
            torch.cuda.synchronize()
        finally:
            if fresh:
                if keep is None:
                    del ops._re_ws[key]
                else:
                    ops._re_ws[key] = keep
        return loss, dd, dlat

    def check(inp, got, step):
        outs = {}
        for dt in (torch.float64, torch.float32):
            a, lat = inp["a"].to(dt).requires_grad_(True), inp["lat"].to(dt).requires_grad_(True)
            v = _robust_elem(a, inp["b"].to(dt), lat, inp["coef"].to(dt))
            v.backward()
            outs[dt] = (v.detach().reshape(1), a.grad, lat.grad)
        for name, g, r64, r32 in zip(("loss", "dd", "dlatent"), got, outs[torch.float64], outs[torch.float32]):
            bound, err = _measured_bound(r32, r64), rel_l2(_np(g), _np(r64))
            print(f"robust_elem D={D} N={inp['a'].shape[0]} step {step} {name}: fp32-CPU distance {rel_l2(_np(r32), _np(r64)):.3g} bound {bound:.3g} kernel {err:.3g}")
            assert err <= bound, (name, step, err, bound)
    # (the grid cannot change here -- see the docstring: the helper's precondition is given N)
    _sequence(shapes, lambda N: N, make, run, check, size=lambda N: N)


# ---- case 5: the contextual core ---------------------------------------------------------------------------------------------
def _cx_blocks(s):
    N, C, h, w = s
    hw = h * w
    tiles = (hw + 63) // 64
    return ((N * tiles * tiles + 7) // 8 * 8, (N * hw + 3) // 4)          # cx_sim_kernel, cx_rows_bwd_kernel (cx_launch)


_CX_SEQ = [(2, 32, 8, 8), (2, 64, 10, 12), (2, 32, 8, 8), (1, 32, 4, 6), (2, 32, 8, 8)]      # h w = 64 (LDS-free forms), 120 (generic), 24


def _cx_inputs(shape, step):
    rng = np.random.RandomState(100 + step)
    y = np.maximum(rng.randn(*shape), 0).astype(np.float32)
    x = np.maximum(0.7 * y + 0.7 * rng.randn(*shape), 0).astype(np.float32)
    return dict(x=torch.from_numpy(x), y=torch.from_numpy(y))


def _cx_ref(inp):
    x = inp["x"].double().requires_grad_(True)
    ref = _cx_loss(x, inp["y"].double())
    ref.backward()
    return ref.item(), x.grad


def test_cx_workspaces_of_equal_size_do_not_exist_among_small_shapes():
    """The contextual core's workspace is cached by BYTE SIZE: two shapes of equal size would share one (matrices, tickets).  Among
    the 528 shapes N = 1..4, C in {32, 64}, 2 <= h <= w <= 12 no two with different (N, C, h w) have the same npp_cx_workspace_bytes
    (the size is 4 (24 (C + 16) + (7 + C / 32) N hw + 3 N + 2 N hw^2 + 160)); shapes of equal (N, C, h w) are one problem to the
    kernels.  The sequences below therefore alternate workspaces of different sizes; this check keeps that statement honest."""
    import npp_amd  # noqa: F401
    from npp_amd._lib import lib
    seen, n = {}, 0
    for C in (32, 64):
        for N in range(1, 5):
            for h in range(2, 13):
                for w in range(h, 13):
                    n += 1
                    seen.setdefault(int(lib().npp_cx_workspace_bytes(N, C, h * w)), set()).add((N, C, h * w))
    assert n == 528 and all(len(v) == 1 for v in seen.values()), [v for v in seen.values() if len(v) > 1]


@pytest.mark.parametrize("want_grad", [True, False], ids=["with_gradient", "value_only"])
def test_cx_core_workspace_at_changing_shapes(dev, want_grad):
    """ops.cx_fwd_bwd on the cached workspaces (ops._cx_ws, keyed by device, byte size and stream; tickets cleared by the first
    launch of the call) with (N, C, h, w) alternating between the LDS-free forms (h w a multiple of 32) and the generic ones: loss
    and dL/dx against the float64 contextual loss with autograd (1e-3 relative / 1e-2 relative L2, the bounds of
    test_cx_core_realistic_size), bits against NaN-filled workspaces (documented as needing no initial content)."""
    from npp_amd import ops
    from npp_amd._lib import lib

    def run(inp, fresh):
        keep = dict(ops._cx_ws)
        N, C, h, w = inp["x"].shape
        if fresh:
            nb = int(lib().npp_cx_workspace_bytes(N, C, h * w))
            ops._cx_ws.clear()
            ops._cx_ws[(dev, nb, ops._stream().value)] = _nan_bytes(nb, dev)
        try:
            loss, dx = ops.cx_fwd_bwd(inp["x"].to(dev), inp["y"].to(dev), want_grad=want_grad)
            torch.cuda.synchronize()
        finally:
            if fresh:
                assert len(ops._cx_ws) == 1                      # (the poisoned workspace was the one used)
                ops._cx_ws.clear()
                ops._cx_ws.update(keep)
        return (loss, dx) if want_grad else (loss,)

    def check(inp, got, step):
        ref, dref = _cx_ref(inp)
        e = rel_l2(_np(got[1]), _np(dref)) if want_grad else 0.0
        print(f"cx_fwd_bwd step {step} {tuple(inp['x'].shape)}: loss {got[0].item():.9g} fp64 {ref:.9g} dx relL2 {e:.3g}")
        assert abs(got[0].item() - ref) < 1e-3 * abs(ref)
        assert e < 1e-2
    _sequence(_CX_SEQ, _cx_blocks, _cx_inputs, run, check, size=lambda s: s[0] * s[1] * s[2] * s[3])


def test_cx_core_flat_output_workspaces_at_changing_shapes(dev):
    """ops.cx_fwd_bwd_flat (dL/dx written into the trunk's flat bf16 gradient tensor, gated by [yact > 0]; a second cached scratch
    keyed by element count holds the un-normalised contraction): same sequence.  The exported gradient against float64 autograd
    times the gate, 1e-2 relative L2 (test_cx_core_realistic_size; one bf16 rounding per element, 2^-9, is inside it); bits against
    NaN-filled workspaces."""
    from npp_amd import ops
    from npp_amd._lib import lib

    def run(inp, fresh):
        keep = dict(ops._cx_ws)
        N, C, h, w = inp["x"].shape
        st = ops._stream().value
        if fresh:
            nb = int(lib().npp_cx_workspace_bytes(N, C, h * w))
            ops._cx_ws.clear()
            ops._cx_ws[(dev, nb, st)] = _nan_bytes(nb, dev)
            ops._cx_ws[(dev, "dxh", N * C * h * w, st)] = _nan_bytes(4 * N * C * h * w, dev).view(torch.float32)
        try:
            x = inp["x"].to(dev)
            yact, dz = ops.trunk_alloc(N, C, h, w, dev), ops.trunk_alloc(N, C, h, w, dev)
            ops.trunk_grad_in(x, None, N, N, C, h, w, yact, as_f16=True)         # the tapped layer's output = the features themselves
            loss = torch.zeros(1, device=dev)
            ops.cx_fwd_bwd_flat(x, inp["y"].to(dev), yact, dz, N, 0.5, 1.0, loss)
            out = ops.trunk_export(dz, N, N, C, h, w)
            torch.cuda.synchronize()
        finally:
            if fresh:
                assert len(ops._cx_ws) == 2
                ops._cx_ws.clear()
                ops._cx_ws.update(keep)
        return loss, out

    def check(inp, got, step):
        ref, dref = _cx_ref(inp)
        gate = (inp["x"].to(torch.float16) > 0).double()
        e = rel_l2(_np(got[1]), _np(dref * gate))
        print(f"cx_fwd_bwd_flat step {step} {tuple(inp['x'].shape)}: loss {got[0].item():.9g} fp64 {ref:.9g} dz relL2 {e:.3g}")
        assert abs(got[0].item() - ref) < 1e-3 * abs(ref)
        assert e < 1e-2
    _sequence(_CX_SEQ, _cx_blocks, _cx_inputs, run, check, size=lambda s: s[0] * s[1] * s[2] * s[3])


# ---- case 6: pixel-loss block partials consumed by the Adam tail --------------------------------------------------------------
def test_pixel_loss_partials_into_the_adam_tail_at_changing_row_counts(dev):
    """The folded iteration: the patch-in launch carries the adaptive pixel loss and leaves [block][8] partial sums plus the block
    count in NPPNet._pl_scratch; the fused Adam launch adds them in block order to the loss word and the latent gradients.  One net,
    one scratch, n_rows = 2048, 26 624, 2048, 256, 2048 (8, 104, 8, 1, 8 blocks), then the rest of 26 624, 256, 2048, 26 624.
    A whole training step per call (forward, patch-in + loss launch, backward chain, weight gradients, Adam + re-pack).
    Checked against the float64 restatement of the robust pixel loss on the step's own predictions: the loss word (rtol 2e-5),
    dL/dpred (rtol 2e-4, atol 1e-8) and the latent gradient as the Adam tail consumed it -- the latents' first moment is cleared
    before the step, so it leaves as (1 - beta1) g -- (d alpha rtol 3e-3 atol 3e-6, d scale rtol 2e-4 atol 1e-7): the bounds of
    test_pixel_loss_golden.  Bits: a twin net taking the same steps whose _pl_scratch is a freshly zeroed tensor at every step."""
    from npp_amd import ops
    from npp_amd.model import NPPNet
    H, Bp, P = 256, 26624, 32
    angles, periods, _ = oracle.synthetic_periodicity(H, 1)
    mk = lambda: NPPNet(angles, periods, oracle.SEED0_FREQS, (H, H), params=oracle.init_params(1, seed=0), device=dev)      # noqa: E731
    nets = {False: mk(), True: mk()}
    assert ops.DETERMINISTIC and nets[False].fused_repack
    shapes = [2048, 26624, 2048, 256, 2048, 26624, 256, 2048, 26624]
    blocks = lambda n: min(1024, (n + 255) // 256)               # noqa: E731  pixel_loss_blocks (csrc/npp_robust.h)
    assert [blocks(n) for n in shapes[:5]] == [8, 104, 8, 1, 8]
    sc, sh = [1 / 0.229, 1 / 0.224, 1 / 0.225], [-0.485 / 0.229, -0.456 / 0.224, -0.406 / 0.225]
    beta1 = float(np.float32(1.0) - np.float32(0.9))             # the kernel's (1.0f - b1)

    def make(n_rows, step):
        g = torch.Generator().manual_seed(900 + step)
        return dict(n=n_rows, coords=torch.randint(0, H, (Bp, 2), generator=g, dtype=torch.int32), gt=torch.rand(n_rows, 3, generator=g),
                    prow=torch.rand(P * P, 3, generator=g), real=torch.rand(1, 3, P, P, generator=g),
                    lat=torch.cat([torch.randn(3, generator=g) * 0.5, torch.randn(3, generator=g) * 0.3]))

    def run(inp, fresh):
        net, n = nets[fresh], inp["n"]
        if fresh and getattr(net, "_pl_scratch", None) is not None:
            net._pl_scratch = torch.zeros(ops.PIXEL_LOSS_SCRATCH, dtype=torch.float32, device=dev)
        net.latents.copy_(inp["lat"].to(dev))                    # (latents away from their initial value: every gradient term is live)
        net.lat_m.zero_()
        net.lat_v.zero_()
        net.zero_grad(force=True)
        net.forward_train(inp["coords"].to(dev))
        ws = net.workspace(Bp)
        ws["dpred"].zero_()
        args = net.pixel_loss_args(Bp, n, inp["gt"].to(dev))
        assert args[11] is net._pl_scratch and args[11] is not None
        x0 = ops.trunk_alloc(2, 16, P, P, dev)
        ops.trunk_patch_in(inp["prow"].to(dev), None, None, inp["real"].to(dev), torch.ones(1, 1, P, P, device=dev), 1, 1, P, False, sc, sh, x0,
                           loss=args)
        pred, dpred = ws["pred"][:n].clone(), ws["dpred"][:n].clone()
        assert float(net.loss_buf[0]) == 0.0 and float(net.dlatent.abs().max()) == 0.0      # the sums wait in the scratch
        net.backward(Bp)
        net.optimizer_step(Bp)
        torch.cuda.synchronize()
        return net.loss_buf.clone(), net.lat_m.clone(), net.latents.clone(), dpred, pred, net.params.clone()

    def check(inp, got, step):
        loss, lat_m, _, dpred, pred = (t.cpu() for t in got[:5])
        p64, l64 = pred.double().requires_grad_(True), inp["lat"].double().requires_grad_(True)
        ref = _pixel_loss(p64, inp["gt"].double(), l64, 1.0)
        ref.backward()
        g = lat_m.double().numpy() / beta1
        print(f"pixel loss n_rows={inp['n']} step {step}: loss {loss.item():.9g} fp64 {ref.item():.9g}; dlatent {g} fp64 {_np(l64.grad)}")
        np.testing.assert_allclose(loss.item(), ref.item(), rtol=2e-5)
        np.testing.assert_allclose(_np(dpred), _np(p64.grad), rtol=2e-4, atol=1e-8)
        np.testing.assert_allclose(g[:3], _np(l64.grad)[:3], rtol=3e-3, atol=3e-6)
        np.testing.assert_allclose(g[3:], _np(l64.grad)[3:], rtol=2e-4, atol=1e-7)
    _sequence(shapes, blocks, make, run, check, size=lambda n: n)


# ---- case 7: ops.light_wgrad on one scratch (same-shape re-use: the contract) -------------------------------------------------
@pytest.mark.parametrize("C,B", [(1, 1024), (9, 2048)])
def test_light_wgrad_det_scratch_reused_at_one_shape(dev, C, B):
    """ops.light_wgrad(..., scratch=ws): tickets that reset themselves + partial tiles; the contract is re-use at the SAME (C, B)
    (NPPNetLightBatch keeps one per workspace), and exactly that is driven: three launches with different data on one scratch, each
    against float64 dW_l = dz_l^T x_l, db_l = sum_rows dz_l for the seven layers (x_0 = x_per, x_l = snake(z_{l-1}), x_f1 = snake(z_3),
    x_pos = [f1 | x_pos | 0], x_rgb = snake(z_p): csrc/npp_light_layout.h) and for bit equality with a freshly zeroed scratch.
    Bound (no earlier test compares this op with a reference at op level): 4 x the relative L2 distance of the float32 CPU
    evaluation from the float64 one per layer, floor 1e-6.  Measured on these inputs (CPU, three launches x seven layers): dW 1.5e-7 ..
    3.5e-7 -> 1e-6 .. 1.4e-6; db 6.5e-8 .. 1.7e-7 -> the floor, 1e-6."""
    from npp_amd import ops
    from npp_amd.light import NPPNetLightBatch, default_light_init
    rng = np.random.RandomState(5)
    cands = [(np.array([10.0 * i, 90.0 + 5.0 * i], np.float32), np.array([9.0 + i, 14.0 - i], np.float32)) for i in range(C)]
    batch = NPPNetLightBatch(cands, (rng.randn(10) * 10).astype(np.float32), (64, 64), default_light_init(256, 4), device=dev)
    assert batch.fused
    d, sr, dr = batch._desc, batch._srow, batch._drow
    dz_row = [dr[0], dr[1], dr[2], dr[3], dr[5], dr[4], dr[6]]                # npp_light_desc order: periodic 0..3, pos, f1, rgb
    x_row = [sr[6], sr[0], sr[1], sr[2], sr[4], sr[3], sr[5]]
    x_snake = [0, 1, 1, 1, 0, 1, 1]
    ws = ops.light_wgrad_det_scratch(C, B, dev)

    def make(shape, step):
        g = torch.Generator().manual_seed(50 * step + C)
        S = torch.randn(C, sr[7], B, generator=g) * 0.8
        S[:, sr[4] + 256 + 42:sr[5]] = 0.0                                    # the 0-pad rows of [f1 | x_pos | 0]
        return dict(S=S, D=torch.randn(C, dr[7], B, generator=g) * 0.1)

    def run(inp, fresh):
        grad = torch.zeros_like(batch.grad)
        ops.light_wgrad(d, inp["S"].to(dev), inp["D"].to(dev), grad, scratch=ops.light_wgrad_det_scratch(C, B, dev) if fresh else ws)
        return (grad,)

    def ref(inp, dt, i):
        n_out, ld = d.n_out[i], d.ld[i]
        dz = inp["D"][:, dz_row[i]:dz_row[i] + n_out].to(dt)
        x = inp["S"][:, x_row[i]:x_row[i] + ld].to(dt)
        x = _snake(x) if x_snake[i] else x
        return torch.einsum("cob,cib->coi", dz, x), dz.sum(2)

    def check(inp, got, step):
        got = got[0].cpu()
        for i in range(7):
            (w64, b64), (w32, b32) = ref(inp, torch.float64, i), ref(inp, torch.float32, i)
            n_out, ld = d.n_out[i], d.ld[i]
            gw = got[:, d.w_off[i]:d.w_off[i] + n_out * ld].reshape(C, n_out, ld)
            gb = got[:, d.b_off[i]:d.b_off[i] + n_out]
            for name, g_, r64, r32 in (("dW", gw, w64, w32), ("db", gb, b64, b32)):
                bound, err = _measured_bound(r32, r64), rel_l2(_np(g_), _np(r64))
                print(f"light_wgrad C={C} B={B} launch {step} layer {i} {name}: fp32-CPU distance {rel_l2(_np(r32), _np(r64)):.3g} bound {bound:.3g} kernel {err:.3g}")
                assert err <= bound, (step, i, name, err, bound)
    _sequence([(C, B)] * 3, lambda s: s, make, run, check, same_shape=True)


# ---- case 8: rank_images across the block-height switch of the backward pass --------------------------------------------------
def test_rank_images_of_26_images_equals_each_image_s_serial_loop(dev):
    """light.rank_images promises every image the bits of its own serial ProposalRanker.rank.  The fp32 backward pass sums the folded
    pixel loss per block, and light_rows_per_wg (csrc/npp_light.hip) takes 64-row blocks once C (B / 32) > 1536 chains-times-tiles ride
    in one launch: 26 images of B = 2048 rows cross that (32 blocks against the single chain's 64), 3 images of 1024 rows
    (test_candidates_of_several_images_in_one_launch_sequence) do not.  rank_images keeps a launch on the serial loop's side of the
    switch by walking larger groups in chunks; scores, order and details must equal the serial loops' bit for bit."""
    from npp_amd import ops
    from npp_amd.light import ProposalRanker, rank_images
    n_img, H, B = 26, 64, 2048
    assert ops.light_part_blocks(n_img, B) != ops.light_part_blocks(1, B)
    assert (ops.light_part_blocks(n_img, B), ops.light_part_blocks(1, B)) == (32, 64)
    data, cand_lists = [], []
    for i in range(n_img):
        img, _ = oracle.synthetic_image(H, noise=0.01, seed=i)
        angles, periods, shifts = oracle.synthetic_periodicity(H, 1)
        pseudo = np.ones((H, H))
        pseudo[20 + i % 5:42 + i % 5, 18 + i % 7:40 + i % 7] = 0                 # a 22 x 22 hole: 3612 known pixels >= B
        i_train, i_val = np.stack(np.nonzero(pseudo), 1), np.stack(np.nonzero(1 - pseudo), 1)
        assert i_train.shape[0] >= B
        cand_lists.append([(angles[0] + 7.0 * j, periods[0] * (1.0 + 0.23 * j), shifts[0]) for j in range(1 + i % 2)])
        data.append((img, i_train, i_val))
    assert ops.DETERMINISTIC
    for carry in (True, False):
        mk = lambda: [ProposalRanker(im, it, iv, device=dev, N_iters=10, N_rand=B, carry_latents=carry) for im, it, iv in data]   # noqa: E731
        rankers = mk()
        assert len({min(rk.N_rand, rk.i_train.shape[0]) for rk in rankers}) == 1            # one group of 26
        serial = [rk.rank(c, topk=10) for rk, c in zip(rankers, cand_lists)]
        together = rank_images(mk(), cand_lists, topk=10)
        bad = [i for i in range(n_img) if serial[i][2] != together[i][2]]
        print(f"rank_images carry={carry}: images whose details differ from the serial loop: {bad}")
        for i in bad[:3]:
            print(f"  image {i}: serial {serial[i][2]} together {together[i][2]}")
        for i, ((d0, o0, det0), (d1, o1, det1)) in enumerate(zip(serial, together)):
            assert det0 == det1, (carry, i, det0, det1)
            assert list(o0) == list(o1)
            np.testing.assert_array_equal(d0, d1)
