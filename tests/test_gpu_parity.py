"""Parity of the HIP path against the oracle, through the C ABI, on a real MI355X.
Tolerances: fp32 kernels (embedder precise, pixel loss, Adam) are compared at fp32
round-off; bf16-MFMA kernels are compared (a) tightly against the oracle with bf16
operand rounding emulated at the same points and (b) loosely against the plain fp32
oracle, the quantity the 0.1 dB end-to-end PSNR budget of BASELINE.json rests on."""
import ctypes as C

import os

import numpy as np
import pytest

import oracle
from comparators import step_from_autograd  # noqa: E402  (tests/comparators.py)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import npp_amd
    npp_amd.lib()          # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def _cfg(K, H=256, W=None):
    from npp_amd import EmbedCfg
    W = W or H
    angles, periods, _ = oracle.synthetic_periodicity(H, K)
    return EmbedCfg.make(angles, periods, oracle.SEED0_FREQS, (H, W)), angles, periods


def _coords(n, H, W, seed=0):
    rng = np.random.RandomState(seed)
    return np.stack([rng.randint(0, H, n), rng.randint(0, W, n)], 1).astype(np.int32)


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def test_mfma_lane_maps(dev):
    from npp_amd import ops
    ops.selftest(dev)


@pytest.mark.parametrize("K,res", [(1, (256, 256)), (3, (211, 325)), (5, (64, 96))])
def test_embed_precise_fp32(dev, golden, K, res):
    from npp_amd import ops, EmbedCfg
    H, W = res
    angles, periods, _ = oracle.synthetic_periodicity(256, K)
    cfg = EmbedCfg.make(angles, periods, oracle.SEED0_FREQS, res)
    c = _coords(1000, H, W, seed=K)
    c[:4] = [[0, 0], [0, W - 1], [H - 1, 0], [H - 1, W - 1]]
    out = ops.embed_fwd(torch.from_numpy(c).to(dev), cfg, torch.float32, precise=True).cpu().numpy()
    ref = oracle.embed(c, angles, periods, oracle.SEED0_FREQS, res)
    assert out.shape == ref.shape == (1000, K * 462)
    np.testing.assert_allclose(out, ref, atol=5e-4)      # same bound as oracle-vs-reference (f*v amplification)
    warp = ops.warp_fwd(torch.from_numpy(c).to(dev), cfg).cpu().numpy()
    for k in range(K):
        v = oracle.periodic_warp(c, angles[k], periods[k], res)
        np.testing.assert_allclose(warp[:, 22 * k:22 * k + 22], v, atol=2e-5)


def test_embed_golden_vectors(dev, golden):
    """Directly against the reference's own outputs (tests/golden/g1_embed.npz)."""
    from npp_amd import ops, EmbedCfg
    g = golden("g1_embed.npz")
    for tag in ("sq", "rect"):
        res = tuple(int(v) for v in g[f"{tag}_res"])
        cfg = EmbedCfg.make(g[f"{tag}_angles"], g[f"{tag}_periods"], g["freqs"], res)
        c = torch.from_numpy(g[f"{tag}_coords"].astype(np.int32)).to(dev)
        out = ops.embed_fwd(c, cfg, torch.float32, precise=True).cpu().numpy()
        np.testing.assert_allclose(out, g[f"{tag}_emb"], atol=5e-4)
        fast = ops.embed_fwd(c, cfg, torch.bfloat16, precise=False).float().cpu().numpy()
        np.testing.assert_allclose(fast, g[f"{tag}_emb"], atol=1.2e-2)   # bf16 output: 2^-8 relative + fast sin
        # fp32 output with the hardware v_sin_f32 path (the HBM-bound variant of config c4)
        fast32 = ops.embed_fwd(c, cfg, torch.float32, precise=False).cpu().numpy()
        err = np.abs(fast32 - g[f"{tag}_emb"]).max()
        print(f"fp32 fast embedder max |err| vs reference ({tag}): {err:.2e}")
        assert err < 5e-5


def test_embed_edge_cases(dev):
    from npp_amd import ops
    cfg, *_ = _cfg(3)
    empty = torch.empty((0, 2), dtype=torch.int32, device=dev)
    assert ops.embed_fwd(empty, cfg).shape == (0, 3 * 462)
    one = torch.tensor([[5, 7]], dtype=torch.int32, device=dev)
    a = ops.embed_fwd(one, cfg).cpu().numpy()
    big = torch.tensor([[5, 7]] * 67, dtype=torch.int32, device=dev)      # ragged vs the 64-row tile
    b = ops.embed_fwd(big, cfg).cpu().numpy()
    assert np.array_equal(b, np.repeat(a, 67, 0))


@pytest.mark.parametrize("tag", ["init", "pert"])
@pytest.mark.parametrize("use_mask", [False, True])
def test_pixel_loss_golden(dev, golden, tag, use_mask):
    from npp_amd import ops
    g = golden("g4_robust.npz")
    k = f"{tag}_{'mask' if use_mask else 'nomask'}"
    pred = torch.from_numpy(g[f"{tag}_pred"]).to(dev)
    gt = torch.from_numpy(g[f"{tag}_gt"]).to(dev)
    mask = torch.from_numpy(g[f"{tag}_mask"]).to(dev).contiguous() if use_mask else None
    lat = torch.from_numpy(np.concatenate([g[f"{tag}_latent_alpha"].ravel(), g[f"{tag}_latent_scale"].ravel()])).to(dev)
    spline, n_knots, xs = ops.load_spline(dev)
    loss = torch.zeros(1, device=dev)
    dlat = torch.zeros(6, device=dev)
    dpred = torch.empty_like(pred)
    ops.pixel_loss(pred, gt, mask, lat, spline, n_knots, xs, 1.0, loss, dpred, dlat)
    np.testing.assert_allclose(loss.item(), g[f"{k}_loss"], rtol=2e-5)
    np.testing.assert_allclose(dpred.cpu().numpy(), g[f"{k}_dpred"], rtol=2e-4, atol=1e-8)
    np.testing.assert_allclose(dlat[:3].cpu().numpy(), g[f"{k}_dla"].ravel(), rtol=3e-3, atol=3e-6)
    np.testing.assert_allclose(dlat[3:].cpu().numpy(), g[f"{k}_dls"].ravel(), rtol=2e-4, atol=1e-7)


@pytest.mark.parametrize("lt", ["l2", "robust_loss"])
@pytest.mark.parametrize("use_mask", [False, True])
def test_pixel_loss_quadratic_switches_golden(dev, golden, lt, use_mask):
    """--loss_type l2 / robust_loss (models/mse_calculator.py:19-23; g4b_quad.npz = the reference's img2mse + autograd): the flat entry
    point (one problem and three stacked ones), the boundary module's img2mse, and the form that rides in the patch-in launch."""
    from npp_amd import ops, reference_api as api
    g = golden("g4b_quad.npz")
    k = f"{lt}_{'mask' if use_mask else 'nomask'}"
    pred = torch.from_numpy(g["pred"]).to(dev)
    gt = torch.from_numpy(g["gt"]).to(dev)
    mask = torch.from_numpy(g["mask"]).to(dev).reshape(-1).contiguous() if use_mask else None
    coef = ops.quad_coef(lt)
    loss, dpred = torch.zeros(1, device=dev), torch.empty_like(pred)
    ops.pixel_loss_quad(pred, gt, mask, coef, 1.0, loss, dpred)
    np.testing.assert_allclose(loss.item(), g[f"{k}_loss"], rtol=2e-5)
    np.testing.assert_allclose(dpred.cpu().numpy(), g[f"{k}_dpred"], rtol=2e-5, atol=1e-9)
    p3 = torch.stack([pred, pred * 0.5, gt]).contiguous()                   # three problems, shared targets
    l3, d3 = torch.zeros(3, device=dev), torch.empty_like(p3)
    ops.pixel_loss_quad(p3, gt, mask, coef, 2.0, l3, d3)
    np.testing.assert_allclose(l3[0].item(), 2.0 * g[f"{k}_loss"], rtol=2e-5)
    np.testing.assert_allclose(d3[0].cpu().numpy(), 2.0 * g[f"{k}_dpred"], rtol=2e-5, atol=1e-9)
    assert l3[2].item() == 0.0 and float(d3[2].abs().max()) == 0.0
    ref_l, ref_d = oracle.img2mse_quad_grads(p3[1].cpu().numpy(), g["gt"], lt, g["mask"] if use_mask else None)
    np.testing.assert_allclose(l3[1].item(), 2.0 * ref_l, rtol=2e-5)
    np.testing.assert_allclose(d3[1].cpu().numpy(), 2.0 * ref_d, rtol=2e-5, atol=1e-9)
    x = pred.clone().requires_grad_(True)                                   # the reference's call signature (mse_calculator.py:13)
    out = api.img2mse(x, gt, lt, None, None if mask is None else mask.reshape(-1, 1))
    out.backward()
    np.testing.assert_allclose(out.item(), g[f"{k}_loss"], rtol=2e-5)
    np.testing.assert_allclose(x.grad.cpu().numpy(), g[f"{k}_dpred"], rtol=2e-5, atol=1e-9)


@pytest.mark.parametrize("lt", ["l2", "robust_loss"])
def test_fit_with_a_quadratic_pixel_loss(dev, lt):
    """CompletionFit(loss_type=...): the loss rides in the patch-in launch like the adaptive one (folded form == separate launches, bit
    for bit on the MLP half), the adaptive latents stay where they were (no gradient reaches them: torch's Adam skips them in the
    reference), and the fit converges."""
    from npp_amd.fit import CompletionFit
    H, K = 128, 1
    img, mask = oracle.synthetic_image(H, seed=3)
    angles, periods, shifts = oracle.synthetic_periodicity(H, K)

    def make():
        return CompletionFit(img, mask, angles, periods, oracle.SEED0_FREQS, oracle.init_params(K, seed=1), device=dev, N_rand=2048, shifts=shifts,
                             seed=4, loss_type=lt, contextual_weight=0.0, perceptual_weight=0.0)
    a, b = make(), make()
    b.fold_launches = False
    lat0 = a.net.latents.clone()
    p0 = a.psnr("known")
    for _ in range(60):
        a.step_full()
        b.step_full()
    torch.cuda.synchronize()
    assert torch.equal(a.net.params, b.net.params)
    assert torch.equal(a.net.latents, lat0)
    p1 = a.psnr("known")
    print(f"{lt}: PSNR {p0:.2f} -> {p1:.2f} dB after 60 iterations")
    assert p1 > p0 + 5.0


def _lpips_plain_head_torch(f0, f1, lin):
    """lpips.py:99-133 with use_robust=False in plain torch: normalize_tensor (eps 1e-10), squared difference, lin 1x1 conv,
    spatial mean, summed over the batch."""
    n0 = f0 / (f0.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    n1 = f1 / (f1.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    return ((n0 - n1).pow(2) * lin[None, :, None, None]).sum(1).mean((1, 2)).sum()


@pytest.mark.parametrize("C,hw", [(64, 24), (256, 12), (512, 6), (256, 27), (512, 27)])
def test_lpips_plain_head_with_gradient(dev, C, hw):
    """npp_lpips_layer with no latents = LPIPS.forward(use_robust=False) (lpips.py:108-109) -- the in-loop head under
    --use_adaptive_perceptual_loss off: value against the forward-only kernel the ranking score uses (pinned to the reference by g10)
    and against torch fp32, gradient against torch autograd.  The 27 x 27 taps have more than 2048 positions (3 x 729), where a
    thread takes C / 16 channels of 16 positions: the 16- and 32-channel forms of the kernel (csrc/npp_lpips.hip lp_launch), which
    no tap of the loop's patch sizes reaches."""
    from npp_amd import ops
    g = torch.Generator().manual_seed(C)
    N = 3
    f0 = torch.rand(N, C, hw, hw, generator=g).to(dev)
    f1 = torch.rand(N, C, hw, hw, generator=g).to(dev)
    lin = (torch.rand(C, generator=g) * 0.1).to(dev)
    loss, ref_fwd, df0 = torch.zeros(1, device=dev), torch.zeros(1, device=dev), torch.empty_like(f0)
    ops.lpips_layer(f0, f1, lin, None, None, 0, 0.0, 2.0 * N, loss, df0, None)           # scale / N = 2: twice the batch sum
    ops.lpips_plain_layer(f0, f1, lin, 2.0, ref_fwd)
    x = f0.clone().requires_grad_(True)
    ref = 2.0 * _lpips_plain_head_torch(x, f1, lin)
    ref.backward()
    np.testing.assert_allclose(loss.item(), ref_fwd.item(), rtol=2e-5)
    np.testing.assert_allclose(loss.item(), ref.item(), rtol=2e-5)
    assert rel_l2(df0.cpu().numpy(), x.grad.cpu().numpy()) < 2e-5
    fwd_only = torch.zeros(1, device=dev)
    ops.lpips_layer(f0, f1, lin, None, None, 0, 0.0, 2.0 * N, fwd_only)
    assert fwd_only.item() == loss.item() or abs(fwd_only.item() - loss.item()) < 1e-6 * abs(loss.item())


def test_lpips_heads_in_one_launch_equal_the_five_launches(dev):
    """npp_lpips_layers (blockIdx.y = tap) against five npp_lpips_layer calls on VGG16-shaped taps: loss word (the fixed-point sums are
    order-independent), feature gradients and latent gradients bit for bit; adaptive and plain heads."""
    from npp_amd import ops
    g = torch.Generator().manual_seed(11)
    N, shapes = 2, [(64, 96), (128, 48), (256, 24), (512, 12), (512, 6)]
    f0s = [torch.rand(N, C, h, h, generator=g).to(dev) for C, h in shapes]
    f1s = [torch.rand(N, C, h, h, generator=g).to(dev) for C, h in shapes]
    lins = [(torch.rand(C, generator=g) * 0.1).to(dev) for C, _ in shapes]
    lats = [torch.cat([torch.randn(C, generator=g) * 0.5, torch.randn(C, generator=g) * 0.3]).to(dev) for C, _ in shapes]
    spline, n_knots, xs = ops.load_spline(dev)
    for robust in (True, False):
        la = lats if robust else None
        l1, l5 = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
        d1 = [torch.empty_like(f) for f in f0s]
        d5 = [torch.empty_like(f) for f in f0s]
        g1 = [torch.zeros_like(t) for t in lats]
        g5 = [torch.zeros_like(t) for t in lats]
        for k in range(5):
            ops.lpips_layer(f0s[k], f1s[k], lins[k], la[k] if robust else None, spline, n_knots, xs, 0.7, l1, d1[k], g1[k] if robust else None)
        ops.lpips_layers(f0s, f1s, lins, la, spline, n_knots, xs, 0.7, l5, d5, g5)
        torch.cuda.synchronize()
        assert abs(l1.item() - l5.item()) <= 1e-6 * abs(l1.item())            # (five float additions in another order)
        for k in range(5):
            assert torch.equal(d1[k], d5[k]), k
            if robust:
                assert torch.equal(g1[k], g5[k]), k


def test_lpips_tap_gradients_written_flat_equal_the_imported_ones(dev):
    """npp_lpips_layers with npp_lpips_tap.dflat (the tap gradient as bf16 straight into the trunk's flat layout) against the fp32
    gradient pushed through npp_trunk_grad_in: the same bytes (interior, border, guard bands), with N < N_total; and LPIPS.fused with
    and without it: dL/dx, loss and latent gradients bit for bit."""
    from npp_amd import ops
    from npp_amd.losses import LPIPS
    g = torch.Generator().manual_seed(3)
    N, Nt, shapes = 2, 4, [(64, 40), (128, 20), (512, 6)]
    f0s = [torch.rand(N, C, h, h, generator=g).to(dev) for C, h in shapes]
    f1s = [torch.rand(N, C, h, h, generator=g).to(dev) for C, h in shapes]
    lins = [(torch.rand(C, generator=g) * 0.1).to(dev) for C, _ in shapes]
    lats = [torch.cat([torch.randn(C, generator=g) * 0.5, torch.randn(C, generator=g) * 0.3]).to(dev) for C, _ in shapes]
    spline, n_knots, xs = ops.load_spline(dev)
    la, lb = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    d = [torch.empty_like(f) for f in f0s]
    ga, gb = [torch.zeros_like(t) for t in lats], [torch.zeros_like(t) for t in lats]
    ops.lpips_layers(f0s, f1s, lins, lats, spline, n_knots, xs, 0.7, la, d, ga)
    want = [ops.trunk_alloc(Nt, C, h, h, dev) for C, h in shapes]
    for k, (C, h) in enumerate(shapes):
        ops.trunk_grad_in(d[k], None, Nt, N, C, h, h, want[k])
    got = [ops.trunk_alloc(Nt, C, h, h, dev) for C, h in shapes]
    ops.lpips_layers(f0s, f1s, lins, lats, spline, n_knots, xs, 0.7, lb, [None] * 3, gb, dflats=[(t, Nt) for t in got])
    torch.cuda.synchronize()
    assert la.item() == lb.item()
    for k in range(3):
        assert float(want[k].float().abs().sum()) > 0
        assert torch.equal(want[k], got[k]), k
        assert torch.equal(ga[k], gb[k]), k
    outs = []
    for flat in (True, False):
        torch.manual_seed(0)
        m = LPIPS(device=dev)
        m.flat_tap_grads = flat
        xy = torch.rand(4, 3, 64, 64, generator=torch.Generator().manual_seed(5)).to(dev)
        loss = torch.zeros(1, device=dev)
        dx = m.fused(xy, 2, 0.5, loss)
        torch.cuda.synchronize()
        outs.append((dx[:2].clone(), loss.clone(), [t.clone() for t in m.dlatents]))
    assert float(outs[0][0].abs().sum()) > 0
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    for a, b in zip(outs[0][2], outs[1][2]):
        assert torch.equal(a, b)


def test_fit_with_the_plain_lpips_head(dev):
    """CompletionFit(use_adaptive_perceptual_loss=False): on a 'same' iteration the explicit loop's gradients equal the autograd loop's,
    the LPIPS latents never move (no gradient reaches them: torch's Adam skips them in the reference), the fit stays finite."""
    from npp_amd.fit import CompletionFit
    H, K = 256, 1
    img, mask = oracle.synthetic_image(H, seed=2)
    angles, periods, shifts = oracle.synthetic_periodicity(H, K)

    def make():
        return CompletionFit(img, mask, angles, periods, oracle.SEED0_FREQS, oracle.init_params(K, seed=2), device=dev, N_rand=2048, shifts=shifts,
                             seed=7, use_adaptive_perceptual_loss=False, perceptual_weight=1e-2)
    a, b = make(), make()
    lat0 = a.percepLoss._lat.clone()
    batch = None
    for _ in range(200):                                   # the first 'same' batch of the stream (20 % of the draws)
        batch = a.sample_batch()
        if batch is not None and batch["source"] == "same":
            break
    assert batch is not None and batch["source"] == "same"
    a.step_from(batch)
    step_from_autograd(b, batch)
    ga, gb = a.net.grads(), b.net.grads()
    for name in ga:
        assert rel_l2(ga[name], gb[name]) < 2e-3, name
    np.testing.assert_allclose(float(a.last_patch_loss[0]), float(b.last_patch_loss[0]), rtol=2e-3)
    for _ in range(30):
        a.step_full()
    torch.cuda.synchronize()
    assert torch.equal(a.percepLoss._lat, lat0) and torch.equal(b.percepLoss._lat, lat0) and a.percepLoss.lat_step == 0
    assert bool(torch.isfinite(a.net.params).all())


@pytest.mark.parametrize("decay", [None, 20])
def test_lpips_branch_as_a_captured_graph_equals_its_launches(dev, decay):
    """CompletionFit.lpips_branch: from its third use on a set of buffers the LPIPS branch of a 'same' iteration (46 launches) is replayed
    as one captured HIP graph -- the same launches with the same arguments: parameters, LPIPS latents and the patch loss must come out
    bit for bit as from the launch-by-launch form.  decay = 20: across two patch-size decays (train.py:137-141: 64 -> 32 -> 16 pixels,
    2 -> 4 -> 8 patches): every batch shape gets buffers and a capture of its own."""
    from npp_amd.fit import CompletionFit
    H, K = 256, 1
    img, mask = oracle.synthetic_image(H, seed=4)
    angles, periods, shifts = oracle.synthetic_periodicity(H, K)

    def make(graph):
        kw = {} if decay is None else {"patch_size_decay": decay}
        f = CompletionFit(img, mask, angles, periods, oracle.SEED0_FREQS, oracle.init_params(K, seed=3), device=dev, N_rand=2048, shifts=shifts,
                          seed=9, perceptual_weight=1e-2, **kw)
        f.lp_graph = graph
        return f
    a, b = make(True), make(False)
    same, losses = 0, []
    for it in range(60 if decay is None else 90):
        ba = None
        while ba is None:
            ba = a.sample_batch()
            bb = b.sample_batch()
        a.step_from(ba)
        b.step_from(bb)
        if ba["source"] == "same":
            same += 1
            losses.append((float(a.last_patch_loss[0]), float(b.last_patch_loss[0])))
    torch.cuda.synchronize()
    replays = [e for e in a._lp_graphs.values() if e[0] is not None]
    print(f"{same} 'same' iterations, {len(replays)} captured graph(s)")
    assert same >= 5 and len(replays) >= 1 and not b._lp_graphs
    if decay is not None:
        assert a.patch_size == b.patch_size == 16 and a.patch_num == 8 and len(replays) >= 2
    # (the reported loss WORD is the sum of the two branches' terms in arrival order -- two streams add to it -- so it may differ in
    # its last bit between any two runs; what is trained on, the gradients, is order-independent)
    assert all(abs(x - y) <= 2e-7 * abs(y) for x, y in losses), losses
    assert torch.equal(a.net.params, b.net.params)
    assert torch.equal(a.percepLoss._lat, b.percepLoss._lat) and a.percepLoss.lat_step == b.percepLoss.lat_step == same


def test_fused_chain_with_tanh_output(dev):
    """render()'s other output nonlinearity (models/helpers.py:57-58, --normalize_type 2) in the fused launches: npp_mlp_fwd_act
    (tanh / raw) and npp_mlp_bwd_act behind it.  The forward against its own raw output; the backward against the sigmoid path fed a
    d pred that gives the same d raw -- every weight gradient must then agree.  With K = 3 and K = 1 and with either training stash:
    each pair is another instantiation of the forward kernel that reads the nonlinearity from its arguments."""
    from npp_amd import ops
    from npp_amd.model import NPPNet
    H, rows = 128, 1024
    old = ops.tune("stash8")
    try:
        for K, s8 in ((3, 1), (3, 0), (1, 1), (1, 0)):
            ops.tune("stash8", s8)
            angles, periods, _ = oracle.synthetic_periodicity(H, K)
            P = oracle.init_params(K, seed=5)
            ns = NPPNet(angles, periods, oracle.SEED0_FREQS, (H, H), params=P, device=dev, ksplit=2, out_act=1)
            nt = NPPNet(angles, periods, oracle.SEED0_FREQS, (H, H), params=P, device=dev, ksplit=2, out_act=2)
            g = torch.Generator().manual_seed(2)
            c = torch.randint(0, H, (rows, 2), generator=g, dtype=torch.int32).to(dev)
            raw = ops.mlp_fwd(c, ns.cfg, ns.wf, ns.params, width=ns.width, out_act=0)
            ns.zero_grad(); nt.zero_grad()
            ns.forward_train(c); nt.forward_train(c)
            ws, wt = ns.workspace(rows), nt.workspace(rows)
            np.testing.assert_allclose(ws["pred"].cpu().numpy(), torch.sigmoid(raw).cpu().numpy(), atol=2e-6)
            np.testing.assert_allclose(wt["pred"].cpu().numpy(), torch.tanh(raw).cpu().numpy(), atol=2e-6)
            np.testing.assert_allclose(nt.render(c).cpu().numpy(), torch.tanh(raw).cpu().numpy(), atol=2e-6)
            dp = torch.randn(rows, 3, generator=g).to(dev) * 1e-3
            s_, t_ = ws["pred"], wt["pred"]
            ws["dpred"].copy_(dp)
            wt["dpred"].copy_(dp * (s_ * (1 - s_)) / (1 - t_ * t_).clamp_min(1e-6))
            ns.backward(rows); nt.backward(rows)
            torch.cuda.synchronize()
            gs, gt_ = ns.grads(), nt.grads()
            for name in gs:
                print(f"K={K} stash8={s8} {name}: rel L2 {rel_l2(gt_[name], gs[name]):.3e}")
                assert rel_l2(gt_[name], gs[name]) < 1e-4, (K, s8, name, rel_l2(gt_[name], gs[name]))
    finally:
        ops.tune("stash8", old)


def test_adam_golden(dev, golden):
    from npp_amd import ops
    g = golden("g9_adam.npz")
    p = torch.from_numpy(np.concatenate([g["p0_init"].ravel(), g["p1_init"].ravel()])).to(dev)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    lr, gs = 5e-4, 0
    for it in range(5):
        # two slabs that sum to the gradient: exercises the split-K reduction
        grad = np.concatenate([g[f"g0_{it}"].ravel(), g[f"g1_{it}"].ravel()])
        slabs = torch.from_numpy(np.stack([0.25 * grad, 0.75 * grad]).astype(np.float32)).to(dev).contiguous()
        ops.adam_step(p, m, v, slabs, 2, p.numel(), lr, it + 1)
        lr = oracle.lr_schedule(gs)
        gs += 1
        got = p.cpu().numpy()
        np.testing.assert_allclose(got[:35], g[f"p0_{it}"].ravel(), rtol=3e-6, atol=2e-7)
        np.testing.assert_allclose(got[35:], g[f"p1_{it}"].ravel(), rtol=3e-6, atol=2e-7)


@pytest.mark.parametrize("K", [1, 3])
def test_pack_device_equals_host_twin(dev, K):
    import npp_amd
    from npp_amd import ops
    from npp_amd._lib import param_layout, check
    lay, total = param_layout(K)
    rng = np.random.RandomState(0)
    flat = rng.randn(total).astype(np.float32)
    wf, wb = ops.pack_weights(torch.from_numpy(flat).to(dev), K)
    L = npp_amd.lib()
    hf = np.zeros(wf.numel(), np.uint8)
    hb = np.zeros(wb.numel(), np.uint8)
    check(L.npp_pack_weights_host(flat.ctypes.data, hf.ctypes.data, hb.ctypes.data, K, 256), "host pack")
    assert np.array_equal(wf.cpu().numpy(), hf)
    assert np.array_equal(wb.cpu().numpy(), hb)


def _net(dev, K, H=256, seed=0, ksplit=3, width=256):
    from npp_amd.model import NPPNet
    angles, periods, _ = oracle.synthetic_periodicity(H, K)
    P = oracle.init_params(K, W=width, seed=seed)
    net = NPPNet(angles, periods, oracle.SEED0_FREQS, (H, H), params=P, device=dev, ksplit=ksplit, width=width)
    return net, P, angles, periods


@pytest.mark.parametrize("K,n,width", [(3, 64, 256), (1, 64, 256), (5, 64, 256), (3, 1000, 256), (1, 1000, 256), (5, 1000, 256),
                                         (3, 1000, 512), (1, 200, 512), (5, 64, 512)])
def test_fused_forward_matches_oracle(dev, K, n, width):
    """width 512 = the reference's default --netwidth (options/arg_config.py:57): the same sources built with -DNPP_WIDTH=512
    (libnpp_hip_w512.so), 8 waves per workgroup."""
    H = 256
    net, P, angles, periods = _net(dev, K, width=width)
    c = _coords(n, H, H, seed=11 + K)
    pred = net.render(torch.from_numpy(c).to(dev)).cpu().numpy()
    emb = oracle.embed(c, angles, periods, oracle.SEED0_FREQS, (H, H))
    raw_b, _ = oracle.mlp_forward(P, emb, K, emulate_bf16=True)
    raw_f, _ = oracle.mlp_forward(P, emb, K)
    assert pred.shape == (n, 3)
    # tight: same bf16 operand rounding, differences = accumulation order + hardware sin
    assert np.abs(pred - oracle.sigmoid(raw_b)).max() < 4e-3
    # loose: against the reference's fp32 maths (bf16 operands, 13 layers deep)
    assert np.abs(pred - oracle.sigmoid(raw_f)).max() < 2e-2
    assert rel_l2(pred, oracle.sigmoid(raw_f)) < 5e-3


@pytest.fixture
def stash_mode(request):
    """npp_tune("stash8") for one test: 1 = the 8-bit training stash (bf8 gradients / fp8 layer inputs, the default), 0 = the
    16-bit one; restored afterwards."""
    from npp_amd import ops
    old = ops.tune("stash8", request.param)
    yield request.param
    ops.tune("stash8", old)


@pytest.mark.parametrize("stash_mode", [1, 0], indirect=True, ids=["stash8", "stash16"])
@pytest.mark.parametrize("K,width", [(3, 256), (1, 256), (5, 256), (3, 512), (1, 512)])
def test_fused_training_step_gradients(dev, K, width, stash_mode):
    """forward(stash) -> pixel loss -> backward chain -> grouped wgrad, against the oracle's
    hand-derived backward (itself pinned to the reference's autograd in test_oracle_golden).  stash8: the oracle emulates the
    8-bit operand roundings of the weight-gradient products (oracle.mlp_backward emulate_stash8) at the same 3 %; the distance
    to the PLAIN fp32 oracle is then the quantisation noise of bf8 x fp8 products on a 677-row batch of random-sign terms."""
    H, n = 256, 640 + 37       # ragged: 677 real rows padded to 704
    net, P, angles, periods = _net(dev, K, ksplit=3, width=width)
    c = _coords(n, H, H, seed=5)
    Bp = (n + 63) // 64 * 64
    cp = np.zeros((Bp, 2), np.int32)
    cp[:n] = c
    rng = np.random.RandomState(2)
    gt = rng.rand(n, 3).astype(np.float32)
    net.zero_grad()
    pred = net.forward_train(torch.from_numpy(cp).to(dev))
    ws = net.workspace(Bp)
    ws["dpred"].zero_()
    net.pixel_loss(Bp, n, torch.from_numpy(gt).to(dev))
    net.backward(Bp)
    torch.cuda.synchronize()
    G = net.grads()
    pred_h = pred.cpu().numpy()[:n]
    # oracle on the same inputs
    emb = oracle.embed(c, angles, periods, oracle.SEED0_FREQS, (H, H))
    raw, cache = oracle.mlp_forward(P, emb, K, emulate_bf16=True)
    pr = oracle.sigmoid(raw)
    la, ls = net.latents[:3].cpu().numpy()[None], net.latents[3:].cpu().numpy()[None]
    loss, dpred, dla, dls = oracle.img2mse_grads(pr, gt, la, ls)
    assert np.abs(pred_h - pr).max() < 4e-3
    assert abs(net.loss_buf.item() - loss) < 2e-3 * abs(loss) + 1e-4
    draw = dpred * pr * (1 - pr)
    Gref = oracle.mlp_backward(P, cache, draw, emulate_bf16=True, emulate_stash8=bool(stash_mode))
    assert set(G) == set(Gref)
    for name in Gref:
        e = rel_l2(G[name], Gref[name])
        assert e < 3e-2, (name, e)
    # the same gradients against the PLAIN fp32 oracle (no bf16 operand rounding emulated): the distance the 16-bit operands put
    # between the fused step and the reference's fp32 autograd, asserted at its measured level (worst tensor 1.3e-2 at W = 256,
    # K = 3; the trajectories g8 / g8k3 / g8c2 show what it does to a fit: <= 0.1 dB)
    raw32, cache32 = oracle.mlp_forward(P, emb, K, emulate_bf16=False)
    pr32 = oracle.sigmoid(raw32)
    _, dpred32, _, _ = oracle.img2mse_grads(pr32, gt, la, ls)
    G32 = oracle.mlp_backward(P, cache32, dpred32 * pr32 * (1 - pr32), emulate_bf16=False)
    gap = {name: rel_l2(G[name], G32[name]) for name in G32}
    worst = max(gap, key=gap.get)
    print(f"gradient gap to the fp32 oracle: worst {worst} {gap[worst]:.3e}, median {float(np.median(list(gap.values()))):.3e}")
    # stash8: per-product relative noise ~7 % (e5m2) and ~3.6 % (e4m3) rms; on this batch of random-sign terms the tensor-level
    # gap is of that order (measured worst 5.7e-2), a fraction of a percent of the minibatch noise of the same sum
    assert gap[worst] < (9e-2 if stash_mode else 4e-2), (worst, gap[worst])
    np.testing.assert_allclose(net.dlatent[:3].cpu().numpy(), dla.ravel(), rtol=5e-2, atol=1e-5)
    np.testing.assert_allclose(net.dlatent[3:].cpu().numpy(), dls.ravel(), rtol=5e-2, atol=1e-5)
    # padded rows contribute nothing: their dpred is zero
    assert float(ws["dpred"][n:].abs().max()) == 0.0


def test_optimizer_step_and_lr_rule(dev):
    K, H, n = 3, 256, 256
    net, P, angles, periods = _net(dev, K, ksplit=2)
    c = torch.from_numpy(_coords(n, H, H)).to(dev)
    gt = torch.rand(n, 3, device=dev)
    before = net.state_dict()
    lrs = []
    for it in range(3):
        net.zero_grad()
        net.forward_train(c)
        net.workspace(n)["dpred"].zero_()
        net.pixel_loss(n, n, gt)
        net.backward(n)
        lrs.append(net.lr)
        net.optimizer_step(n)
    # first two steps run at lrate exactly, then the decayed value (train.py:253-263)
    assert lrs[0] == lrs[1] == 5e-4 and abs(lrs[2] - 5e-4 * 0.1 ** (1 / 50000)) < 1e-12
    after = net.state_dict()
    moved = max(np.abs(after[k] - before[k]).max() for k in before)
    assert 1e-4 < moved < 5e-3          # |delta| ~ lr per Adam step
    # one Adam step on the oracle from the kernel's own gradient reproduces the update
    net2, P2, *_ = _net(dev, K, ksplit=2)
    net2.zero_grad(); net2.forward_train(c); net2.workspace(n)["dpred"].zero_(); net2.pixel_loss(n, n, gt); net2.backward(n)
    G = net2.grads()
    st = oracle.adam_init(P2)
    Pn = oracle.adam_step({k: v.copy() for k, v in P2.items()}, G, st, 5e-4)
    net2.optimizer_step(n)
    got = net2.state_dict()
    for k in Pn:
        np.testing.assert_allclose(got[k], Pn[k], rtol=1e-5, atol=2e-7, err_msg=k)


# ---------------------------------------------------------------- patch-loss rows (a9-a13)
def test_patch_gather_matches_reference_glimpse(dev, golden):
    from npp_amd import ops
    g = golden("g5_sampler.npz")
    img = g["glimpse_img"][0]                                   # (3,H,W)
    hwc = torch.from_numpy(np.ascontiguousarray(img.transpose(1, 2, 0))).to(dev)
    msk = torch.from_numpy(np.ascontiguousarray(img[0])).to(dev)
    cen = torch.from_numpy(g["glimpse_offs_xy"][:, ::-1].astype(np.int32).copy()).to(dev)   # reference offsets are (x,y)
    rgb, m = ops.patch_gather(hwc, msk, cen, 16)
    assert np.array_equal(rgb.cpu().numpy(), g["glimpse_out"])              # bit-exact: it is a copy
    assert np.array_equal(m.cpu().numpy()[:, 0], g["glimpse_out"][:, 0])


@pytest.mark.parametrize("tag", ["a", "b", "same", "w"])
def test_cx_core_golden(dev, golden, tag):
    from npp_amd import ops
    g = golden("g6_cx.npz")
    x = torch.from_numpy(g[f"{tag}_x"]).to(dev)
    y = torch.from_numpy(g[f"{tag}_y"]).to(dev)
    w = torch.from_numpy(g[f"{tag}_w"]).to(dev) if f"{tag}_w" in g.files else None
    loss, dx = ops.cx_fwd_bwd(x, y, 0.5, w)
    np.testing.assert_allclose(loss.item(), g[f"{tag}_loss"], rtol=5e-4, atol=5e-5)
    ref = g[f"{tag}_dx"]
    got = dx.cpu().numpy()
    if np.linalg.norm(ref) < 1e-6:
        assert np.abs(got - ref).max() < 1e-6
    else:
        assert rel_l2(got, ref) < 5e-3
    # scale and forward-only
    loss2, none = ops.cx_fwd_bwd(x, y, 0.5, w, scale=0.001, want_grad=False)
    assert none is None and abs(loss2.item() - 0.001 * float(g[f"{tag}_loss"])) < 1e-6 + 1e-3 * abs(0.001 * float(g[f"{tag}_loss"]))


def test_cx_core_realistic_size(dev):
    """(6,256,24,24): the relu3_4 shape of 96x96 patches; against the oracle."""
    from npp_amd import ops
    rng = np.random.RandomState(0)
    y = np.maximum(rng.randn(6, 256, 24, 24), 0).astype(np.float32)
    x = np.maximum(0.7 * y + 0.7 * rng.randn(6, 256, 24, 24), 0).astype(np.float32)
    loss, dx = ops.cx_fwd_bwd(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev))
    lo, dxo = oracle.cx_backward(x, y)
    assert abs(loss.item() - lo) < 1e-3 * abs(lo)
    assert rel_l2(dx.cpu().numpy(), dxo) < 1e-2


@pytest.mark.parametrize("shape", [(1, 32, 47, 50), (2, 64, 33, 65), (1, 32, 48, 52)])
def test_cx_core_whole_image_crop_size(dev, shape):
    """hw > 2048 positions (the crops the proposal ranking scores, NPP_proposal/search.py:180-197, are whole-image sized):
    the column-chunked row pass, value and gradient against the oracle; and the value-only form the ranking's score takes (128 x 128
    tiles, row sums and column maxima as two streaming reads: other summation orders, so equal to round-off, not to the bit)."""
    from npp_amd import ops
    rng = np.random.RandomState(3)
    y = np.maximum(rng.randn(*shape), 0).astype(np.float32)
    x = np.maximum(0.7 * y + 0.7 * rng.randn(*shape), 0).astype(np.float32)
    assert shape[2] * shape[3] > 2048
    loss, dx = ops.cx_fwd_bwd(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev))
    lo, dxo = oracle.cx_backward(x, y)
    assert abs(loss.item() - lo) < 1e-3 * abs(lo)
    assert rel_l2(dx.cpu().numpy(), dxo) < 1e-2
    loss2, none = ops.cx_fwd_bwd(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), want_grad=False)
    assert none is None and abs(loss2.item() - lo) < 1e-3 * abs(lo) and abs(loss2.item() - loss.item()) < 2e-5 * abs(lo)
    loss3, _ = ops.cx_fwd_bwd(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), want_grad=False)
    assert loss3.item() == loss2.item()                       # (no order-dependent float sum: run to run the same bits)
    # stale workspace bytes must not matter (the padding of the tiled arrays is never written): poison the cached workspaces with NaN
    # bit patterns, then with huge finite values, and ask again -- found in round 6 as a score that depended on which tests ran before
    for fill in (255, 127):
        for ws in ops._cx_ws.values():
            ws.fill_(fill)
        loss4, _ = ops.cx_fwd_bwd(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), want_grad=False)
        assert loss4.item() == loss2.item(), fill
        for ws in ops._cx_ws.values():
            ws.fill_(fill)
        loss5, dx5 = ops.cx_fwd_bwd(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev))
        assert loss5.item() == loss.item() and torch.equal(dx5, dx), fill


def test_lpips_head_golden(dev, golden):
    from npp_amd import ops
    g = golden("g7_lpips.npz")
    spline, n_knots, xs = ops.load_spline(dev)
    loss = torch.zeros(1, device=dev)
    N = g["f0_0"].shape[0]
    for k in range(5):
        f0 = torch.from_numpy(g[f"f0_{k}"]).to(dev)
        f1 = torch.from_numpy(g[f"f1_{k}"]).to(dev)
        lin = torch.from_numpy(g[f"lin{k}"]).to(dev)
        lat = torch.from_numpy(np.concatenate([g[f"la{k}"].ravel(), g[f"ls{k}"].ravel()])).to(dev)
        df0 = torch.empty_like(f0)
        dlat = torch.zeros_like(lat)
        ops.lpips_layer(f0, f1, lin, lat, spline, n_knots, xs, 1.0, loss, df0, dlat)
        C = f0.shape[1]
        assert rel_l2(df0.cpu().numpy(), g[f"df0_{k}"]) < 2e-3, k
        np.testing.assert_allclose(dlat[:C].cpu().numpy(), g[f"dla{k}"].ravel(), rtol=1e-2, atol=2e-6)
        np.testing.assert_allclose(dlat[C:].cpu().numpy(), g[f"dls{k}"].ravel(), rtol=2e-3, atol=2e-7)
    np.testing.assert_allclose(loss.item(), g["loss"], rtol=5e-5)


def test_lpips_plain_head_golden(dev, golden):
    """LPIPS.forward(use_robust=False, normalize=True) + autograd by the reference's own code (g7b_lpips_plain.npz: the features and
    vendored lin weights of g7, tests/golden/make_golden_lpips_plain.py): value and feature gradients of the plain head, tap by tap and
    all five taps in one launch."""
    from npp_amd import ops
    g, gp = golden("g7_lpips.npz"), golden("g7b_lpips_plain.npz")
    N = g["f0_0"].shape[0]
    f0s = [torch.from_numpy(g[f"f0_{k}"]).to(dev) for k in range(5)]
    f1s = [torch.from_numpy(g[f"f1_{k}"]).to(dev) for k in range(5)]
    lins = [torch.from_numpy(g[f"lin{k}"]).to(dev) for k in range(5)]
    loss1, loss5 = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    d5 = [torch.empty_like(f) for f in f0s]
    for k in range(5):
        df0 = torch.empty_like(f0s[k])
        ops.lpips_layer(f0s[k], f1s[k], lins[k], None, None, 0, 0.0, 1.0, loss1, df0)
        assert rel_l2(df0.cpu().numpy(), gp[f"df0_{k}"]) < 1e-4, k
    ops.lpips_layers(f0s, f1s, lins, None, None, 0, 0.0, 1.0, loss5, d5)
    for k in range(5):
        assert rel_l2(d5[k].cpu().numpy(), gp[f"df0_{k}"]) < 1e-4, k
    np.testing.assert_allclose(loss1.item(), gp["loss"], rtol=2e-5)
    np.testing.assert_allclose(loss5.item(), gp["loss"], rtol=2e-5)


def test_sampler_reproduces_reference_sequence(dev, golden):
    """The product sampler (summed-area counts + HIP gather) against the reference's own
    24-call sequence: modes, k, centres, crops, weights and RNG consumption."""
    from npp_amd.sampler import GridPatchSampler
    g = golden("g5_sampler.npz")
    H = int(g["H"])
    img, mask = oracle.synthetic_image(H)
    i_train = np.stack(np.nonzero(mask[..., 0]), 1)
    i_val = np.stack(np.nonzero(1 - mask[..., 0]), 1)
    code = {"val": 0, "train": 1, "same": 2}
    for tag, P, nsamp in (("p64", 64, 2), ("p32", 32, 4)):
        rng = np.random.RandomState(0)
        S = GridPatchSampler(torch.from_numpy((img * mask)[None]).to(dev), torch.from_numpy(mask[None]).to(dev), nsamp, P,
                             H, H, i_train, i_val, [g["shifts"].tolist()], False, rng=rng)
        assert S.pool_train.shape[0] == int(g[f"{tag}_pool_train_n"]) and S.pool_val.shape[0] == int(g[f"{tag}_pool_val_n"])
        for it in range(24):
            real, rmask, fake, fmask, coords, source, k, w = S.sample_patches(3, 0.3)
            assert k == g[f"{tag}_k"][it], (tag, it)
            if k == 0:
                continue
            assert code[source] == g[f"{tag}_modes"][it]
            assert np.array_equal(coords[:, P // 2, P // 2].cpu().numpy(), g[f"{tag}_centres"][it])
            np.testing.assert_allclose(fake.double().sum().item(), g[f"{tag}_fake_sum"][it], rtol=1e-6)
            np.testing.assert_allclose(fmask.double().sum().item(), g[f"{tag}_fmask_sum"][it], rtol=1e-6)
            if source != "same":
                wv = np.sort(w.cpu().numpy().reshape(nsamp, -1), 1)
                np.testing.assert_allclose(wv, g[f"{tag}_weights_sorted"][it][:, :k], atol=1e-6)
            if it < 3:
                assert np.array_equal(fake[:, 0].cpu().numpy(), g[f"{tag}_fake_{it}"])
                assert real.shape == g[f"{tag}_real_{it}"].shape and rmask.shape == g[f"{tag}_rmask_{it}"].shape
                if source == "same":
                    assert np.array_equal(real.cpu().numpy(), g[f"{tag}_real_{it}"])
        np.testing.assert_array_equal(rng.uniform(0, 1, 4), g[f"{tag}_rng_after"])


def test_full_loop_with_patch_losses(dev):
    """train.py:133-264 end to end on a 256^2 synthetic image: pixel + contextual (+ LPIPS on
    'same' iterations) losses, all three patch sources exercised, fit still converges."""
    from npp_amd.fit import CompletionFit
    H, K = 256, 1
    img, mask = oracle.synthetic_image(H)
    angles, periods, shifts = oracle.synthetic_periodicity(H, K)
    fit = CompletionFit(img, mask, angles, periods, oracle.SEED0_FREQS, oracle.init_params(K, seed=0), device=dev,
                        N_rand=8192, shifts=shifts, seed=0)
    assert fit.patch_size == 64
    seen = set()
    lat0 = [l.clone() for l in fit.percepLoss.latents]
    for it in range(120):
        ok = fit.step_full()
        if ok:
            seen.add(fit.last_source)
            assert torch.isfinite(fit.last_patch_loss).all()
    assert seen == {"val", "train", "same"}
    assert fit.psnr() > 28.5 and fit.psnr("unknown") > 27.0
    # LPIPS robust latents were trained (only on 'same' iterations), adaptive_pix latents too
    assert any((a - b).abs().max() > 0 for a, b in zip(lat0, fit.percepLoss.latents))
    assert fit.net.global_step == 120 - fit.skipped



def test_complete_loop_at_the_reference_default_width_512(dev):
    """--netwidth 512 (options/arg_config.py:57) through the complete loop (sampler, fused chain of libnpp_hip_w512.so, pixel +
    contextual + LPIPS losses, Adam): converges like the W = 256 fit, and the explicit loop equals its autograd comparator."""
    from npp_amd.fit import CompletionFit
    H, K, Wn = 256, 3, 512
    img, mask = oracle.synthetic_image(H)
    angles, periods, shifts = oracle.synthetic_periodicity(H, K)

    def make():
        return CompletionFit(img, mask, angles, periods, oracle.SEED0_FREQS, oracle.init_params(K, W=Wn, seed=0), device=dev,
                             N_rand=4096, shifts=shifts, seed=1, width=Wn)
    a, b = make(), make()
    batch = a.materialise_batch(a.draw_batch())
    a.step_from(batch)
    step_from_autograd(b, batch)
    ga, gb = a.net.grads(), b.net.grads()
    for name in ga:
        assert rel_l2(ga[name], gb[name]) < 2e-3, name
    fit = make()
    assert fit.net.width == Wn and fit.net.n_params == 3836932 - 513
    p0 = fit.psnr()
    for it in range(60):
        fit.step_full()
    assert bool(torch.isfinite(fit.net.params).all()) and fit.psnr() > max(p0 + 8.0, 26.0)


def test_config_c5_shape_k5_with_patch_losses(dev):
    """BASELINE.json configs[4] shape at reduced image size: top-5 proposals (NPP_Net with a 4-proposal scale layer,
    in 2310) with the contextual loss every iteration and LPIPS on 'same' iterations, through the explicit loop."""
    from npp_amd.fit import CompletionFit
    H, K = 256, 5
    img, mask = oracle.synthetic_image(H)
    angles, periods, shifts = oracle.synthetic_periodicity(H, K)
    fit = CompletionFit(img, mask, angles, periods, oracle.SEED0_FREQS, oracle.init_params(K, seed=0), device=dev,
                        N_rand=4096, shifts=shifts, seed=1, ksplit=4)
    p0 = fit.psnr()
    seen = set()
    for it in range(60):
        if fit.step_full():
            seen.add(fit.last_source)
            assert torch.isfinite(fit.last_patch_loss).all() and torch.isfinite(fit.net.loss_buf).all()
    assert {"val", "train"} <= seen
    assert fit.psnr() > max(p0 + 8.0, 26.0)


def test_fast_rng_mode_fits_like_reference_mode(dev):
    """rng_mode='fast' (Generator.choice instead of full-population permutations) draws the same kind of samples:
    distinct in-range pixel rows / patch centres, and the fit reaches the same quality."""
    from npp_amd.fit import CompletionFit
    H, K = 256, 1
    img, mask = oracle.synthetic_image(H)
    angles, periods, shifts = oracle.synthetic_periodicity(H, K)
    res = {}
    for mode in ("reference", "fast"):
        fit = CompletionFit(img, mask, angles, periods, oracle.SEED0_FREQS, oracle.init_params(K, seed=0), device=dev,
                            N_rand=8192, shifts=shifts, seed=0, rng_mode=mode)
        b = None
        while b is None:
            b = fit.sample_batch()
        pix = b["coords"][:b["n_pix"]].cpu().numpy()
        assert len({(int(r), int(c)) for r, c in pix}) == b["n_pix"]              # without replacement
        assert mask[pix[:, 0], pix[:, 1], 0].min() == 1.0                          # all from the known (train) pool
        for it in range(100):
            fit.step_full()
        res[mode] = fit.psnr()
    assert res["fast"] > 28.5 and abs(res["fast"] - res["reference"]) < 0.5


def test_fit_trajectory_vs_reference_g8(dev, golden):
    """BASELINE.json: 'outputs match the reference NPP_completion/train.py PyTorch path on the same input image within
    0.1 dB PSNR'.  g8_fit.npz is the trajectory of the REFERENCE's own modules driven like train.py:164-263 (pixel-loss
    loop, PyTorch CPU fp32) on the synthetic 256^2 image; the HIP fit starts from the same weights (seed-0 default init),
    the same Fourier frequencies and draws the same pixel rows (same NumPy stream).  Measured: the two curves agree to
    0.01 dB at every checkpoint from iteration 1 (12.77 dB) to 300 (30.71 dB known / 30.12 dB unknown); asserted: 0.05 dB
    (bf16 MFMA operands vs fp32), half of BASELINE.json's 0.1 dB budget."""
    import sys
    import os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from refinit import reference_init
    from npp_amd.fit import CompletionFit
    g = golden("g8_fit.npz")
    H, N_rand = int(g["H"]), int(g["N_rand"])
    img, mask = oracle.synthetic_image(H)
    angles, periods, _ = oracle.synthetic_periodicity(H, 1)
    fit = CompletionFit(img, mask, angles, periods, g["freqs"], reference_init(1), device=dev, N_rand=N_rand, seed=0, ksplit=4,
                        rng_mode="reference")
    traj = {int(r[0]): r[1:] for r in g["traj"]}
    got = {}
    for i in range(1, 301):
        fit.step()
        if i in traj:
            got[i] = (fit.psnr("known"), fit.psnr("unknown"))
    assert sorted(got) == sorted(traj)
    for i, (pk, pu) in got.items():
        assert abs(pk - traj[i][0]) < 0.05 and abs(pu - traj[i][1]) < 0.05, (i, pk, pu, traj[i][:2])
    np.testing.assert_allclose(fit.net.latents.cpu().numpy(), np.concatenate([g["latent_alpha"], g["latent_scale"]], 1).reshape(-1),
                               atol=3e-3)                                   # the adaptive-loss latents end in the same place


def test_full_loop_trajectory_vs_reference_g8b(dev, golden):
    """The complete loop body against the reference's own modules (g8b_fit_patch.npz: models.sampler.GridPatchSampler +
    table gathers + NPP_Net_top1 + img2mse + the patch plumbing of train.py:200-236 + contextual_loss on a VGG19[0:18]-shaped
    trunk with the same fixed-seed weights, LPIPS term off on both sides): same weights, frequencies and NumPy stream.
    The patch-source / k sequence must be identical; PSNR checkpoints within 0.1 dB (the trunk runs in fp16/bf16 here and
    torch.topk's tie order among equidistant lattice candidates is backend-defined)."""
    import sys
    import os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from refinit import reference_init
    from npp_amd.fit import CompletionFit
    g = golden("g8b_fit_patch.npz")
    H, N_rand = int(g["H"]), int(g["N_rand"])
    img, mask = oracle.synthetic_image(H)
    angles, periods, shifts = oracle.synthetic_periodicity(H, 1)
    fit = CompletionFit(img, mask, angles, periods, g["freqs"], reference_init(1), device=dev, N_rand=N_rand, seed=0, ksplit=4,
                        shifts=shifts, rng_mode="reference", use_perceptual_loss=False)
    assert fit.patch_size == 64 and fit.patch_num == 2
    traj = {int(r[0]): r[1:] for r in g["traj"]}
    code = {"val": 0, "train": 1, "same": 2}
    for i in range(1, 101):
        ok = fit.step_full()
        d = fit.last_draw
        assert (code[d["source"]], d["k"]) == tuple(int(v) for v in g["seq"][i - 1]), i      # the sampler's decisions, call by call
        assert ok == (d["k"] > 0)
        if i in traj:
            pk, pu = fit.psnr("known"), fit.psnr("unknown")
            assert abs(pk - traj[i][0]) < 0.1 and abs(pu - traj[i][1]) < 0.1, (i, pk, pu, traj[i])
    assert fit.net.global_step == int(g["global_step"])


def test_fit_trajectory_vs_reference_g8k3(dev, golden):
    """The same as g8 for BASELINE config c2's network: NPP_Net with top-3 proposals (models/networks.py:56-95; scale layer on
    the two coarse-level proposals), the reference's own modules driven like train.py:164-263 for 150 iterations
    (g8k3_fit.npz).  Same weights (seed-0 default init in the reference's construction order), frequencies and NumPy stream."""
    import sys
    import os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from refinit import reference_init
    from npp_amd.fit import CompletionFit
    g = golden("g8k3_fit.npz")
    H, N_rand, K = int(g["H"]), int(g["N_rand"]), int(g["K"])
    assert K == 3
    img, mask = oracle.synthetic_image(H)
    angles, periods, _ = oracle.synthetic_periodicity(H, K)
    fit = CompletionFit(img, mask, angles, periods, g["freqs"], reference_init(K), device=dev, N_rand=N_rand, seed=0, ksplit=4,
                        rng_mode="reference")
    traj = {int(r[0]): r[1:] for r in g["traj"]}
    got = {}
    for i in range(1, max(traj) + 1):
        fit.step()
        if i in traj:
            got[i] = (fit.psnr("known"), fit.psnr("unknown"))
    for i, (pk, pu) in got.items():
        assert abs(pk - traj[i][0]) < 0.05 and abs(pu - traj[i][1]) < 0.05, (i, pk, pu, traj[i][:2])
    np.testing.assert_allclose(fit.net.latents.cpu().numpy(), np.concatenate([g["latent_alpha"], g["latent_scale"]], 1).reshape(-1),
                               atol=3e-3)


def test_fit_trajectory_vs_reference_g8c2_full_size(dev, golden):
    """BASELINE config c2 at its REAL size -- 512 x 512 image, top-3 proposals, W = 256, 8192 rows per iteration -- against the
    reference's own modules driven like train.py:164-263 for 60 iterations (g8c2_fit.npz, tests/golden/make_golden_fit.py --c2):
    PSNR over the known / unknown pixels within 0.1 dB (BASELINE.json's budget) at every checkpoint, adaptive-loss latents 3e-3."""
    import sys
    import os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from refinit import reference_init
    from npp_amd.fit import CompletionFit
    g = golden("g8c2_fit.npz")
    H, N_rand, K = int(g["H"]), int(g["N_rand"]), int(g["K"])
    assert (H, K, int(g["W"])) == (512, 3, 256)
    img, mask = oracle.synthetic_image(H)
    angles, periods, _ = oracle.synthetic_periodicity(H, K)
    fit = CompletionFit(img, mask, angles, periods, g["freqs"], reference_init(K), device=dev, N_rand=N_rand, seed=0, rng_mode="reference")
    traj = {int(r[0]): r[1:] for r in g["traj"]}
    for i in range(1, max(traj) + 1):
        fit.step()
        if i in traj:
            pk, pu = fit.psnr("known"), fit.psnr("unknown")
            assert abs(pk - traj[i][0]) < 0.1 and abs(pu - traj[i][1]) < 0.1, (i, pk, pu, traj[i][:2])
    np.testing.assert_allclose(fit.net.latents.cpu().numpy(), np.concatenate([g["latent_alpha"], g["latent_scale"]], 1).reshape(-1),
                               atol=3e-3)


def test_fit_trajectory_vs_reference_g8c5_full_size(dev, golden):
    """BASELINE config c5's network at its REAL size -- 512 x 512 image, top-5 proposals (a 4-proposal scale layer, 2310 inputs),
    W = 256, 8192 rows per iteration -- against the reference's own modules for 60 iterations (g8c5_fit.npz, make_golden_fit.py --c5):
    PSNR within 0.1 dB at every checkpoint, latents 3e-3."""
    import sys
    import os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from refinit import reference_init
    from npp_amd.fit import CompletionFit
    g = golden("g8c5_fit.npz")
    H, N_rand, K = int(g["H"]), int(g["N_rand"]), int(g["K"])
    assert (H, K, int(g["W"])) == (512, 5, 256)
    img, mask = oracle.synthetic_image(H)
    angles, periods, _ = oracle.synthetic_periodicity(H, K)
    fit = CompletionFit(img, mask, angles, periods, g["freqs"], reference_init(K), device=dev, N_rand=N_rand, seed=0, rng_mode="reference")
    traj = {int(r[0]): r[1:] for r in g["traj"]}
    for i in range(1, max(traj) + 1):
        fit.step()
        if i in traj:
            pk, pu = fit.psnr("known"), fit.psnr("unknown")
            assert abs(pk - traj[i][0]) < 0.1 and abs(pu - traj[i][1]) < 0.1, (i, pk, pu, traj[i][:2])
    np.testing.assert_allclose(fit.net.latents.cpu().numpy(), np.concatenate([g["latent_alpha"], g["latent_scale"]], 1).reshape(-1),
                               atol=3e-3)


def test_fit_trajectory_vs_reference_g8s1024(dev, golden):
    """A 1024 x 1024 image (the grid size of BASELINE configs c2 / c4: coordinates beyond 512, 1 M-pixel renders), top-3 proposals,
    W = 256: 40 iterations of the reference's own modules (g8s1024_fit.npz, make_golden_fit.py --s1024), PSNR within 0.1 dB at every
    checkpoint, latents 3e-3."""
    import sys
    import os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from refinit import reference_init
    from npp_amd.fit import CompletionFit
    g = golden("g8s1024_fit.npz")
    H, N_rand, K = int(g["H"]), int(g["N_rand"]), int(g["K"])
    assert (H, K, int(g["W"])) == (1024, 3, 256)
    img, mask = oracle.synthetic_image(H)
    angles, periods, _ = oracle.synthetic_periodicity(H, K)
    fit = CompletionFit(img, mask, angles, periods, g["freqs"], reference_init(K), device=dev, N_rand=N_rand, seed=0, rng_mode="reference")
    traj = {int(r[0]): r[1:] for r in g["traj"]}
    for i in range(1, max(traj) + 1):
        fit.step()
        if i in traj:
            pk, pu = fit.psnr("known"), fit.psnr("unknown")
            assert abs(pk - traj[i][0]) < 0.1 and abs(pu - traj[i][1]) < 0.1, (i, pk, pu, traj[i][:2])
    np.testing.assert_allclose(fit.net.latents.cpu().numpy(), np.concatenate([g["latent_alpha"], g["latent_scale"]], 1).reshape(-1),
                               atol=3e-3)


def test_fit_trajectory_vs_reference_g8k5(dev, golden):
    """g8k3's recipe for BASELINE config c5's network: NPP_Net with top-5 proposals (a 4-proposal scale layer, 2310 inputs), the
    reference's own modules for 100 iterations (g8k5_fit.npz, make_golden_fit.py --k5)."""
    import sys
    import os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from refinit import reference_init
    from npp_amd.fit import CompletionFit
    g = golden("g8k5_fit.npz")
    H, N_rand, K = int(g["H"]), int(g["N_rand"]), int(g["K"])
    assert K == 5
    img, mask = oracle.synthetic_image(H)
    angles, periods, _ = oracle.synthetic_periodicity(H, K)
    fit = CompletionFit(img, mask, angles, periods, g["freqs"], reference_init(K), device=dev, N_rand=N_rand, seed=0, rng_mode="reference")
    traj = {int(r[0]): r[1:] for r in g["traj"]}
    for i in range(1, max(traj) + 1):
        fit.step()
        if i in traj:
            pk, pu = fit.psnr("known"), fit.psnr("unknown")
            assert abs(pk - traj[i][0]) < 0.1 and abs(pu - traj[i][1]) < 0.1, (i, pk, pu, traj[i][:2])
    np.testing.assert_allclose(fit.net.latents.cpu().numpy(), np.concatenate([g["latent_alpha"], g["latent_scale"]], 1).reshape(-1),
                               atol=3e-3)


def test_fit_trajectory_vs_reference_g8w512(dev, golden):
    """g8k3's recipe at the reference's DEFAULT width (--netwidth 512, options/arg_config.py:57): the reference's NPP_Net(W = 512)
    driven like train.py:164-263 for 100 iterations (g8w512_fit.npz, tests/golden/make_golden_fit.py --w512) against the fused
    chain of libnpp_hip_w512.so from the same initial weights, frequencies and NumPy stream."""
    import sys
    import os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from refinit import reference_init
    from npp_amd.fit import CompletionFit
    g = golden("g8w512_fit.npz")
    H, N_rand, K, Wn = int(g["H"]), int(g["N_rand"]), int(g["K"]), int(g["W"])
    assert (K, Wn) == (3, 512)
    img, mask = oracle.synthetic_image(H)
    angles, periods, _ = oracle.synthetic_periodicity(H, K)
    fit = CompletionFit(img, mask, angles, periods, g["freqs"], reference_init(K, W=Wn), device=dev, N_rand=N_rand, seed=0,
                        rng_mode="reference", width=Wn)
    traj = {int(r[0]): r[1:] for r in g["traj"]}
    got = {}
    for i in range(1, max(traj) + 1):
        fit.step()
        if i in traj:
            got[i] = (fit.psnr("known"), fit.psnr("unknown"))
    for i, (pk, pu) in got.items():
        assert abs(pk - traj[i][0]) < 0.1 and abs(pu - traj[i][1]) < 0.1, (i, pk, pu, traj[i][:2])       # BASELINE: within 0.1 dB
    np.testing.assert_allclose(fit.net.latents.cpu().numpy(), np.concatenate([g["latent_alpha"], g["latent_scale"]], 1).reshape(-1),
                               atol=3e-3)


def test_full_loop_with_lpips_trajectory_vs_reference_g8c(dev, golden):
    """g8b with the LPIPS term ON (VERDICT r1 #5a): the reference's own LPIPS.forward (externel_lib/lpips/lpips.py:92-133, the
    vendored lin weights, its per-layer AdaptiveLossFunction latents in the SAME Adam as the network, helpers.py:147-151)
    on a fixed-seed VGG16-shaped trunk, added on 'same' iterations exactly like train.py:241-251.  Asserted: the patch-source / k
    sequence call by call, the weighted patch loss of the first iterations (before the two fits' roundings have moved the
    parameters apart), the PSNR checkpoints within BASELINE's 0.1 dB, and where the 2 x 1472 LPIPS latents end up."""
    import sys
    import os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from refinit import reference_init
    from npp_amd.fit import CompletionFit
    g = golden("g8c_fit_lpips.npz")
    H, N_rand = int(g["H"]), int(g["N_rand"])
    img, mask = oracle.synthetic_image(H)
    angles, periods, shifts = oracle.synthetic_periodicity(H, 1)
    fit = CompletionFit(img, mask, angles, periods, g["freqs"], reference_init(1), device=dev, N_rand=N_rand, seed=0, ksplit=4,
                        shifts=shifts, rng_mode="reference", use_perceptual_loss=True,
                        lpips_lin_weights=[g[f"lin{k}"] for k in range(5)])
    traj = {int(r[0]): r[1:] for r in g["traj"]}
    ploss = {int(r[0]): r[1] for r in g["patch_loss"]}
    code = {"val": 0, "train": 1, "same": 2}
    n_same = 0
    for i in range(1, 101):
        ok = fit.step_full()
        d = fit.last_draw
        assert (code[d["source"]], d["k"]) == tuple(int(v) for v in g["seq"][i - 1]), i
        assert ok == (d["k"] > 0) == (i in ploss)
        if ok:
            n_same += d["source"] == "same"
            if i <= 30:
                # 'same' iterations (real := fake, k = 1) have no tie among equidistant lattice candidates to break, so their
                # patch loss = 1e-3 (CX + mean LPIPS-robust) is comparable value by value; on the others torch.topk's
                # backend-defined tie order picks other real patches and only the scale is comparable
                got = float(fit.last_patch_loss[0])
                tol = 3e-2 if d["source"] == "same" else 0.35
                assert abs(got - ploss[i]) < tol * abs(ploss[i]), (i, d["source"], got, ploss[i])
        if i in traj:
            pk, pu = fit.psnr("known"), fit.psnr("unknown")
            assert abs(pk - traj[i][0]) < 0.1 and abs(pu - traj[i][1]) < 0.1, (i, pk, pu, traj[i])
    assert n_same == len(g["lpips_values"]) and fit.net.global_step == int(g["global_step"])
    for k, lat in enumerate(fit.percepLoss.latents):                    # [latent_alpha (C) | latent_scale (C)] per tap
        want = np.concatenate([g[f"la{k}"].reshape(-1), g[f"ls{k}"].reshape(-1)])
        np.testing.assert_allclose(lat.cpu().numpy(), want, atol=2e-3)


def test_complete_iteration_at_c2_size_vs_reference_g8c2(dev, golden):
    """g8c at BASELINE config c2's REAL size: 512^2, NPP_Net with the top-3 proposals, 8192 pixel rows + 2 patches of 96^2 against
    3 real patches, the contextual loss every iteration and the reference's LPIPS.forward on 'same' ones -- 60 iterations of
    train.py:166-266 run by the reference itself (tests/golden/make_golden_fit_patch.py --c2).  The bench's workload, pinned."""
    import sys
    import os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from refinit import reference_init
    from npp_amd.fit import CompletionFit
    g = golden("g8c2_loop.npz")
    H, N_rand, K = int(g["H"]), int(g["N_rand"]), int(g["K"])
    assert (H, K) == (512, 3)
    img, mask = oracle.synthetic_image(H)
    angles, periods, shifts = oracle.synthetic_periodicity(H, K)
    fit = CompletionFit(img, mask, angles, periods, g["freqs"], reference_init(K), device=dev, N_rand=N_rand, seed=0, ksplit=4,
                        shifts=shifts, rng_mode="reference", use_perceptual_loss=True,
                        lpips_lin_weights=[g[f"lin{k}"] for k in range(5)])
    assert fit.patch_size == int(g["P"]) == 96
    traj = {int(r[0]): r[1:] for r in g["traj"]}
    ploss = {int(r[0]): r[1] for r in g["patch_loss"]}
    code = {"val": 0, "train": 1, "same": 2}
    n_same = 0
    for i in range(1, 61):
        ok = fit.step_full()
        d = fit.last_draw
        assert (code[d["source"]], d["k"]) == tuple(int(v) for v in g["seq"][i - 1]), i
        assert ok == (d["k"] > 0) == (i in ploss)
        if ok:
            n_same += d["source"] == "same"
            if i <= 20:
                got = float(fit.last_patch_loss[0])
                tol = 3e-2 if d["source"] == "same" else 0.35           # see g8c: topk ties on the other sources
                assert abs(got - ploss[i]) < tol * abs(ploss[i]), (i, d["source"], got, ploss[i])
        if i in traj:
            pk, pu = fit.psnr("known"), fit.psnr("unknown")
            assert abs(pk - traj[i][0]) < 0.1 and abs(pu - traj[i][1]) < 0.1, (i, pk, pu, traj[i])
    assert n_same == len(g["lpips_values"]) and fit.net.global_step == int(g["global_step"])
    for k, lat in enumerate(fit.percepLoss.latents):
        want = np.concatenate([g[f"la{k}"].reshape(-1), g[f"ls{k}"].reshape(-1)])
        np.testing.assert_allclose(lat.cpu().numpy(), want, atol=2e-3)


def test_full_length_c2_fit_vs_reference_output_g8c2_full(dev, golden):
    """The OUTPUT, not a prefix (VERDICT r5 "Missing #2"): BASELINE config c2's complete fit for the reference's full iteration
    count -- `for i in trange(1, 2001)`, NPP_completion/train.py:133, options/arg_config.py:96 -- including the patch-size decay
    that fires at i = 2000 (train.py:137-141: patch 96 -> 48, patch_num 2 -> 4), against g8c2_full.npz (the reference's modules
    driven for all 2000 iterations, tests/golden/make_golden_fit_full.py, tie order defined as in g8d).  Asserted: the (patch
    source, k) of every iteration; the weighted patch loss of EVERY source to 3 % over the first 60 iterations (the bench's own
    workload; 'val' / 'train' iterations could only be held to 35 % against the unstable-tie golden g8c2_loop); PSNR vs the ground
    truth within 0.1 dB of the reference at iterations 100 / 250 / 500 / 1000 / 1500 / 2000; the decay; and the fitted IMAGE against the
    reference's fitted image (uint8): PSNR(HIP, reference) above the floors below -- two fits whose every step differs at
    rounding level (bf16 / 8-bit-stash operands here, fp32 there) agree with each other far better than either agrees with the
    ground truth (31.3 / 29.4 dB)."""
    from npp_amd.fit import CompletionFit
    from refinit import reference_init
    g = golden("g8c2_full.npz")
    H, N_rand, K, n_it = int(g["H"]), int(g["N_rand"]), int(g["K"]), int(g["n_iters"])
    assert (H, K, n_it) == (512, 3, 2000)
    img, mask = oracle.synthetic_image(H)
    angles, periods, shifts = oracle.synthetic_periodicity(H, K)
    fit = CompletionFit(img, mask, angles, periods, g["freqs"], reference_init(K), device=dev, N_rand=N_rand, seed=0, ksplit=4,
                        shifts=shifts, rng_mode="reference", use_perceptual_loss=True, patch_size_decay=int(g["decay"]),
                        lpips_lin_weights=[g[f"lin{k}"] for k in range(5)])
    assert fit.patch_size == int(g["P"]) == 96
    traj = {int(r[0]): r[1:] for r in g["traj"]}
    ploss = {int(r[0]): r[1] for r in g["patch_loss"]}
    code = {"val": 0, "train": 1, "same": 2}
    n_same, worst = 0, {}
    for i in range(1, n_it + 1):
        ok = fit.step_full()
        d = fit.last_draw
        assert (code[d["source"]], d["k"]) == tuple(int(v) for v in g["seq"][i - 1]), i
        assert (d["P"], d["n_p"]) == tuple(int(v) for v in g["sizes"][i - 1]), i        # (the draw's own sizes: the sampler runs one iteration ahead)
        assert ok == (d["k"] > 0) == (i in ploss)
        if ok:
            n_same += d["source"] == "same"
            if i <= 60:
                rel = abs(float(fit.last_patch_loss[0]) - ploss[i]) / abs(ploss[i])
                worst[d["source"]] = max(worst.get(d["source"], 0.0), rel)
                assert rel < 3e-2, (i, d["source"], float(fit.last_patch_loss[0]), ploss[i])
        if i in traj:
            pk, pu = fit.psnr("known"), fit.psnr("unknown")
            assert abs(pk - traj[i][0]) < 0.1 and abs(pu - traj[i][1]) < 0.1, (i, pk, pu, traj[i])
    assert set(worst) == {"val", "train", "same"}
    assert (fit.patch_size, fit.patch_num) == (48, 4)                        # the decay of iteration 2000 happened
    assert n_same == len(g["lpips_values"]) and fit.net.global_step == int(g["global_step"])
    # the output
    out = fit.render_image().clamp(0, 1).cpu().numpy()
    ref = g["final_image_u8"].astype(np.float32) / 255.0
    m = mask.astype(np.float32)

    def psnr_between(a, b, w):
        return float(-10 * np.log10((((a - b) ** 2) * w).sum() / (w.sum() * 3)))
    pk, pu = psnr_between(out, ref, m), psnr_between(out, ref, 1 - m)
    print(f"fitted image vs the reference's fitted image: {pk:.2f} dB over known pixels, {pu:.2f} dB over unknown; "
          f"worst early patch-loss deviation per source {worst}")
    # measured: 55.1 / 53.9 dB with the 8-bit stash, 58.1 / 58.0 dB with the 16-bit one (the uint8 golden's own floor is 58.9 dB)
    assert pk > 48.0 and pu > 46.0, (pk, pu)
    fit.close()


def test_native_stream_and_prefetch_reproduce_numpy_sequence(dev):
    """rng_mode='reference' (the library's MT19937) draws exactly what rng_mode='numpy' (np.random.RandomState) draws, with
    and without the producer thread: same patch sources, centres, pixel rows, skipped iterations -- the reference's stream
    (models/sampler.py:260,324; train.py:172)."""
    from npp_amd.fit import CompletionFit
    H, K = 256, 1
    img, mask = oracle.synthetic_image(H)
    angles, periods, shifts = oracle.synthetic_periodicity(H, K)
    seqs = {}
    for tag, mode, pf in (("numpy", "numpy", 0), ("native", "reference", 0), ("native+prefetch", "reference", 3)):
        fit = CompletionFit(img, mask, angles, periods, oracle.SEED0_FREQS, oracle.init_params(K, seed=0), device=dev,
                            N_rand=4096, shifts=shifts, seed=5, rng_mode=mode, prefetch=pf)
        seq = []
        for it in range(25):
            ok = fit.step_full()
            d = fit.last_draw
            seq.append((ok, d["source"], d["k"], d["cen"].tolist(), None if d["real_cen"] is None else d["real_cen"].tolist(),
                        d["pix"].tolist() if ok else None))
        seqs[tag] = (seq, fit.net.params.cpu().numpy().copy())
        fit.close()
    for tag in ("native", "native+prefetch"):
        assert seqs[tag][0] == seqs["numpy"][0]                                # every draw of every iteration, exactly
        # same draws -> same fit (not bit-identical: the contextual-loss kernels reduce with float atomics)
        assert rel_l2(seqs[tag][1], seqs["numpy"][1]) < 2e-2


def test_training_step_is_bit_reproducible(dev):
    """No atomics on the gradient path: split-K slabs + a fixed summation order make two runs of
    the same step produce identical bits (weights after 3 optimiser steps)."""
    K, H, n = 3, 256, 1024
    outs = []
    for rep in range(2):
        net, P, angles, periods = _net(dev, K, ksplit=4)
        c = torch.from_numpy(_coords(n, H, H, seed=3)).to(dev)
        gt = torch.from_numpy(np.random.RandomState(1).rand(n, 3).astype(np.float32)).to(dev)
        for it in range(3):
            net.zero_grad(); net.forward_train(c); net.workspace(n)["dpred"].zero_()
            net.pixel_loss(n, n, gt); net.backward(n); net.optimizer_step(n)
        outs.append(net.params.cpu().numpy().copy())
    assert np.array_equal(outs[0], outs[1])


def test_complete_iteration_is_bit_reproducible(dev):
    """Round 4: no float atomics left on the path of the complete iteration -- the contextual core sums its channel-tile partials in
    a fixed order, the pixel loss and its latent gradients are summed by the last-arriving block in block order, the LPIPS head adds
    fixed-point integers -- so two runs of the same 30 iterations (all three patch sources, the LPIPS branch on its side stream)
    end at identical bits: network parameters, Adam moments, pixel-loss and LPIPS latents."""
    from npp_amd.fit import CompletionFit
    H, K = 256, 3
    img, mask = oracle.synthetic_image(H)
    angles, periods, shifts = oracle.synthetic_periodicity(H, K)
    outs = []
    for rep in range(2):
        fit = CompletionFit(img, mask, angles, periods, oracle.SEED0_FREQS, oracle.init_params(K, seed=0), device=dev, N_rand=4096,
                            shifts=shifts, seed=4)
        seen = set()
        for _ in range(30):
            if fit.step_full():
                seen.add(fit.last_source)
        torch.cuda.synchronize()
        assert seen == {"val", "train", "same"}
        outs.append([t.clone() for t in (fit.net.params, fit.net.m, fit.net.v, fit.net.latents, fit.percepLoss._lat)])
    for a, b in zip(*outs):
        assert torch.equal(a, b), float((a - b).abs().max())


def test_two_fits_on_two_streams_equal_their_serial_runs(dev):
    """Two fits of the SAME shape interleaved on two streams (bench.py's throughput mode, config c3 with more images than GPUs): every
    scratch buffer a launch sequence keeps across launches -- the contextual core's matrices and last-arriver tickets, the LPIPS
    accumulators -- is per stream, so each fit ends at the bits of its own serial run."""
    from npp_amd.fit import CompletionFit
    H, K = 256, 3
    angles, periods, shifts = oracle.synthetic_periodicity(H, K)

    def make(seed, stream=None):
        img, mask = oracle.synthetic_image(H, seed=seed)               # (another noise draw: a second image of the same shape)
        return CompletionFit(img, mask, angles, periods, oracle.SEED0_FREQS, oracle.init_params(K, seed=seed), device=dev, N_rand=4096,
                             shifts=shifts, seed=4 + seed)

    def state(f):
        return [t.clone() for t in (f.net.params, f.net.m, f.net.v, f.net.latents, f.percepLoss._lat)]
    serial = []
    for seed in (0, 1):
        f = make(seed)
        pool = []
        while len(pool) < 12:
            b = f.sample_batch()
            if b is not None:
                pool.append(b)
        for b in pool:
            f.step_from(b)
        torch.cuda.synchronize()
        serial.append(state(f))
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    fits, pools = [], []
    for seed in (0, 1):
        with torch.cuda.stream(streams[seed]):
            f = make(seed)
            pool = []
            while len(pool) < 12:
                b = f.sample_batch()
                if b is not None:
                    pool.append(b)
        fits.append(f)
        pools.append(pool)
    torch.cuda.synchronize()
    assert {b["source"] for b in pools[0]} | {b["source"] for b in pools[1]} == {"val", "train", "same"}
    for i in range(12):
        for r in range(2):
            with torch.cuda.stream(streams[r]):
                fits[r].step_from(pools[r][i])
    torch.cuda.synchronize()
    for r in range(2):
        for a, b in zip(serial[r], state(fits[r])):
            assert torch.equal(a, b), (r, float((a - b).abs().max()))


def test_patch_plumbing_inside_the_first_trunk_launch_is_bit_identical(dev):
    """npp_conv_pair_fwd_patch (the patch batch composed inside the first block's fused launch, the adaptive pixel loss in the launch's
    last blocks: no npp_trunk_patch_in launch on 'val' / 'train' iterations) against the separate launches: identical parameters, Adam
    moments and latents after iterations of every patch source."""
    from npp_amd.fit import CompletionFit
    H, K = 256, 3
    img, mask = oracle.synthetic_image(H)
    angles, periods, shifts = oracle.synthetic_periodicity(H, K)
    outs = []
    for mask_bits in (15, 7):
        fit = CompletionFit(img, mask, angles, periods, oracle.SEED0_FREQS, oracle.init_params(K, seed=0), device=dev, N_rand=4096,
                            shifts=shifts, seed=4)
        fit.contextualLoss.hip_trunk.fuse_pairs = mask_bits
        assert fit.contextualLoss.hip_trunk.can_compose_input(fit.patch_size, fit.patch_size) == (mask_bits == 15)
        seen = set()
        for _ in range(16):
            if fit.step_full():
                seen.add(fit.last_source)
        torch.cuda.synchronize()
        assert {"val", "train"} <= seen
        outs.append([t.clone() for t in (fit.net.params, fit.net.m, fit.net.v, fit.net.latents, fit.last_patch_loss)])
    for a, b in zip(*outs):
        assert torch.equal(a, b), float((a - b).abs().max())


def test_minimal_and_ragged_batches(dev):
    """One 64-row tile (the smallest launch) and a batch that is not a multiple of the tile."""
    K, H = 3, 256
    net, P, angles, periods = _net(dev, K)
    for n in (1, 64, 65, 200):
        c = _coords(n, H, H, seed=n)
        pred = net.render(torch.from_numpy(c).to(dev)).cpu().numpy()
        emb = oracle.embed(c, angles, periods, oracle.SEED0_FREQS, (H, H))
        raw, _ = oracle.mlp_forward(P, emb, K, emulate_bf16=True)
        assert pred.shape == (n, 3) and np.abs(pred - oracle.sigmoid(raw)).max() < 4e-3


def test_error_reporting_on_bad_arguments(dev):
    """Bad sizes / pointers are rejected on the host with a status and a message, never launched."""
    import ctypes as C
    import npp_amd
    from npp_amd import ops
    L = npp_amd.lib()
    cfg, *_ = _cfg(3)
    c = torch.zeros((100, 2), dtype=torch.int32, device=dev)        # 100 rows: not a multiple of 64
    with pytest.raises(npp_amd.NppError, match="multiple of 64"):
        ops.mlp_fwd(c, cfg, torch.empty(16, device=dev), torch.empty(16, device=dev))
    c64 = torch.zeros((64, 2), dtype=torch.int32, device=dev)
    with pytest.raises(npp_amd.NppError, match="width"):                     # no fused library for this width (dense.py serves it)
        ops.mlp_fwd(c64, cfg, torch.empty(16, device=dev), torch.empty(16, device=dev), width=384)
    from npp_amd._lib import check as _check
    with pytest.raises(npp_amd.NppError, match="width"):                     # each library rejects the other's width on the host
        _check(npp_amd.lib(512).npp_mlp_fwd(c64.data_ptr(), 64, C.byref(cfg), 256, c64.data_ptr(), c64.data_ptr(), c64.data_ptr(), None,
                                            None), "npp_mlp_fwd", 512)
    with pytest.raises(npp_amd.NppError, match="width"):
        _check(L.npp_mlp_fwd(c64.data_ptr(), 64, C.byref(cfg), 512, c64.data_ptr(), c64.data_ptr(), c64.data_ptr(), None, None),
               "npp_mlp_fwd")
    with pytest.raises(npp_amd.NppError, match="null"):
        L.npp_mlp_fwd.restype = C.c_int
        from npp_amd._lib import check
        check(L.npp_mlp_fwd(None, 64, C.byref(cfg), 256, None, None, None, None, None), "npp_mlp_fwd")
    bad = _cfg(3)[0]
    bad.periods[0][0] = 0.5          # period + offset(-1) <= 0
    with pytest.raises(npp_amd.NppError, match="period"):
        ops.embed_fwd(c64, bad)
    with pytest.raises(TypeError):
        ops.embed_fwd(c64.long(), cfg)


def test_remapping_variant_with_style_loss(dev):
    """NPP_remapping's loop (train.py:158-300): trains on the whole image, the clear (sharp) region is the 'val' pool and
    the sampler mask, blurry pixels carry the 0.3-weighted pixel loss (gt_mask = clear_mask, mse_calculator.py:17), and the
    Gram-matrix style loss joins the contextual loss.  Synthetic check of the task itself: a band of the lattice image is
    box-blurred; after the fit the prediction inside the band is closer to the SHARP pattern than the blurred input is."""
    from npp_amd.fit import CompletionFit
    H, K = 256, 1
    clean, _ = oracle.synthetic_image(H, noise=0.01)
    angles, periods, shifts = oracle.synthetic_periodicity(H, K)
    blurred = clean.copy()
    band = slice(96, 160)
    k = 9
    pad = np.pad(clean, ((k // 2, k // 2), (k // 2, k // 2), (0, 0)), mode="edge")
    box = sum(pad[dy:dy + H, dx:dx + H] for dy in range(k) for dx in range(k)) / (k * k)
    blurred[band] = box[band]
    clear = np.ones((H, H, 1), np.float32)
    clear[band] = 0
    fit = CompletionFit(blurred, np.ones((H, H, 1), np.float32), angles, periods, oracle.SEED0_FREQS, oracle.init_params(K, seed=0),
                        device=dev, N_rand=8192, shifts=shifts, seed=0, rng_mode="fast", task="remapping", clear_mask=clear,
                        contextual_weight=0.01, use_perceptual_loss=False)
    assert fit.style is not None and fit.i_train.shape[0] == H * H and fit.i_val.shape[0] == int(clear.sum())
    lat0 = [l.clone() for l in fit.style.latents]
    for it in range(200):
        fit.step_full()
        assert torch.isfinite(fit.last_patch_loss).all()
    pred = fit.render_image().cpu().numpy()

    def psnr(a, b):
        return -10 * np.log10(np.mean((a - b) ** 2))
    p_in, p_out = psnr(blurred[band], clean[band]), psnr(pred[band], clean[band])
    assert p_out > p_in + 3.0, (p_in, p_out)                          # the band was re-synthesised from the sharp periodic content
    assert psnr(pred[:90], clean[:90]) > 27.0
    assert any((a - b).abs().max() > 0 for a, b in zip(lat0, fit.style.latents))     # style latents are trained


@pytest.mark.parametrize("mode", ["reference", "fast"])
def test_checkpoint_resume_continues_the_same_fit(dev, mode):
    """state_dict() / load_state_dict() (the reference has no checkpointing): a fit resumed in a FRESH
    object draws the same samples and ends at the same weights as the uninterrupted one."""
    from npp_amd.fit import CompletionFit
    H, K = 256, 1
    img, mask = oracle.synthetic_image(H)
    angles, periods, shifts = oracle.synthetic_periodicity(H, K)

    def make():
        return CompletionFit(img, mask, angles, periods, oracle.SEED0_FREQS, oracle.init_params(K, seed=0), device=dev, N_rand=4096,
                             shifts=shifts, seed=11, rng_mode=mode, use_perceptual_loss=False)
    a = make()
    for _ in range(12):
        a.step_full()
    sd = a.state_dict()
    tail_a = []
    for _ in range(10):
        a.step_full()
        tail_a.append((a.last_draw["source"], a.last_draw["k"], a.last_draw["cen"].tolist(), a.last_draw["pix"][:8].tolist()))
    b = make()
    b.load_state_dict(sd)
    tail_b = []
    for _ in range(10):
        b.step_full()
        tail_b.append((b.last_draw["source"], b.last_draw["k"], b.last_draw["cen"].tolist(), b.last_draw["pix"][:8].tolist()))
    assert tail_a == tail_b
    assert (a.net.global_step, a.net.opt_step, a.iteration) == (b.net.global_step, b.net.opt_step, b.iteration)
    assert rel_l2(b.net.params.cpu().numpy(), a.net.params.cpu().numpy()) < 5e-3     # float atomics in the CX kernels: not bitwise
    assert abs(a.psnr() - b.psnr()) < 0.05


@pytest.mark.parametrize("source", ["val", "same"])
def test_folded_launches_equal_the_separate_ones(dev, source):
    """npp_trunk_patch_in_loss (pixel loss riding in the patch-in launch) and npp_mlp_bwd_patch (npp_patch_compose_bwd formed inside
    the backward launch) against the separate launches on the same batch: dL/dpred bit-identical on the pixel rows and on the
    patch rows up to the float atomics of the contextual-loss kernels, same loss, same parameters after the step."""
    from npp_amd.fit import CompletionFit
    H, K = 256, 3
    img, mask = oracle.synthetic_image(H)
    angles, periods, shifts = oracle.synthetic_periodicity(H, K)

    def make(fold):
        f = CompletionFit(img, mask, angles, periods, oracle.SEED0_FREQS, oracle.init_params(K, seed=0), device=dev, N_rand=2048,
                          shifts=shifts, seed=3)
        f.fold_launches = fold
        return f
    a, b = make(True), make(False)
    batch = None
    for _ in range(40):
        d = a.draw_batch()
        if d is not None and d["source"] == source:
            batch = a.materialise_batch(d)
            break
    assert batch is not None
    a.step_from(batch)
    b.step_from(batch)
    n_pix, n, bp = batch["n_pix"], batch["n"], batch["bp"]
    da, db = a.net.workspace(bp)["dpred"], b.net.workspace(bp)["dpred"]
    assert torch.equal(da[:n_pix], db[:n_pix])
    # (two runs of the SAME path differ by ~1e-3 here: the contextual-loss kernels reduce with float atomics and the similarity
    # normalisation amplifies the last bits -- the budget of test_gpu_fullsize's explicit-vs-autograd comparison)
    assert rel_l2(da[n_pix:n].cpu().numpy(), db[n_pix:n].cpu().numpy()) < 6e-3 and (n == bp or float(da[n:].abs().max()) == 0.0)
    assert abs(float(a.net.loss_buf[0]) - float(b.net.loss_buf[0])) < 1e-6 * abs(float(b.net.loss_buf[0])) + 1e-9
    assert rel_l2(a.net.params.cpu().numpy(), b.net.params.cpu().numpy()) < 2e-4


@pytest.mark.parametrize("K,width", [(3, 256), (1, 256), (5, 256), (3, 512)])
def test_fused_adam_repack_equals_adam_then_pack(dev, K, width):
    """npp_adam_step_net_pack (optimizer.step() + the scatter of every updated weight into both bf16 packs, one launch) against
    npp_adam_step_net followed by npp_pack_weights: parameters, Adam moments, latents and both packs bit-identical after three
    training steps from the same state."""
    H, n = 256, 512
    c = torch.from_numpy(_coords(n, H, H)).to(dev)
    gt = torch.rand(n, 3, device=dev)
    nets = []
    for fused in (True, False):
        net, *_ = _net(dev, K, ksplit=3, width=width)
        net.fused_repack = fused
        for _ in range(3):
            net.zero_grad()
            net.forward_train(c)
            net.workspace(n)["dpred"].zero_()
            net.pixel_loss(n, n, gt)
            net.backward(n)
            net.optimizer_step(n)
        nets.append(net)
    a, b = nets
    for name in ("params", "m", "v", "latents", "lat_m", "lat_v", "wf", "wb"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


def _run_task_golden(dev, g, fit, n_iters=100, loss_tol=0.03, n_loss=20, loss_tol_all=0.05):
    """Shared body of the g8r / g8s / g8d tests: sampler decisions call by call, weighted patch loss of the first iterations value
    by value (the goldens use the stable tie order, tests/golden/make_golden_fit_tasks.py), PSNR checkpoints within BASELINE's
    0.1 dB, pixel-loss latents, LR clock.  The loss values are compared over the first 20 iterations: the contextual core reduces
    with float atomics, so two runs of THIS code drift apart by a few percent of a 1e-7-sized loss by iteration 30 (seen once in
    ~10 runs at 3.6 %); the PSNR checkpoints and latents cover the rest of the trajectory."""
    traj = {int(r[0]): r[1:] for r in g["traj"]}
    ploss = {int(r[0]): r[1] for r in g["patch_loss"]}
    code = {"val": 0, "train": 1, "same": 2}
    n_same = 0
    dev_all = []
    for i in range(1, n_iters + 1):
        ok = fit.step_full()
        d = fit.last_draw
        assert (code[d["source"]], d["k"]) == tuple(int(v) for v in g["seq"][i - 1]), i
        assert ok == (d["k"] > 0) == (i in ploss)
        if ok:
            n_same += d["source"] == "same"
            got = float(fit.last_patch_loss[0])
            dev_all.append((abs(got - ploss[i]) / abs(ploss[i]), i, d["source"]))
            if i <= n_loss:
                assert abs(got - ploss[i]) < loss_tol * abs(ploss[i]), (i, d["source"], got, ploss[i])
        if i in traj:
            pk, pu = fit.psnr("known"), fit.psnr("unknown")
            assert abs(pk - traj[i][0]) < 0.1 and abs(pu - traj[i][1]) < 0.1, (i, pk, pu, traj[i])
    # round 4: the contextual core, the pixel loss and the LPIPS head no longer reduce with float atomics, so the patch loss of
    # EVERY iteration is a reproducible number of THIS code (test_complete_iteration_is_bit_reproducible).  Against the reference's
    # values the later iterations still cannot be asserted value by value: once the loss is 1e-7-sized it is a sum over arg-max
    # assignments that flip under fp32 round-off differences between two correct implementations (worst single iteration 70 % at
    # iteration 40 of g8s); the median deviation over the whole run is what is asserted.
    worst = max(dev_all)
    med = float(np.median([v[0] for v in dev_all]))
    print(f"patch loss vs reference over {len(dev_all)} iterations: worst {worst[0]:.3%} at iteration {worst[1]} ({worst[2]}), median {med:.3%}")
    assert med < loss_tol_all, (med, worst)
    assert fit.net.global_step == int(g["global_step"])
    np.testing.assert_allclose(fit.net.latents.cpu().numpy(), np.concatenate([g["latent_alpha"], g["latent_scale"]], 1).reshape(-1),
                               atol=3e-3)
    return n_same


def test_remapping_loop_trajectory_vs_reference_g8r(dev, golden):
    """NPP_remapping/train.py:158-300 driven from the reference's modules (g8r_fit_remap.npz: GridPatchSampler on the clear mask,
    img2mse with gt_mask = clear_mask, contextual_loss + VGG16FeatureExtractor.style_loss (adaptive) on comp / pred patches, all
    latents in one Adam): the build's CompletionFit(task='remapping') from the same weights, frequencies and NumPy stream --
    identical sampler decisions, patch loss (style + 0.01 CX) within 3 %, PSNR within 0.1 dB on the clear / blurry regions, and
    where the style latents end up (level 0 in full, a fixed sample of the two larger levels)."""
    import sys
    import os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from refinit import reference_init
    from npp_amd.fit import CompletionFit
    g = golden("g8r_fit_remap.npz")
    H, N_rand = int(g["H"]), int(g["N_rand"])
    img, _ = oracle.synthetic_image(H)
    angles, periods, shifts = oracle.synthetic_periodicity(H, 1)
    clear = np.ones((H, H, 1), np.float32)
    clear[H // 3:H // 2] = 0.0
    fit = CompletionFit(img, np.ones((H, H, 1), np.float32), angles, periods, g["freqs"], reference_init(1), device=dev, N_rand=N_rand,
                        seed=0, ksplit=4, shifts=shifts, rng_mode="reference", task="remapping", clear_mask=clear,
                        contextual_weight=0.01, style_weight=1.0, use_perceptual_loss=False)
    assert fit.patch_size == 64 and fit.i_train.shape[0] == H * H
    _run_task_golden(dev, g, fit)
    for k in range(3):
        lat = fit.style.latents[k].cpu().numpy()
        D = lat.size // 2
        idx = g[f"sidx{k}"]
        np.testing.assert_allclose(lat[:D][idx], g[f"sla{k}"], atol=3e-3)
        np.testing.assert_allclose(lat[D:][idx], g[f"sls{k}"], atol=3e-3)


def test_remapping_loop_at_1024sq_vs_reference_g8r1024(dev, golden):
    """BASELINE config c4's grid: NPP_remapping/train.py:158-300 driven from the reference's modules at 1024^2,
    K = 3, P = 160 (g8r1024_fit_remap.npz, make_golden_fit_tasks.py --remap1024: 1 048 576 'train' rows, 2 patches of 160^2 against
    3 real ones, Gram style loss + 0.01 CX) for 16 iterations -- identical sampler decisions call by call, the weighted patch loss
    (style + 0.01 CX) of EVERY iteration within 3 %, PSNR on the clear / blurry regions within 0.1 dB at iterations 1 / 4 / 8 / 12 /
    16, the pixel-loss latents and a fixed sample of the style latents."""
    import sys
    import os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from refinit import reference_init
    from npp_amd.fit import CompletionFit
    g = golden("g8r1024_fit_remap.npz")
    H, N_rand, K, P = int(g["H"]), int(g["N_rand"]), int(g["K"]), int(g["P"])
    assert (H, K, P) == (1024, 3, 160)
    img, _ = oracle.synthetic_image(H)
    angles, periods, shifts = oracle.synthetic_periodicity(H, K)
    clear = np.ones((H, H, 1), np.float32)
    clear[H // 3:H // 2] = 0.0
    fit = CompletionFit(img, np.ones((H, H, 1), np.float32), angles, periods, g["freqs"], reference_init(K), device=dev, N_rand=N_rand,
                        seed=0, ksplit=4, shifts=shifts, rng_mode="reference", task="remapping", clear_mask=clear, patch_size=P,
                        contextual_weight=0.01, style_weight=1.0, use_perceptual_loss=False)
    assert fit.patch_size == P and fit.i_train.shape[0] == H * H
    _run_task_golden(dev, g, fit, n_iters=len(g["seq"]), n_loss=len(g["seq"]))
    for k in range(3):
        lat = fit.style.latents[k].cpu().numpy()
        D = lat.size // 2
        idx = g[f"sidx{k}"]
        np.testing.assert_allclose(lat[:D][idx], g[f"sla{k}"], atol=3e-3)
        np.testing.assert_allclose(lat[D:][idx], g[f"sls{k}"], atol=3e-3)


def test_segmentation_loop_trajectory_vs_reference_g8s(dev, golden):
    """NPP_segmentation/train.py:148-290 driven from the reference's modules (g8s_fit_segment.npz): the initial periodic region
    is the known mask and the 'train' pool, the input image is what is trained and sampled on, contextual weight 0.005, no
    LPIPS, and the learning rate never decays (`global_step += 1` is outside the reference's loop, :408 -- reproduced)."""
    import sys
    import os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from refinit import reference_init
    from npp_amd.fit import CompletionFit
    g = golden("g8s_fit_segment.npz")
    H, N_rand = int(g["H"]), int(g["N_rand"])
    img, _ = oracle.synthetic_image(H)
    angles, periods, shifts = oracle.synthetic_periodicity(H, 1)
    yy, xx = np.meshgrid(np.arange(H), np.arange(H), indexing="ij")
    period = (1.0 - (((yy - 0.6 * H) ** 2 + (xx - 0.4 * H) ** 2) < (H / 8) ** 2).astype(np.float32))[..., None]
    fit = CompletionFit(img, period, angles, periods, g["freqs"], reference_init(1), device=dev, N_rand=N_rand, seed=0, ksplit=4,
                        shifts=shifts, rng_mode="reference", task="segmentation", masked_img=img, contextual_weight=0.005,
                        use_perceptual_loss=False)
    assert int(g["global_step"]) == 0 and fit.net.lr_clock is False
    # (contextual weight 0.005 on patches the fit reproduces almost exactly by then: from ~iteration 25 on the weighted patch
    #  loss is ~2e-6 and the fp16 trunk's rounding is 5 % of it)
    _run_task_golden(dev, g, fit, n_loss=20)
    assert fit.net.lr == 5e-4


def test_full_loop_with_lpips_stable_ties_vs_reference_g8d(dev, golden):
    """g8c with the reference's tie order DEFINED (torch.topk replaced by its stable realisation while the golden was made): the
    weighted patch loss of 'val' / 'train' iterations is then comparable value by value too -- asserted at 3 % for every source,
    where g8c had to allow 35 % for the backend-defined choice among equidistant lattice candidates."""
    import sys
    import os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from refinit import reference_init
    from npp_amd.fit import CompletionFit
    g = golden("g8d_fit_lpips_stable.npz")
    H, N_rand = int(g["H"]), int(g["N_rand"])
    img, mask = oracle.synthetic_image(H)
    angles, periods, shifts = oracle.synthetic_periodicity(H, 1)
    fit = CompletionFit(img, mask, angles, periods, g["freqs"], reference_init(1), device=dev, N_rand=N_rand, seed=0, ksplit=4,
                        shifts=shifts, rng_mode="reference", use_perceptual_loss=True,
                        lpips_lin_weights=[g[f"lin{k}"] for k in range(5)])
    n_same = _run_task_golden(dev, g, fit)
    assert n_same == len(g["lpips_values"])
    for k, lat in enumerate(fit.percepLoss.latents):
        want = np.concatenate([g[f"la{k}"].reshape(-1), g[f"ls{k}"].reshape(-1)])
        np.testing.assert_allclose(lat.cpu().numpy(), want, atol=2e-3)
