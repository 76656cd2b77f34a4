"""The exact-fp32 fit (NPPNet / CompletionFit precision="fp32": npp_mlp_fwd32_train, npp_mlp_bwd32, npp_mlp_wgrad32): gradients
against the PLAIN fp32 oracle, the stash changing nothing, bit reproducibility, the optimiser and pack plumbing, and the
reference trajectories of tests/test_gpu_parity.py run in fp32."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import npp_amd
    npp_amd.lib()          # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def _coords(n, H, W, seed=0):
    rng = np.random.RandomState(seed)
    return np.stack([rng.randint(0, H, n), rng.randint(0, W, n)], 1).astype(np.int32)


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _net(dev, K, H=256, seed=0, ksplit=3, width=256, out_act=1):
    from npp_amd.model import NPPNet
    angles, periods, _ = oracle.synthetic_periodicity(H, K)
    P = oracle.init_params(K, W=width, seed=seed)
    net = NPPNet(angles, periods, oracle.SEED0_FREQS, (H, H), params=P, device=dev, ksplit=ksplit, width=width, out_act=out_act,
                 precision="fp32")
    return net, P, angles, periods


def _batch(n, H=256):
    c = _coords(n, H, H, seed=5)
    Bp = (n + 63) // 64 * 64
    cp = np.zeros((Bp, 2), np.int32)
    cp[:n] = c
    gt = np.random.RandomState(2).rand(n, 3).astype(np.float32)
    return c, cp, Bp, gt


@functools.lru_cache(maxsize=None)
def _oracle_step(K, width, n, out_act):
    """The plain fp32 oracle on the batch of _batch(n) with the initial latents: prediction, loss, dL/dpred, latent and parameter
    gradients (computed once per case, read-only)."""
    from npp_amd.model import LATENT_ALPHA_INIT
    H = 256
    angles, periods, _ = oracle.synthetic_periodicity(H, K)
    P = oracle.init_params(K, W=width, seed=0)
    c, _, _, gt = _batch(n)
    emb = oracle.embed(c, angles, periods, oracle.SEED0_FREQS, (H, H))
    raw, cache = oracle.mlp_forward(P, emb, K, emulate_bf16=False)
    pr = oracle.sigmoid(raw) if out_act == 1 else np.tanh(raw).astype(np.float32)
    la, ls = np.full((1, 3), LATENT_ALPHA_INIT, np.float32), np.zeros((1, 3), np.float32)
    loss, dpred, dla, dls = oracle.img2mse_grads(pr, gt, la, ls)
    draw = dpred * pr * (1 - pr) if out_act == 1 else dpred * (1 - pr * pr)
    G = oracle.mlp_backward(P, cache, draw, emulate_bf16=False)
    return pr, float(loss), dla, dls, G


def _check_gradients(dev, K, width, n, out_act=1):
    net, P, angles, periods = _net(dev, K, ksplit=3, width=width, out_act=out_act)
    c, cp, Bp, gt = _batch(n)
    net.zero_grad()
    pred = net.forward_train(torch.from_numpy(cp).to(dev))
    ws = net.workspace(Bp)
    ws["dpred"].zero_()
    net.pixel_loss(Bp, n, torch.from_numpy(gt).to(dev))
    net.backward(Bp)
    torch.cuda.synchronize()
    G = net.grads()
    pred_h = pred.cpu().numpy()[:n]
    pr, loss, dla, dls, Gref = _oracle_step(K, width, n, out_act)
    gap = {name: rel_l2(G[name], Gref[name]) for name in Gref} if set(G) == set(Gref) else {}
    worst = max(gap, key=gap.get) if gap else None
    perr, lerr = float(np.abs(pred_h - pr).max()), abs(net.loss_buf.item() - loss) / abs(loss)
    print(f"fp32 fit K={K} W={width} n={n} act={out_act}: worst gradient {worst} rel-L2 {gap.get(worst, float('nan')):.3e}, "
          f"median {float(np.median(list(gap.values()) or [np.nan])):.3e}, |pred-oracle| {perr:.3e}, loss rel {lerr:.3e}")
    assert set(G) == set(Gref)
    assert gap[worst] < 3e-4, (worst, gap[worst])
    assert perr < 5e-5
    assert lerr < 1e-5
    np.testing.assert_allclose(net.dlatent[:3].cpu().numpy(), dla.ravel(), rtol=1e-3)
    np.testing.assert_allclose(net.dlatent[3:].cpu().numpy(), dls.ravel(), rtol=1e-3)
    assert float(ws["dpred"][n:].abs().max()) == 0.0 if Bp > n else True      # padded rows contribute nothing
    return net


@pytest.mark.parametrize("n", [677, 64])
@pytest.mark.parametrize("K,width", [(3, 256), (1, 256), (5, 256), (3, 512), (1, 512)])
def test_fp32_training_step_gradients_vs_plain_oracle(dev, K, width, n):
    """forward (fp32 stash) -> pixel loss -> fp32 data-gradient chain -> fp32 weight gradients, against the oracle's plain fp32
    backward (pinned to the reference's autograd in test_oracle_golden; 1.0e-6 from float64 autograd on these inputs).  n = 677:
    11 row tiles over 3 slabs (uneven); n = 64: one row tile, two of the three slabs own no row and must hold zeros.  Bound 3e-4:
    the one the other fp32-MFMA training chains are held to (tests/test_gpu_light.py)."""
    net = _check_gradients(dev, K, width, n)
    if n == 64:
        slabs = net._ws_last["gslabs"].view(3, -1)
        assert float(slabs[0].abs().max()) == 0.0 and float(slabs[1].abs().max()) == 0.0 and float(slabs[2].abs().max()) > 0.0


def test_fp32_training_step_gradients_tanh_output(dev):
    """out_act = 2 (--normalize_type 2): d raw = d pred (1 - pred^2)."""
    _check_gradients(dev, 1, 256, 677, out_act=2)


@pytest.mark.parametrize("width", [256, 512])
def test_fp32_stash_changes_nothing(dev, width):
    """forward_train's prediction is the render's, bit for bit, on the same padded rows."""
    net, *_ = _net(dev, 3, width=width)
    _, cp, Bp, _ = _batch(677)
    ct = torch.from_numpy(cp).to(dev)
    pred = net.forward_train(ct).clone()
    assert torch.equal(pred, net.render_fp32(ct))


def _one_step(net, cp, n, gt, dev, step=True):
    Bp = cp.shape[0]
    net.zero_grad()
    net.forward_train(torch.from_numpy(cp).to(dev))
    ws = net.workspace(Bp)
    ws["dpred"].fill_(3.0)                       # whatever an earlier iteration left
    net.pixel_loss(Bp, n, torch.from_numpy(gt).to(dev))
    ws["dpred"][n:].zero_()                      # as the loop does
    net.backward(Bp)
    G = net.grads()
    if step:
        net.optimizer_step(Bp)
    return G


def test_fp32_step_is_bit_reproducible_and_independent_of_earlier_batches(dev):
    c, cp, Bp, gt = _batch(677)
    a, *_ = _net(dev, 3)
    b, *_ = _net(dev, 3)
    Ga, Gb = _one_step(a, cp, 677, gt, dev), _one_step(b, cp, 677, gt, dev)
    for k in Ga:
        assert np.array_equal(Ga[k], Gb[k]), k
    for name in ("params", "m", "v"):              # (the unfolded pixel-loss launch adds its latent gradients by float atomics: not asserted)
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    # a smaller batch after a larger one on the same net == the smaller batch on a fresh net
    c2, cp2, Bp2, gt2 = _batch(100)
    assert Bp2 == 128
    x, *_ = _net(dev, 3)
    y, *_ = _net(dev, 3)
    _one_step(x, cp, 677, gt, dev, step=False)
    Gx, Gy = _one_step(x, cp2, 100, gt2, dev), _one_step(y, cp2, 100, gt2, dev)
    for k in Gx:
        assert np.array_equal(Gx[k], Gy[k]), k
    assert torch.equal(x.params, y.params) and torch.equal(x.workspace(128)["pred"], y.workspace(128)["pred"])


def test_fp32_optimizer_steps_and_packs(dev):
    from npp_amd import ops
    K, H, n = 3, 256, 256
    net, P, angles, periods = _net(dev, K, ksplit=2)
    c_h = _coords(n, H, H)
    c = torch.from_numpy(c_h).to(dev)
    gt_h = np.random.RandomState(3).rand(n, 3).astype(np.float32)
    gt = torch.from_numpy(gt_h).to(dev)
    r_bf16_0, r_fp32_0 = net.render(c).clone(), net.render_fp32(c).clone()
    assert float((r_bf16_0 - r_fp32_0).abs().max()) < 2e-2
    old8 = ops.tune("stash8", 0)                 # no effect on an fp32 net: flipped mid-way, the result must not notice
    emb = oracle.embed(c_h, angles, periods, oracle.SEED0_FREQS, (H, H))
    Po, st = {k: v.copy() for k, v in P.items()}, oracle.adam_init(P)
    lrs = []
    try:
        for it in range(3):
            lat = net.latents.cpu().numpy()
            net.zero_grad()
            net.forward_train(c)
            net.workspace(n)["dpred"].zero_()
            net.pixel_loss(n, n, gt)
            net.backward(n)
            lrs.append(net.lr)
            net.optimizer_step(n)
            if it == 0:
                ops.tune("stash8", 1)
            raw, cache = oracle.mlp_forward(Po, emb, K, emulate_bf16=False)
            pr = oracle.sigmoid(raw)
            _, dpred, _, _ = oracle.img2mse_grads(pr, gt_h, lat[None, :3], lat[None, 3:])
            oracle.adam_step(Po, oracle.mlp_backward(Po, cache, dpred * pr * (1 - pr), emulate_bf16=False), st, lrs[-1])
    finally:
        ops.tune("stash8", old8)
    assert lrs[0] == lrs[1] == 5e-4 and abs(lrs[2] - 5e-4 * 0.1 ** (1 / 50000)) < 1e-12
    got = net.state_dict()
    for k in Po:
        e = rel_l2(got[k], Po[k])
        assert e < 2e-3, (k, e)
    r_bf16, r_fp32 = net.render(c), net.render_fp32(c)
    d_pair, d_step = float((r_bf16 - r_fp32).abs().max()), float((r_bf16 - r_bf16_0).abs().max())
    print(f"after 3 fp32 steps: |render - render_fp32| {d_pair:.3e}, |render - render before| {d_step:.3e}")
    assert d_pair < 2e-2 < d_step
    pr = oracle.sigmoid(oracle.mlp_forward(Po, emb, K, emulate_bf16=False)[0])
    assert float(np.abs(r_fp32.cpu().numpy() - pr).max()) < 2e-3          # render_fp32 follows the stepped weights


# ---- reference trajectories (the goldens and constructions of tests/test_gpu_parity.py, precision="fp32") --------------------
def _pixel_fit(dev, g, K):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from refinit import reference_init
    from npp_amd.fit import CompletionFit
    H, N_rand = int(g["H"]), int(g["N_rand"])
    img, mask = oracle.synthetic_image(H)
    angles, periods, _ = oracle.synthetic_periodicity(H, K)
    return CompletionFit(img, mask, angles, periods, g["freqs"], reference_init(K), device=dev, N_rand=N_rand, seed=0, ksplit=4,
                         rng_mode="reference", precision="fp32")


def test_fp32_fit_trajectory_vs_reference_g8(dev, golden):
    """test_fit_trajectory_vs_reference_g8 in fp32, the checkpoints up to iteration 150, the same 0.05 dB."""
    g = golden("g8_fit.npz")
    fit = _pixel_fit(dev, g, 1)
    traj = {int(r[0]): r[1:] for r in g["traj"] if int(r[0]) <= 150}
    assert max(traj) == 150
    for i in range(1, 151):
        fit.step()
        if i in traj:
            pk, pu = fit.psnr("known"), fit.psnr("unknown")
            assert abs(pk - traj[i][0]) < 0.05 and abs(pu - traj[i][1]) < 0.05, (i, pk, pu, traj[i][:2])


def test_fp32_fit_trajectory_vs_reference_g8k3(dev, golden):
    """test_fit_trajectory_vs_reference_g8k3 in fp32: 150 iterations, 0.05 dB per checkpoint, latents 3e-3."""
    g = golden("g8k3_fit.npz")
    assert int(g["K"]) == 3
    fit = _pixel_fit(dev, g, 3)
    traj = {int(r[0]): r[1:] for r in g["traj"]}
    for i in range(1, max(traj) + 1):
        fit.step()
        if i in traj:
            pk, pu = fit.psnr("known"), fit.psnr("unknown")
            assert abs(pk - traj[i][0]) < 0.05 and abs(pu - traj[i][1]) < 0.05, (i, pk, pu, traj[i][:2])
    np.testing.assert_allclose(fit.net.latents.cpu().numpy(), np.concatenate([g["latent_alpha"], g["latent_scale"]], 1).reshape(-1),
                               atol=3e-3)


def test_fp32_full_loop_trajectory_vs_reference_g8b(dev, golden):
    """test_full_loop_trajectory_vs_reference_g8b in fp32 (the unfolded launch sequence; the trunk stays fp16): identical sampler
    decisions call by call, PSNR within 0.1 dB, the LR clock."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from refinit import reference_init
    from npp_amd.fit import CompletionFit
    g = golden("g8b_fit_patch.npz")
    H, N_rand = int(g["H"]), int(g["N_rand"])
    img, mask = oracle.synthetic_image(H)
    angles, periods, shifts = oracle.synthetic_periodicity(H, 1)
    fit = CompletionFit(img, mask, angles, periods, g["freqs"], reference_init(1), device=dev, N_rand=N_rand, seed=0, ksplit=4,
                        shifts=shifts, rng_mode="reference", use_perceptual_loss=False, precision="fp32")
    assert fit.patch_size == 64 and fit.patch_num == 2 and not fit.fold_launches
    traj = {int(r[0]): r[1:] for r in g["traj"]}
    code = {"val": 0, "train": 1, "same": 2}
    for i in range(1, 101):
        ok = fit.step_full()
        d = fit.last_draw
        assert (code[d["source"]], d["k"]) == tuple(int(v) for v in g["seq"][i - 1]), i
        assert ok == (d["k"] > 0)
        if i in traj:
            pk, pu = fit.psnr("known"), fit.psnr("unknown")
            assert abs(pk - traj[i][0]) < 0.1 and abs(pu - traj[i][1]) < 0.1, (i, pk, pu, traj[i])
    assert fit.net.global_step == int(g["global_step"])


def test_fp32_remapping_loop_trajectory_vs_reference_g8r(dev, golden):
    """The first 50 iterations of test_remapping_loop_trajectory_vs_reference_g8r in fp32 with that test's per-iteration assertions:
    sampler decisions, the weighted patch loss of the first 20 iterations within 3 %, PSNR checkpoints within 0.1 dB; the style
    latents still train."""
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
                        contextual_weight=0.01, style_weight=1.0, use_perceptual_loss=False, precision="fp32")
    assert fit.patch_size == 64 and fit.i_train.shape[0] == H * H
    style0 = [t.clone() for t in fit.style.latents]
    traj = {int(r[0]): r[1:] for r in g["traj"]}
    ploss = {int(r[0]): r[1] for r in g["patch_loss"]}
    code = {"val": 0, "train": 1, "same": 2}
    n_ok = 0
    for i in range(1, 51):
        ok = fit.step_full()
        d = fit.last_draw
        assert (code[d["source"]], d["k"]) == tuple(int(v) for v in g["seq"][i - 1]), i
        assert ok == (d["k"] > 0) == (i in ploss)
        n_ok += bool(ok)
        if ok and i <= 20:
            got = float(fit.last_patch_loss[0])
            assert abs(got - ploss[i]) < 0.03 * abs(ploss[i]), (i, d["source"], got, ploss[i])
        if i in traj:
            pk, pu = fit.psnr("known"), fit.psnr("unknown")
            assert abs(pk - traj[i][0]) < 0.1 and abs(pu - traj[i][1]) < 0.1, (i, pk, pu, traj[i])
    assert fit.net.global_step == n_ok and fit.style.lat_step > 0
    assert all(not torch.equal(a, b) for a, b in zip(style0, fit.style.latents))
