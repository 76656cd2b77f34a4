"""NPP_Net_light's training chains on the 16-bit matrix pipe (csrc/npp_light16.hip + the light job table of npp_mlp_wgrad.hip;
models/networks.py:176-263, NPP_proposal/search.py:85-215) against the exact-fp32 chains (csrc/npp_light.hip, themselves pinned to the
reference's trajectories g10 / g10d): one step tensor by tensor at the bf16 tolerance of the main loop's MLP (3e-2 rel-L2, the level
tests/test_gpu_parity.py asserts for it), the loss trajectory, and what the precision must not change: the ranking."""
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
    npp_amd.lib()
    return torch.device("cuda:0")


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _pair(dev, C, H=96, seed=11):
    from npp_amd.light import NPPNetLightBatch, default_light_init
    rng = np.random.RandomState(seed)
    angles = np.array([[0.0, 90.0], [30.0, 120.0], [10.0, 80.0], [45.0, 135.0], [5.0, 95.0],
                       [20.0, 110.0], [60.0, 150.0], [15.0, 100.0], [35.0, 125.0]], np.float32)[:C]
    periods = np.array([[12.0, 9.0], [7.0, 15.0], [20.0, 6.0], [11.0, 11.0], [16.0, 8.0],
                        [9.0, 13.0], [14.0, 10.0], [8.0, 18.0], [17.0, 7.0]], np.float32)[:C]
    freqs = (rng.randn(10) * 10).astype(np.float32)
    init = default_light_init(256, 4)
    cands = [(angles[i], periods[i]) for i in range(C)]
    n32 = NPPNetLightBatch(cands, freqs, (H, H), init, device=dev, fused=True, precision="fp32")
    n16 = NPPNetLightBatch(cands, freqs, (H, H), init, device=dev, fused=True, precision="bf16")
    assert n16.bf16 and not n32.bf16
    return n32, n16, rng


@pytest.mark.parametrize("C,B", [(3, 256), (5, 64), (1, 2048), (1, 64), (9, 128)])
def test_bf16_chains_vs_fp32_chains_one_step(dev, C, B):
    """Same weights, same rows: predictions, the loss words, every weight / bias gradient of every candidate (the split-K slabs summed),
    and the packs after the Adam launch against a fresh pack of the updated master weights.  (1, 64): one work item, the seven surplus
    workgroups of the grid leave before any barrier; (9, 128): 18 items on a grid of 24, three per XCD with an uneven last XCD -- the
    smallest shapes at which the candidate-contiguous XCD numbering and the ring's hand-over to "no next part" can go wrong."""
    from npp_amd import ops
    H = 96
    n32, n16, rng = _pair(dev, C, H)
    coords = torch.from_numpy(np.stack([rng.randint(0, H, 2 * B), rng.randint(0, H, 2 * B)], 1).astype(np.int32)).to(dev)
    tabs = [n_.embed(coords) for n_ in n32.nets]
    x_pos_all, x_per_all = tabs[0][0], torch.stack([t[1] for t in tabs])
    gt_all = torch.from_numpy(rng.rand(2 * B, 3).astype(np.float32)).to(dev)
    idx = torch.from_numpy(rng.permutation(2 * B)[:B]).to(dev)
    n32.fused_adam = False                                   # keeps the fp32 gradients for the comparison
    l32 = n32.train_step(x_pos_all, x_per_all, gt_all[idx], idx=idx).clone()
    l16 = n16.train_step(x_pos_all, x_per_all, gt_all[idx], idx=idx).clone()
    torch.cuda.synchronize()
    p32, p16 = n32._ws[("fused", B)]["pred"].cpu().numpy(), n16._ws[("bf16", B)]["pred"].cpu().numpy()
    print(f"C={C} B={B}: pred max |d| {np.abs(p32 - p16).max():.2e}; loss {l32.cpu().numpy()} vs {l16.cpu().numpy()}")
    np.testing.assert_allclose(p16, p32, atol=2e-2)
    np.testing.assert_allclose(l16.cpu().numpy(), l32.cpu().numpy(), rtol=2e-2)
    g16 = n16._ws[("bf16", B)]["gslabs"].sum(1)             # (C, n_pad)
    worst = 0.0
    for name in n32.dw:
        for part, blob in (("dw", n32.dw), ("db", n32.db)):
            ref = blob[name]
            off = ref.storage_offset() - n32.grad.storage_offset()
            for ci in range(C):
                a = ref[ci].cpu().numpy()
                b_ = g16[ci, off:off + a.size].cpu().numpy().reshape(a.shape)
                e = rel_l2(b_, a)
                worst = max(worst, e)
                assert e < 3e-2, (name, part, ci, e)
    print(f"  worst gradient rel-L2 {worst:.2e}")
    # the Adam launch's scatter == a fresh pack of the updated master weights, bit for bit
    fresh = torch.zeros_like(n16._pack16)
    ops.light16_pack(n16._desc, n16.params, fresh)
    torch.cuda.synchronize()
    assert torch.equal(fresh, n16._pack16)
    # pad columns of the stored matrices stay exactly zero
    w = n16.w["pos_linears.0"]
    assert float(w[:, :, 298:].abs().max()) == 0.0


def test_bf16_fit_tracks_the_fp32_fit(dev):
    """40 iterations from the same start on the same rows: the loss words of every candidate stay within 3 % of the fp32 chains'
    (Adam's normalised steps turn bf16 round-off of small gradients into different trajectories; the loss level is what the score sees)."""
    C, B, H = 3, 512, 96
    n32, n16, rng = _pair(dev, C, H)
    coords = torch.from_numpy(np.stack([rng.randint(0, H, 4 * B), rng.randint(0, H, 4 * B)], 1).astype(np.int32)).to(dev)
    tabs = [n_.embed(coords) for n_ in n32.nets]
    x_pos_all, x_per_all = tabs[0][0], torch.stack([t[1] for t in tabs])
    img, _ = oracle.synthetic_image(H, noise=0.01)
    gt_all = torch.from_numpy(img[coords.cpu().numpy()[:, 0], coords.cpu().numpy()[:, 1]].astype(np.float32)).to(dev)
    worst = 0.0
    for it in range(40):
        idx = torch.from_numpy(rng.permutation(4 * B)[:B]).to(dev)
        a = n32.train_step(x_pos_all, x_per_all, gt_all[idx], idx=idx).clone()
        b_ = n16.train_step(x_pos_all, x_per_all, gt_all[idx], idx=idx).clone()
        d = float(((a - b_).abs() / a.abs().clamp_min(1e-3)).max())
        worst = max(worst, d)
    torch.cuda.synchronize()
    print(f"worst relative loss gap over 40 iterations: {worst:.3e}; final {a.cpu().numpy()} vs {b_.cpu().numpy()}")
    assert worst < 3e-2
    assert n16.nets[0].opt_step == n32.nets[0].opt_step == 40
    assert bool(torch.isfinite(n16.params).all())


def test_ranking_is_the_same_in_bf16(dev):
    """VERDICT r3 item 7's criterion: the ranking order and the top-k set of the 9-candidate set (the bench's construction: three
    proposals, each also rotated / stretched twice) are those of the fp32 path."""
    from npp_amd.light import ProposalRanker
    H = 128
    img, _ = oracle.synthetic_image(H, noise=0.01)
    angles, periods, shifts = oracle.synthetic_periodicity(H, 3)
    pseudo = np.ones((H, H), np.float32)
    pseudo[40:88, 36:92] = 0
    i_train, i_val = np.stack(np.nonzero(pseudo), 1), np.stack(np.nonzero(1 - pseudo), 1)
    cands = [(angles[i % 3] + 3.0 * (i // 3), periods[i % 3] * (1.0 + 0.11 * (i // 3)), shifts[i % 3]) for i in range(9)]
    out = {}
    for prec in ("fp32", "bf16"):
        rk = ProposalRanker(img, i_train, i_val, device=dev, N_iters=150, N_rand=2048, rng_mode="fast", precision=prec)
        d, order, details = rk.rank(cands, topk=9)
        out[prec] = (np.asarray(d), list(order))
        print(prec, "order", list(order), "scores", np.round(np.asarray(d), 4))
    assert out["bf16"][1][:3] == out["fp32"][1][:3], out                     # the winners, in order
    assert set(out["bf16"][1][:5]) == set(out["fp32"][1][:5])
    np.testing.assert_allclose(out["bf16"][0], out["fp32"][0], rtol=0.1)


def test_g10d_candidates_rank_the_same_in_bf16(dev, golden):
    """The two candidates of the reference trajectory g10d (NPP_proposal/search.py:85-147 run with the reference's modules): the bf16
    fits end at the fp32 fits' loss level (2 %) and order the two candidates the same way."""
    from npp_amd.light import ProposalRanker
    g = golden("g10d_light_fit.npz")
    cands = [(g[f"c{i}.angles"], g[f"c{i}.periods"]) for i in range(2)]
    n_it, n_rand = int(g["n_iters"]), int(g["n_rand"])
    if n_rand % 64:
        pytest.skip("the fixture's batch is not a multiple of 64 rows")
    i_val = np.array([[20, 30], [21, 31], [43, 59]], np.int32)
    res = {}
    for prec in ("fp32", "bf16"):
        rk = ProposalRanker(g["masked_img"], g["i_train"], i_val, device=dev, N_iters=n_it, N_rand=n_rand, lrate=float(g["lrate"]),
                            lrate_decay=int(g["lrate_decay"]), record_losses=True, precision=prec)
        rk.fit_candidates(cands)
        res[prec] = torch.cat(rk.loss_log, 1).cpu().numpy()
    tail32, tail16 = res["fp32"][-10:].mean(0), res["bf16"][-10:].mean(0)
    print("final loss level fp32", tail32, "bf16", tail16)
    np.testing.assert_allclose(tail16, tail32, rtol=2e-2, atol=2e-3)
    assert np.argsort(tail16).tolist() == np.argsort(tail32).tolist()
    np.testing.assert_allclose(res["fp32"][:, 0], g["c0.loss"], rtol=2e-4)       # (the fp32 path is the pinned one)


@pytest.mark.parametrize("lt", ["l2", "robust_loss"])
def test_candidate_fits_with_a_quadratic_pixel_loss(dev, lt):
    """--loss_type l2 / robust_loss (models/mse_calculator.py:19-23) in the candidate fits: the fused fp32 chains, the layer-by-layer path
    and the 16-bit chains take the non-adaptive loss through its own launch (d pred handed to the data-gradient chain); the latents stay."""
    from npp_amd.light import NPPNetLightBatch, default_light_init
    H, B, C = 96, 256, 3
    rng = np.random.RandomState(5)
    angles = np.array([[0.0, 90.0], [30.0, 120.0], [10.0, 80.0]], np.float32)
    periods = np.array([[12.0, 9.0], [7.0, 15.0], [20.0, 6.0]], np.float32)
    freqs = (rng.randn(10) * 10).astype(np.float32)
    init = default_light_init(256, 4)
    cands = [(angles[i], periods[i]) for i in range(C)]
    mk = lambda **kw: NPPNetLightBatch(cands, freqs, (H, H), init, device=dev, loss_type=lt, **kw)      # noqa: E731
    nets = [mk(fused=True, precision="fp32"), mk(fused=False), mk(fused=True, precision="bf16")]
    coords = torch.from_numpy(np.stack([rng.randint(0, H, 2 * B), rng.randint(0, H, 2 * B)], 1).astype(np.int32)).to(dev)
    tabs = [n_.embed(coords) for n_ in nets[0].nets]
    x_pos_all, x_per_all = tabs[0][0], torch.stack([t[1] for t in tabs])
    gt_all = torch.from_numpy(rng.rand(2 * B, 3).astype(np.float32)).to(dev)
    lat0 = nets[0].latents.clone()
    for it in range(8):
        idx = torch.from_numpy(rng.permutation(2 * B)[:B]).to(dev)
        losses = [n_.train_step(x_pos_all[idx].contiguous(), x_per_all[:, idx].contiguous(), gt_all[idx]).clone() for n_ in nets]
        np.testing.assert_allclose(losses[0].cpu().numpy(), losses[1].cpu().numpy(), rtol=2e-5)
        np.testing.assert_allclose(losses[2].cpu().numpy(), losses[0].cpu().numpy(), rtol=2e-2)
        ref = oracle.img2mse_quad_grads(nets[1]._ws[B]["pred"][0].cpu().numpy(), gt_all[idx].cpu().numpy(), lt)[0] if it == 0 else None
        if ref is not None:
            np.testing.assert_allclose(losses[1][0].item(), ref, rtol=2e-5)
    assert rel_l2(nets[0].params.cpu().numpy(), nets[1].params.cpu().numpy()) < 2e-5
    for n_ in nets:
        assert torch.equal(n_.latents, lat0)


def test_bf16_candidate_fits_reproducible_and_across_images(dev):
    """Round 6: the 16-bit candidate fits without order-dependent float sums (npp_light16_bwd_det: the blocks' loss / latent-gradient
    sums by plain stores, added in block order by npp_light16_adam_pack_det; the weight gradients were slab sums already) and with
    candidate k of every image of a rank in one launch sequence (npp_light16_fwd_multi, per-candidate targets): per image the bits of
    its own serial bf16 ranking -- scores, order -- run to run and against light.rank_images; chained and independent candidates;
    images of different sizes and candidate counts."""
    from npp_amd import ops
    from npp_amd.light import ProposalRanker, rank_images
    assert ops.DETERMINISTIC
    rankers, cand_lists = [], []
    for i, (H, Wd, ncand) in enumerate([(128, 128, 3), (96, 144, 2), (128, 128, 3)]):
        img, mask = oracle.synthetic_image(max(H, Wd), noise=0.01, seed=i)
        img = img[:H, :Wd]
        angles, periods, shifts = oracle.synthetic_periodicity(128, 1)
        pseudo = np.ones((H, Wd))
        pseudo[30 + 5 * i:70, 40:80 + 4 * i] = 0
        i_train, i_val = np.stack(np.nonzero(pseudo), 1), np.stack(np.nonzero(1 - pseudo), 1)
        cand_lists.append([(angles[0] + 7.0 * j, periods[0] * (1.0 + 0.23 * j), shifts[0]) for j in range(ncand)])
        rankers.append((img, i_train, i_val))
    for carry in (True, False):
        mk = lambda: [ProposalRanker(im, it, iv, device=dev, N_iters=40, N_rand=1024, carry_latents=carry, precision="bf16")   # noqa: E731
                      for im, it, iv in rankers]
        serial = [rk.rank(c, topk=10) for rk, c in zip(mk(), cand_lists)]
        serial2 = [rk.rank(c, topk=10) for rk, c in zip(mk(), cand_lists)]
        together = rank_images(mk(), cand_lists, topk=10)
        again = rank_images(mk(), cand_lists, topk=10)
        for (d0, o0, det0), (d3, o3, det3), (d1, o1, det1), (d2, o2, det2) in zip(serial, serial2, together, again):
            assert det0 == det3                                              # the serial bf16 loop, run to run
            assert list(o0) == list(o1) == list(o2) and det1 == det2
            assert det0 == det1, (carry, det0, det1)                         # stacked across images = the image's own loop, to the bit
            np.testing.assert_array_equal(d0, d1)
