"""rng_mode="device" on the GPU: the two launches (npp_dev_sampler_decide / npp_dev_sampler_pixels) against the NumPy restatement
bit for bit, and the fits that draw with them: reproducible from (seed, draw index), stacked = stand-alone, resumable, and of the
reference mode's quality."""
import numpy as np
import pytest

import oracle
import dev_sampler_restatement as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEED = 20261018


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import npp_amd
    npp_amd.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cases():
    return [R.case_image(), R.case_image(64, 64, ((10, 30, 12, 40),), 6), R.case_image(40, 136, ((8, 30, 50, 90),), 7)]


def _consts(c, ratio, seed, dev, n_train=None):
    from npp_amd.dev_sampler import ImageConsts
    return ImageConsts(c["sat"], c["pool_val"], c["pool_train"], len(c["known"]) if n_train is None else n_train, c["shifts_dydx"],
                       ratio, seed, c["H"], c["W"], c["P"], dev)


def _blob(consts, dev):
    from npp_amd.dev_sampler import _images_blob
    return torch.from_numpy(np.frombuffer(bytes(_images_blob([k.image for k in consts])), np.uint8).copy()).to(dev)


def _same(rec, topk, want):
    from npp_amd.dev_sampler import parse_record
    got = parse_record(rec, topk)
    assert (got["source"], got["k"], got["t"]) == (want["source"], want["k"], want["t"])
    np.testing.assert_array_equal(got["cen"], want["cen"])
    if want["real"] is None:
        assert got["real_cen"] is None
    else:
        np.testing.assert_array_equal(got["real_cen"].astype(np.int32), want["real"])
    if want["weights"] is None:
        assert got["weights"] is None
    else:
        assert np.array_equal(got["weights"], want["weights"])
    # what the launch leaves in the record is exactly what npp_patch_gather takes: fake centres, then the n_p k real ones
    n = want["cen"].shape[0] * (1 + (0 if want["real"] is None else want["k"]))
    np.testing.assert_array_equal(rec[4:4 + 2 * n].reshape(n, 2), R.centres_i32(want))


@pytest.mark.parametrize("n_p", [2, 4])
@pytest.mark.parametrize("ratio", [0.3, 0.035, 0.0])
def test_decision_launch_equals_the_restatement(dev, cases, n_p, ratio):
    """One image (72 x 104), 64 draws, every field; then M = 3 images of different sizes, seeds and draw indices in one launch."""
    from npp_amd import ops
    topk = 3
    words = ops.dev_sampler_record_words(n_p, topk)
    k1 = [_consts(cases[0], ratio, SEED, dev)]
    imgs = _blob(k1, dev)
    rec = torch.zeros((64, 1, words), dtype=torch.int32, device=dev)
    for t in range(64):
        ops.dev_sampler_decide(imgs, 1, [t], n_p, topk, rec[t])
    got = rec.cpu().numpy()
    want = R.case_draws(cases[0], n_p, topk, ratio, SEED, range(64))
    for t in range(64):
        _same(got[t, 0], topk, want[t])
    assert {w["source"] for w in want} == {"val", "train", "same"}
    seeds, t0 = [SEED, 3, 2 ** 40 + 5], [5, 0, 77]
    k3 = [_consts(c, ratio, s, dev) for c, s in zip(cases, seeds)]
    imgs3 = _blob(k3, dev)
    rec3 = torch.zeros((16, 3, words + 3), dtype=torch.int32, device=dev)          # (a record stride beyond the minimum)
    for j in range(16):
        ops.dev_sampler_decide(imgs3, 3, [t + j for t in t0], n_p, topk, rec3[j])
    got3 = rec3.cpu().numpy()
    for j in range(16):
        for i, c in enumerate(cases):
            _same(got3[j, i], topk, R.case_draws(c, n_p, topk, ratio, seeds[i], [t0[i] + j])[0])
        assert not got3[j, :, words:].any()


@pytest.mark.parametrize("N,n", R.PIXEL_CASES)
def test_pixel_row_launch_equals_the_restatement(dev, cases, N, n):
    from npp_amd import ops
    imgs = _blob([_consts(cases[0], 0.3, SEED, dev, n_train=N)], dev)
    for t in (0, 1, 4000000000):
        pix = torch.full((1, n + 5), -1, dtype=torch.int64, device=dev)
        ops.dev_sampler_pixels(imgs, 1, [t], n, pix, N)
        got = pix.cpu().numpy()
        np.testing.assert_array_equal(got[0, :n], R.pixels(N, n, SEED, t))
        assert (got[0, n:] == -1).all()                                                 # nothing beyond n_pix is written
    with pytest.raises(ValueError):
        ops.dev_sampler_pixels(imgs, 1, [0], N + 1, torch.zeros((1, N + 1), dtype=torch.int64, device=dev), N)


def test_pixel_row_launch_for_three_images(dev, cases):
    from npp_amd import ops
    Ns, seeds, ts, n = [64, 4097, 245000], [SEED, 3, 2 ** 40 + 5], [9, 0, 123456], 64
    imgs = _blob([_consts(c, 0.3, s, dev, n_train=N) for c, s, N in zip(cases, seeds, Ns)], dev)
    pix = torch.zeros((3, n), dtype=torch.int64, device=dev)
    ops.dev_sampler_pixels(imgs, 3, ts, n, pix, min(Ns))
    got = pix.cpu().numpy()
    for i in range(3):
        np.testing.assert_array_equal(got[i], R.pixels(Ns[i], n, seeds[i], ts[i]))


# ---- fits ------------------------------------------------------------------------------------------------------------------
def _fit(dev, H=256, K=1, i=0, seed=0, N_rand=4096, ksplit=None, **kw):
    from npp_amd.fit import CompletionFit
    img, mask = oracle.synthetic_image(H, seed=i)
    angles, periods, shifts = oracle.synthetic_periodicity(H, K)
    a = np.asarray(angles, np.float64) + 0.3 * i
    return CompletionFit(img, mask, a, periods, oracle.SEED0_FREQS, oracle.init_params(K, seed=i), device=dev, N_rand=N_rand,
                         shifts=shifts, seed=seed, ksplit=ksplit, **kw)


def _want_draw(f, d, t):
    """The restatement's draw t of fit f at the patch size draw d was taken with (the fit may already have decayed past it for the
    draw it materialises ahead): the summed-area table is the sampler's own, the pools are filtered here."""
    ps, P, n_p = f.patch_sampler, d["P"], d["n"]
    return R.draw(ps.sat, R.filtered(f.i_val, f.H, f.W, P), R.filtered(f.i_train, f.H, f.W, P), [tuple(s) for s in ps.selected_shifts],
                  f.H, f.W, P, n_p, f.topk, f.invalid_ratio, f.seed, t)


def _check_last_draw(f, t):
    d = f.last_draw
    w = _want_draw(f, d, t)
    assert (d["source"], d["k"], d["t"]) == (w["source"], w["k"], t)
    np.testing.assert_array_equal(d["cen"], w["cen"])
    if w["real"] is not None:
        np.testing.assert_array_equal(np.rint(d["real_cen"]).astype(np.int32), w["real"])
        assert np.array_equal(d["weights"], w["weights"])
    if w["k"] > 0:
        np.testing.assert_array_equal(d["pix"].cpu().numpy(), R.pixels(f.i_train.shape[0], f.N_rand, f.seed, t))


def test_two_device_mode_fits_are_bit_identical_and_draw_the_restatement(dev):
    runs = []
    for _ in range(2):
        f = _fit(dev, rng_mode="device", seed=0)
        for t in range(10):
            f.step_full()
            _check_last_draw(f, t)
        torch.cuda.synchronize()
        assert f.iteration == 10 and f.net.opt_step == 10 - f.skipped
        runs.append(f.net.params.clone())
    assert torch.equal(runs[0], runs[1])


def test_stack_of_device_mode_fits_equals_the_stand_alone_fits(dev):
    """Three device-mode fits in one StackedFit -- ONE decision launch and ONE pixel-row launch per iteration for all of them --
    against each fit alone, across a patch-size decay at iteration 6.  Criterion: the one tests/test_gpu_stack.py applies to a
    reference-mode stack that re-forms across a decay (rel-L2 2e-3, 0.1 dB: the re-formed stack picks the split-K of its new batch
    shape, so weight gradients sum in another order from there on), plus its per-iteration checks: every image drew its own
    sequence (sources and draws equal the restatement's) and took the same number of steps."""
    from npp_amd.stack import StackedFit
    M, iters = 3, 10                                               # (decays are due at iterations 6 and 12: one inside)
    kw = dict(rng_mode="device", patch_size_decay=6)
    mk = lambda ks: [_fit(dev, i=i, seed=10 + i, ksplit=ks, **kw) for i in range(M)]
    probe = StackedFit(mk(None))
    ks = probe.ksplit
    assert probe._pool is None                                     # no host draws: no thread pool
    del probe
    alone, sources = mk(ks), []
    for f in alone:
        src = []
        for t in range(iters):
            f.step_full()
            _check_last_draw(f, t)
            src.append(f.last_draw["source"] if f.last_draw["k"] > 0 else None)
        sources.append(src)
    st = StackedFit(mk(ks), ksplit=ks)
    P0, n_restack, got = st.P, 0, [[] for _ in range(M)]
    for t in range(iters):
        if st.shape_change_due():
            st = st.restacked()
            n_restack += 1
        st.step_full()
        for i in range(M):
            got[i].append(st.last_sources[i])
    torch.cuda.synchronize()
    assert got == sources
    assert n_restack == 1 and st.P == P0 // 2 and st.n_p == 4
    for i in range(M):
        a, b = alone[i].net, st.fits[i].net
        assert (a.opt_step, a.global_step, alone[i].patch_size, alone[i].patch_num) == (
            b.opt_step, b.global_step, st.fits[i].patch_size, st.fits[i].patch_num)
        pa, pb = a.params.cpu().numpy().astype(np.float64), b.params.cpu().numpy().astype(np.float64)
        e = float(np.linalg.norm(pa - pb) / np.linalg.norm(pa))
        print(f"image {i}: params rel-L2 {e:.2e}")
        assert e < 2e-3
        np.testing.assert_allclose(b.latents.cpu().numpy(), a.latents.cpu().numpy(), atol=2e-4)
        assert alone[i].percepLoss.lat_step == st.fits[i].percepLoss.lat_step
        assert abs(alone[i].psnr("known") - st.fits[i].psnr("known")) < 0.1


def test_device_mode_fits_like_reference_mode(dev):
    """The bound of test_fast_rng_mode_fits_like_reference_mode: 100 iterations at 256^2, K = 1 -- above 28.5 dB and within 0.5 dB
    of the reference mode fitted here."""
    res = {}
    for mode in ("reference", "device"):
        fit = _fit(dev, N_rand=8192, rng_mode=mode, seed=0)
        for _ in range(100):
            fit.step_full()
        res[mode] = fit.psnr()
    print(f"PSNR known after 100 iterations: reference {res['reference']:.2f} dB, device {res['device']:.2f} dB")
    assert res["device"] > 28.5 and abs(res["device"] - res["reference"]) < 0.5


def test_state_dict_continues_the_same_sequence(dev):
    """state_dict() after 5 iterations, loaded into a fresh fit: draws 5..9 and the parameters after them are those of the fit that
    ran through (the draw materialised ahead at the time of the snapshot is not state: it is drawn again from t)."""
    a = _fit(dev, rng_mode="device", seed=4)
    for _ in range(5):
        a.step_full()
    sd = a.state_dict()
    assert sd["t"] == 5 and sd["rng_mode"] == "device"
    b = _fit(dev, rng_mode="device", seed=4)
    b.load_state_dict(sd)
    for t in range(5, 10):
        a.step_full()
        b.step_full()
        assert b.last_draw["t"] == a.last_draw["t"] == t
        _check_last_draw(b, t)
    torch.cuda.synchronize()
    assert torch.equal(a.net.params, b.net.params) and a.net.opt_step == b.net.opt_step
    with pytest.raises(ValueError, match="device"):
        b.load_state_dict(_fit(dev, rng_mode="fast", seed=4).state_dict())
