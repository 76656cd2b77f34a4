"""The periodicity search's GPU front end (`--front_end gpu`, npp_amd.frontend; csrc/npp_frontend.hip) against its host
definitions: cvlite.py, scipy.ndimage and search.find_mask_centroid / pseudo_mask_split.  Every comparison is bit-exact; there are
no tolerances in this feature.  The far-point walk is compared with the stable-sort restatement (the tie rule the GPU path states)
and, on inputs whose result no tie rule can change, with today's host function as well."""
import functools
import json
import os
import sys
import warnings

import numpy as np
import pytest
import scipy.ndimage as ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import oracle  # noqa: E402
from npp_amd import cvlite, search  # noqa: E402

import frontend_restatement as fr  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    return torch.device("cuda:0")


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


@functools.lru_cache(None)
def _images():
    """name -> uint8 image: the blur / Canny cases."""
    rng = np.random.RandomState(5)
    step = np.zeros((64, 64), np.uint8)
    step[:, 32:] = 200
    mixed = np.zeros((64, 64), np.uint8)
    mixed[:, 32:] = 20                                                     # |dx| = 80: weak only ...
    mixed[:20, 32:] = 200                                                  # ... pulled in by the strong part it is connected to
    weak = np.zeros((64, 64), np.uint8)
    weak[:, 32:] = 20
    return {"const9": np.full((9, 9), 50, np.uint8),
            "rand17x23": rng.randint(0, 256, (17, 23)).astype(np.uint8),
            "step64": step, "step64T": step.T.copy(), "mixed64": mixed, "weak64": weak,
            "ramp64": np.fromfunction(lambda y, x: 3 * x + y // 2, (64, 64)).astype(np.uint8),
            "diag64": np.fromfunction(lambda y, x: (x + y >= 64) * 180, (64, 64)).astype(np.uint8),
            "rand64": rng.randint(0, 256, (64, 64)).astype(np.uint8),
            "smooth64": (ndimage.gaussian_filter(rng.rand(64, 64), 2.0) * 2000).clip(0, 255).astype(np.uint8),
            "rand130x67": rng.randint(0, 256, (130, 67)).astype(np.uint8),
            "smooth130x67": (ndimage.gaussian_filter(rng.rand(130, 67), 1.5) * 1500).clip(0, 255).astype(np.uint8)}


@functools.lru_cache(None)
def _walks():
    """name -> (mask, centroids, distances, unique) of the stable restatement: the fixture masks, the 96 x 96 block of the
    pseudo-mask test, and a strip on which fewer than three points qualify."""
    out = {name: m for name, m in fr.golden_masks()}
    block = np.ones((96, 96), np.uint8)
    block[30:60, 34:70] = 0
    out["block96"] = block
    strip = np.ones((12, 40), np.uint8)
    strip[:, :3] = 0
    out["strip12x40"] = strip
    return {k: (m,) + (fr.find_mask_centroid_stable(m, threshold_ratio=3.0) if k == "strip12x40" else fr.find_mask_centroid_stable(m))
            for k, m in out.items()}


# ---- resizes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dsts", [((211, 325), [(104, 162), (52, 81)]), ((7, 5), [(3, 2)]), ((5, 9), [(11, 20)]), ((1, 40), [(1, 13), (3, 80)]),
                                      ((64, 64), [(64, 64), (32, 32)])])
def test_resizes_equal_cvlite(src, dsts):
    from npp_amd import frontend
    rng = np.random.RandomState(src[0] * 1000 + src[1])
    a = rng.randint(0, 256, src).astype(np.uint8)
    lin_h, lin_d = a, _up(a)
    for (h, w) in dsts:
        assert np.array_equal(frontend.resize_nearest(_up(a), (w, h)).cpu().numpy(), cvlite.resize_nearest(a, (w, h))), (src, h, w, "nearest")
        lin_h, lin_d = cvlite.resize_linear_u8(lin_h, (w, h)), frontend.resize_linear_u8(lin_d, (w, h))      # chained, as im2act does
        assert lin_d.is_cuda and lin_d.cpu().numpy().dtype == np.uint8 and tuple(lin_d.shape) == (h, w)
        assert np.array_equal(lin_d.cpu().numpy(), lin_h), (src, h, w, "linear")


# ---- normalise ------------------------------------------------------------------------------------------------------------------
def test_normalize_equals_cvlite():
    from npp_amd import frontend
    rng = np.random.RandomState(3)
    act = (rng.randn(66, 13, 17) * np.exp(rng.randn(66, 1, 1) * 3)).astype(np.float32)
    act[0] = 5.0                                                           # a constant channel: zeros, not 0 / 0
    act[1] = -np.abs(act[1]) - 1.0                                         # only negative values
    act[2] = np.linspace(-1, 3, 13 * 17, dtype=np.float32).reshape(13, 17)
    got = frontend.normalize_to_uint8(_up(act)).cpu().numpy()
    want = cvlite.normalize_to_uint8(act, channel_idx=(1, 2))
    assert got.dtype == np.uint8 and (got[0] == 0).all() and got[2].min() == 0 and got[2].max() == 255
    assert np.array_equal(got, want)


# ---- blur and Canny -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["const9", "rand17x23", "step64", "step64T", "mixed64", "weak64", "ramp64", "diag64", "rand64", "smooth64",
                                  "rand130x67", "smooth130x67"])
def test_blur_and_canny_equal_cvlite(name):
    from npp_amd import frontend
    img = _images()[name]
    d = _up(img)
    blur = cvlite.gaussian_blur3_u8(img)
    assert np.array_equal(frontend.gaussian_blur3_u8(d).cpu().numpy(), blur), name
    for low, high in ((10, 100), (10.9, 100.9), (40, 41)):
        assert np.array_equal(frontend.canny_u8(d, low, high).cpu().numpy(), cvlite.canny_u8(img, low, high)), (name, low, high)
    assert np.array_equal(frontend.canny_u8(_up(blur), 10, 100).cpu().numpy(), cvlite.canny_u8(blur, 10, 100)), name
    mask = np.zeros(img.shape, np.float32)
    mask[1:, : img.shape[1] - 2] = 1                                       # touches the top-left borders
    assert np.array_equal(frontend.canny_masked(d, _up(mask)).cpu().numpy(), cvlite.canny_masked(img, mask)), name


@pytest.mark.parametrize("shape", [(64, 64), (130, 67)])
def test_blur_and_canny_batched_equal_the_single_calls(shape):
    """All cases of one shape as ONE (C, h, w) call (a batch has one shape; the other shapes run as single-channel batches above)."""
    from npp_amd import frontend
    imgs = [v for v in _images().values() if v.shape == shape]
    assert len(imgs) >= 2
    d = _up(np.stack(imgs))
    assert np.array_equal(frontend.gaussian_blur3_u8(d).cpu().numpy(), np.stack([cvlite.gaussian_blur3_u8(i) for i in imgs]))
    assert np.array_equal(frontend.canny_u8(d, 10, 100).cpu().numpy(), np.stack([cvlite.canny_u8(i, 10, 100) for i in imgs]))


def test_hysteresis_travels_through_every_tile_and_is_8_connected():
    """A 64 x 64 one-pixel-wide weak spiral whose only strong pixel is its inner end: the mark has to cross every 32 x 32 tile many
    times.  And weak components that touch a strong one only diagonally (kept) or not at all (dropped), on both sides of a tile
    border."""
    from npp_amd import ops
    spiral, length = fr.spiral_marks(64)
    diag = np.zeros((64, 64), np.uint8)
    diag[10, 10] = 2
    diag[11, 11] = diag[12, 12] = diag[12, 13] = 1                          # diagonal contact only: 8-connected, not 4-connected
    diag[31, 31] = 2
    diag[32, 32] = diag[33, 33] = 1                                        # ... across the corner of four tiles
    diag[40, 10] = 2
    diag[40, 12] = diag[40, 13] = 1                                        # one pixel apart: not connected
    diag[50:55, 31] = 1
    diag[55, 32] = 2                                                       # across a vertical tile border, diagonally
    none = spiral.copy()
    none[none == 2] = 1                                                    # no strong pixel at all
    maps = np.stack([spiral, diag, none, spiral[::-1, ::-1].copy(), spiral.T.copy()])
    want = np.stack([fr.hysteresis(m) for m in maps])
    assert want[0].sum() == length and want[2].sum() == 0 and want[1][12, 13] and want[1][33, 33] and not want[1][40, 12] and want[1][50, 31]
    for batch in (maps[:1], maps[1:2], maps):
        marks = _up(batch)
        rounds = 0
        while int(ops.canny_hysteresis(marks, 8)[-1].item()):
            rounds += 8
            assert rounds <= 8 * 400
        # the spiral crosses a tile border some sixty times and a round runs each of the four tiles once: one batch of 8 cannot do
        assert rounds >= 8 or not np.array_equal(batch[0], spiral)
        assert np.array_equal(ops.canny_finish(marks).cpu().numpy(), np.stack([fr.hysteresis(m) for m in batch]).astype(np.uint8) * 255)


def test_edge_count_equals_the_act2edge_loop():
    from npp_amd import frontend, proposal
    rng = np.random.RandomState(11)
    act = np.stack([ndimage.gaussian_filter(rng.randn(40, 56), s) for s in np.linspace(0.5, 3.0, 66)]).astype(np.float32)
    mask = np.ones((1, 40, 56), np.float32)
    mask[0, :9, 20:41] = 0                                                 # a hole that touches the border
    mask[0, 25:30, 50:] = 0
    act *= mask
    a, m = _up(act), _up(mask)
    want = proposal.act2edge(a, m)
    got = proposal.act2edge(a, m, front_end="gpu")
    assert got.is_cuda and got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape) == (2, 40, 56)
    assert float(want[0].max()) >= 3.0
    assert np.array_equal(got.cpu().numpy(), want.numpy())
    assert np.array_equal(frontend.edge_count(a[:1], m[0]).cpu().numpy(), proposal.act2edge(a[:1], m)[0].numpy())


# ---- distance transform ---------------------------------------------------------------------------------------------------------
def _edt_cases():
    rng = np.random.RandomState(2)
    a = np.ones((37, 53), np.uint8)
    a[:6, 40:] = 0
    a[20:24, 0:3] = 0
    corner = np.ones((29, 31), np.uint8)
    corner[28, 30] = 0
    row = np.ones((1, 40), np.uint8)
    row[0, 7] = row[0, 30] = 0
    col = np.ones((300, 7), np.uint8)
    col[150, 3] = col[299, 0] = 0
    wide = (rng.rand(5, 1500) > 0.002).astype(np.uint8)                    # more than one LDS chunk of columns
    wide[0, 0] = 0
    return {"border37x53": a, "corner29x31": corner, "row1x40": row, "col300x7": col, "wide5x1500": wide,
            "noise64": (rng.rand(64, 64) > 0.05).astype(np.uint8)}


def test_distance_sq_equals_scipy_edt():
    from npp_amd import frontend
    cases = dict(_edt_cases())
    cases.update({name: m for name, m in fr.golden_masks()})
    for name, m in cases.items():
        want = np.rint(ndimage.distance_transform_edt(m) ** 2).astype(np.int64)
        got = frontend.distance_sq(_up(m)).cpu().numpy()
        assert got.dtype == np.int32 and np.array_equal(got, want), name
    assert np.array_equal(frontend.distance_sq(_up(cases["border37x53"].astype(np.float64) * 0.5)).cpu().numpy(),
                          np.rint(ndimage.distance_transform_edt(cases["border37x53"]) ** 2))     # any dtype: non-zero = known
    with pytest.raises(ValueError, match="no unknown pixel"):
        frontend.distance_sq(_up(np.ones((9, 11), np.uint8)))


# ---- far-point selection --------------------------------------------------------------------------------------------------------
def test_find_mask_centroid_equals_the_stable_walk():
    from npp_amd import frontend
    agree_with_host = []
    for name, (m, cents, dist, unique) in _walks().items():
        kw = dict(threshold_ratio=3.0) if name == "strip12x40" else {}
        got_c, got_d = frontend.find_mask_centroid(_up(m), **kw)
        assert got_c == cents and got_d == dist, (name, got_c, cents)
        if unique:
            host_c, host_d = search.find_mask_centroid(m.astype(np.float64), **kw)
            assert got_c == host_c and got_d == host_d, (name, "host function")
            agree_with_host.append(name)
    assert len(_walks()["strip12x40"][1]) < 3                              # fewer than topk qualify: fewer are returned
    golden_unique = [n for n in agree_with_host if "/" in n]
    assert len(golden_unique) >= 2, golden_unique
    m = _walks()["block96"][0]
    c5, d5 = frontend.find_mask_centroid(m.astype(np.float32), topk=5, threshold_ratio=0.2, device="cuda:0")    # NumPy in, other parameters
    r5 = fr.find_mask_centroid_stable(m, topk=5, threshold_ratio=0.2)
    assert (c5, d5) == (r5[0], r5[1]) and len(c5) == 5
    c0, d0 = frontend.find_mask_centroid(_up(m), topk=4, threshold_ratio=0.0)                                  # threshold 0: the four largest keys
    r0 = fr.find_mask_centroid_stable(m, topk=4, threshold_ratio=0.0)
    assert (c0, d0) == (r0[0], r0[1])


def test_pseudo_mask_split_equals_the_host_function_fed_the_stable_centroids(monkeypatch):
    from npp_amd import frontend
    for name in ("block96", sorted(k for k in _walks() if "/" in k)[3]):
        m, cents, dist, _ = _walks()[name]
        rng = np.random.RandomState(len(name))
        valid = (rng.rand(*m.shape) > 0.01).astype(np.float64)
        known = m.astype(np.float64) * valid
        stable = fr.find_mask_centroid_stable(known)
        monkeypatch.setattr(search, "find_mask_centroid", lambda mask, s=stable: (s[0], s[1]))
        want_p, want_t, want_v = search.pseudo_mask_split(m.astype(np.float64), valid)
        monkeypatch.undo()
        got_p, got_t, got_v = frontend.pseudo_mask_split(_up(m.astype(np.float64)), _up(valid))
        assert got_p.is_cuda and got_t.is_cuda and tuple(got_p.shape) == want_p.shape
        assert np.array_equal(got_p.cpu().numpy(), want_p), name
        assert np.array_equal(got_t.cpu().numpy(), want_t) and np.array_equal(got_v.cpu().numpy(), want_v), name
        assert len(want_v) > 0 and len(want_t) + len(want_v) == int(known.sum())
        got2 = frontend.pseudo_mask_split(m.astype(np.float64)[..., None], valid[..., None], device="cuda:0")    # NumPy (H,W,1) in
        assert np.array_equal(got2[1].cpu().numpy(), want_t) and np.array_equal(got2[2].cpu().numpy(), want_v)


# ---- the chain and the driver ---------------------------------------------------------------------------------------------------
def test_feature_chain_is_identical_on_both_front_ends():
    """im2act and search_periodicity_by_feat (gray, gray + edges, AlexNet conv1 + edges) on a non-square image whose sides are no
    multiples of 4: the same activation, mask and candidates bit for bit.  The convolution itself (npp_linear_fwd, not part of the
    front end) does not repeat its own sums bit for bit from call to call, so both front ends are handed ONE evaluation of it; that
    the extractor takes the image from the device as well is checked to the tolerance of the existing chain test."""
    import torch
    from npp_amd import proposal
    img, mask = oracle.synthetic_image(256, noise=0.01)
    im8 = np.uint8(np.clip(img * mask, 0, 1) * 255)[:211, :254]
    m8 = np.uint8(mask[..., 0])[:211, :254]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        alex = proposal.AlexConv1(None, device=_dev(), allow_random=True)
    assert tuple(alex(_up(im8)).shape) == (64, 56, 64) and float((alex(_up(im8)) - alex(im8)).abs().max()) < 1e-3

    class Frozen:
        device, out = alex.device, alex(im8)

        def __call__(self, im):
            assert tuple(im.shape) == im8.shape
            return self.out
    conv1 = Frozen()
    for kw in (dict(gray_only=True), dict(conv1=conv1)):
        a_h, m_h = proposal.im2act(im8, m8, device=_dev(), **kw)
        a_g, m_g = proposal.im2act(im8, m8, device=_dev(), front_end="gpu", **kw)
        assert torch.equal(a_h, a_g) and torch.equal(m_h, m_g)
        a_t, _ = proposal.im2act(_up(im8), _up(m8), device=_dev(), front_end="gpu", **kw)                   # device tensors in
        assert torch.equal(a_h, a_t)
        e_h, e_g = proposal.act2edge(a_h[:-1], m_h), proposal.act2edge(a_g[:-1], m_g, front_end="gpu")
        assert np.array_equal(e_h.numpy(), e_g.cpu().numpy())
    for kw in (dict(gray_only=True), dict(gray_only=True, edge_searching=True), dict(conv1=conv1, edge_searching=True)):
        host = proposal.search_periodicity_by_feat(im8, m8, repeat_range=(2, 12, 5), device=_dev(), **kw)
        gpu = proposal.search_periodicity_by_feat(im8, m8, repeat_range=(2, 12, 5), device=_dev(), front_end="gpu", **kw)
        assert len(host[0]) >= 1 and len(host[0]) == len(gpu[0])
        for h, g in zip(host, gpu):
            assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(h, g)), kw


def test_search_driver_with_the_gpu_front_end(tmp_path):
    """search.main on the 256 x 256 synthetic directory with --front_end gpu and with host: both write a loadable config.odgt, the
    gpu one says so, the candidates are identical, and where the pseudo mask's centroids do not depend on a tie rule the ranking
    distances are identical too.  Then two images through run.search_all with the switch among the flags."""
    from npp_amd import io as nio, run
    H = 256
    srcs = []
    for i in range(2):
        img, mask = oracle.synthetic_image(H, noise=0.01, seed=i)
        srcs.append(nio.write_detected_dir(str(tmp_path / "input" / f"img{i}"), img, mask, np.ones_like(mask), [[0, 0]], [[1, 1]], [[[1, 0], [0, 1]]]))
    flags = ["--N_iters", "40", "--N_rand", "1024", "--search_range", "2", "12", "5", "--topk_detection", "3", "--random-trunks", "--rng_mode", "fast"]
    odgt = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for fe in ("host", "gpu"):
            out = tmp_path / f"det_{fe}"
            assert search.main(["--datadir", srcs[0], "--outdir", str(out), "--front_end", fe] + flags) == 0
            d = nio.load_npp_completion(str(out / "img0"), p_topk=2)
            assert len(d["angles"]) == 2 and d["img"].shape == (H, H, 3)
            odgt[fe] = json.loads(open(out / "img0" / "config.odgt").readline())
        # the candidates before ranking, and the split that feeds the ranker
        args_h = search.parse(["--datadir", srcs[0], "--front_end", "host"] + flags)
        args_g = search.parse(["--datadir", srcs[0], "--front_end", "gpu"] + flags)
        _, imgs, _, trunks = search._load(search.parse(["--datadir", srcs[0], "--outdir", str(tmp_path / "unused")] + flags))
        cand_h, rk_h = search.prepare_image(imgs[0].astype(np.float32), imgs[2], imgs[3], args_h, None, trunks)
        cand_g, rk_g = search.prepare_image(imgs[0].astype(np.float32), imgs[2], imgs[3], args_g, None, trunks)
    assert "front_end" not in odgt["host"] and odgt["gpu"]["front_end"] == "gpu"
    assert len(cand_h) == len(cand_g) >= 1
    for (a0, p0, s0), (a1, p1, s1) in zip(cand_h, cand_g):
        assert np.array_equal(a0, a1) and np.array_equal(p0, p1) and s0 == s1
    known = imgs[2][..., 0] * imgs[3][..., 0]
    cents, dist, unique = fr.find_mask_centroid_stable(known)
    if unique:
        assert np.array_equal(rk_h.i_train, rk_g.i_train) and np.array_equal(rk_h.i_val, rk_g.i_val)
        for key in ("selected_angles", "selected_periods", "selected_shifts", "distances"):
            assert odgt["host"][key] == odgt["gpu"][key], key
    else:                                                                  # tied centroids: the split may differ, the known pixels it covers may not
        assert sorted(map(tuple, np.concatenate([rk_g.i_train, rk_g.i_val]))) == sorted(map(tuple, np.concatenate([rk_h.i_train, rk_h.i_val])))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        det = str(tmp_path / "det_all")
        assert run.search_all(srcs, det, ["--device", "cuda:0"] + flags + ["--front_end", "gpu"]) == [None, None]
    both = [json.loads(open(os.path.join(det, f"img{i}", "config.odgt")).readline()) for i in range(2)]
    assert all(o["front_end"] == "gpu" and o["distances"] == sorted(o["distances"]) for o in both)
    assert all(len(nio.load_npp_completion(os.path.join(det, f"img{i}"), p_topk=2)["angles"]) == 2 for i in range(2))
