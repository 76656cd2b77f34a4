"""GPU checks of the initial coarse segmentation: every kernel of csrc/npp_slic.hip against the float64 restatement in
slic_restatement.py (each SLIC round from the GPU's OWN state, so that one flipped near-tie cannot snowball into a false failure),
then the pipeline by what it is for -- finding planted non-periodic regions -- and end to end through the loader and the training
command."""
import os

import numpy as np
import pytest

import slic_restatement as R

pytestmark = pytest.mark.gpu

SP_SIZE, SP_REGUL = 20, 0.1
M = (SP_SIZE * SP_REGUL) ** 1.5


@pytest.fixture(scope="module")
def dev():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import npp_amd
    npp_amd.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def scene():
    return R.make_scene()


def _random_image(shape, seed):
    """Smooth blobs + noise: colour structure for SLIC to follow, every 8-bit value in play."""
    import scipy.ndimage as ndi
    rs = np.random.RandomState(seed)
    a = ndi.gaussian_filter(rs.rand(*shape, 3), (6, 6, 0))
    a = (a - a.min()) / (a.max() - a.min()) + rs.normal(0, 0.03, a.shape)
    return np.uint8(np.rint(np.clip(a, 0, 1) * 255))


def _mask_with_far_strip(shape):
    """Top part valid + one far row (FAR_ROW from the bottom, off the start grid for both shapes): the row's pixels have no centre
    within +-2S (the all-centres branch of assign)."""
    mask = np.zeros(shape, bool)
    mask[:shape[0] * 2 // 5] = True
    mask[-FAR_ROW] = True
    mask[3:9, 5:11] = False
    return mask


FAR_ROW = 7
CASES = {"scene": None, "211x325": ((211, 325), 3), "97x64": ((97, 64), 4)}


def _case(name):
    if name == "scene":
        img, valid = R.make_scene()[:2]
        return img, valid
    shape, seed = CASES[name]
    return _random_image(shape, seed), _mask_with_far_strip(shape)


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# fp32 cube root and power: ~1e-5 relative on values up to 100; the blur: 9 taps of 1e-7
PREPARE_BOUND = 1e-3


@pytest.mark.parametrize("name", list(CASES))
def test_prepare(dev, name):
    from npp_amd import ops
    img, _ = _case(name)
    lab = ops.slic_prepare(_t(img, dev), float(img.min()), float(img.max()), M).cpu().numpy().astype(np.float64) * M
    ref = R.prepare(img)
    err = float(np.abs(lab - ref).max())
    print(f"prepare {name}: max abs error {err:.3e} Lab units (L range {ref[0].min():.1f}..{ref[0].max():.1f})")
    assert lab.shape == (3,) + img.shape[:2]
    assert err <= PREPARE_BOUND


def _slic_state(dev, img, mask, extra_empty_centre=True):
    """The GPU's prepared planes and start centres as init_segment.slic builds them (+ one centre nobody can pick: far in colour)."""
    import torch
    from npp_amd import ops, init_segment as iseg
    _, S, pos = iseg.slic_geometry(mask, SP_SIZE)
    lab = ops.slic_prepare(_t(img, dev), float(img.min()), float(img.max()), M)
    t_pos = _t(pos.astype(np.float32), dev)
    centres = torch.cat([t_pos, lab[:, t_pos[:, 0].long(), t_pos[:, 1].long()].t()], 1)
    if extra_empty_centre:
        far = torch.tensor([[pos[0, 0], pos[0, 1], 1e4, 1e4, 1e4]], dtype=torch.float32, device=dev)
        centres = torch.cat([centres, far], 0)
    return lab, _t(mask.astype(np.uint8), dev), centres.contiguous(), float(np.float32(S))


@pytest.mark.parametrize("name", list(CASES))
def test_assign_and_update_round_by_round(dev, name):
    """Ten rounds; each is checked from the GPU's own centres and labels.  assign: the restatement's D2 of the label the GPU chose
    <= the restatement's minimum (1 + 1e-5) + 1e-6 (D2 is a sum of five fp32 squares: relative rounding below 1e-6), so labels
    differ from the restatement's argmin only at such near-ties; label 0 exactly outside the mask.  update: centres within 1e-4 of
    the restatement's means of the GPU's labels (fp32 results of exact integer / 2^-20 fixed-point sums); empty centres untouched."""
    from npp_amd import ops
    img, mask = _case(name)
    lab, t_mask, centres, S = _slic_state(dev, img, mask)
    lab64 = lab.cpu().numpy().astype(np.float64)
    K = centres.shape[0]
    labels = None
    far_rows = 0
    for it in range(10):
        c64 = centres.cpu().numpy().astype(np.float64)
        labels = ops.slic_assign(lab, t_mask, centres, S, labels)
        lg = labels.cpu().numpy()
        assert ((lg == 0) == ~mask).all() and lg.max() <= K
        ref_labels, dmin = R.assign(lab64, mask, c64, S)
        dg = R.d2_of_labels(lab64, c64, S, lg)
        worst = float((dg[mask] - dmin[mask]).max())
        ndiff = int((lg != ref_labels).sum())
        print(f"{name} round {it}: {ndiff} labels differ from the float64 argmin, worst D2 excess {worst:.2e}")
        assert (dg[mask] <= dmin[mask] * (1 + 1e-5) + 1e-6).all()
        far_rows += R.pixels_without_candidate(mask, c64, S)
        before = centres.clone()
        ops.slic_update(lab, labels, centres)
        ref = R.update(lab64, lg, c64)
        got = centres.cpu().numpy().astype(np.float64)
        err = float(np.abs(got - ref).max())
        print(f"{name} round {it}: centres max abs error {err:.2e}")
        assert err <= 1e-4
        empty = np.bincount(lg.ravel(), minlength=K + 1)[1:] == 0
        assert empty[-1] and (centres[_t(empty, dev)] == before[_t(empty, dev)]).all()
    if name != "scene":
        assert far_rows > 0                      # the far strip's pixels had no centre in their window: the all-centres branch ran


def _check_features(dev, img, labels, N):
    from npp_amd import ops
    count, feat = ops.slic_features(_t(img, dev), _t(labels.astype(np.int32), dev), N)
    count, feat = count.cpu().numpy(), feat.cpu().numpy().astype(np.float64)
    rc, rcen, rf = R.features(img, labels)
    assert (count == rc).all()                                                        # exact
    assert (feat[:, 5:8] == rf[:, 3:6]).all()                                         # medians exact
    np.testing.assert_allclose(feat[:, :2], rcen, rtol=1e-4, atol=1e-3)
    np.testing.assert_allclose(feat[:, 2:5], rf[:, 0:3], rtol=1e-4, atol=1e-3)
    np.testing.assert_allclose(feat[:, 8:11], rf[:, 6:9], rtol=1e-4, atol=1e-3)
    return count, feat


def test_features(dev, scene):
    from npp_amd import init_segment as iseg
    img, valid = scene[:2]
    sp = iseg.slic(img, valid, SP_SIZE, SP_REGUL, device=dev)                         # the repaired label image
    _check_features(dev, img, sp, int(sp.max()))
    for shape, n_sp, seed in (((211, 325), 300, 7), ((97, 64), 40, 8)):             # superpixels scattered over the whole frame
        rs = np.random.RandomState(seed)
        im = rs.randint(0, 256, shape + (3,)).astype(np.uint8)
        labels = rs.randint(0, n_sp + 1, shape).astype(np.int32)
        labels[0, 0] = n_sp
        count, _ = _check_features(dev, im, labels, n_sp)
        assert (count % 2 == 0).any() and (count % 2 == 1).any()                      # both median forms
    # a label without pixels: count 0 and NaN from the kernel, zeros from the host wrapper
    from npp_amd import ops
    labels[labels == 5] = 6
    count, feat = ops.slic_features(_t(im, dev), _t(labels, dev), n_sp)
    assert int(count[4]) == 0 and bool(feat[4].isnan().all()) and not bool(feat[5].isnan().any())
    _, cen, feats = iseg.superpixel_features(im, labels, device=dev)
    assert (feats[4] == 0).all() and (cen[4] == 0).all()


def _run_all(dev, img, mask):
    from npp_amd import ops
    lab, t_mask, centres, S = _slic_state(dev, img, mask, extra_empty_centre=False)
    labels = ops.slic_assign(lab, t_mask, centres, S)
    ops.slic_update(lab, labels, centres)
    labels2 = ops.slic_assign(lab, t_mask, centres, S)
    count, feat = ops.slic_features(_t(img, dev), labels2, centres.shape[0])
    return [t.cpu().numpy() for t in (lab, labels, centres, labels2, count, feat)]


def test_shapes_change_between_calls(dev):
    """Two image sizes back to back through the same entry points, then the first again: nothing kept from one call may serve the
    next at another shape."""
    a, b = _case("97x64"), _case("211x325")
    first = _run_all(dev, *a)
    other = _run_all(dev, *b)
    again = _run_all(dev, *a)
    for x, y in zip(first, again):
        assert np.array_equal(x, y, equal_nan=True)
    for (img, mask), out in ((a, first), (b, other)):
        lab, labels, centres, labels2, count, feat = out
        assert np.abs(lab.astype(np.float64) * M - R.prepare(img)).max() <= PREPARE_BOUND
        assert ((labels == 0) == ~mask).all() and ((labels2 == 0) == ~mask).all()
        rc, rcen, rf = R.features(img, labels2)
        n = len(rc)
        assert (count[:n] == rc).all() and (count[n:] == 0).all()
        has = rc > 0
        assert (feat[:n][has, 5:8] == rf[has, 3:6]).all()


def test_pipeline_is_reproducible(dev, scene):
    from npp_amd import init_segment as iseg
    img, valid = scene[:2]
    a = iseg.initial_segmentation(img, valid, device=dev)
    b = iseg.initial_segmentation(img, valid, device=dev)
    assert sorted(a) == ["non_period_mask", "period_mask", "proba", "seg", "slic"]
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_pipeline_finds_the_planted_regions(dev, scene):
    """IoU of the GPU pipeline's period_mask >= the restatement's - 0.02 (one superpixel is ~0.6 % of the image: a handful of
    boundary superpixels may fall the other way, a lost region may not); the disc and the block >= 90 % inside non_period_mask.
    The restatement's own figures (CPU): IoU 0.9998, disc 1.000, block 1.000; the test prints the GPU pipeline's."""
    from npp_amd import init_segment as iseg
    img, valid, truth, disc, block = scene
    out = iseg.initial_segmentation(img, valid, device=dev)
    ref = R.pipeline(img, valid)
    v, vr = R.iou(out["period_mask"], truth), R.iou(ref["period_mask"], truth)
    in_disc = (out["non_period_mask"] & disc).sum() / disc.sum()
    in_block = (out["non_period_mask"] & block & valid).sum() / (block & valid).sum()
    print(f"GPU pipeline: IoU {v:.4f} (restatement {vr:.4f}), disc {in_disc:.3f}, block {in_block:.3f}, "
          f"{out['slic'].max()} superpixels (restatement {ref['slic'].max()})")
    assert v >= vr - 0.02
    assert in_disc >= 0.9 and in_block >= 0.9
    assert not (out["period_mask"] & out["non_period_mask"]).any()
    assert not out["period_mask"][~valid].any() and not out["non_period_mask"][~valid].any()


def _scene_dir(tmp_path, scene):
    from npp_amd import io as nio
    img, valid = scene[:2]
    th = np.deg2rad(20.0)
    d1 = 9.0 * np.array([np.cos(th), np.sin(th)])                                    # the lattice's two displacements (dx, dy)
    d2 = 10.8 * np.array([-np.sin(th), np.cos(th)])
    cross = abs(d1[0] * d2[1] - d1[1] * d2[0])
    angles = [[180.0 - np.degrees(np.arctan2(d2[1], d2[0])), 180.0 - np.degrees(np.arctan2(d1[1], d1[0]))]]
    periods = [[cross / np.linalg.norm(d2), cross / np.linalg.norm(d1)]]
    shifts = [[d1.tolist(), d2.tolist()]]
    f = img.astype(np.float64) / 255.0 + 1e-9                                        # (write_detected_dir truncates: stay on the 8-bit values)
    return nio.write_detected_dir(str(tmp_path / "scene"), f, np.ones(valid.shape), valid.astype(np.float64), angles, periods, shifts)


def test_loader_and_training_command_end_to_end(dev, scene, tmp_path):
    from PIL import Image
    from npp_amd import io as nio, train, init_segment as iseg
    img, valid = scene[:2]
    d = _scene_dir(tmp_path, scene)
    assert (np.asarray(Image.open(os.path.join(d, "gt_img.png")).convert("RGB")) == img).all()
    with pytest.raises(FileNotFoundError, match="period_mask.png"):
        nio.load_npp_segmentation(d, 1, init_seg=None)
    out = nio.load_npp_segmentation(d, 1, init_seg="auto", device=dev)
    assert out["init_seg_source"] == "computed" and out["period_mask"].shape == (256, 256, 1)
    direct = iseg.initial_segmentation(img, valid, device=dev)
    assert ((out["period_mask"][..., 0] > 0) == direct["period_mask"]).all()
    assert ((out["non_period_mask"][..., 0] > 0) == direct["non_period_mask"]).all()
    base = str(tmp_path / "res")
    argv = ["--datadir", d, "--basedir", base, "--p_topk", "1", "--task", "segmentation", "--random-trunks", "--N_iters", "31",
            "--i_testset", "30", "--netwidth", "256"]
    plan = train._plan(argv)
    assert plan is not None and not os.path.exists(base)                              # planning creates nothing
    assert np.array_equal(plan.d["period_mask"], out["period_mask"])
    train.main(argv)
    root = os.path.join(base, "segmentation_top1", "scene")
    init = np.asarray(Image.open(os.path.join(root, "segment_init.png")).convert("L")) > 127
    assert (init == (out["non_period_mask"][..., 0] > 0)).all()                       # white where non-periodic
    assert os.path.exists(os.path.join(root, "testset_000030", "segment.png"))
    # with the two PNGs present, 'auto' reads them
    blob = np.zeros((256, 256))
    blob[100:140, 60:120] = 1
    nio.imsave(os.path.join(d, "non_period_mask.png"), np.repeat(blob[..., None], 3, 2))
    nio.imsave(os.path.join(d, "period_mask.png"), np.repeat(1.0 - blob[..., None], 3, 2))
    plan = train._plan(argv + ["--init_segmentation", "auto", "--expname", "second"])
    assert plan.d["init_seg_source"] == "files" and (plan.d["non_period_mask"][..., 0] == blob).all()
    assert (plan.d["period_mask"][..., 0] == (1 - blob) * valid).all()
    plan = train._plan(argv + ["--init_segmentation", "compute", "--expname", "third"])
    assert plan.d["init_seg_source"] == "computed" and np.array_equal(plan.d["period_mask"], out["period_mask"])
