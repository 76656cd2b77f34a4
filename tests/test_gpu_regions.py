"""GPU checks of the connected-component kernels (csrc/npp_regions.hip) and of the two consumers that opt into them.  The kernels
against scipy.ndimage.label and direct NumPy statements (regions_restatement.py) on every case, with every output and scratch buffer
pre-filled with garbage; changing shapes on one stream; run-to-run identity; the SLIC connectivity repair, the final non-periodic
mask and the training command against their host paths.  Every comparison is exact."""
import contextlib
import os

import numpy as np
import pytest
import scipy.ndimage as ndi

import regions_restatement as R

pytestmark = pytest.mark.gpu
CASES = R.cases()


@pytest.fixture(scope="module")
def dev():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import npp_amd
    npp_amd.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def yardstick():
    return {cid: R.label(img) for cid, img in CASES}


@contextlib.contextmanager
def garbage_empty():
    """Every torch.empty on the GPU -- the outputs and the scratch of the ops.cc_* wrappers -- comes back filled with 0x5A bytes
    (int32 1515870810: neither 0, nor -1, nor an index of any image here)."""
    import torch
    real = torch.empty

    def empty(*a, **k):
        t = real(*a, **k)
        if t.is_cuda and t.numel():
            t.view(torch.uint8).fill_(0x5A)
        return t
    torch.empty = empty
    try:
        yield
    finally:
        torch.empty = real


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _run(dev, img, colour):
    """label -> number -> stats through the ops wrappers, as NumPy."""
    from npp_amd import ops
    root = ops.cc_label(_t(img.astype(np.int32), dev))
    numbered, count = ops.cc_number(root)
    C = int(count.item())
    st = ops.cc_stats(numbered, C, _t(colour, dev))
    return [root.cpu().numpy(), numbered.cpu().numpy(), C] + [s.cpu().numpy() for s in st]


@pytest.mark.parametrize("cid,img", CASES, ids=[c for c, _ in CASES])
def test_kernels_equal_the_yardstick_over_garbage(dev, cid, img, yardstick):
    want, C = yardstick[cid]
    colour = R.colour_of(img.shape)
    with garbage_empty():
        root, numbered, n, sizes, sums, border, boxes = _run(dev, img, colour)
    idx = np.arange(img.size).reshape(img.shape)
    first = ndi.minimum(idx, want, np.arange(1, C + 1)).astype(np.int64) if C else np.zeros(0, np.int64)
    assert np.array_equal(root, np.where(want > 0, np.concatenate([[-1], first])[want], -1))
    assert n == C and np.array_equal(numbered, want)
    w_sizes, w_sums, w_border, w_boxes = R.stats(want, C, colour)
    assert np.array_equal(sizes, w_sizes) and np.array_equal(sums, w_sums)
    assert np.array_equal(border, w_border) and np.array_equal(boxes, w_boxes)


def test_public_module_on_the_device(dev):
    """regions.* with a CUDA device: tensors stay tensors, NumPy comes back as NumPy, and the masks equal SciPy's / the host twins'."""
    import torch
    from npp_amd import regions, segment
    for name in ("rings", "frame", "random0.59", "serpentine", "zeros", "ones"):
        m = R.contents(97, 130)[name]
        with garbage_empty():
            got = regions.fill_holes(m, dev)
            got_t = regions.fill_holes(_t(m, dev))
            small = regions.remove_small_objects(_t(m, dev), 7, dev)
        assert isinstance(got, np.ndarray) and got.dtype == bool and np.array_equal(got, ndi.binary_fill_holes(m)), name
        assert isinstance(got_t, torch.Tensor) and got_t.is_cuda and np.array_equal(got_t.cpu().numpy(), got)
        assert small.is_cuda and np.array_equal(small.cpu().numpy(), segment.remove_small_objects(m, 7)), name
    m = R.planted_pair()
    for min_size in (1, 2, 499, 500, 501):
        assert np.array_equal(regions.remove_small_objects(m, min_size, dev), segment.remove_small_objects(m, min_size)), min_size
    numbered, C = regions.label(R.blocky(65, 63, 3), dev)
    want, Cw = R.label(R.blocky(65, 63, 3))
    assert C == Cw and isinstance(numbered, np.ndarray) and np.array_equal(numbered, want)


def test_two_shapes_alternate_on_one_stream(dev, yardstick):
    """Nothing kept from one call may serve the next at another shape: (97,130) and (211,325) three times in turn, no
    synchronisation in between, results exact every time."""
    a, b = "97x130-random0.59", "211x325-serpentine"
    imgs = dict(CASES)
    from npp_amd import ops
    outs = []
    with garbage_empty():
        for _ in range(3):
            for cid in (a, b):
                numbered, count = ops.cc_number(ops.cc_label(_t(imgs[cid].astype(np.int32), dev)))
                st = ops.cc_stats(numbered, yardstick[cid][1], _t(R.colour_of(imgs[cid].shape), dev))
                outs.append((cid, numbered, count, st))
    for cid, numbered, count, st in outs:
        want, C = yardstick[cid]
        assert int(count.item()) == C and np.array_equal(numbered.cpu().numpy(), want)
        for got, ref in zip(st, R.stats(want, C, R.colour_of(want.shape))):
            assert np.array_equal(got.cpu().numpy(), ref)


def test_two_runs_are_bit_identical(dev):
    imgs = dict(CASES)
    for cid in ("211x325-random0.59", "211x325-blocky", "65x63-spiral"):
        colour = R.colour_of(imgs[cid].shape)
        first = _run(dev, imgs[cid], colour)
        with garbage_empty():
            again = _run(dev, imgs[cid], colour)
        for x, y in zip(first, again):
            assert np.array_equal(x, y), cid


# ---- the SLIC connectivity repair on the labels the SLIC kernels leave ----------------------------------------------------------------
FAR_ROW = 7


def _slic_case(name):
    """The `scene` and `97x64` inputs of test_gpu_init_segment.py, rebuilt here."""
    if name == "scene":
        import slic_restatement as S
        return S.make_scene()[:2]
    shape, seed = (97, 64), 4
    rs = np.random.RandomState(seed)
    a = ndi.gaussian_filter(rs.rand(*shape, 3), (6, 6, 0))
    a = (a - a.min()) / (a.max() - a.min()) + rs.normal(0, 0.03, a.shape)
    img = np.uint8(np.rint(np.clip(a, 0, 1) * 255))
    mask = np.zeros(shape, bool)
    mask[:shape[0] * 2 // 5] = True
    mask[-FAR_ROW] = True
    mask[3:9, 5:11] = False
    return img, mask


@pytest.mark.parametrize("name", ["scene", "97x64"])
def test_enforce_connectivity_on_the_device_equals_the_host_path(dev, name):
    from npp_amd import init_segment as iseg
    img, mask = _slic_case(name)
    labels, S = iseg.slic_raw(img, mask, 20, 0.1, device=dev)
    want = iseg.enforce_connectivity(labels, 0.5 * S * S, img)
    with garbage_empty():
        got = iseg.enforce_connectivity(labels, 0.5 * S * S, img, cc_device=dev)
    assert got.dtype == want.dtype and np.array_equal(got, want)
    assert np.array_equal(iseg.enforce_connectivity(labels, 0.5 * S * S, img, cc_device="cpu"), want)
    assert np.array_equal(iseg.slic(img, mask, 20, 0.1, device=dev, cc_device=dev), want)


# ---- the final non-periodic mask ---------------------------------------------------------------------------------------------------
def _eval_pair():
    """96 x 130: the 'fitted' image and the 'input' differ by 0.5 gray on a disc (about 700 pixels), on a ring whose hole (the same in both)
    must be filled, and on specks below 500 pixels that must go."""
    H, W = 96, 130
    yy, xx = np.mgrid[:H, :W]
    rs = np.random.RandomState(2)
    base = 0.25 + 0.1 * np.sin(yy / 3.0)[..., None] * np.cos(xx / 4.0)[..., None] + rs.uniform(0, 0.02, (H, W, 3))
    disc = (yy - 30) ** 2 + (xx - 30) ** 2 < 15 ** 2
    d2 = (yy - 60) ** 2 + (xx - 95) ** 2
    ring = (d2 < 18 ** 2) & (d2 >= 7 ** 2)
    specks = np.zeros((H, W), bool)
    specks[80:83, 10:14] = True
    specks[5:9, 120:124] = True
    specks[88, 60:75] = True
    planted = disc | ring | specks
    other = base + 0.5 * planted[..., None]
    return base.astype(np.float32), other.astype(np.float32), disc, ring, d2 < 18 ** 2, specks


def test_segmentation_eval_final_mask_on_the_device(dev):
    import warnings
    from npp_amd import segment
    pred, blur, disc, ring, ring_filled, specks = _eval_pair()
    H, W = disc.shape
    valid = np.ones((H, W, 1), np.float32)
    cand = np.ones((H, W, 1), np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        alex = segment.AlexFeatures(None, device=dev)
    lins = [np.full(c, 1.0 / c, np.float32) for c in (64, 192, 384, 256, 256)]
    host = segment.segmentation_eval(pred, blur, valid, cand, alex, lins, l1_thresh=0.15, lpips_thresh=1e9, lpips_layers=2)
    gpu = segment.segmentation_eval(pred, blur, valid, cand, alex, lins, l1_thresh=0.15, lpips_thresh=1e9, lpips_layers=2, final_mask="gpu")
    a, b = host["non_period_mask_final"], gpu["non_period_mask_final"]
    assert a.shape == b.shape == (H, W, 1) and a.dtype == b.dtype and np.array_equal(a, b)
    assert np.array_equal(b[..., 0] > 0, disc | ring_filled)                             # hole filled, specks gone: the test has teeth
    assert sorted(host) == sorted(gpu)
    for k in ("l1_img", "l1_mask"):
        assert host[k].dtype == gpu[k].dtype and np.array_equal(host[k], gpu[k]), k
    assert len(host["lpips_maps"]) == len(gpu["lpips_maps"]) == 2
    for x, y in zip(host["lpips_maps"], gpu["lpips_maps"]):
        assert np.array_equal(x, y)


# ---- the training command -------------------------------------------------------------------------------------------------------
def _scene_dir(tmp_path, scene):
    """The directory recipe of test_gpu_init_segment.py's end-to-end test."""
    from npp_amd import io as nio
    img, valid = scene[:2]
    th = np.deg2rad(20.0)
    d1 = 9.0 * np.array([np.cos(th), np.sin(th)])
    d2 = 10.8 * np.array([-np.sin(th), np.cos(th)])
    cross = abs(d1[0] * d2[1] - d1[1] * d2[0])
    angles = [[180.0 - np.degrees(np.arctan2(d2[1], d2[0])), 180.0 - np.degrees(np.arctan2(d1[1], d1[0]))]]
    periods = [[cross / np.linalg.norm(d2), cross / np.linalg.norm(d1)]]
    shifts = [[d1.tolist(), d2.tolist()]]
    f = img.astype(np.float64) / 255.0 + 1e-9
    return nio.write_detected_dir(str(tmp_path / "scene"), f, np.ones(valid.shape), valid.astype(np.float64), angles, periods, shifts)


def test_training_command_with_components_on_the_gpu(dev, tmp_path):
    from PIL import Image
    import slic_restatement as S
    from npp_amd import train
    d = _scene_dir(tmp_path, S.make_scene())
    base = str(tmp_path / "res")
    argv = ["--datadir", d, "--basedir", base, "--p_topk", "1", "--task", "segmentation", "--random-trunks", "--N_iters", "31",
            "--i_testset", "30", "--netwidth", "256"]
    train.main(argv + ["--expname", "hostcc"])
    train.main(argv + ["--expname", "gpucc", "--components", "gpu"])
    for rel in ("segment_init.png", os.path.join("testset_000030", "non_period_mask_final.png")):
        a = np.asarray(Image.open(os.path.join(base, "hostcc_top1", "scene", rel)))
        b = np.asarray(Image.open(os.path.join(base, "gpucc_top1", "scene", rel)))
        assert a.shape == b.shape and np.array_equal(a, b), rel
    init = np.asarray(Image.open(os.path.join(base, "gpucc_top1", "scene", "segment_init.png")).convert("L")) > 127
    assert init.any() and not init.all()
