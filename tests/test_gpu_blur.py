"""GPU checks of the remapping task's blur detection (csrc/npp_blur.hip, npp_amd.blur): the gray conversion and the morphology bit
for bit, the singular-value share against LAPACK within a bound set from LAPACK's own fp32 error, the clear mask of a scene whose
mask is not trivial exactly, and the loader and training command on that scene.

The float bound: d32 is the distance between the float64 reference and the SAME formula (in float64) on the singular values
np.linalg.svd returns for float32 windows, computed here on the CPU per case (4.3e-8 on g13 and 7.6e-8 on g13b for the normalised
map); the GPU may be 16 x d32 away (a Jacobi sweep spends more rotations per column than LAPACK's bidiagonal path).  The map test
uses exactly that.  In the raw-share test d32 is exactly 0 or ~1e-16 for many cases (a constant image; sv_num = 20, where numerator
and denominator are the same sum), which no second float64 algorithm can meet: there, and only there, the bound is FLOOR = 32 eps
of float64 (7.1e-15) instead -- the order of the float64 reference's own roundoff over 20 singular values (n eps); everywhere
else it is the plain 16 x d32.  Every figure is printed before it is asserted (pytest -s shows them).  Recorded on an MI355X (profiles/blur_time.txt):
map distance 7.0e-15 on g13 and 7.2e-15 on g13b, raw share within 8.9e-16 in all 72 cases."""
import os

import numpy as np
import pytest
import scipy.ndimage as ndi

import blur_restatement as R

pytestmark = pytest.mark.gpu

FACTOR = 16.0
FLOOR = 32 * np.finfo(np.float64).eps           # the float64 reference's own roundoff (see above)


@pytest.fixture(scope="module")
def dev():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import npp_amd
    npp_amd.lib()
    return torch.device("cuda:0")


_cache = {}


def _golden_case(golden, name):
    """Golden + its fp32-LAPACK map and d32, once per module."""
    if name not in _cache:
        from npp_amd import io as nio
        g = golden(name)
        sv32 = R.singular_values(nio.rgb_to_gray_u8(g["img"]), np.float32)
        map32 = R.normalise(R.share(sv32.astype(np.float64), 3))
        d32 = float(np.abs(map32 - g["blur_map"]).max())
        _cache[name] = (g, d32)
    return _cache[name]


# ---- 1. the map against the reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g13_blur.npz", "g13b_blur_mask.npz"])
def test_map_against_the_reference(dev, golden, name):
    from npp_amd import blur
    g, d32 = _golden_case(golden, name)
    bm, clear = blur.get_blur_map(g["img"], thresh=50, device=dev)
    assert bm.dtype == np.float64 and clear.dtype == np.float64 and bm.shape == g["blur_map"].shape == clear.shape
    dist = float(np.abs(bm - g["blur_map"]).max())
    print(f"{name}: d32 = {d32:.3e}, bound = {FACTOR * d32:.3e}, GPU map distance = {dist:.3e}")
    assert 1e-8 < d32 < 1e-6                                      # the yardstick itself is in the range it was measured in
    assert dist <= FACTOR * d32
    assert bm.min() == 0.0 and bm.max() == 1.0
    assert set(np.unique(clear).tolist()) <= {0.0, 255.0}
    assert np.array_equal(clear, g["clear"])


# ---- 2. the raw share on the windows that can go wrong ----------------------------------------------------------------------------
SHAPES = [(11, 11), (11, 37), (33, 65), (97, 64)]
CONTENTS = R.CONTENTS
_content = R.content


@pytest.mark.parametrize("kind", CONTENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_raw_share_on_hard_windows(dev, shape, kind):
    from npp_amd import blur
    gray = _content(kind, shape)
    sv64, sv32 = R.singular_values(gray, np.float64), R.singular_values(gray, np.float32).astype(np.float64)
    if kind in ("constant", "checkerboard", "rank3"):
        rank = {"constant": 1, "checkerboard": 2, "rank3": 3}[kind]
        assert (sv64[..., rank:] < 1e-9 * sv64[..., :1]).all() and (sv64[..., rank - 1] > 1e-3).any()
    for sv_num in (1, 3, 20):
        ref = R.share(sv64, sv_num)
        d32 = float(np.abs(R.share(sv32, sv_num) - ref).max())
        got = blur.sv_share(gray, sv_num, dev).cpu().numpy()
        assert got.dtype == np.float64 and got.shape == shape
        dist = float(np.abs(got - ref).max())
        bound = max(FACTOR * d32, FLOOR)
        print(f"{kind} {shape} sv_num={sv_num}: d32 = {d32:.3e}, bound = {bound:.3e}, GPU distance = {dist:.3e}")
        assert dist <= bound
        if kind == "zero":
            assert (got == 0).all()                               # 0 / (0 + 1e-6)


def test_share_is_bit_equal_across_changing_shapes(dev):
    """large, small, large in one process: nothing is kept between launches, so every call equals the same call made again (and
    the two large calls each other) bit for bit."""
    from npp_amd import blur
    order = [(97, 64), (11, 11), (97, 64)]
    imgs = [_content("saturated", s, seed=3) for s in order]
    first = [blur.sv_share(g, 3, dev).cpu().numpy() for g in imgs]
    second = [blur.sv_share(g, 3, dev).cpu().numpy() for g in imgs]
    for a, b in zip(first, second):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert np.array_equal(first[0].view(np.uint64), first[2].view(np.uint64))


def test_small_images_and_bad_arguments_are_refused(dev):
    from npp_amd import blur
    for shape in [(10, 40), (40, 10)]:
        with pytest.raises(ValueError, match="image smaller than the blur window"):
            blur.sv_share(np.zeros(shape, np.uint8), 3, dev)
        with pytest.raises(ValueError, match="image smaller than the blur window"):
            blur.get_blur_map(np.zeros(shape + (3,), np.uint8), device=dev)
    for sv_num in (0, 21):
        with pytest.raises(ValueError, match="sv_num"):
            blur.sv_share(np.zeros((16, 16), np.uint8), sv_num, dev)


# ---- 3. gray conversion -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (97, 131), (16, 256)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_gray_conversion_is_bit_equal(dev, shape):
    import torch
    from npp_amd import io as nio, ops
    rs = np.random.RandomState(5)
    img = rs.randint(0, 256, shape + (3,)).astype(np.uint8)
    if shape != (1, 1):
        img[0, 0], img[0, 1] = 255, 0                              # the extremes
    got = ops.rgb_to_gray_u8(torch.from_numpy(img).to(dev)).cpu().numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, nio.rgb_to_gray_u8(img))


# ---- 4. morphology -------------------------------------------------------------------------------------------------------------------
def _masks(shape):
    rs = np.random.RandomState(7)
    H, W = shape
    out = {f"density {p}": rs.rand(H, W) < p for p in (0.1, 0.5, 0.98)}
    out["ones"] = np.ones(shape, bool)
    out["zeros"] = np.zeros(shape, bool)
    corner = np.zeros(shape, bool)
    corner[0, W - 1] = True
    out["corner pixel"] = corner
    return out


@pytest.mark.parametrize("iterations", [1, 20, 40])
@pytest.mark.parametrize("shape", [(11, 11), (64, 64), (97, 131)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_morphology_equals_scipy(dev, shape, iterations):
    from npp_amd import blur
    for name, m in _masks(shape).items():
        ero = blur.binary_erosion(m, iterations, dev).cpu().numpy()
        dil = blur.binary_dilation(m, iterations, dev).cpu().numpy()
        assert ero.dtype == np.uint8 and set(np.unique(ero).tolist()) <= {0, 1} and set(np.unique(dil).tolist()) <= {0, 1}
        assert np.array_equal(ero.astype(bool), ndi.binary_erosion(m, iterations=iterations)), (name, "erosion")
        assert np.array_equal(dil.astype(bool), ndi.binary_dilation(m, iterations=iterations)), (name, "dilation")


# ---- 5. the mask end to end ------------------------------------------------------------------------------------------------------------
def test_mask_end_to_end(dev, golden):
    from npp_amd import blur
    g, d32 = _golden_case(golden, "g13b_blur_mask.npz")
    bound = FACTOR * d32
    margin = float(np.abs(g["blur_map"] - np.percentile(g["blur_map"], int(g["thresh"]))).min())
    print(f"margin of the golden map to its threshold = {margin:.3e}, 2 x map bound = {2 * bound:.3e}")
    assert margin > 2 * bound                                     # no pixel can change sides, the threshold's own shift included
    _, clear = blur.get_blur_map(g["img"], thresh=int(g["thresh"]), device=dev)
    assert np.array_equal(clear, g["clear"])
    assert 0.3 < float((clear > 0).mean()) < 0.6                  # neither empty nor full


# ---- 6. / 7. loader and training command ---------------------------------------------------------------------------------------------
def _detected_dir(tmp_path, img_u8):
    from npp_amd import io as nio
    H, W = img_u8.shape[:2]
    d1, d2 = np.array([9.0, 0.0]), np.array([-3.0, 7.0])                             # the scene's lattice displacements (dx, dy)
    cross = abs(d1[0] * d2[1] - d1[1] * d2[0])
    angles = [[180.0 - np.degrees(np.arctan2(d2[1], d2[0])), 180.0 - np.degrees(np.arctan2(d1[1], d1[0]))]]
    periods = [[cross / np.linalg.norm(d2), cross / np.linalg.norm(d1)]]
    f = img_u8.astype(np.float64) / 255.0 + 1e-9                                     # (write_detected_dir truncates: stay on the 8-bit values)
    return nio.write_detected_dir(str(tmp_path / "g13b"), f, np.ones((H, W)), np.ones((H, W)), angles, periods, [[d1.tolist(), d2.tolist()]])


def test_loader_on_the_gpu_equals_the_host_loader(dev, golden, tmp_path):
    from PIL import Image
    from npp_amd import io as nio
    g = golden("g13b_blur_mask.npz")
    d = _detected_dir(tmp_path, g["img"])
    assert (np.asarray(Image.open(os.path.join(d, "gt_img.png")).convert("RGB")) == g["img"]).all()
    host = nio.load_npp_remapping(d, 1)
    gpu = nio.load_npp_remapping(d, 1, blur_device="cuda:0")
    assert gpu["clear_mask"].dtype == host["clear_mask"].dtype and gpu["clear_mask"].shape == (150, 230, 1)
    assert np.array_equal(gpu["clear_mask"], host["clear_mask"])
    assert np.array_equal(host["clear_mask"][..., 0] * 255, g["clear"])
    assert np.array_equal(gpu["img"], host["img"])


def test_training_command_with_gpu_blur_detection(dev, golden, tmp_path):
    from npp_amd import train
    g = golden("g13b_blur_mask.npz")
    d = _detected_dir(tmp_path, g["img"])
    base = str(tmp_path / "res")
    argv = ["--datadir", d, "--basedir", base, "--p_topk", "1", "--task", "remapping", "--blur_detection", "gpu", "--random-trunks",
            "--N_iters", "6", "--i_testset", "5", "--i_print", "5", "--netwidth", "256", "--N_rand", "2048", "--rng_mode", "fast"]
    plan = train._plan(argv)
    assert np.array_equal(plan.d["clear_mask"][..., 0] * 255, g["clear"])
    fit = train.main(argv)
    assert fit is not None and fit.pixel_mask is not None
    assert os.path.isdir(os.path.join(base, "remapping_top1", "g13b", "testset_000005"))
