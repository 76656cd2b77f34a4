"""CPU checks of the GPU blur detection's host side (npp_amd.blur, the loader and command-line switches).  No GPU calls."""
import inspect

import numpy as np
import pytest
import scipy.ndimage as ndi

import blur_restatement as R
from npp_amd import blur, io as nio, train


def test_blur_detection_flag_parses_and_defaults_to_host():
    assert train.parse(["--datadir", "x"]).blur_detection == "host"
    assert train.parse(["--datadir", "x", "--task", "remapping", "--blur_detection", "gpu"]).blur_detection == "gpu"
    with pytest.raises(SystemExit):
        train.parse(["--datadir", "x", "--blur_detection", "elsewhere"])


def test_loader_signature_has_blur_device_none():
    p = inspect.signature(nio.load_npp_remapping).parameters
    assert "blur_device" in p and p["blur_device"].default is None


def test_other_window_sizes_are_refused_by_name():
    img = np.zeros((32, 32, 3), np.uint8)
    with pytest.raises(ValueError, match=r"io\.get_blur_map"):
        blur.get_blur_map(img, win_size=8)


def test_host_finishing_reproduces_the_golden_mask(golden):
    """normalise -> percentile -> `>` of blur.finish on an UN-normalised map (the golden's, spread affinely over [0.3, 0.8] like a
    raw share), SciPy for the morphology: the golden's map to rounding and its clear mask exactly."""
    g = golden("g13b_blur_mask.npz")
    raw = 0.3 + 0.5 * g["blur_map"]
    assert raw.min() == 0.3 and raw.max() == 0.8
    bm, binary = blur.finish(raw, int(g["thresh"]))
    assert bm.dtype == np.float64 and bm.min() == 0.0 and bm.max() == 1.0
    assert np.abs(bm - g["blur_map"]).max() < 1e-15
    binary = ndi.binary_dilation(ndi.binary_erosion(binary, iterations=20), iterations=40)
    clear = (~binary).astype(np.float64) * 255
    assert np.array_equal(clear, g["clear"])
    assert 0.3 < (clear > 0).mean() < 0.6


def test_golden_scene_is_the_recipe_and_matches_the_host_path(golden):
    """g13b's image is the documented recipe and io.get_blur_map (the host restatement g13 pins) gives its map and mask."""
    g = golden("g13b_blur_mask.npz")
    assert g["img"].shape == (150, 230, 3) and g["img"].dtype == np.uint8 and g["img"].size // 3 % 2 == 0
    assert np.array_equal(R.make_image(), g["img"])                                  # the recipe the timing tool scales up
    assert g["blur_map"].max() == g["blur_map"][20:60, 30:70].max()                   # the flat patch holds the maximum
    bm, clear = nio.get_blur_map(g["img"], thresh=int(g["thresh"]))
    assert np.abs(bm - g["blur_map"]).max() < 1e-9
    assert np.array_equal(clear, g["clear"])


@pytest.mark.parametrize("kind", R.CONTENTS + ["uniform"])
def test_jacobi_restatement_converges_within_the_sweep_cap(kind):
    """What the kernel's cap of 16 sweeps rests on: its loop, restated in NumPy with the same ordering and tolerance, on every
    window of a 24 x 29 image of each kind (every window touches a mirrored border or lies inside): at most 12 sweeps including the
    confirming one, nothing still rotating, the share within 1e-13 of LAPACK's; with the tolerance at 1e-6 still within 1e-11."""
    blocks = R.windows(R.content(kind, (24, 29), seed=1)).reshape(-1, 20, 20)
    ref = np.linalg.svd(blocks, compute_uv=False)
    sv, used, rotating = R.jacobi_singular_values(blocks)
    assert used.max() <= 12 and not rotating.any()
    sv = -np.sort(-sv, 1)
    loose = -np.sort(-R.jacobi_singular_values(blocks, tol=1e-6)[0], 1)
    for n in (1, 3, 20):
        assert np.abs(R.share(sv, n) - R.share(ref, n)).max() < 1e-13
        assert np.abs(R.share(loose, n) - R.share(ref, n)).max() < 1e-11
    print(kind, "sweeps", used.max())
