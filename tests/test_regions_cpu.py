"""CPU checks of the connected-component entries (include/npp_hip.h npp_cc_*) through the library's plain C++ twins: the definitions
against scipy.ndimage.label and direct NumPy statements (regions_restatement.py) on every case the GPU tests run, the two mask
operations built on them against SciPy / segment.remove_small_objects, the opt-in path of the SLIC connectivity repair against the
host path, and the command-line flag.  No GPU calls."""
import os
import re

import numpy as np
import pytest
import scipy.ndimage as ndi

import regions_restatement as R
from npp_amd import init_segment as iseg, ops, regions, segment, train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.cases()


@pytest.fixture(scope="module")
def yardstick():
    """id -> (numbered, C) by scipy.ndimage.label, computed once."""
    return {cid: R.label(img) for cid, img in CASES}


@pytest.mark.parametrize("cid,img", CASES, ids=[c for c, _ in CASES])
def test_host_twins_equal_the_yardstick(cid, img, yardstick):
    want, C = yardstick[cid]
    lab = img.astype(np.int32)
    root = ops.cc_label_host(lab)
    # the definition itself: -1 outside, else the smallest row-major index of the component
    idx = np.arange(lab.size).reshape(lab.shape)
    first = ndi.minimum(idx, want, np.arange(1, C + 1)).astype(np.int64) if C else np.zeros(0, np.int64)
    assert np.array_equal(root, np.where(want > 0, np.concatenate([[-1], first])[want], -1))
    numbered, n = ops.cc_number_host(root)
    assert n == C and numbered.dtype == np.int32 and np.array_equal(numbered, want)
    got, n2 = regions.label(img)                                                        # the public face, device=None
    assert n2 == C and np.array_equal(got, want)
    colour = R.colour_of(lab.shape)
    sizes, sums, border, boxes = regions.component_stats(numbered, C, colour)
    w_sizes, w_sums, w_border, w_boxes = R.stats(want, C, colour)
    assert sizes.dtype == np.int64 and np.array_equal(sizes, w_sizes) and np.array_equal(sizes, np.bincount(want.ravel(), minlength=C + 1)[1:])
    assert sums.dtype == np.int64 and np.array_equal(sums, w_sums)
    assert np.array_equal(border, w_border) and np.array_equal(boxes, w_boxes)
    s0 = regions.component_stats(numbered, C)                                           # no image: no sums
    assert s0[1].shape == (C, 0) and np.array_equal(s0[0], w_sizes)


@pytest.mark.parametrize("cid,img", [(c, i) for c, i in CASES if i.dtype == bool], ids=[c for c, i in CASES if i.dtype == bool])
def test_fill_holes_and_remove_small_objects(cid, img):
    assert np.array_equal(regions.fill_holes(img), ndi.binary_fill_holes(img))
    assert np.array_equal(regions.fill_holes(img, "cpu"), ndi.binary_fill_holes(img))
    for min_size in (1, 2, 7):
        got = regions.remove_small_objects(img, min_size)
        assert got.dtype == bool and np.array_equal(got, segment.remove_small_objects(img, min_size))


def test_remove_small_objects_at_the_exact_size_of_a_planted_component():
    m = R.planted_pair()
    numbered, C = regions.label(m)
    assert sorted(regions.component_stats(numbered, C)[0].tolist()) == [3, 499, 500]
    for min_size in (1, 2, 3, 4, 499, 500, 501):
        got = regions.remove_small_objects(m, min_size)
        assert np.array_equal(got, segment.remove_small_objects(m, min_size)), min_size
    kept = regions.remove_small_objects(m, 500)
    assert kept[2:22, 2:27].all() and int(kept.sum()) == 500                            # the 499 beside it is gone
    # on the (H, W, 1) array the reference passes, skimage's connectivity=1 partition is the 2-D one
    assert np.array_equal(segment.remove_small_objects(m[..., None], 500)[..., 0], kept)


def test_torch_cpu_tensors_come_back_as_tensors():
    import torch
    m = R.contents(17, 33)["rings"]
    numbered, C = regions.label(torch.from_numpy(m))
    assert isinstance(numbered, torch.Tensor) and np.array_equal(numbered.numpy(), R.label(m)[0]) and C == R.label(m)[1]
    out = regions.fill_holes(torch.from_numpy(m))
    assert isinstance(out, torch.Tensor) and out.dtype == torch.bool and np.array_equal(out.numpy(), ndi.binary_fill_holes(m))


def _min_sizes(labels):
    return (4.0, 30.5, 0.5 * 400.0)


@pytest.mark.parametrize("shape", [(17, 33), (65, 63), (97, 130), (211, 325)])
def test_enforce_connectivity_cc_device_cpu_equals_the_host_path(shape):
    labels = R.blocky(*shape, seed=shape[0])
    colour = R.colour_of(shape, seed=shape[1])
    for min_size in _min_sizes(labels):
        want = iseg.enforce_connectivity(labels, min_size, colour)
        got = iseg.enforce_connectivity(labels, min_size, colour, cc_device="cpu")
        assert got.dtype == want.dtype == np.int32 and np.array_equal(got, want), min_size
    want = iseg.enforce_connectivity(labels, 20, colour, max_size=45)
    assert np.array_equal(iseg.enforce_connectivity(labels, 20, colour, max_size=45, cc_device="cpu"), want)


def test_enforce_connectivity_cc_device_cpu_on_the_scene():
    """The labels of slic_restatement's scene as they can be formed without a GPU: two assign / update rounds of the float64
    restatement (the fragment structure is there from the first round on)."""
    import slic_restatement as S
    img, valid = S.make_scene()[:2]
    labels, step = S.slic_raw(img, valid, 20, 0.1, n_iter=2)
    want = iseg.enforce_connectivity(labels, 0.5 * step * step, img)
    got = iseg.enforce_connectivity(labels, 0.5 * step * step, img, cc_device="cpu")
    assert np.array_equal(got, want) and int(want.max()) > 10
    assert not got[~valid].any()


def test_the_device_path_refuses_a_float_colour_by_name():
    labels = R.blocky(17, 33, seed=1)
    colour = R.colour_of((17, 33))
    with pytest.raises(TypeError, match="colour"):
        iseg.enforce_connectivity(labels, 10, colour.astype(np.float64), cc_device="cpu")
    with pytest.raises(TypeError, match="colour"):
        iseg.enforce_connectivity(labels, 10, colour[..., 0], cc_device="cpu")
    iseg.enforce_connectivity(labels, 10, colour.astype(np.float64))                    # the host path takes it, as before


def test_entry_points_validate_on_the_host():
    import ctypes as C
    import npp_amd
    L = npp_amd.lib()
    fake = C.c_void_p(64)                                                              # never dereferenced: validation comes first
    assert L.npp_cc_label(fake, 0, 5, C.c_void_p(128), None) < 0 and b"npp_cc_label" in L.npp_last_error_string()
    assert L.npp_cc_label(fake, 65536, 32768, C.c_void_p(128), None) < 0               # H W = 2^31
    assert L.npp_cc_label(fake, 4, 4, fake, None) < 0                                  # in place
    assert L.npp_cc_label_host(None, 4, 4, fake) < 0
    assert L.npp_cc_number_scratch_bytes(0, 1) < 0
    assert L.npp_cc_number_scratch_bytes(3, 5) == (15 + 1) * 4 and L.npp_cc_number_scratch_bytes(32, 33) == (1056 + 2) * 4
    assert L.npp_cc_number(fake, 3, 5, fake, fake, fake, 63, None) < 0 and b"scratch" in L.npp_last_error_string()
    assert L.npp_cc_stats(fake, 3, 5, 2, None, 3, fake, fake, fake, fake, None) < 0    # channels without an image
    assert L.npp_cc_stats(fake, 3, 5, 2, fake, 5, fake, fake, fake, fake, None) < 0    # more than 4 channels
    assert L.npp_cc_stats(fake, 3, 5, 16, None, 0, fake, None, fake, fake, None) < 0   # more components than pixels
    assert L.npp_cc_stats_host(fake, 3, 5, -1, None, 0, fake, None, fake, fake) < 0
    # no components: the (empty) outputs may be null pointers, with or without an image
    zero, px = np.zeros((1, 1), np.int32), np.zeros((1, 1, 3), np.uint8)
    assert L.npp_cc_stats_host(zero.ctypes.data, 1, 1, 0, px.ctypes.data, 3, None, None, None, None) == 0
    assert L.npp_cc_stats(fake, 1, 1, 0, fake, 3, None, None, None, None, None) == 0   # nothing to launch


def test_components_flag_parses_and_defaults_to_host():
    assert train.parse(["--datadir", "x"]).components == "host"
    assert train.parse(["--datadir", "x", "--task", "segmentation", "--components", "gpu"]).components == "gpu"
    with pytest.raises(SystemExit):
        train.parse(["--datadir", "x", "--components", "elsewhere"])


def test_run_passes_components_through_train_args():
    import shlex
    a = train.parse(["--datadir", "."] + ["--task", "segmentation"] + shlex.split("--components gpu --netwidth 256"))
    assert a.components == "gpu" and a.task == "segmentation"


def test_segmentation_eval_refuses_an_unknown_final_mask():
    class _NoDevice:
        device = "cpu"
    with pytest.raises(ValueError, match="final_mask"):
        segment.segmentation_eval(None, None, None, None, _NoDevice(), None, final_mask="elsewhere")


def test_the_header_declares_the_new_entries():
    hdr = open(os.path.join(ROOT, "include", "npp_hip.h")).read()
    declared = set(re.findall(r"\b(npp_cc_[a-z0-9_]+)\s*\(", hdr))
    assert declared == {"npp_cc_label", "npp_cc_number", "npp_cc_number_scratch_bytes", "npp_cc_stats", "npp_cc_label_host",
                        "npp_cc_number_host", "npp_cc_stats_host"}
    from npp_amd._lib import SYMBOLS
    assert declared <= set(SYMBOLS)
