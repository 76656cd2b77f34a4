"""The periodicity search's GPU front end (`--front_end gpu`, npp_amd.frontend), the parts that need no GPU: the switch and its
refusals, the C ABI of the new entries, the integer threshold of the far-point walk and the restatement the GPU tests compare with."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import npp_amd
from npp_amd import frontend, proposal, search
from npp_amd._lib import SYMBOLS

import frontend_restatement as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("npp_resize_nearest_u8", "npp_resize_linear_u8", "npp_normalize_u8", "npp_gaussian_blur3_u8", "npp_canny_mark",
           "npp_canny_hysteresis", "npp_canny_finish", "npp_edge_count", "npp_edt_sq", "npp_far_points")


def test_front_end_switch_parses_and_defaults_to_host():
    assert search.parse(["--datadir", "x"]).front_end == "host"
    assert search.parse(["--datadir", "x", "--front_end", "gpu"]).front_end == "gpu"
    assert search.parse(["--datadir", "x", "--front_end", "host"]).front_end == "host"
    with pytest.raises(SystemExit):
        search.parse(["--datadir", "x", "--front_end", "opencv"])


def test_unknown_front_end_is_refused_by_name():
    im, m = np.zeros((8, 8, 3), np.uint8), np.ones((8, 8), np.uint8)
    for call in (lambda: proposal.im2act(im, m, gray_only=True, front_end="opencv"),
                 lambda: proposal.act2edge(None, None, front_end="opencv"),
                 lambda: proposal.search_periodicity_by_feat(im, m, gray_only=True, front_end="opencv")):
        with pytest.raises(ValueError, match="opencv"):
            call()


def test_header_and_symbols_agree_on_the_new_entries():
    hdr = open(os.path.join(ROOT, "include", "npp_hip.h")).read()
    declared = set(re.findall(r"\b(npp_[a-z0-9_]+)\s*\(", hdr))
    for name in ENTRIES:
        assert name in declared and name in SYMBOLS, name
        assert len(re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr).group(1).split(",")) == len(SYMBOLS[name][1]), name
    assert "#define NPP_FAR_POINTS_SCRATCH_BYTES 2048" in hdr
    from npp_amd import ops
    assert ops.FAR_POINTS_SCRATCH_BYTES == 2048 and ops.EDT_MAX_DIM == 32767


def test_null_pointers_and_bad_shapes_are_reported_by_name():
    L = npp_amd.lib()
    p = C.c_void_p(256)                                                   # never dereferenced: the checks come first
    calls = {
        "npp_resize_nearest_u8": [(None, 4, 4, p, 2, 2, None), (p, 4, 4, None, 2, 2, None), (p, 4, 4, C.c_void_p(512), 0, 2, None)],
        "npp_resize_linear_u8": [(None, 4, 4, p, 2, 2, None), (p, 4, 4, None, 2, 2, None), (p, 0, 4, C.c_void_p(512), 2, 2, None)],
        "npp_normalize_u8": [(None, 1, 4, 4, p, None), (p, 1, 4, 4, None, None), (p, 0, 4, 4, p, None), (p, 65536, 4, 4, p, None)],
        "npp_gaussian_blur3_u8": [(None, 1, 4, 4, p, None), (p, 1, 4, 4, None, None), (p, 1, 4, 4, p, None)],
        "npp_canny_mark": [(None, 1, 4, 4, 10, 100, p, None), (p, 1, 4, 4, 10, 100, None, None), (p, 1, 4, 4, 100, 10, C.c_void_p(512), None)],
        "npp_canny_hysteresis": [(None, 1, 4, 4, 8, p, None), (p, 1, 4, 4, 8, None, None), (p, 1, 4, 4, 0, p, None)],
        "npp_canny_finish": [(None, 1, 4, 4, p, None), (p, 1, 4, 4, None, None)],
        "npp_edge_count": [(None, 1, 4, 4, p, p, None), (p, 1, 4, 4, None, p, None), (p, 1, 4, 4, p, None, None)],
        "npp_edt_sq": [(None, 4, 4, p, C.c_void_p(512), None), (p, 4, 4, None, p, None), (p, 4, 4, p, None, None),
                       (p, 4, 32768, C.c_void_p(512), C.c_void_p(1024), None), (p, 4, 4, C.c_void_p(512), C.c_void_p(512), None)],
        "npp_far_points": [(None, 4, 4, 3, 1, p, p, None), (p, 4, 4, 3, 1, None, p, None), (p, 4, 4, 3, 1, p, None, None),
                           (p, 4, 4, 17, 1, p, p, None), (p, 4, 4, 3, -1, p, p, None)],
    }
    assert set(calls) == set(ENTRIES)
    for name, argss in calls.items():
        for args in argss:
            assert getattr(L, name)(*args) < 0, (name, args)
            assert name.encode() in L.npp_last_error_string(), (name, args)


def test_n_min_is_the_float_rule():
    for H in list(range(1, 40)) + [96, 211, 325, 676, 1024, 32767]:
        for W in (1, 7, H, H + 13):
            for ratio in (0.3, 0.25, 0.0, 1.5):
                n = frontend.n_min(H, W, ratio)
                thr = min(H, W) * ratio
                if n == 2 ** 31 - 1:                                      # capped to the kernel's int32: beyond every pair of pixels
                    assert thr > np.sqrt(2.0) * 32766
                    continue
                assert np.sqrt(n) >= thr and (n == 0 or not np.sqrt(n - 1) >= thr), (H, W, ratio, n)
                if min(H, W) <= 700:
                    assert n == fr.n_min(H, W, ratio)
    # the integer comparison decides every pair of pixels as the host's float comparison does
    H, W = 23, 37
    n = frontend.n_min(H, W)
    d2 = np.arange(0, H * H + W * W)
    assert np.array_equal(d2 >= n, np.sqrt(d2) >= min(H, W) * 0.3)


def test_restatement_walks_like_the_host_function():
    masks = fr.golden_masks()
    assert len(masks) == 8 and sorted(m.shape for _, m in masks)[0] == (211, 325) and max(m.shape[0] for _, m in masks) == 676
    for name, m in masks:
        cents, dist, _ = fr.find_mask_centroid_stable(m)
        host_c, host_d = search.find_mask_centroid(m.astype(np.float64))
        assert dist[0] == host_d[0] and len(cents) == len(host_c) == 3, name
        assert dist == sorted(dist, reverse=True)
        thr = min(m.shape) * 0.3
        for i in range(3):
            for j in range(i):
                assert np.hypot(cents[i][0] - cents[j][0], cents[i][1] - cents[j][1]) >= thr
    m, length = fr.spiral_marks(64)
    assert length > 900 and int((m == 2).sum()) == 1 and fr.hysteresis(m).sum() == length
    m[m == 2] = 1
    assert fr.hysteresis(m).sum() == 0
