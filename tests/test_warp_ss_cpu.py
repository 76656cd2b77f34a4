"""The antialiased image warp without a GPU: the host twin of npp_warp_image_u8_ss against the NumPy restatement bit for bit, the
rule's branches counted on the restatement, cases whose result follows without it (block means, a stripe texture, the darkest
sample, a source one pixel high), the refusals by name and the rectify command's --supersample path on the CPU."""
import ctypes as C
import os

import numpy as np
import pytest

import view_restatement as R
import warp_ss_restatement as W
import npp_amd
from npp_amd import ops, view

SRC, CANVAS = W.WARP_SRC, W.WARP_CANVAS
MODES = ("nearest", "bilinear")


# ---- host twin = restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduce", W.REDUCES)
@pytest.mark.parametrize("ss", W.SS)
@pytest.mark.parametrize("mode", MODES)
def test_host_twin_equals_the_restatement_bit_for_bit(mode, ss, reduce):
    for Cn in (1, 3, 4):
        src = W.warp_source(Cn)
        for name, M in W.WARP_MAPS.items():
            out, inside = view.warp_image(src, M, CANVAS, mode, supersample=ss, reduce=reduce)
            rout, rin = W.warp_image_ss(src, M, CANVAS, mode, ss, reduce)
            assert out.shape == CANVAS + src.shape[2:] and out.dtype == np.uint8 and inside.shape == CANVAS and inside.dtype == np.uint8
            assert np.array_equal(out, rout), (name, Cn)
            assert np.array_equal(inside, rin), (name, Cn)
            assert not out[inside == 0].any() and set(np.unique(inside)) <= {0, 255}


def _ss_entry(src, M, size, mode, ss, reduce):
    """npp_warp_image_u8_ss_host itself (ops takes the point entry at the defaults) -> (return code, out, inside)."""
    src = np.ascontiguousarray(src, np.uint8)
    out = np.full(tuple(size) + src.shape[2:], 0xA5, np.uint8)
    inside = np.full(tuple(size), 0xA5, np.uint8)
    m = (C.c_double * 9)(*np.asarray(M, np.float64).reshape(9))
    rc = npp_amd.lib().npp_warp_image_u8_ss_host(C.c_void_p(src.ctypes.data), src.shape[0], src.shape[1], 1 if src.ndim == 2 else src.shape[2],
                                                 size[0], size[1], m, mode, ss, reduce, C.c_void_p(out.ctypes.data),
                                                 C.c_void_p(inside.ctypes.data))
    return rc, out, inside


@pytest.mark.parametrize("mode", MODES)
def test_one_sample_is_the_point_warp_byte_for_byte(mode):
    for Cn in (1, 3, 4):
        src = W.warp_source(Cn)
        for name, M in W.WARP_MAPS.items():
            want, win = R.warp_image(src, M, CANVAS, mode)                      # today's rule
            for reduce in (0, 1):
                rc, out, inside = _ss_entry(src, M, CANVAS, MODES.index(mode), 1, reduce)
                assert rc == 0 and np.array_equal(out, want) and np.array_equal(inside, win), (name, Cn, reduce)
            out, inside = view.warp_image(src, M, CANVAS, mode, supersample=1, reduce="min")
            assert np.array_equal(out, want) and np.array_equal(inside, win), (name, Cn)


# ---- the cases exercise the rule's branches (counted on the restatement) ---------------------------------------------------------------
@pytest.mark.parametrize("ss", (2, 4, 8))
@pytest.mark.parametrize("mode", MODES)
def test_cases_reach_partial_pixels_and_centres_outside(mode, ss):
    src = W.warp_source(3)
    for name in ("affine", "projective", "horizon"):
        counts, centre = W.sample_counts(src, W.WARP_MAPS[name], CANVAS, mode, ss)
        n = counts.sum(-1)
        assert int(((n > 0) & (n < ss * ss)).sum()) >= 10, name                 # some but not all samples count
        orphan = ~centre & (n > 0)                                               # samples count, the centre is outside
        assert int(orphan.sum()) >= 5, name
        for reduce in W.REDUCES:
            out, inside = W.warp_image_ss(src, W.WARP_MAPS[name], CANVAS, mode, ss, reduce)
            assert not out[orphan].any() and not inside[orphan].any(), (name, reduce)
            got, gin = view.warp_image(src, W.WARP_MAPS[name], CANVAS, mode, supersample=ss, reduce=reduce)
            assert not got[orphan].any() and not gin[orphan].any(), (name, reduce)
    for name, border in (("identity", 79), ("shift", 71)):
        counts, centre = W.sample_counts(src, W.WARP_MAPS[name], CANVAS, mode, ss)
        n = counts.sum(-1)
        assert int(((n > 0) & (n < ss * ss)).sum()) == (border if mode == "bilinear" else 0), name
        assert not (~centre & (n > 0)).any()


def test_smallest_branch_counts_are_those_of_the_affine_nearest_case():
    counts, centre = W.sample_counts(W.warp_source(3), W.WARP_MAPS["affine"], CANVAS, "nearest", 2)
    n = counts.sum(-1)
    assert int(((n > 0) & (n < 4)).sum()) == 14 and int((~centre & (n > 0)).sum()) == 6


# ---- results that follow without the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("S", (2, 4, 8))
def test_block_means_are_exact(S):
    src, M, size, want = W.block_mean_case(S)
    for mode in MODES:
        out, inside = view.warp_image(src, M, size, mode, supersample=S)
        assert np.array_equal(out, want), mode
        assert (inside == 255).all()


def test_supersampling_removes_the_alias_of_a_stripe_texture():
    src, M, size = W.stripe_case()
    out, inside = view.warp_image(src, M, size, "bilinear")
    assert (out == 0).all() and (inside == 255).all()                 # point sampling: a 50 % grey texture comes out black
    out, inside = view.warp_image(src, M, size, "bilinear", supersample=4)
    assert (out == 128).all() and (inside == 255).all()


@pytest.mark.parametrize("S", (2, 4, 8))
def test_min_takes_the_darkest_sample(S):
    src, M, size, mean = W.block_min_case(S)
    for mode in MODES:
        out, inside = view.warp_image(src, M, size, mode, supersample=S, reduce="min")
        assert (out == 0).all() and (inside == 255).all(), mode
        out, inside = view.warp_image(src, M, size, mode, supersample=S, reduce="mean")
        assert (out == mean).all() and (inside == 255).all(), mode


def test_no_sample_counts_although_the_centre_is_in():
    src = np.arange(20, 200, 20, dtype=np.uint8).reshape(1, 9)
    out, inside = view.warp_image(src, np.eye(3), (1, 9), "bilinear")
    assert np.array_equal(out, src) and (inside == 255).all()
    out, inside = view.warp_image(src, np.eye(3), (1, 9), "bilinear", supersample=2)      # 0 <= y <= 0 admits no fractional offset
    assert (out == 0).all() and (inside == 0).all()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_entry_refuses_bad_arguments_by_name():
    src = W.warp_source(3)
    L = npp_amd.lib()
    for ss in (3, 16, 0, -2):
        rc, out, inside = _ss_entry(src, np.eye(3), CANVAS, 1, ss, 0)
        assert rc == -1 and b"npp_warp_image_u8_ss_host" in L.npp_last_error_string() and b"ss=%d" % ss in L.npp_last_error_string()
        assert (out == 0xA5).all() and (inside == 0xA5).all()                                 # nothing was written
    for reduce in (2, -1):
        rc, out, inside = _ss_entry(src, np.eye(3), CANVAS, 1, 2, reduce)
        assert rc == -1 and b"reduce=%d" % reduce in L.npp_last_error_string() and (out == 0xA5).all()
    # the point warp's checks through the new entry
    bad = np.eye(3)
    bad[1, 2] = np.inf
    for args, msg in (((src, np.eye(3), CANVAS, 2, 2, 0), b"mode=2"), ((src, bad, CANVAS, 1, 2, 0), b"m[5]"),
                      ((src, np.eye(3), (0, 4), 1, 2, 0), b"bad shape"), ((np.zeros((4, 4, 5), np.uint8), np.eye(3), (4, 4), 1, 2, 0), b"C=5")):
        rc, out, _ = _ss_entry(*args)
        assert rc == -1 and msg in L.npp_last_error_string() and b"npp_warp_image_u8_ss_host" in L.npp_last_error_string(), msg
    fake = C.c_void_p(64)                                                                     # never dereferenced: validation comes first
    m = (C.c_double * 9)(*np.eye(3).reshape(9))
    for entry, tail in ((L.npp_warp_image_u8_ss_host, ()), (L.npp_warp_image_u8_ss, (None,))):
        assert entry(None, 4, 4, 3, 4, 4, m, 1, 2, 0, fake, None, *tail) == -1 and b"null pointer" in L.npp_last_error_string()
        assert entry(fake, 4, 4, 3, 4, 4, m, 1, 2, 0, fake, None, *tail) == -1                  # the output needs an array of its own
        assert entry(fake, 4, 4, 3, 4, 4, m, 1, 3, 0, C.c_void_p(128), None, *tail) == -1 and b"ss=3" in L.npp_last_error_string()
        assert entry(fake, 4, 4, 3, 4, 4, m, 1, 2, 2, C.c_void_p(128), None, *tail) == -1 and b"reduce=2" in L.npp_last_error_string()


def test_python_refuses_bad_values_by_name_before_a_device_is_touched():
    src = W.warp_source(3)
    for device in (None, "cuda:0"):                       # refused before the device is looked at: no GPU is needed to see it
        for ss in (3, 16, 0, 2.0, True):
            with pytest.raises(ValueError, match="supersample"):
                view.warp_image(src, np.eye(3), CANVAS, supersample=ss, device=device)
        with pytest.raises(ValueError, match="reduce"):
            view.warp_image(src, np.eye(3), CANVAS, supersample=2, reduce="max", device=device)
        with pytest.raises(ValueError, match="mode"):
            view.warp_image(src, np.eye(3), CANVAS, "cubic", supersample=2, device=device)
    with pytest.raises(ValueError, match="reduce"):
        ops.warp_image_u8_host(src, np.eye(3), CANVAS, reduce="max")
    with pytest.raises(npp_amd.NppError, match="C=5"):
        view.warp_image(np.zeros((4, 4, 5), np.uint8), np.eye(3), (4, 4), supersample=2)


# ---- the command -------------------------------------------------------------------------------------------------------------------
FILES = ("gt_img.png", "valid_mask.png", "unknown_mask.png", "masked_img.png")
def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def test_rectify_supersample_one_writes_the_bytes_of_a_run_without_the_flag(tmp_path, capsys):
    from npp_amd import rectify
    _, _, argv = W.rectify_inputs(tmp_path)
    a = rectify.main(argv + ["--outdir", str(tmp_path / "a"), "--device", "cpu"])
    said_a = capsys.readouterr().out
    b = rectify.main(argv + ["--outdir", str(tmp_path / "b"), "--device", "cpu", "--supersample", "1"])
    said_b = capsys.readouterr().out
    for name in FILES + ("view.json",):
        assert open(os.path.join(a, name), "rb").read() == open(os.path.join(b, name), "rb").read(), name
    assert "samples per canvas pixel" not in said_a and "WARNING" in said_a
    assert said_a.splitlines()[0] == said_b.splitlines()[0]                                    # the density line of a point warp
    assert "1 x 1 samples per canvas pixel" in said_b.splitlines()[-1]


def test_rectify_supersample_writes_the_restatements_folder(tmp_path, capsys):
    from npp_amd import rectify
    photo, mask, argv = W.rectify_inputs(tmp_path)
    r2p, _ = view.quad_to_rect(np.asarray(W.RECTIFY_QUAD).reshape(4, 2), (24, 30))
    auto = view.supersample_for(r2p, (24, 30))
    assert auto == 4 and view.sampling_density(r2p, (24, 30))[1] > 4 * view.MINIFY_WARN / 2    # a minifying quad
    out = {}
    for flag in ("4", "auto"):
        out[flag] = rectify.main(argv + ["--outdir", str(tmp_path / flag), "--device", "cpu", "--supersample", flag])
        said = capsys.readouterr().out.splitlines()
        assert "4 x 4 samples per canvas pixel" in said[0] and "4 x 4 samples per canvas pixel" in said[-1]
        assert ("(auto)" in said[-1]) == (flag == "auto")
        v = view.read(os.path.join(out[flag], "view.json"))
        gt, valid = W.warp_image_ss(photo, v["rect_to_photo"], (24, 30), "bilinear", 4, "mean")
        known = W.warp_image_ss(mask, v["rect_to_photo"], (24, 30), "nearest", 4, "min")[0]
        assert 0 < (known == 255).mean() < 1 and (valid == 255).mean() > 0.5
        assert np.array_equal(_png(os.path.join(out[flag], "gt_img.png")), gt)
        assert np.array_equal(_png(os.path.join(out[flag], "valid_mask.png")), valid)
        assert np.array_equal(_png(os.path.join(out[flag], "unknown_mask.png")), known)
        assert np.array_equal(_png(os.path.join(out[flag], "masked_img.png")), gt * ((known >= 128) & (valid == 255))[..., None])
        # min, not mean: a canvas pixel any of whose counted samples reads unknown is unknown
        assert (known <= W.warp_image_ss(mask, v["rect_to_photo"], (24, 30), "nearest", 4, "mean")[0]).all()
        assert set(np.unique(known)) <= {0, 255}
    for name in FILES + ("view.json",):
        assert open(os.path.join(out["4"], name), "rb").read() == open(os.path.join(out["auto"], name), "rb").read(), name
    plain = rectify.main(argv + ["--outdir", str(tmp_path / "plain"), "--device", "cpu"])
    assert open(os.path.join(plain, "view.json")).read() == open(os.path.join(out["4"], "view.json")).read()
    assert not np.array_equal(_png(os.path.join(plain, "gt_img.png")), _png(os.path.join(out["4"], "gt_img.png")))


def test_rectify_refuses_a_bad_supersample(tmp_path, capsys):
    from npp_amd import rectify
    _, _, argv = W.rectify_inputs(tmp_path)
    for bad in ("3", "16", "many"):
        with pytest.raises(SystemExit):
            rectify.main(argv + ["--outdir", str(tmp_path / "x"), "--device", "cpu", "--supersample", bad])
        assert "--supersample" in capsys.readouterr().err
    assert not (tmp_path / "x").exists()


def test_header_declares_the_entry_points():
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "npp_hip.h")).read()
    for name in ("npp_warp_image_u8_ss", "npp_warp_image_u8_ss_host"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in npp_amd._lib.SYMBOLS
        for w in npp_amd.FUSED_WIDTHS:
            assert hasattr(npp_amd.lib(w), name)
