"""Perspective views without a GPU: the float64 host geometry of view.py, the host twins of the view rule (npp_view_coords_host,
npp_warp_image_u8_host) against the NumPy restatement bit for bit, and the two commands' argument checks and CPU path."""
import os
import re

import numpy as np
import pytest

import view_restatement as R
import npp_amd
from npp_amd import ops, view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIT = (24, 40)             # the fit's image size of the inside byte: smaller than what the views reach, so 0, 1 and 3 all occur


# ---- host geometry -----------------------------------------------------------------------------------------------------------------
def test_homography_reproduces_its_points_and_inverts():
    src = np.array([[0, 0], [0, 63], [47, 63], [47, 0]], np.float64)
    dst = np.array([[5.5, 3.25], [9.0, 57.5], [40.25, 60.0], [44.0, 7.75]])
    M = view.homography_from_points(src, dst)
    assert M.shape == (3, 3) and M.dtype == np.float64 and M[2, 2] == 1.0
    assert np.abs(view.apply(M, src) - dst).max() < 1e-9
    Mi = view.invert(M)
    assert np.abs(view.apply(Mi, dst) - src).max() < 1e-9
    back = view.invert(Mi)
    assert np.abs(back / back[2, 2] - M).max() < 1e-9
    # more than four correspondences of an exact map: least squares finds it again
    rng = np.random.RandomState(0)
    more = rng.uniform(0, 60, (9, 2))
    M9 = view.homography_from_points(more, view.apply(M, more))
    assert np.abs(M9 - M).max() < 1e-9
    r2p, p2r = view.quad_to_rect(dst, (48, 64))
    assert np.abs(r2p - M).max() < 1e-9 and np.abs(view.apply(p2r, dst) - src).max() < 1e-9


def test_degenerate_points_and_singular_matrices_raise_by_name():
    src = np.array([[0, 0], [0, 10], [10, 10], [10, 0]], np.float64)
    with pytest.raises(ValueError, match="collinear"):
        view.homography_from_points(src, np.array([[0, 0], [5, 5], [10, 10], [10, 0]], np.float64))      # three on one line
    with pytest.raises(ValueError, match="collinear"):
        view.homography_from_points(np.array([[0, 0], [1, 1], [2, 2], [3, 3]], np.float64), src)
    with pytest.raises(ValueError, match="N >= 4"):
        view.homography_from_points(src[:3], src[:3])
    with pytest.raises(ValueError, match="singular"):
        view.invert(np.array([[1.0, 2, 3], [2, 4, 6], [0, 0, 1]]))
    with pytest.raises(ValueError, match="non-finite"):
        view.check_matrix(np.array([[1.0, 0, 0], [0, np.nan, 0], [0, 0, 1]]))
    with pytest.raises(ValueError, match="non-finite"):
        view.check_matrix(np.array([[1.0, 0, 0], [0, 1e300, 0], [0, 0, 1]]))                            # infinite once stored as fp32


def test_sampling_density_and_view_file(tmp_path):
    lo, hi = view.sampling_density(R.affine(0.5, 0.5, 3.0, 4.0), (10, 12))
    assert lo == hi == 2.0                                         # scale 1/2: every second target pixel
    lo, hi = view.sampling_density(R.PROJECTIVE, R.CANVAS)
    J = []
    for i, j in ((0, 0), (36, 52), (18, 26)):                      # finite differences of the map at two corners and the centre
        e = 1e-6
        p = view.apply(R.PROJECTIVE, [[i, j], [i + e, j], [i, j + e]])
        J.append(np.sqrt(abs(np.linalg.det((p[1:] - p[0]) / e))))
    assert lo - 1e-4 <= min(J) and max(J) <= hi + 1e-4 and abs(hi - max(J)) < 1e-4 and abs(lo - min(J)) < 1e-4
    assert "WARNING" in view.density_report(R.PROJECTIVE, R.CANVAS, "x") and "WARNING" not in view.density_report(np.eye(3), (4, 4), "x")
    assert view.sampling_density(R.HORIZON, R.CANVAS)[1] == np.inf
    quad = np.array([[5.5, 3.25], [9.0, 57.5], [40.25, 60.0], [44.0, 7.75]])
    r2p, p2r = view.quad_to_rect(quad, (20, 30))
    path = view.write(str(tmp_path / "view.json"), (48, 64), (20, 30), quad, r2p, p2r)
    v = view.read(path)
    assert v["photo_size"] == (48, 64) and v["rect_size"] == (20, 30) and np.array_equal(v["quad_yx"], quad)
    assert np.array_equal(v["rect_to_photo"], r2p) and np.array_equal(v["photo_to_rect"], p2r)       # repr round trip of doubles
    (tmp_path / "bad.json").write_text('{"photo_size": [4, 4]}')
    with pytest.raises(ValueError, match="not a view.json"):
        view.read(str(tmp_path / "bad.json"))


# ---- the render rule's host twin ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["AFFINE", "PROJECTIVE", "HORIZON"])
def test_view_coords_host_equals_the_restatement_bit_for_bit(name):
    M = getattr(R, name)
    yx, inside = view.canvas_coords(M, R.CANVAS, res=FIT, return_inside=True)
    ryx, rin = R.view_coords(M, R.CANVAS, FIT)
    assert yx.dtype == np.float32 and inside.dtype == np.uint8
    assert np.array_equal(yx.view(np.uint32), ryx.view(np.uint32)) and np.array_equal(inside, rin)
    assert bool(np.isfinite(yx).all())
    if name == "HORIZON":
        m = M.reshape(9).astype(np.float32)
        i, j = np.divmod(np.arange(R.CANVAS[0] * R.CANVAS[1]), R.CANVAS[1])
        d = (m[6] * i.astype(np.float32) + m[7] * j.astype(np.float32)) + m[8]
        assert (d == 0).any() and (d < 0).any() and (d > 0).any()
        assert not inside[d <= 0].any() and not yx[d <= 0].any() and inside[d > 0].all()
    else:
        assert set(np.unique(inside)) == {1, 3}
    # a chunk that starts mid-row is the same slice
    a, b = view.canvas_coords(M, R.CANVAS, res=FIT, start=777, n=300, return_inside=True)
    assert np.array_equal(a.view(np.uint32), ryx[777:1077].view(np.uint32)) and np.array_equal(b, rin[777:1077])


@pytest.mark.parametrize("sy,sx,y0,x0", R.POW2_VIEWS)
def test_power_of_two_affine_views_give_the_grid_positions(sy, sx, y0, x0):
    from npp_amd.model import canvas_coords
    g = canvas_coords(R.CANVAS, origin=(y0, x0), scale=(sy, sx))
    v = view.canvas_coords(R.affine(sy, sx, y0, x0), R.CANVAS)
    assert np.array_equal(g.view(np.uint32), v.view(np.uint32))


def test_view_coords_host_refuses_bad_arguments():
    def call(start, n, width, M=np.eye(3)):
        return ops.view_coords_host(ops.view_arg(start, n, width, M), FIT)
    bad = np.eye(3)
    bad[1, 0] = np.nan
    for args, msg in (((0, 4, 16, bad), r"m\[3\].*not finite"), ((0, 4, 0), "canvas width 0"), ((-1, 4, 16), ">= 0"),
                      (((1 << 24) * 16, 1, 16), r"2\^24"), ((0, 4, (1 << 24) + 1), r"2\^24")):
        with pytest.raises(npp_amd.NppError, match=r"failed \(-1\).*" + msg):
            call(*args)
    assert call(5, 0, 16)[0].shape == (0, 2)


# ---- the warp's host twin ----------------------------------------------------------------------------------------------------------
SRC, CANVAS, WARP_MAPS, _src = R.WARP_SRC, R.WARP_CANVAS, R.WARP_MAPS, R.warp_source


@pytest.mark.parametrize("mode", ["nearest", "bilinear"])
@pytest.mark.parametrize("C", [1, 3, 4])
def test_warp_host_equals_the_restatement_bit_for_bit(mode, C):
    src = _src(C)
    for name, M in WARP_MAPS.items():
        out, inside = view.warp_image(src, M, CANVAS, mode)
        rout, rin = R.warp_image(src, M, CANVAS, mode)
        assert out.shape == CANVAS + src.shape[2:] and out.dtype == np.uint8 and inside.shape == CANVAS
        assert np.array_equal(out, rout), name
        assert np.array_equal(inside, rin), name
        assert not out[inside == 0].any() and set(np.unique(inside)) <= {0, 255}
    assert 0 < (R.warp_image(src, WARP_MAPS["projective"], CANVAS, mode)[1] == 255).mean() < 1
    assert (R.warp_image(src, WARP_MAPS["horizon"], CANVAS, mode)[1][16:] == 0).all()


@pytest.mark.parametrize("mode", ["nearest", "bilinear"])
def test_warp_identity_and_integer_translation_are_exact(mode):
    src = _src(3, seed=1)
    out, inside = view.warp_image(src, np.eye(3), SRC, mode)
    assert np.array_equal(out, src) and (inside == 255).all()
    out, inside = view.warp_image(src, WARP_MAPS["shift"], CANVAS, mode)           # canvas (i, j) reads source (i - 4, j + 6)
    want, win = np.zeros(CANVAS + (3,), np.uint8), np.zeros(CANVAS, np.uint8)
    want[4:4 + 23, 0:25] = src[:, 6:31]
    win[4:4 + 23, 0:25] = 255
    assert np.array_equal(out, want) and np.array_equal(inside, win)


def test_warp_host_refuses_bad_arguments():
    src = _src(3)
    with pytest.raises(ValueError, match="mode"):
        view.warp_image(src, np.eye(3), CANVAS, "cubic")
    with pytest.raises(ValueError, match="non-finite"):
        view.warp_image(src, np.full((3, 3), np.inf), CANVAS)
    with pytest.raises(npp_amd.NppError, match="C=5"):
        view.warp_image(np.zeros((4, 4, 5), np.uint8), np.eye(3), (4, 4))


# ---- the commands ------------------------------------------------------------------------------------------------------------------
def _photo(tmp_path, seed=3):
    from PIL import Image
    photo = np.random.RandomState(seed).randint(0, 256, (48, 64, 3)).astype(np.uint8)
    Image.fromarray(photo).save(tmp_path / "photo.png")
    return photo, str(tmp_path / "photo.png")


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def test_rectify_on_the_cpu_writes_the_input_folder(tmp_path):
    from PIL import Image
    from npp_amd import rectify
    photo, path = _photo(tmp_path)
    mask = np.full((48, 64), 255, np.uint8)
    mask[10:30, 20:40] = 0
    Image.fromarray(mask).save(tmp_path / "mask.png")
    quad = [-6.0, 3.25, 9.0, 57.5, 40.25, 70.0, 44.0, 7.75]             # two corners outside the photograph: valid_mask has a hole
    out = rectify.main(["--photo", path, "--quad", *map(str, quad), "--size", "33", "41", "--mask", str(tmp_path / "mask.png"),
                        "--outdir", str(tmp_path / "in"), "--device", "cpu"])
    assert sorted(os.listdir(out)) == ["gt_img.png", "masked_img.png", "unknown_mask.png", "valid_mask.png", "view.json"]
    v = view.read(os.path.join(out, "view.json"))
    assert v["photo_size"] == (48, 64) and v["rect_size"] == (33, 41)
    assert np.array_equal(v["quad_yx"].reshape(-1), quad)
    gt, valid = R.warp_image(photo, v["rect_to_photo"], (33, 41), "bilinear")
    known = R.warp_image(mask, v["rect_to_photo"], (33, 41), "nearest")[0]
    assert 0 < (valid == 255).mean() < 1 and 0 < (known == 255).mean() < 1
    assert np.array_equal(_png(os.path.join(out, "valid_mask.png")), valid)
    assert np.array_equal(_png(os.path.join(out, "gt_img.png")), gt)
    assert np.array_equal(_png(os.path.join(out, "unknown_mask.png")), known)
    assert np.array_equal(_png(os.path.join(out, "masked_img.png")), gt * ((known == 255) & (valid == 255))[..., None])
    # the folder is what the loaders read: white = known
    from npp_amd import io as nio
    assert nio._imread_gray(os.path.join(out, "unknown_mask.png")).max() == 1.0


def test_rectify_of_an_axis_aligned_quad_is_the_crop(tmp_path):
    from npp_amd import rectify
    photo, path = _photo(tmp_path)
    out = rectify.main(["--photo", path, "--quad", "7", "11", "7", "50", "39", "50", "39", "11", "--size", "33", "40",
                        "--outdir", str(tmp_path / "crop"), "--device", "cpu"])
    assert np.array_equal(_png(os.path.join(out, "gt_img.png")), photo[7:40, 11:51])
    assert (_png(os.path.join(out, "valid_mask.png")) == 255).all() and (_png(os.path.join(out, "unknown_mask.png")) == 255).all()
    assert np.array_equal(_png(os.path.join(out, "masked_img.png")), photo[7:40, 11:51])


def test_rectify_checks_its_arguments(tmp_path, capsys):
    from npp_amd import rectify
    _, path = _photo(tmp_path)
    good = ["--photo", path, "--quad", "7", "11", "7", "50", "39", "50", "39", "11", "--size", "33", "40", "--device", "cpu"]
    full = tmp_path / "full"
    full.mkdir()
    (full / "x.txt").write_text("x")
    for argv, name in ((good + ["--outdir", str(full)], "--outdir"),
                       (good[:2] + ["--quad", "0", "0", "10", "10", "20", "20", "30", "0"] + good[11:] + ["--outdir", str(tmp_path / "a")], "--quad"),
                       (good[:11] + ["--size", "33", "0", "--device", "cpu", "--outdir", str(tmp_path / "b")], "--size"),
                       (["--photo", str(tmp_path / "none.png")] + good[2:] + ["--outdir", str(tmp_path / "c")], "--photo")):
        with pytest.raises(SystemExit):
            rectify.main(argv)
        err = capsys.readouterr().err
        assert re.search(r"error: .*" + name, err), (name, err)
    assert not any((tmp_path / d).exists() for d in "abc")


def test_render_refuses_view_with_a_grid_switch(tmp_path, capsys):
    from npp_amd import render
    base = ["--model", str(tmp_path / "m.npz"), "--out", str(tmp_path / "o.png"), "--view", str(tmp_path / "view.json")]
    for extra, name in ((["--scale", "2"], "--scale"), (["--origin", "0", "0"], "--origin"), (["--size", "8", "8"], "--size")):
        with pytest.raises(SystemExit):
            render.parse(base + extra)
        assert re.search(name + r" cannot be combined with --view", capsys.readouterr().err)
    with pytest.raises(SystemExit):
        render.parse(base[:4] + ["--into", "p.png"])
    assert "need --view" in capsys.readouterr().err
    args, _ = render.parse(base + ["--into", "p.png", "--beyond"])
    assert args.view and args.into == "p.png" and args.beyond and args.mask is None
    args, _ = render.parse(base[:4])                                 # without --view: the defaults of before
    assert args.scale == (1.0, 1.0) and args.origin == [0.0, 0.0] and args.size is None and args.view is None


def test_composite_replaces_exactly_the_selected_pixels():
    torch = pytest.importorskip("torch")
    rng = np.random.RandomState(5)
    photo = rng.randint(0, 256, (6, 7, 3)).astype(np.uint8)
    render = torch.from_numpy(rng.uniform(-0.2, 1.2, (6, 7, 3)).astype(np.float32))
    inside = rng.choice([0, 1, 3], (6, 7)).astype(np.uint8)
    mask = rng.choice([0, 255], (6, 7)).astype(np.uint8)
    r8 = np.uint8(np.rint(np.clip(render.numpy().astype(np.float64), 0, 1) * 255.0))              # io.imsave's conversion
    for beyond in (False, True):
        for m in (None, mask):
            sel = (inside != 0) if beyond else (inside == 3)
            sel = sel & (m == 0) if m is not None else sel
            got = view.composite(photo, render, inside, mask=m, beyond=beyond).numpy()
            assert got.dtype == np.uint8 and np.array_equal(got, np.where(sel[..., None], r8, photo))


def test_header_declares_the_view_entry_points():
    hdr = open(os.path.join(ROOT, "include", "npp_hip.h")).read()
    for name in ("npp_mlp_fwd_view", "npp_mlp_fwd32_view", "npp_view_coords_host", "npp_warp_image_u8", "npp_warp_image_u8_host"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in npp_amd._lib.SYMBOLS
        for w in npp_amd.FUSED_WIDTHS:
            assert hasattr(npp_amd.lib(w), name)
    assert re.search(r"int64_t start, n;[^}]*int32_t width;[^}]*float m\[9\];[^}]*\} npp_view;", hdr)
