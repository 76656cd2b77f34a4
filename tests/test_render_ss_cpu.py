"""Supersampled renders without a GPU: the host twins of the sampling rule (npp_grid_samples_host, npp_view_samples_host) against
the NumPy restatement bit for bit, the refusals by name, the choice of S from a density, the density report and the render command's
--supersample flag."""
import os
import re

import numpy as np
import pytest

import render_ss_restatement as S
import view_restatement as R
import npp_amd
from npp_amd import ops, view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIT = (24, 40)
TOTAL = R.CANVAS[0] * R.CANVAS[1]
MID = (777, 300)           # a launch that starts and ends mid-row


def _u(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_offsets_are_exact_and_centred():
    for ss in S.SS:
        off = S.offsets(ss).astype(np.float64)
        assert np.array_equal(off, (2 * np.arange(ss) + 1) / (2 * ss) - 0.5) and off.sum() == 0
    assert _u(S.offsets(1))[0] == 0                                   # ss = 1: +0.0, the pixel centre


@pytest.mark.parametrize("ss", S.SS)
def test_grid_samples_host_equals_the_restatement_bit_for_bit(ss):
    for origin, scale in ((S.GRID_ORIGIN, S.GRID_SCALE), ((0.0, 0.0), (1.0, 1.0)), ((-0.0, 5.5), (0.25, 8.0))):
        want = S.grid_samples(R.CANVAS, origin, scale, ss)
        got = ops.grid_samples_host(ops.grid_arg(0, TOTAL, R.CANVAS[1], origin, scale), ss)
        assert got.dtype == np.float32 and got.shape == (TOTAL * ss * ss, 2)
        assert np.array_equal(_u(got), _u(want)), (origin, scale)
        part = ops.grid_samples_host(ops.grid_arg(MID[0], MID[1], R.CANVAS[1], origin, scale), ss)
        assert np.array_equal(_u(part), _u(want[MID[0] * ss * ss:(MID[0] + MID[1]) * ss * ss]))
        assert np.array_equal(_u(part), _u(S.grid_samples(R.CANVAS, origin, scale, ss, *MID)))
    if ss == 1:                                                       # ss = 1 is the point launch's canvas
        from npp_amd.model import canvas_coords
        assert np.array_equal(_u(got), _u(canvas_coords(R.CANVAS, origin=(-0.0, 5.5), scale=(0.25, 8.0))))


def _views():
    return [("pow2%d" % k, R.affine(*p)) for k, p in enumerate(R.POW2_VIEWS)] + [("AFFINE", R.AFFINE), ("PROJECTIVE", R.PROJECTIVE),
                                                                                 ("SS_HORIZON", S.SS_HORIZON)]


@pytest.mark.parametrize("ss", S.SS)
@pytest.mark.parametrize("name,M", _views())
def test_view_samples_host_equals_the_restatement_bit_for_bit(ss, name, M):
    wyx, wc, win = S.view_samples(M, R.CANVAS, FIT, ss)
    yx, c, inside = ops.view_samples_host(ops.view_arg(0, TOTAL, R.CANVAS[1], M), ss, FIT)
    assert yx.dtype == np.float32 and c.dtype == np.uint8 and inside.dtype == np.uint8
    assert np.array_equal(_u(yx), _u(wyx)) and np.array_equal(c, wc.astype(np.uint8)) and np.array_equal(inside, win)
    assert bool(np.isfinite(yx).all()) and not yx[c == 0].any()
    a, b, d = ops.view_samples_host(ops.view_arg(MID[0], MID[1], R.CANVAS[1], M), ss, FIT)
    lo, hi = MID[0] * ss * ss, (MID[0] + MID[1]) * ss * ss
    assert np.array_equal(_u(a), _u(wyx[lo:hi])) and np.array_equal(b, wc[lo:hi]) and np.array_equal(d, win[MID[0]:MID[0] + MID[1]])
    if ss == 1:                                                       # ss = 1 is the point launch
        pyx, pin = ops.view_coords_host(ops.view_arg(0, TOTAL, R.CANVAS[1], M), FIT)
        assert np.array_equal(_u(yx), _u(pyx)) and np.array_equal(inside, pin) and np.array_equal(c != 0, pin != 0)
    if name.startswith("pow2"):                                       # a power-of-two affine view has the grid's sample positions
        sy, sx, y0, x0 = R.POW2_VIEWS[int(name[4:])]
        assert np.array_equal(_u(yx), _u(S.grid_samples(R.CANVAS, (y0, x0), (sy, sx), ss))) and c.all()


def test_ss_horizon_cuts_through_pixels():
    _, centre = R.view_coords(S.SS_HORIZON, R.CANVAS, FIT)
    for ss, full, part, lost in ((2, 475, 15, 15), (4, 467, 23, 21), (8, 464, 26, 24)):
        _, c, inside = S.view_samples(S.SS_HORIZON, R.CANVAS, FIT, ss)
        c = c.reshape(TOTAL, ss * ss)
        assert int(c.all(1).sum()) == full
        assert int((c.any(1) & ~c.all(1) & (centre != 0)).sum()) == part
        assert int((c.any(1) & (centre == 0)).sum()) == lost
        assert not ((centre != 0) & ~c.any(1)).any()
        assert np.array_equal(inside, centre)                        # hence the bytes of the point launch, whatever ss


def test_average_is_the_sequential_fp32_sum():
    rng = np.random.RandomState(3)
    o = rng.uniform(-1, 1, (5, 16, 3)).astype(np.float32)
    mask = rng.rand(5, 16) < 0.6
    mask[0] = False
    mean, count = S.average(o, mask)
    for p in range(1, 5):
        for ch in range(3):
            acc = np.float32(0)
            for s in range(16):
                if mask[p, s]:
                    acc = np.float32(acc + o[p, s, ch])
            assert mean[p, ch] == np.float32(acc / np.float32(count[p]))
    assert count[0] == 0 and not S.pixel_colours(o, mask, np.array([3, 1, 0, 3, 1]))[[0, 2]].any()
    assert np.array_equal(S.average(o)[1], np.full(5, 16))


def test_refusals_by_name():
    g = ops.grid_arg(0, 4, 16)
    for bad in (3, 0, -2, 16, 2.0, True):
        with pytest.raises(ValueError, match="supersample"):
            ops.grid_samples_host(g, bad)
    for ss, word in ((3, "ss=3"), (0, "ss=0")):                       # ... and the library itself
        with pytest.raises(npp_amd.NppError, match=r"failed \(-1\).*" + word + " must be 1, 2, 4 or 8"):
            ops.check(npp_amd.lib().npp_grid_samples_host(ops.C.byref(g), ss, None), "npp_grid_samples_host")
    for arg in (ops.grid_arg((1 << 20) * 16, 1, 16), ops.grid_arg(0, 4, (1 << 20) + 1)):
        with pytest.raises(npp_amd.NppError, match=r"failed \(-1\).*ss=2.*2\^20"):
            ops.grid_samples_host(arg, 2)
        assert ops.grid_samples_host(arg, 1).shape == (arg.n, 2)      # ss = 1 keeps the 2^24 limit
    with pytest.raises(npp_amd.NppError, match=r"failed \(-1\).*2\^20"):
        ops.view_samples_host(ops.view_arg((1 << 20) * 16, 1, 16, np.eye(3)), 2, FIT)
    with pytest.raises(npp_amd.NppError, match=r"failed \(-1\).*too many for one launch"):
        big = ops.grid_arg(0, (1 << 31) * 2, 1 << 20)                 # 2^32 pixels pass alone, 2^38 rows do not (refused before any write)
        ops.check(npp_amd.lib().npp_grid_samples_host(ops.C.byref(big), 8, None), "npp_grid_samples_host")
    assert ops.grid_samples_host(ops.grid_arg(5, 0, 16), 4).shape == (0, 2)           # n == 0 stays a no-op
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match="supersample=2.*tensor of positions"):
        ops.render(torch.zeros((64, 2), dtype=torch.float32), None, None, None, supersample=2)
    with pytest.raises(ValueError, match="supersample 3"):
        ops.render(g, None, None, None, supersample=3)


def test_supersample_for_and_the_auto_rule():
    from npp_amd import render
    w = view.MINIFY_WARN
    for dens, want in ((0.2, 1), (1.0, 1), (w, 1), (w + 1e-9, 2), (2 * w, 2), (2 * w + 1e-9, 4), (4 * w, 4), (4.001 * w, 8), (8 * w, 8),
                       (100.0, 8), (np.inf, 8)):
        assert view.supersample_for_density(dens) == want, dens
    assert view.supersample_for(np.eye(3), (8, 8)) == 1
    assert view.supersample_for(R.affine(0.5, 0.5, 3.0, 4.0), (10, 12)) == 2            # density 2 everywhere
    assert view.supersample_for(R.affine(0.25, 0.125, 0.0, 0.0), (10, 12)) == 4         # sqrt(4 * 8) = 5.66
    assert view.supersample_for(R.HORIZON, R.CANVAS) == 8                               # not in view somewhere: infinite
    hi = view.sampling_density(R.PROJECTIVE, R.CANVAS)[1]
    assert view.supersample_for(R.PROJECTIVE, R.CANVAS) == view.supersample_for_density(hi)
    for scale, want in (((1.0, 1.0), 1), ((2.0, 3.0), 1), ((0.5, 0.5), 2), ((0.5, 1.0), 2), ((1.0, 0.25), 4), ((0.1, 0.1), 8)):
        assert render.auto_supersample(scale) == want, scale


def test_density_report_default_text_is_unchanged():
    for M, size in ((R.PROJECTIVE, R.CANVAS), (np.eye(3), (4, 4)), (R.HORIZON, R.CANVAS)):
        lo, hi = view.sampling_density(M, size)
        line = f"x: {lo:.3f} .. {hi:.3f} target pixels per canvas pixel"
        if hi > view.MINIFY_WARN:
            line += f"  WARNING: minifies by more than {view.MINIFY_WARN} -- point sampling aliases there (no antialiasing)"
        assert view.density_report(M, size, "x") == line == view.density_report(M, size, "x", supersample=1)
    M = R.affine(0.5, 0.5, 0.0, 0.0)                                                    # density 2
    assert "WARNING" in view.density_report(M, (8, 8), "x")
    two = view.density_report(M, (8, 8), "x", supersample=2)
    assert "2 x 2 samples" in two and "WARNING" not in two
    four = view.density_report(R.affine(0.125, 0.125, 0.0, 0.0), (8, 8), "x", supersample=4)       # 8 / 4 = 2 per sample
    assert "4 x 4 samples" in four and "WARNING" in four


def test_render_parse_accepts_and_refuses_the_flag(tmp_path, capsys):
    from npp_amd import render
    base = ["--model", str(tmp_path / "m.npz"), "--out", str(tmp_path / "o.png")]
    args, _ = render.parse(base)
    assert args.supersample == 1 and not args.supersample_given
    for word, want in (("1", 1), ("2", 2), ("4", 4), ("8", 8), ("auto", "auto")):
        args, _ = render.parse(base + ["--supersample", word, "--scale", "0.5"])
        assert args.supersample == want and args.supersample_given
    args, _ = render.parse(base + ["--view", "v.json", "--supersample", "auto"])
    assert args.supersample == "auto" and args.view == "v.json"
    for word in ("3", "0", "16", "2.0", "-2", "Auto"):
        with pytest.raises(SystemExit):
            render.parse(base + ["--supersample=" + word])
        assert re.search(r"--supersample .*must be 1, 2, 4, 8 or auto", capsys.readouterr().err)


def test_header_declares_the_supersampled_entry_points():
    hdr = open(os.path.join(ROOT, "include", "npp_hip.h")).read()
    for name in ("npp_mlp_fwd_grid_ss", "npp_mlp_fwd32_grid_ss", "npp_mlp_fwd_view_ss", "npp_mlp_fwd32_view_ss", "npp_grid_samples_host",
                 "npp_view_samples_host"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in npp_amd._lib.SYMBOLS
        for w in npp_amd.FUSED_WIDTHS:
            assert hasattr(npp_amd.lib(w), name)
