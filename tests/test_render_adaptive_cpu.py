"""Adaptive supersampling without a GPU: the host twin of the class rule (npp_view_ss_classes_host) against the NumPy restatement
byte for byte, the properties of the test view, the refusals of the new entry points by message, the render command's
--supersample adaptive and the density report's line."""
import os
import re

import numpy as np
import pytest

import render_adaptive_restatement as A
import render_ss_restatement as S
import view_restatement as R
import npp_amd
from npp_amd import ops, view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIT = (24, 40)
TOTAL = R.CANVAS[0] * R.CANVAS[1]
WINDOWS = ((0, TOTAL), (777, 300), (53 * 5 + 17, 1), (TOTAL - 17, 17))      # whole canvas; sub-windows that start mid-row
VIEWS = {"ADAPT_VIEW": A.ADAPT_VIEW, "AFFINE": R.AFFINE, "PROJECTIVE": R.PROJECTIVE, "HORIZON": R.HORIZON, "SS_HORIZON": S.SS_HORIZON}


def test_the_test_view_has_the_stated_properties():
    cls, inside, margin = A.classes(A.ADAPT_VIEW, R.CANVAS, FIT)
    assert {k: int((cls == k).sum()) for k in (0, 1, 2, 4, 8)} == A.ADAPT_COUNTS and sum(A.ADAPT_COUNTS.values()) == TOTAL
    assert (327 % 64, 465 % 16, 291 % 4) == (7, 1, 3)                            # every class that can end in a ragged tile does
    m = A.ADAPT_VIEW.reshape(9)
    assert np.array_equal(m.astype(np.float32).astype(np.float64), m)            # dyadic: exact in fp32
    i, j = np.divmod(np.arange(TOTAL), R.CANVAS[1])
    assert int((((m[6] * i + m[7] * j) + m[8]) == 0).sum()) == 7                 # d exactly 0
    rows = cls.reshape(R.CANVAS)
    assert int((rows != rows[:, :1]).any(1).sum()) == 25                         # canvas rows that change class inside the row
    assert int((np.diff(rows.astype(int), axis=1) != 0).sum()) == 26             # ... one of them twice
    assert margin.min() > 0.005                                                   # no pixel within 0.5 % of a threshold
    assert view.supersample_for(A.ADAPT_VIEW, R.CANVAS) == 8
    rows_adaptive = sum(k * k * n for k, n in A.ADAPT_COUNTS.items())
    assert (rows_adaptive, TOTAL * 64) == (38267, 125504)


@pytest.mark.parametrize("name", list(VIEWS))
def test_host_twin_equals_the_restatement_byte_for_byte(name):
    M = VIEWS[name]
    for start, n in WINDOWS:
        want, win, _ = A.classes(M, R.CANVAS, FIT, start, n)
        cls, inside = ops.view_ss_classes_host(ops.view_arg(start, n, R.CANVAS[1], M), FIT)
        assert cls.dtype == np.uint8 and cls.shape == (n,)
        assert np.array_equal(cls, want) and np.array_equal(inside, win), (name, start, n)
        _, point = ops.view_coords_host(ops.view_arg(start, n, R.CANVAS[1], M), FIT)
        assert np.array_equal(inside, point) and np.array_equal(cls == 0, point == 0)      # class 0 <=> inside byte 0
        assert set(np.unique(cls)) <= {0, 1, 2, 4, 8}
    assert np.array_equal(view.supersample_classes(M, R.CANVAS, FIT).reshape(-1), A.classes(M, R.CANVAS, FIT)[0])


def test_the_rule_is_supersample_for_density_at_the_pixel_centre():
    for M in (A.ADAPT_VIEW, R.PROJECTIVE, S.SS_HORIZON):
        cls, _, margin = A.classes(M, R.CANVAS, FIT)
        m = np.asarray(M, np.float64)
        i, j = np.divmod(np.arange(TOTAL), R.CANVAS[1])
        d = (m[2, 0] * i + m[2, 1] * j) + m[2, 2]
        ok = (cls != 0) & (margin > 1e-9)                                          # away from a threshold the two forms agree
        dens = np.sqrt(abs(np.linalg.det(m)) / np.abs(d[ok]) ** 3)
        assert np.array_equal(cls[ok], [view.supersample_for_density(x) for x in dens])


def test_affine_views_have_one_class():
    assert (view.supersample_classes(R.AFFINE, R.CANVAS) == 1).all()              # |det| = 1.013: density 1.007
    assert (view.supersample_classes(A.QUARTER, R.CANVAS) == 4).all()             # scale 1/4: density 4
    assert (view.supersample_classes(R.affine(0.5, 0.5, 0.0, 0.0), R.CANVAS) == 2).all()
    assert (view.supersample_classes(R.affine(0.125, 0.0625, 1.0, 2.0), R.CANVAS) == 8).all()
    assert (view.supersample_classes(A.BEHIND, R.CANVAS) == 0).all()


def test_refusals_of_the_class_entry_points_by_message():
    L = npp_amd.lib()
    cls = np.full(8, 77, np.uint8)
    cp = ops.C.c_void_p(cls.ctypes.data)
    v = ops.view_arg(0, 4, 16, np.eye(3))
    for fn, who, extra in ((L.npp_view_ss_classes_host, "npp_view_ss_classes_host", ()), (L.npp_view_ss_classes, "npp_view_ss_classes", (None,))):
        for bad, word in ((ops.view_arg(0, 4, 0, np.eye(3)), "canvas width 0"), (ops.view_arg(-1, 4, 16, np.eye(3)), "start=-1"),
                          (ops.view_arg(0, -4, 16, np.eye(3)), "n=-4"), (ops.view_arg((1 << 24) * 16, 1, 16, np.eye(3)), r"2\^24")):
            with pytest.raises(npp_amd.NppError, match=r"failed \(-1\).*" + who + ": .*" + word):
                ops.check(fn(ops.C.byref(bad), FIT[0], FIT[1], cp, None, *extra), who)
        nan = ops.view_arg(0, 4, 16, np.eye(3))
        nan.m[4] = float("nan")
        with pytest.raises(npp_amd.NppError, match=r"failed \(-1\).*" + who + r": matrix entry m\[4\]"):
            ops.check(fn(ops.C.byref(nan), FIT[0], FIT[1], cp, None, *extra), who)
        with pytest.raises(npp_amd.NppError, match=r"failed \(-1\).*" + who + ": null view"):
            ops.check(fn(None, FIT[0], FIT[1], cp, None, *extra), who)
        with pytest.raises(npp_amd.NppError, match=r"failed \(-1\).*" + who + ": image size 0 x 40"):
            ops.check(fn(ops.C.byref(v), 0, FIT[1], cp, None, *extra), who)
        with pytest.raises(npp_amd.NppError, match=r"failed \(-1\).*" + who + ": null pointer"):
            ops.check(fn(ops.C.byref(v), FIT[0], FIT[1], None, None, *extra), who)
        ops.check(fn(ops.C.byref(ops.view_arg(5, 0, 16, np.eye(3))), FIT[0], FIT[1], None, None, *extra), who)      # n == 0: a no-op
    assert (cls == 77).all()                                                       # nothing was written
    assert ops.view_ss_classes_host(ops.view_arg(5, 0, 16, np.eye(3)), FIT)[0].shape == (0,)


def test_refusals_of_the_listed_entry_points_by_message():
    """Every refusal comes before any pointer is read or anything is launched: the pointers here are null or host memory."""
    cfg = npp_amd._lib.EmbedCfg.make(np.zeros((1, 2)), np.full((1, 2), 8.0), np.ones(10), FIT)
    pix = np.arange(4, dtype=np.int64)
    pp = ops.C.c_void_p(pix.ctypes.data)
    ok = ops.view_arg(0, 4, 16, np.eye(3))
    for w in npp_amd.FUSED_WIDTHS:
        L = npp_amd.lib(w)
        for fn, who in ((L.npp_mlp_fwd_view_list, "npp_mlp_fwd_view_list"), (L.npp_mlp_fwd32_view_list, "npp_mlp_fwd32_view_list")):
            def call(v=ok, ss=2, p=pp, n=4, c=cfg, width=w, ptr=pp, act=1):
                return ops.check(fn(ops.C.byref(v) if v is not None else None, ss, p, n, ops.C.byref(c) if c is not None else None,
                                    width, ptr, ptr, ptr, None, act, None), who, w)
            for kw, word in ((dict(v=None), "null view"), (dict(v=ops.view_arg(0, 4, 0, np.eye(3))), "canvas width 0"),
                             (dict(v=ops.view_arg(-1, 4, 16, np.eye(3))), "start=-1"),
                             (dict(v=ops.view_arg((1 << 20) * 16, 1, 16, np.eye(3))), r"ss=2: row indices would reach 2\^20"),
                             (dict(ss=3), "ss=3 must be 1, 2, 4 or 8"), (dict(ss=0), "ss=0 must be 1, 2, 4 or 8"),
                             (dict(p=None), "null pixel list with n_list=4"), (dict(n=-1), "n_list=-1 must be >= 0"),
                             (dict(n=(1 << 31) * 2, ss=8), r"n_list=4294967296 x ss\^2=64 rows are too many for one launch"),
                             (dict(c=None), "null cfg"), (dict(ptr=None), "null pointer"), (dict(act=3), "out_act=3")):
                with pytest.raises(npp_amd.NppError, match=r"failed \(-1\).*" + who + ": .*" + word):
                    call(**kw)
            with pytest.raises(npp_amd.NppError, match=r"failed \(-3\).*" + who + ": width"):
                call(width=w + 1)
            call(n=0)                                                              # n_list == 0: a no-op
            call(n=0, p=None)
            call(v=ops.view_arg(5, 0, 16, np.eye(3)), ptr=None)                    # an empty window: nothing can be listed in it
    torch = pytest.importorskip("torch")
    for src in (ops.grid_arg(0, 4, 16), torch.zeros((64, 2), dtype=torch.float32)):
        with pytest.raises(ValueError, match="pixels: only a view_arg"):
            ops.render(src, None, None, None, pixels=torch.zeros(4, dtype=torch.int64))


def test_render_parse_takes_adaptive(tmp_path, capsys):
    from npp_amd import render
    base = ["--model", str(tmp_path / "m.npz"), "--out", str(tmp_path / "o.png")]
    args, _ = render.parse(base + ["--view", "v.json", "--supersample", "adaptive"])
    assert args.supersample == "adaptive" and args.supersample_given and args.view == "v.json"
    args, _ = render.parse(base + ["--scale", "0.25", "--supersample", "adaptive"])
    assert args.supersample == "adaptive" and render.auto_supersample(args.scale) == 4
    assert "adaptive" in render._ss_note(args, 4) and "4 x 4 samples per pixel" in render._ss_note(args, 4)
    for word in ("Adaptive", "adapt", "per-pixel"):
        with pytest.raises(SystemExit):
            render.parse(base + ["--supersample=" + word])
        assert re.search(r"--supersample .*must be 1, 2, 4, 8 or auto, or adaptive", capsys.readouterr().err)


def test_density_report_names_the_class_shares_and_the_row_ratio():
    line = view.density_report(A.ADAPT_VIEW, R.CANVAS, "x", supersample="adaptive")
    lo, hi = view.sampling_density(A.ADAPT_VIEW, R.CANVAS)
    assert line.startswith(f"x: {lo:.3f} .. {hi:.3f} target pixels per canvas pixel; adaptive samples per pixel: ")
    n_in = TOTAL - A.ADAPT_COUNTS[0]
    for k in (1, 2, 4, 8):
        assert f"{k} x {k} on {100 * A.ADAPT_COUNTS[k] / n_in:.1f} %" in line
    assert "38267 chain rows, 0.305 of uniform 8 x 8" in line                      # 38267 / (37 * 53 * 64)
    shares, rows, ratio, top = view.class_rows(A.classes(A.ADAPT_VIEW, R.CANVAS, FIT)[0], auto=8)
    assert rows == 38267 and top == 8 and ratio == 38267 / 125504 and abs(sum(shares.values()) - 1) < 1e-12
    one = view.density_report(R.AFFINE, R.CANVAS, "x", supersample="adaptive")
    assert "1 x 1 on 100.0 %" in one and "1.000 of uniform 1 x 1" in one
    assert "0 chain rows" in view.adaptive_note(view.supersample_classes(A.BEHIND, R.CANVAS))


def test_header_declares_the_adaptive_entry_points():
    hdr = open(os.path.join(ROOT, "include", "npp_hip.h")).read()
    for name in ("npp_view_ss_classes", "npp_view_ss_classes_host", "npp_mlp_fwd_view_list", "npp_mlp_fwd32_view_list"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in npp_amd._lib.SYMBOLS
        for w in npp_amd.FUSED_WIDTHS:
            assert hasattr(npp_amd.lib(w), name)
