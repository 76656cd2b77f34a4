"""CPU checks of the quality report (npp_amd.metrics, npp_amd.evaluate): the restatement's two forms against each other and against
closed forms, the region bookkeeping of metrics.report with the two kernels stubbed by the restatement, the command line's argument
parsing and JSON keys, and the launchers' argument checks (host code: nothing is launched).  No GPU calls."""
import ctypes as C
import json
import math

import numpy as np
import pytest

import metrics_restatement as R


def test_metrics_module_imports():
    """The one test that cannot pass without the feature: the module, its entry points and its C ABI exist."""
    import npp_amd
    from npp_amd import metrics, evaluate                                # noqa: F401
    for name in ("ssim_map", "ssim", "psnr", "mae", "report"):
        assert callable(getattr(metrics, name))
    L = npp_amd.lib()
    for name in ("npp_ssim_map", "npp_region_sums_blocks", "npp_region_sums"):
        assert hasattr(L, name)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def test_window_is_normalised_and_symmetric():
    g = R.window()
    assert g.shape == (11,) and abs(g.sum() - 1.0) < 1e-15 and np.array_equal(g, g[::-1]) and g.argmax() == 5
    assert abs(g[4] / g[5] - math.exp(-1.0 / 4.5)) < 1e-15


# How far two float64 forms that add the 11 taps in different orders may lie apart.  A moment is two passes of 11 taps: relative
# error <= 22 u, u = 2^-53, i.e. <= 2.5e-15 for values <= 1.  sigma_xy = E[xy] - mu_x mu_y then carries <= 3 x that, 7.4e-15, in each
# form, and the factors (2 sigma_xy + C2) and (sigma_x^2 + sigma_y^2 + C2) it sits in are no smaller than sigma^2-sum + C2, so the
# index differs by at most ~4 x 7.4e-15 / (sigma_x^2 + sigma_y^2 + C2) between the forms.  Noise (window variances >= 0.02 per image)
# stays below 1e-12 in the worst case and in practice -- roundings do not all point one way -- a decade or two lower: the forms are
# held to 1e-13 there.  Flat and ramp images have variances near 0, so 1 / C2 = 1.1e3 amplifies: 4 x 7.4e-15 / 9e-4 = 3.3e-11 is all
# float64 guarantees, and all that is asserted (measured: 9.2e-14 on flat, up to 3.4e-13 on the ramps).
FORMS_BOUND = {"noise": 1e-13, "saturated": 1e-13, "flat": 3.3e-11, "ramp": 3.3e-11}


@pytest.mark.parametrize("kind", R.CONTENTS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_two_forms_agree(shape, kind):
    a, b = R.content(kind, shape)
    s1, s2 = R.ssim_map_slices(a, b), R.ssim_map_scipy(a, b)
    assert s1.shape == s2.shape == (shape[0] - 10, shape[1] - 10) and s1.dtype == np.float64
    dist = float(np.abs(s1 - s2).max())
    print(f"{kind} {shape}: |slices - scipy| = {dist:.3e}, bound {FORMS_BOUND[kind]:.1e}")
    assert dist <= FORMS_BOUND[kind]
    assert (s1 <= 1.0 + 1e-12).all() and (s1 >= -1.0 - 1e-12).all()


@pytest.mark.parametrize("form", [R.ssim_map_slices, R.ssim_map_scipy], ids=["slices", "scipy"])
def test_closed_forms(form):
    a, b = R.content("noise", (23, 31))
    assert (form(a, a) == 1.0).all()                                      # identical images: exactly 1
    assert np.array_equal(form(a, b), form(b, a))                         # symmetric in its arguments
    c1, c2 = np.float32([0.2, 0.5, 0.9]), np.float32([0.3, 0.5, 0.1])     # two constant images, per channel: zero variances, the C2
    fa, fb = np.broadcast_to(c1, (23, 31, 3)), np.broadcast_to(c2, (23, 31, 3))   # factors cancel
    x, y = c1.astype(np.float64), c2.astype(np.float64)
    want = float(((2 * x * y + R.C1) / (x * x + y * y + R.C1)).mean())
    assert np.abs(form(fa, fb) - want).max() <= 1e-12


def test_small_images_are_refused_by_the_restatement():
    with pytest.raises(ValueError, match="at least 11"):
        R.ssim_map_slices(np.zeros((10, 40, 3)), np.zeros((10, 40, 3)))


# ---- metrics.report's bookkeeping, the two kernels stubbed by the restatement ------------------------------------------------------------
@pytest.fixture
def stubbed(monkeypatch):
    import torch
    from npp_amd import metrics, ops

    def ssim_map(a, b):
        return torch.from_numpy(R.ssim_map_slices(a.numpy(), b.numpy()))

    def region_sums(a, b, w, smap=None):
        a64, b64, w64 = a.numpy().astype(np.float64), b.numpy().astype(np.float64), w.numpy().astype(np.float64)
        d = a64 - b64
        wi = w64[5:-5, 5:-5]
        row = [w64.sum(), (w64 * (d * d).sum(-1)).sum(), (w64 * np.abs(d).sum(-1)).sum(),
               0.0 if smap is None else wi.sum(), 0.0 if smap is None else (wi * smap.numpy()).sum()]
        return torch.tensor([row, [0.0] * 5], dtype=torch.float64)       # (two "blocks": the host adds them)
    monkeypatch.setattr(ops, "ssim_map", ssim_map)
    monkeypatch.setattr(ops, "region_sums", region_sums)
    return metrics


def test_report_regions_add_up_under_a_valid_mask(stubbed):
    a, b = R.content("noise", (47, 33))
    m = R.mask("hole", (47, 33))
    v = np.ones((47, 33), np.float32)
    v[:, :7] = 0
    rep = stubbed.report(a, b, m, v, device="cpu")
    assert set(rep) == {"all", "known", "unknown"}
    for r in rep.values():
        assert set(r) == {"pixels", "psnr", "ssim", "mae"}
    assert rep["all"]["pixels"] == int(v.sum()) and isinstance(rep["all"]["pixels"], int)
    assert rep["known"]["pixels"] == int((m * v).sum()) and rep["unknown"]["pixels"] == int(((1 - m) * v).sum())
    assert rep["known"]["pixels"] + rep["unknown"]["pixels"] == rep["all"]["pixels"] < 47 * 33
    want = R.report(a, b, m, v)
    for name in rep:
        for k in ("psnr", "ssim", "mae"):
            assert abs(rep[name][k] - want[name][k]) <= 1e-12, (name, k)
    json.dumps(rep)                                                        # plain Python numbers
    # masks as the loaders give them ((H,W,1)) and as files hold them (uint8, 255 = member); uint8 images
    rep2 = stubbed.report(a, b, m[..., None], np.uint8(v * 255), device="cpu")
    assert rep2 == rep
    a8, b8 = np.uint8(a * 255), np.uint8(b * 255)
    rep8 = stubbed.report(a8, b8, m, v, device="cpu")
    assert rep8 == stubbed.report((a8 / 255.0).astype(np.float32), (b8 / 255.0).astype(np.float32), m, v, device="cpu")


def test_report_empty_and_border_only_regions(stubbed):
    a, b = R.content("noise", (30, 24))
    rep = stubbed.report(a, b, np.ones((30, 24), np.float32), device="cpu")            # nothing unknown
    assert rep["unknown"] == {"pixels": 0, "psnr": None, "ssim": None, "mae": None}
    assert rep["known"] == rep["all"] and rep["all"]["pixels"] == 30 * 24 and rep["all"]["ssim"] is not None
    m = np.ones((30, 24), np.float32)
    m[:5, :] = 0                                                                       # unknown = the top five rows: no SSIM value there
    m[:, 19:] = 0                                                                      # ... and the last five columns
    rep = stubbed.report(a, b, m, device="cpu")
    u = rep["unknown"]
    assert u["pixels"] == 5 * 24 + 25 * 5 and u["ssim"] is None and math.isfinite(u["psnr"]) and math.isfinite(u["mae"])
    assert rep["known"]["ssim"] is not None
    m[5, 5] = 0                                                                        # one unknown pixel with a value: its own
    rep = stubbed.report(a, b, m, device="cpu")
    assert abs(rep["unknown"]["ssim"] - R.ssim_map_slices(a, b)[0, 0]) <= 1e-15


def test_single_figures_and_the_psnr_floor(stubbed):
    a, b = R.content("ramp", (20, 26))
    w = R.mask("border_hole", (20, 26))
    want = R.region_figures(a, b, w)
    assert abs(stubbed.psnr(a, b, w, device="cpu") - want["psnr"]) <= 1e-12
    assert abs(stubbed.mae(a, b, w, device="cpu") - want["mae"]) <= 1e-15
    assert abs(stubbed.ssim(a, b, w, device="cpu") - want["ssim"]) <= 1e-12
    assert abs(stubbed.ssim(a, b, device="cpu") - float(R.ssim_map_slices(a, b).mean())) <= 1e-12
    assert stubbed.psnr(a, a, device="cpu") == 200.0 and stubbed.mae(a, a, device="cpu") == 0.0 and stubbed.ssim(a, a, device="cpu") == 1.0
    assert stubbed.psnr(a, b, np.zeros((20, 26), np.float32), device="cpu") is None
    with pytest.raises(ValueError, match="differ in size"):
        stubbed.psnr(a, b[:, :20], device="cpu")
    with pytest.raises(ValueError, match="region"):
        stubbed.psnr(a, b, np.ones((20, 25), np.float32), device="cpu")


def test_quantised_equals_the_dumped_file(tmp_path):
    """metrics.quantised (what --eval_metrics judges) is bit for bit the image io.dump_testset writes and io._imread_rgb reads back."""
    import torch
    from npp_amd import io as nio, metrics
    rs = np.random.RandomState(3)
    pred = (rs.rand(19, 23, 3) * 1.2 - 0.1).astype(np.float32)                         # beyond [0, 1]: clipped
    m, v = R.mask("hole", (19, 23))[..., None], np.ones((19, 23, 1), np.float32)
    v[:3] = 0
    nio.dump_testset(str(tmp_path), pred, pred, pred, m, v)
    back = nio._imread_rgb(str(tmp_path / "pred_rgb_img.png")).astype(np.float32)
    got = metrics.quantised(torch.from_numpy(pred), m, v).numpy()
    assert got.dtype == np.float32 and np.array_equal(got, back)


# ---- the launchers' argument checks (host code) ----------------------------------------------------------------------------------------
def test_launchers_validate_on_the_host():
    import npp_amd
    L = npp_amd.lib()
    fake = C.c_void_p(64)                                                  # never dereferenced: validation comes first
    for H, W in [(10, 40), (40, 10)]:
        assert L.npp_ssim_map(fake, fake, H, W, fake, None) < 0
        assert b"at least 11" in L.npp_last_error_string()
    assert L.npp_ssim_map(None, fake, 40, 40, fake, None) < 0
    assert L.npp_region_sums_blocks(1, 1) == 1 and L.npp_region_sums_blocks(16, 17) == 2 and L.npp_region_sums_blocks(1024, 1024) == 256
    assert L.npp_region_sums_blocks(0, 5) < 0
    assert L.npp_region_sums(fake, fake, None, None, 40, 40, fake, None) < 0          # no weights
    assert L.npp_region_sums(fake, fake, fake, fake, 10, 40, fake, None) < 0          # a map needs an image that has one


# ---- the command line ----------------------------------------------------------------------------------------------------------------------
def test_evaluate_argument_parsing():
    from npp_amd import evaluate
    a = evaluate.parse(["--pred", "p.png", "--gt", "g.png", "--mask", "m.png", "--json", "r.json"])
    assert (a.pred, a.gt, a.mask, a.valid, a.json, a.results, a.datadir) == ("p.png", "g.png", "m.png", None, "r.json", None, None)
    a = evaluate.parse(["--results", "res", "--datadir", "det"])
    assert (a.results, a.datadir, a.pred) == ("res", "det", None)
    for bad in (["--pred", "p.png"], [], ["--pred", "p.png", "--gt", "g.png", "--results", "r", "--datadir", "d"],
                ["--results", "r"], ["--results", "r", "--datadir", "d", "--mask", "m.png"]):
        with pytest.raises(SystemExit):
            evaluate.parse(bad)


def test_evaluate_json_keys_and_mask_polarity(stubbed, tmp_path, capsys):
    """The whole command on files, kernels stubbed: white in unknown_mask.png is KNOWN (io.load_npp_completion), the report goes to
    stdout as one JSON object and to --json, and the directory form finds the newest test set and adds its iteration."""
    from npp_amd import evaluate, io as nio
    a, b = R.content("noise", (40, 36))
    m, v = R.mask("hole", (40, 36)), np.ones((40, 36), np.float32)
    v[:, :4] = 0
    det = nio.write_detected_dir(str(tmp_path / "det"), b.astype(np.float64) + 1e-9, m, v, [[0.0, 90.0]], [[8.0, 8.0]], [[[8.0, 0.0], [0.0, 8.0]]])
    nio.imsave(str(tmp_path / "pred.png"), a)
    out = tmp_path / "report.json"
    rep = evaluate.main(["--pred", str(tmp_path / "pred.png"), "--gt", f"{det}/gt_img.png", "--mask", f"{det}/unknown_mask.png",
                         "--valid", f"{det}/valid_mask.png", "--json", str(out), "--device", "cpu"])
    printed = capsys.readouterr().out.strip()
    assert "\n" not in printed and json.loads(printed) == rep == json.loads(out.read_text())
    assert set(rep) == {"all", "known", "unknown"} and all(set(r) == {"pixels", "psnr", "ssim", "mae"} for r in rep.values())
    assert rep["known"]["pixels"] == int((m * v).sum()) and rep["unknown"]["pixels"] == int(((1 - m) * v).sum())
    a8 = nio._imread_rgb(str(tmp_path / "pred.png")).astype(np.float32)
    b8 = nio._imread_rgb(f"{det}/gt_img.png").astype(np.float32)
    want = R.report(a8, b8, m, v)
    for name in want:
        for k in ("psnr", "ssim", "mae"):
            assert abs(rep[name][k] - want[name][k]) <= 1e-12
    # the directory form: the newest of two test sets
    res = tmp_path / "res"
    for it, img in ((5, b8), (10, a8)):
        nio.dump_testset(str(res / f"testset_{it:06d}"), img, b8, b8 * m[..., None], m[..., None], v[..., None])
    rep2 = evaluate.main(["--results", str(res), "--datadir", det, "--device", "cpu"])
    assert rep2["iteration"] == 10 and set(rep2) == {"all", "known", "unknown", "iteration"}
    assert rep2["known"]["pixels"] == rep["known"]["pixels"]
    assert abs(rep2["unknown"]["psnr"] - rep["unknown"]["psnr"]) <= 1e-12          # (valid pixels only: the dump blacks out the others)


def test_train_flag_is_off_by_default():
    from npp_amd import train
    assert train.parse(["--datadir", "x"]).eval_metrics is False
    assert train.parse(["--datadir", "x", "--eval_metrics"]).eval_metrics is True
