"""GPU checks of the quality report (csrc/npp_metrics.hip, npp_amd.metrics, npp_amd.evaluate, train.py --eval_metrics) against the
float64 restatement of tests/metrics_restatement.py.

The map bound, |GPU - restatement| <= 1e-9 on every map value: a moment is a sum of 121 non-negative products, so its relative
rounding error is about 121 x 2^-53 = 1.3e-14 in either implementation; the cancellation in sigma^2 and sigma_xy is amplified by at
most 1 / C2 = 1.1e3, which gives about 3e-11 for both together; 1e-9 leaves a factor of about 30.  The region figures are quotients
of float64 sums of a few thousand such values: 1e-9 (dB for the PSNR) as well, pixel counts exact.  Every measured figure is printed
before it is asserted (pytest -s shows them)."""
import json
import math
import os

import numpy as np
import pytest

import metrics_restatement as R
import oracle

pytestmark = pytest.mark.gpu

MAP_BOUND = 1e-9
FIG_BOUND = 1e-9


@pytest.fixture(scope="module")
def dev():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import npp_amd
    npp_amd.lib()
    return torch.device("cuda:0")


_cache = {}


def _case(kind, shape):
    """Image pair + the restatement's map, once per module (read-only)."""
    key = (kind, shape)
    if key not in _cache:
        a, b = R.content(kind, shape)
        smap = R.ssim_map_slices(a, b)
        smap.setflags(write=False)
        _cache[key] = (a, b, smap)
    return _cache[key]


def _bits(rep):
    """A report as a tuple of exact bit patterns (None stays None)."""
    return tuple(None if rep[r][k] is None else np.float64(rep[r][k]).view(np.uint64).item() for r in ("all", "known", "unknown")
                 for k in ("pixels", "psnr", "ssim", "mae"))


def _check_report(got, want, what):
    for name in ("all", "known", "unknown"):
        assert got[name]["pixels"] == want[name]["pixels"], (what, name)
        for k in ("psnr", "ssim", "mae"):
            g, w = got[name][k], want[name][k]
            assert (g is None) == (w is None), (what, name, k)
            if g is not None:
                print(f"{what} {name} {k}: GPU {g:.12g}, restatement {w:.12g}, distance {abs(g - w):.3e}")
                assert abs(g - w) <= FIG_BOUND, (what, name, k)


# ---- 1. the map against the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.CONTENTS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_map_against_the_restatement(dev, shape, kind):
    from npp_amd import metrics
    a, b, want = _case(kind, shape)
    got = metrics.ssim_map(a, b, device=dev)
    assert str(got.dtype) == "torch.float64" and tuple(got.shape) == (shape[0] - 10, shape[1] - 10) and got.is_cuda
    got = got.cpu().numpy()
    dist = float(np.abs(got - want).max())
    print(f"{kind} {shape}: max |GPU - restatement| = {dist:.3e} (bound {MAP_BOUND:.0e}), map in [{got.min():.6f}, {got.max():.6f}]")
    assert np.isfinite(got).all() and dist <= MAP_BOUND


# ---- 2. closed forms -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(47, 33), (130, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_identical_images_give_exactly_one_and_the_psnr_floor(dev, shape):
    from npp_amd import metrics
    a, _, _ = _case("noise", shape)
    got = metrics.ssim_map(a, a.copy(), device=dev).cpu().numpy()
    assert (got == 1.0).all()
    rep = metrics.report(a, a.copy(), R.mask("hole", shape), device=dev)
    for r in rep.values():
        assert r["psnr"] == 200.0 and r["ssim"] == 1.0 and r["mae"] == 0.0
    assert metrics.psnr(a, a.copy(), device=dev) == 200.0 and metrics.ssim(a, a.copy(), device=dev) == 1.0


def test_constant_images_match_their_closed_form(dev):
    from npp_amd import metrics
    c1, c2 = np.float32([0.2, 0.5, 0.9]), np.float32([0.3, 0.5, 0.1])
    fa, fb = np.ascontiguousarray(np.broadcast_to(c1, (47, 33, 3))), np.ascontiguousarray(np.broadcast_to(c2, (47, 33, 3)))
    x, y = c1.astype(np.float64), c2.astype(np.float64)
    want = float(((2 * x * y + R.C1) / (x * x + y * y + R.C1)).mean())
    got = metrics.ssim_map(fa, fb, device=dev).cpu().numpy()
    dist = float(np.abs(got - want).max())
    print(f"constant images: closed form {want:.15f}, max distance {dist:.3e}")
    assert dist <= 1e-12
    sym = metrics.ssim_map(fb, fa, device=dev).cpu().numpy()
    assert np.array_equal(sym, got)


# ---- 3. report against the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mkind", R.MASKS)
@pytest.mark.parametrize("shape", [(47, 33), (130, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_report_against_the_restatement(dev, shape, mkind):
    from npp_amd import metrics
    a, b, _ = _case("ramp" if mkind == "hole" else "noise", shape)
    m = R.mask(mkind, shape)
    v = np.ones(shape, np.float32)
    v[:, -3:] = 0                                                         # a valid mask: the last three columns do not count
    assert 0 < (m * v).sum() < v.sum()
    _check_report(metrics.report(a, b, m, v, device=dev), R.report(a, b, m, v), f"{mkind} {shape}")
    _check_report(metrics.report(a, b, m, device=dev), R.report(a, b, m), f"{mkind} {shape} (no valid mask)")
    w = m * v
    for fn, key in ((metrics.psnr, "psnr"), (metrics.mae, "mae"), (metrics.ssim, "ssim")):
        assert abs(fn(a, b, w, device=dev) - R.region_figures(a, b, w)[key]) <= FIG_BOUND


def test_empty_and_border_only_regions(dev):
    from npp_amd import metrics
    shape = (47, 33)
    a, b, smap = _case("noise", shape)
    rep = metrics.report(a, b, np.ones(shape, np.float32), device=dev)
    assert rep["unknown"] == {"pixels": 0, "psnr": None, "ssim": None, "mae": None}
    assert rep["known"] == rep["all"] and rep["all"]["pixels"] == 47 * 33
    assert abs(rep["all"]["ssim"] - float(smap.mean())) <= FIG_BOUND
    m = np.ones(shape, np.float32)
    m[:5] = 0
    m[-5:] = 0
    m[:, :5] = 0
    m[:, -5:] = 0                                                         # unknown = exactly the 5-pixel border
    rep = metrics.report(a, b, m, device=dev)
    u = rep["unknown"]
    assert u["pixels"] == 47 * 33 - 37 * 23 and u["ssim"] is None and math.isfinite(u["psnr"]) and math.isfinite(u["mae"])
    _check_report(rep, R.report(a, b, m), "border only")
    assert metrics.ssim(a, b, 1 - m, device=dev) is None and metrics.psnr(a, b, np.zeros(shape, np.float32), device=dev) is None


# ---- 4. reproducibility, changing shapes, refused sizes -----------------------------------------------------------------------------------
def test_two_calls_give_identical_bits(dev):
    from npp_amd import metrics
    shape = (130, 70)
    a, b, _ = _case("noise", shape)
    m = R.mask("irregular", shape)
    first, second = metrics.report(a, b, m, device=dev), metrics.report(a, b, m, device=dev)
    assert _bits(first) == _bits(second)
    m1, m2 = metrics.ssim_map(a, b, device=dev).cpu().numpy(), metrics.ssim_map(a, b, device=dev).cpu().numpy()
    assert np.array_equal(m1.view(np.uint64), m2.view(np.uint64))


def test_shapes_change_between_calls(dev):
    """130 x 70, 12 x 37, 130 x 70 again in one process: no entry keeps scratch, so every call equals the same call made afresh."""
    from npp_amd import metrics
    order = [(130, 70), (12, 37), (130, 70)]
    reps, maps = [], []
    for s in order:
        a, b, want = _case("saturated", s)
        got = metrics.ssim_map(a, b, device=dev).cpu().numpy()
        assert np.abs(got - want).max() <= MAP_BOUND
        maps.append(got)
        reps.append(metrics.report(a, b, R.mask("border_hole", s), device=dev))
        _check_report(reps[-1], R.report(a, b, R.mask("border_hole", s)), f"sequence {s}")
    assert np.array_equal(maps[0].view(np.uint64), maps[2].view(np.uint64)) and _bits(reps[0]) == _bits(reps[2])


def test_small_images_are_refused(dev):
    from npp_amd import metrics
    for shape in [(10, 40), (40, 10)]:
        z = np.zeros(shape + (3,), np.float32)
        with pytest.raises(ValueError, match="at least 11"):
            metrics.ssim_map(z, z, device=dev)
        with pytest.raises(ValueError, match="at least 11"):
            metrics.report(z, z, np.ones(shape, np.float32), device=dev)
    z = np.zeros((10, 40, 3), np.float32)
    assert metrics.psnr(z, z + 0.5, device=dev) == pytest.approx(-10 * math.log10(0.25), abs=1e-12)      # no window needed


# ---- 5. the fit and the training command ----------------------------------------------------------------------------------------------------
def _scene(H=64):
    img, mask = oracle.synthetic_image(H)
    return img, mask, oracle.synthetic_periodicity(H, 1)


def test_report_equals_the_fits_own_psnr(dev):
    from npp_amd import metrics
    from npp_amd.fit import CompletionFit
    img, mask, (angles, periods, _) = _scene()
    fit = CompletionFit(img, mask, angles, periods, oracle.SEED0_FREQS, oracle.init_params(1, seed=0), device=dev, N_rand=2048, rng_mode="fast")
    for _ in range(5):
        fit.step()
    rep = metrics.report(fit.render_image(), fit.img, fit.mask, device=dev)
    for region in ("known", "unknown"):
        own = fit.psnr(region)
        print(f"{region}: report {rep[region]['psnr']:.9f} dB, CompletionFit.psnr {own:.9f} dB, distance {abs(rep[region]['psnr'] - own):.3e}")
    # (fp32 against float64 summation of about 1e4 squared errors of order 1e-2)
    assert abs(rep["known"]["psnr"] - fit.psnr("known")) <= 1e-4
    assert 0.0 < rep["known"]["ssim"] < 1.0 and rep["known"]["pixels"] + rep["unknown"]["pixels"] == 64 * 64
    fit.close()


def test_training_command_with_eval_metrics(dev, tmp_path, capsys):
    """The same synthetic lattice at 96^2, not 64^2: the training command samples 64-pixel patches (the smallest size the loaders give),
    whose centres must lie more than 32 pixels from every border -- at 64^2 both patch pools are empty and the sampler cannot draw;
    96 is the next multiple of 32."""
    from npp_amd import evaluate, io as nio, metrics, train
    img, mask, (angles, periods, shifts) = _scene(96)
    d = nio.write_detected_dir(str(tmp_path / "detected" / "syn"), img, mask, np.ones_like(mask), angles, periods, shifts)
    common = ["--datadir", d, "--p_topk", "1", "--random-trunks", "--N_iters", "6", "--i_testset", "5", "--i_print", "5", "--netwidth", "256",
              "--N_rand", "2048", "--rng_mode", "fast"]
    # without the flag: no metrics.json, no SSIM field
    fit = train.main(common + ["--basedir", str(tmp_path / "plain")])
    assert fit is not None
    out = capsys.readouterr().out
    plain = tmp_path / "plain" / "completion_top1" / "syn"
    assert sorted(os.listdir(plain)) == ["testset_000005"] and "SSIM" not in out
    assert [l for l in out.splitlines() if l.startswith("[EVAL]")][0].endswith(" dB")
    # with it
    fit = train.main(common + ["--basedir", str(tmp_path / "res"), "--eval_metrics"])
    out = capsys.readouterr().out
    res = tmp_path / "res" / "completion_top1" / "syn"
    assert sorted(os.listdir(res)) == ["metrics.json", "testset_000005"]
    rep = json.loads((res / "metrics.json").read_text())
    assert set(rep) == {"all", "known", "unknown", "iteration"} and rep["iteration"] == 5
    line = [l for l in out.splitlines() if l.startswith("[EVAL]")][0]
    assert line.endswith(f", SSIM known {rep['known']['ssim']:.4f} unknown {rep['unknown']['ssim']:.4f}")
    # the figures are report's on the dumped image, and the command line reproduces the file from the two directories
    loaded = nio.load_npp_completion(d, 1)
    dumped = nio._imread_rgb(str(res / "testset_000005" / "pred_rgb_img.png")).astype(np.float32)
    want = metrics.report(dumped, loaded["img"], loaded["mask"], loaded["valid_mask"], device=dev)
    want["iteration"] = 5
    assert rep == want
    again = evaluate.main(["--results", str(res), "--datadir", d, "--json", str(tmp_path / "again.json")])
    assert again == rep and (tmp_path / "again.json").read_text() == (res / "metrics.json").read_text()
    _check_report({k: rep[k] for k in ("all", "known", "unknown")}, R.report(dumped, loaded["img"], loaded["mask"], loaded["valid_mask"]),
                  "metrics.json")
