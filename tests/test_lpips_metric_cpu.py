"""CPU checks of LPIPS as a quality figure (npp_amd.metrics.LPIPSMetric, metrics.report(lpips=), evaluate --lpips, train --eval_lpips):
the torch restatement (tests/lpips_restatement.py) against the reference's own LPIPS.forward (golden g16_lpips_image.npz) and against
closed forms, the report's bookkeeping with the kernels and the trunk stubbed by the restatement, the launchers' argument checks
(host code: nothing is launched) and the command lines' argument parsing.  No GPU calls.

Measured here (printed by the tests, recorded in DESIGN.md 6g), relative L2 per array against the golden:

* restatement in float32: 0.0 for the map, every tap and the scalar of both nets -- the same torch calls in the same order give the
  same bits.  The bound is 4 x the measured value, so equality is what is asserted (condition: the bound stays below 1e-5; it does);
* restatement in float64: map 1.9e-7 (vgg) / 2.6e-7 (alex), scalar 7.0e-8 / 9.5e-8, taps 2.3e-7 .. 6.6e-7, except the two deepest VGG
  taps, 2.6e-6 and 5.0e-5: the fixed-seed trunk maps both images to nearly the same deep features (tap means 1.4e-5 and 1.2e-8
  against 2.6e-2 for relu1_2), so those maps are differences of nearly equal fp32 numbers.  That is the reference's fp32 error, not
  the restatement's: it equals the distance of the float32 restatement from the float64 one, which is what the test holds it to."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import lpips_restatement as LR
import metrics_restatement as MR

NETS = ("vgg", "alex")
FP32_VS_GOLDEN = 0.0                        # measured rel-L2 of the float32 restatement against the golden, every array (docstring)
FP32_BOUND = 4 * FP32_VS_GOLDEN
assert FP32_BOUND < 1e-5

_cache = {}


def _golden(golden, net):
    """The golden's arrays of one net and the restatement in both dtypes on its inputs, once per module (read-only)."""
    if net not in _cache:
        z = golden("g16_lpips_image.npz")
        sd = LR.vgg_state_dict(int(z["vgg_seed"])) if net == "vgg" else LR.alex_state_dict(int(z["alex_seed"]), biases=True)
        lins = [z[f"{net}_lin{k}"] for k in range(5)]
        a, b = z[f"{net}_in0"], z[f"{net}_in1"]
        g = {"map": z[f"{net}_val"], "taps": [z[f"{net}_tap{k}"] for k in range(5)], "scalar": float(z[f"{net}_scalar"])}
        _cache[net] = dict(sd=sd, lins=lins, a=a, b=b, golden=g, f32=LR.lpips(net, sd, lins, a, b, torch.float32),
                           f64=LR.lpips(net, sd, lins, a, b, torch.float64))
    return _cache[net]


def _arrays(r):
    return [("map", r["map"])] + [(f"tap{k}", t) for k, t in enumerate(r["taps"])] + [("scalar", np.float64(r["scalar"]))]


def test_module_and_abi_exist():
    """Cannot pass without the feature: the class, the report's keyword, the flags and the C ABI exist."""
    import inspect
    import npp_amd
    from npp_amd import evaluate, metrics, ops, train
    assert callable(metrics.LPIPSMetric) and "lpips" in inspect.signature(metrics.report).parameters
    for name in ("map", "taps", "scalar", "region"):
        assert callable(getattr(metrics.LPIPSMetric, name))
    for name in ("lpips_tap_map", "lpips_compose", "map_region_sums"):
        assert callable(getattr(ops, name))
    L = npp_amd.lib()
    for name in ("npp_lpips_tap_map", "npp_lpips_compose", "npp_map_region_sums_blocks", "npp_map_region_sums"):
        assert hasattr(L, name)
    assert evaluate.parse(["--pred", "p", "--gt", "g"]).lpips is None and train.parse(["--datadir", "x"]).eval_lpips is None


# ---- the restatement against the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", NETS)
def test_float32_restatement_against_the_golden(golden, net):
    c = _golden(golden, net)
    for (name, got), (_, want) in zip(_arrays(c["f32"]), _arrays(c["golden"])):
        assert np.shape(got) == np.shape(want)
        dist = LR.rel_l2(got, want)
        print(f"{net} {name}: rel-L2(float32 restatement, golden) = {dist:.3e} (bound {FP32_BOUND:.1e})")
        assert dist <= FP32_BOUND, (net, name, dist)


@pytest.mark.parametrize("net", NETS)
def test_float64_restatement_against_the_golden(golden, net):
    """The yardstick of the GPU tests lies from the golden exactly as far as the reference's float32 arithmetic lies from float64:
    rel-L2(float64, golden) <= rel-L2(float32 restatement, float64 restatement) + the float32 bound above, per array."""
    c = _golden(golden, net)
    for (name, r64), (_, r32), (_, want) in zip(_arrays(c["f64"]), _arrays(c["f32"]), _arrays(c["golden"])):
        dist, fp32 = LR.rel_l2(r64, want), LR.rel_l2(r32, r64)
        print(f"{net} {name}: rel-L2(float64 restatement, golden) = {dist:.3e}, rel-L2(float32, float64) = {fp32:.3e}")
        assert dist <= fp32 * (1 + 1e-6) + FP32_BOUND and dist < 1e-4, (net, name, dist, fp32)


# ---- closed forms ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("net", NETS)
def test_identical_images_give_zero(golden, net, dtype):
    c = _golden(golden, net)
    r = LR.lpips(net, c["sd"], c["lins"], c["a"], c["a"].copy(), dtype)
    assert (r["map"] == 0).all() and all((t == 0).all() for t in r["taps"]) and r["scalar"] == 0.0


def test_a_single_position_tap_upsamples_to_a_constant():
    """Taps of a 24 x 17 image: relu5_3 is 1 x 1.  With every other tap equal in both images the map is that tap's one value."""
    shapes = [(64, 24, 17), (128, 12, 8), (256, 6, 4), (512, 3, 2), (512, 1, 1)]
    f0 = [LR.sparse_features(s, 10 + k) for k, s in enumerate(shapes)]
    f1 = [f.copy() for f in f0]
    f1[4] = LR.sparse_features(shapes[4], 99, dead_positions=0)
    lins = [np.abs(np.random.RandomState(k).randn(s[0])).astype(np.float32) for k, s in enumerate(shapes)]
    r = LR.head_on_features(f0, f1, lins, (24, 17))
    v = float(r["taps"][4][0, 0])
    # (the four bilinear weights of a pixel add up to 1 within a rounding or two)
    assert v > 0 and np.abs(r["map"] - v).max() <= 1e-15 * v and abs(r["scalar"] - v) <= 1e-15 * v


def test_scalar_is_not_the_mean_of_the_map(golden):
    """The two numbers of the report differ: bilinear upsampling does not keep a map's mean (alex: 19 x 16 -> 80 x 67 and on; vgg: the
    ratios 2, 4, 8 do keep it, 52 / 6 and 52 / 3 of the two deepest taps do not -- a small share of a small term, but not rounding)."""
    a, v = _golden(golden, "alex")["f64"], _golden(golden, "vgg")["f64"]
    rel = abs(a["scalar"] - a["map"].mean()) / a["scalar"]
    print(f"alex: scalar {a['scalar']:.9f}, mean of the map {a['map'].mean():.9f}, relative difference {rel:.3e}")
    print(f"vgg: scalar {v['scalar']:.12f}, mean of the map {v['map'].mean():.12f}")
    assert rel > 1e-5 and abs(v["scalar"] - v["map"].mean()) > 1e-12
    assert abs(sum(float(t.mean()) for t in a["taps"]) - a["scalar"]) <= 1e-15


# ---- metrics.report's bookkeeping: kernels and trunk stubbed by the restatement -----------------------------------------------------------
class _StubVgg:
    def __init__(self, sd):
        self.sd, self._buf, self._acts = sd, {"stale": 1}, [1]

    def _forward(self, x, scale, shift):
        sc, sh = torch.tensor(scale, dtype=torch.float32).view(1, 3, 1, 1), torch.tensor(shift, dtype=torch.float32).view(1, 3, 1, 1)
        return LR.vgg_features(self.sd, x * sc + sh)


class _StubAlex:
    def __init__(self, sd):
        self.sd = sd

    def features_nhwc(self, x):
        return [f.permute(0, 2, 3, 1).contiguous() for f in LR.alex_features(self.sd, x)]


@pytest.fixture
def stubbed(monkeypatch):
    from npp_amd import metrics, ops
    F = torch.nn.functional

    def ssim_map(a, b):
        return torch.from_numpy(MR.ssim_map_slices(a.numpy(), b.numpy()))

    def region_sums(a, b, w, smap=None):
        a64, b64, w64 = a.numpy().astype(np.float64), b.numpy().astype(np.float64), w.numpy().astype(np.float64)
        d = a64 - b64
        wi = w64[5:-5, 5:-5]
        row = [w64.sum(), (w64 * (d * d).sum(-1)).sum(), (w64 * np.abs(d).sum(-1)).sum(),
               0.0 if smap is None else wi.sum(), 0.0 if smap is None else (wi * smap.numpy()).sum()]
        return torch.tensor([row, [0.0] * 5], dtype=torch.float64)

    def lpips_tap_map(f0, f1, lin, layout="nchw"):
        if layout == "nhwc":
            f0, f1 = f0.permute(2, 0, 1), f1.permute(2, 0, 1)
        return torch.from_numpy(LR.head_on_features([f0.numpy()], [f1.numpy()], [lin.numpy()], (1, 1))["taps"][0])

    def lpips_compose(maps, H, W):
        return sum(F.interpolate(m[None, None], size=(H, W), mode="bilinear", align_corners=False)[0, 0] for m in maps)

    def map_region_sums(dmap, weight=None):
        w = torch.ones_like(dmap) if weight is None else weight.double()
        return torch.stack([torch.stack([w.sum(), (w * dmap).sum()]), torch.zeros(2, dtype=torch.float64)])     # (two "blocks")

    def build_trunk(net, sd, dev):
        if sd is None:
            sd = LR.vgg_state_dict() if net == "vgg" else LR.alex_state_dict()
        return _StubVgg(sd) if net == "vgg" else _StubAlex(sd)
    for name, fn in (("ssim_map", ssim_map), ("region_sums", region_sums), ("lpips_tap_map", lpips_tap_map), ("lpips_compose", lpips_compose),
                     ("map_region_sums", map_region_sums)):
        monkeypatch.setattr(ops, name, fn)
    monkeypatch.setattr(metrics, "_build_trunk", build_trunk)
    return metrics


def _expected(net, sd, lins, a, b):
    """The stubs' pipeline written out: float32 trunk of the restatement, float64 head on its features."""
    feats = LR.vgg_features if net == "vgg" else LR.alex_features
    f0, f1 = feats(sd, LR.preprocess(a, torch.float32)), feats(sd, LR.preprocess(b, torch.float32))
    return LR.head_on_features([f[0].numpy() for f in f0], [f[0].numpy() for f in f1], lins, a.shape[:2])


@pytest.mark.parametrize("net", NETS)
def test_report_with_lpips_keys_and_regions(stubbed, golden, net):
    c = _golden(golden, net)
    a, b = c["a"], c["b"]
    hw = a.shape[:2]
    m = MR.mask("hole", hw)
    v = np.ones(hw, np.float32)
    v[:, :7] = 0
    lp = stubbed.LPIPSMetric(net, trunk_state_dict=c["sd"], lin_weights=c["lins"], device="cpu")
    rep = stubbed.report(a, b, m, v, device="cpu", lpips=lp)
    assert set(rep) == {"all", "known", "unknown", "lpips_image"} and set(rep["lpips_image"]) == {"net", "scalar"}
    assert rep["lpips_image"]["net"] == net
    for r in ("all", "known", "unknown"):
        assert set(rep[r]) == {"pixels", "psnr", "ssim", "mae", "lpips"}
    assert rep["known"]["pixels"] + rep["unknown"]["pixels"] == rep["all"]["pixels"] == int(v.sum())
    want = _expected(net, c["sd"], c["lins"], a, b)
    # (the stub trunk folds 2x - 1 and the scaling layer as one affine map, the restatement in the reference's three steps: float32
    # roundings of the trunk's input, a few 1e-7 on the figures)
    for r, w in (("all", v), ("known", m * v), ("unknown", (1 - m) * v)):
        assert abs(rep[r]["lpips"] - LR.region_mean(want["map"], w)) <= 1e-5 * LR.region_mean(want["map"], w), r
    assert abs(rep["lpips_image"]["scalar"] - want["scalar"]) <= 1e-5 * want["scalar"]
    # known + unknown weighted sums add up to the all region's
    parts = sum(rep[r]["lpips"] * rep[r]["pixels"] for r in ("known", "unknown"))
    assert abs(parts - rep["all"]["lpips"] * rep["all"]["pixels"]) <= 1e-12 * parts
    assert rep["lpips_image"]["scalar"] != rep["all"]["lpips"]
    json.dumps(rep)
    # without the metric: today's dict exactly, and the same figures inside the extended one
    plain = stubbed.report(a, b, m, v, device="cpu")
    assert set(plain) == {"all", "known", "unknown"} and all(set(r) == {"pixels", "psnr", "ssim", "mae"} for r in plain.values())
    assert plain == stubbed.report(a, b, m, v, device="cpu", lpips=None)
    assert plain == {r: {k: rep[r][k] for k in ("pixels", "psnr", "ssim", "mae")} for r in plain}
    # the single figures agree with the report's, and the trunk's buffers were released
    assert lp.region(a, b, m * v) == rep["known"]["lpips"] and lp.scalar(a, b) == rep["lpips_image"]["scalar"]
    assert lp.region(a, b) == pytest.approx(float(lp.map(a, b).mean()), rel=1e-12) and len(lp.taps(a, b)) == 5
    if net == "vgg":
        assert lp.trunk._buf == {} and lp.trunk._acts == []


def test_report_empty_region_reports_none(stubbed, golden):
    c = _golden(golden, "vgg")
    lp = stubbed.LPIPSMetric("vgg", trunk_state_dict=c["sd"], lin_weights=c["lins"], device="cpu")
    rep = stubbed.report(c["a"], c["b"], np.ones(c["a"].shape[:2], np.float32), device="cpu", lpips=lp)       # nothing unknown
    assert rep["unknown"] == {"pixels": 0, "psnr": None, "ssim": None, "mae": None, "lpips": None}
    assert rep["known"] == rep["all"] and rep["all"]["lpips"] > 0
    assert lp.region(c["a"], c["b"], np.zeros(c["a"].shape[:2], np.float32)) is None


def test_construction_and_sizes_are_refused_by_name(stubbed):
    with pytest.raises(ValueError, match=r"vgg16-\*\.pth"):
        stubbed.LPIPSMetric("vgg", device="cpu")
    with pytest.raises(ValueError, match=r"alexnet-owt-\*\.pth"):
        stubbed.LPIPSMetric("alex", device="cpu")
    with pytest.raises(ValueError, match="net"):
        stubbed.LPIPSMetric("squeeze", device="cpu", allow_random=True)
    with pytest.warns(UserWarning, match="RANDOM") as rec:
        lp = stubbed.LPIPSMetric("vgg", device="cpu", allow_random=True)
    assert sum("RANDOM" in str(w.message) for w in rec) == 1
    for shape in [(15, 40), (40, 15)]:
        z = np.zeros(shape + (3,), np.float32)
        with pytest.raises(ValueError, match="at least 16"):
            lp.map(z, z)
        with pytest.raises(ValueError, match="at least 16"):
            stubbed.report(z, z, np.ones(shape, np.float32), device="cpu", lpips=lp)
    assert lp.map(np.zeros((16, 16, 3), np.float32), np.zeros((16, 16, 3), np.float32)).shape == (16, 16)
    with pytest.warns(UserWarning):
        la = stubbed.LPIPSMetric("alex", device="cpu", allow_random=True)
    z = np.zeros((30, 40, 3), np.float32)
    with pytest.raises(ValueError, match="at least 31"):
        la.scalar(z, z)
    assert [tuple(t.shape) for t in la.taps(np.zeros((31, 31, 3), np.float32), np.zeros((31, 31, 3), np.float32))] == \
        [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)]


# ---- the launchers' argument checks (host code) ----------------------------------------------------------------------------------------
def test_launchers_validate_on_the_host():
    import npp_amd
    L = npp_amd.lib()
    fake, ERR_ARG = C.c_void_p(64), -1                                      # never dereferenced: validation comes first
    tap = lambda f0, f1, Cc, h, w, layout, lin, out: L.npp_lpips_tap_map(f0, f1, Cc, h, w, layout, lin, out, None)      # noqa: E731
    for bad in [(None, fake, 4, 3, 3, 0, fake, fake), (fake, None, 4, 3, 3, 0, fake, fake), (fake, fake, 4, 3, 3, 0, None, fake),
                (fake, fake, 4, 3, 3, 0, fake, None)]:
        assert tap(*bad) == ERR_ARG and b"null pointer" in L.npp_last_error_string()
    assert tap(fake, fake, 0, 3, 3, 0, fake, fake) == ERR_ARG and b"C=0" in L.npp_last_error_string()
    for h, w in [(0, 3), (3, 0), (-1, 3)]:
        assert tap(fake, fake, 4, h, w, 1, fake, fake) == ERR_ARG and b"empty" in L.npp_last_error_string()
    for layout in (-1, 4, 17):
        assert tap(fake, fake, 4, 3, 3, layout, fake, fake) == ERR_ARG and b"unknown layout code" in L.npp_last_error_string()
    ptrs, one = (C.c_void_p * 2)(64, 64), (C.c_int32 * 2)(3, 3)
    assert L.npp_lpips_compose(ptrs, one, one, 2, 8, 0, fake, None) == ERR_ARG and b"empty" in L.npp_last_error_string()
    assert L.npp_lpips_compose(ptrs, one, one, 2, 8, 8, None, None) == ERR_ARG
    assert L.npp_lpips_compose(ptrs, one, one, 0, 8, 8, fake, None) == ERR_ARG
    assert L.npp_lpips_compose(ptrs, one, one, 9, 8, 8, fake, None) == ERR_ARG
    assert L.npp_lpips_compose((C.c_void_p * 2)(64, None), one, one, 2, 8, 8, fake, None) == ERR_ARG and b"tap 1" in L.npp_last_error_string()
    assert L.npp_lpips_compose(ptrs, (C.c_int32 * 2)(3, 0), one, 2, 8, 8, fake, None) == ERR_ARG and b"tap 1" in L.npp_last_error_string()
    assert L.npp_map_region_sums_blocks(1, 1) == 1 and L.npp_map_region_sums_blocks(16, 17) == 2
    assert L.npp_map_region_sums_blocks(1024, 1024) == 256 and L.npp_map_region_sums_blocks(0, 5) == ERR_ARG
    assert L.npp_map_region_sums(None, None, 4, 4, fake, None) == ERR_ARG and L.npp_map_region_sums(fake, None, 4, 4, None, None) == ERR_ARG
    assert L.npp_map_region_sums(fake, fake, 0, 4, fake, None) == ERR_ARG and b"empty" in L.npp_last_error_string()


# ---- the command lines ------------------------------------------------------------------------------------------------------------------
def test_argument_parsing():
    from npp_amd import evaluate, train
    a = evaluate.parse(["--pred", "p.png", "--gt", "g.png"])
    assert (a.lpips, a.vgg16, a.alexnet, a.lpips_lin, a.random_trunks) == (None, None, None, None, False)
    a = evaluate.parse(["--results", "r", "--datadir", "d", "--lpips", "alex", "--alexnet", "a.pth", "--lpips_lin", "l.pth", "--random-trunks"])
    assert (a.lpips, a.alexnet, a.lpips_lin, a.random_trunks) == ("alex", "a.pth", "l.pth", True)
    with pytest.raises(SystemExit):
        evaluate.parse(["--pred", "p.png", "--gt", "g.png", "--lpips", "squeeze"])
    t = train.parse(["--datadir", "x"])
    assert t.eval_lpips is None and t.eval_metrics is False
    assert train.parse(["--datadir", "x", "--eval_metrics", "--eval_lpips", "vgg"]).eval_lpips == "vgg"
    with pytest.raises(SystemExit):
        train.parse(["--datadir", "x", "--eval_lpips", "squeeze"])


def test_train_refuses_eval_lpips_without_eval_metrics(tmp_path):
    from npp_amd import train
    with pytest.raises(SystemExit, match="--eval_metrics"):
        train._plan(["--datadir", str(tmp_path / "nothing"), "--random-trunks", "--eval_lpips", "vgg"])


def test_missing_checkpoint_stops_naming_it(stubbed, tmp_path, monkeypatch):
    from npp_amd import evaluate, io as nio
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("TORCH_HOME", str(tmp_path / "torch_home"))
    a, b = LR.lattice_pair(40, 36)
    nio.imsave(str(tmp_path / "a.png"), a)
    nio.imsave(str(tmp_path / "b.png"), b)
    for net, name in (("vgg", "vgg16"), ("alex", "alexnet")):
        with pytest.raises(SystemExit, match=name):
            evaluate.main(["--pred", "a.png", "--gt", "b.png", "--lpips", net, "--device", "cpu"])
    with pytest.raises(FileNotFoundError, match="vgg16"):
        evaluate.main(["--pred", "a.png", "--gt", "b.png", "--lpips", "vgg", "--vgg16", "nowhere.pth", "--device", "cpu"])


def test_evaluate_with_lpips_writes_what_it_prints(stubbed, tmp_path, capsys, monkeypatch):
    from npp_amd import evaluate, io as nio
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("TORCH_HOME", str(tmp_path / "torch_home"))
    a, b = LR.lattice_pair(40, 36)
    nio.imsave("a.png", a)
    nio.imsave("b.png", b)
    plain = evaluate.main(["--pred", "a.png", "--gt", "b.png", "--device", "cpu"])
    plain_text = capsys.readouterr().out
    assert "lpips" not in plain_text and set(plain) == {"all", "known", "unknown"}
    with pytest.warns(UserWarning, match="RANDOM"):
        rep = evaluate.main(["--pred", "a.png", "--gt", "b.png", "--lpips", "vgg", "--random-trunks", "--json", "r.json", "--device", "cpu"])
    printed = capsys.readouterr().out.strip()
    assert "\n" not in printed and json.loads(printed) == rep and (tmp_path / "r.json").read_text() == printed + "\n"
    assert rep["lpips_image"]["net"] == "vgg" and rep["unknown"]["lpips"] is None and rep["all"]["lpips"] > 0
    assert {r: {k: rep[r][k] for k in plain[r]} for r in plain} == plain
    assert os.path.exists("r.json")


def test_run_table_gains_an_lpips_column(tmp_path, capsys):
    import types
    from npp_amd import run
    for name, lp in (("one", 0.12345), ("two", None)):
        d = tmp_path / "completion_top1" / name
        d.mkdir(parents=True)
        (d / "metrics.json").write_text(json.dumps({"unknown": {"pixels": 9, "psnr": 20.0, "ssim": 0.5, "mae": 0.1, "lpips": lp}}))
    args = types.SimpleNamespace(train_args="--eval_metrics --eval_lpips vgg", task="completion", basedir=str(tmp_path), p_topk=1)
    run.metrics_table(args, ["one", "two", "gone"])
    rows = capsys.readouterr().out.splitlines()
    assert rows[0].split() == ["image", "PSNR", "unknown", "SSIM", "unknown", "LPIPS", "unknown"]
    assert rows[1].split() == ["one", "20.00", "dB", "0.5000", "0.1235"] and rows[2].split()[-1] == "n/a" and rows[3].split() == ["gone", "-", "-", "-"]
    args.train_args = "--eval_metrics"
    run.metrics_table(args, ["one"])
    rows = capsys.readouterr().out.splitlines()
    assert "LPIPS" not in rows[0] and rows[1].split() == ["one", "20.00", "dB", "0.5000"]
