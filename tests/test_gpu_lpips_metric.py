"""GPU checks of LPIPS as a quality figure (csrc/npp_lpips_map.hip, npp_amd.metrics.LPIPSMetric, metrics.report(lpips=), evaluate
--lpips, train --eval_lpips) against the torch restatement of tests/lpips_restatement.py and the reference's own LPIPS.forward
(golden g16_lpips_image.npz).  Every measured figure is printed before it is asserted (pytest -s shows them); the measured ratios
are recorded in DESIGN.md 6g.

The shapes are the smallest at which the kernels can still go wrong: a 24 x 17 image (relu5_3 is 1 x 1; 408 pixels are two blocks of
the reduction, the second ragged), 40 x 52 (the ratios 52 / 6 and 52 / 3), and for the head alone the position counts around 16384,
where the launcher changes from split channels to one lane per position."""
import json
import os

import numpy as np
import pytest
import torch

import lpips_restatement as LR
import metrics_restatement as MR
import oracle

pytestmark = pytest.mark.gpu

HEAD_BOUND = 1e-10            # test 1 (its docstring)
TRUNK_FACTOR = 16             # test 2: tests/test_gpu_trunk32.py::test_trunk32_vs_float64's factor


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import npp_amd
    npp_amd.lib()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64).tolist() if x is not None else None


# ---- 1. head, composition and reduction alone, on given features ---------------------------------------------------------------------
TAP_SETS = {"24x17": ((24, 17), [(64, 24, 17), (128, 12, 8), (256, 6, 4), (512, 3, 2), (512, 1, 1)]),
            "40x52": ((40, 52), [(64, 40, 52), (128, 20, 26), (256, 10, 13), (512, 5, 6), (512, 2, 3)])}
_head_cache = {}


def _head_case(name):
    """Features, lins and the float64 restatement on them, once per module (read-only)."""
    if name not in _head_cache:
        HW, shapes = TAP_SETS[name]
        f0 = [LR.sparse_features(s, 100 + k) for k, s in enumerate(shapes)]
        f1 = [LR.sparse_features(s, 200 + k) for k, s in enumerate(shapes)]
        f1[1][:, 0, 0] = f0[1][:, 0, 0]                                      # one position where the two images agree: exactly 0
        lins = [np.abs(np.random.RandomState(300 + k).randn(s[0])).astype(np.float32) * 0.1 for k, s in enumerate(shapes)]
        want = LR.head_on_features(f0, f1, lins, HW)
        for a in [want["map"]] + want["taps"]:
            a.setflags(write=False)
        _head_cache[name] = (HW, f0, f1, lins, want)
    return _head_cache[name]


@pytest.mark.parametrize("layout", ["nchw", "nchw_lane", "nchw_split", "nhwc"])
@pytest.mark.parametrize("name", list(TAP_SETS))
def test_head_compose_and_reduction_on_given_features(dev, name, layout):
    """No trunk: random fp32 taps with exact zeros at 30 % of the entries and a few all-zero positions (the + 1e-10 branch), every
    layout code, against the float64 restatement on the same fp32 features.

    The bound.  The fp32 features are exact inputs of both sides.  A squared norm is a float64 sum of at most 512 non-negative
    terms, each one rounding from exact: relative error <= 513 u, u = 2^-53, in any summation order; square root, + 1e-10 and the
    two divisions add a few u.  A tap value is again a float64 sum of at most 512 non-negative terms lin_c e_c^2, each a few
    roundings from exact, where e_c is a difference of two numbers in [0, 1] with absolute error of a few hundred u: relative
    error of the sum of order 512 x 2^-53 = 6e-14 plus the same order from the norms, in either implementation and whatever the
    order of the channels.  The bilinear weights are formed from the same float64 expression (a few ulp) and the five-term sum
    adds five roundings.  Asserted: |GPU - restatement| <= 1e-10 max(D) on every map value (1e-10 max(d_k) on a tap's), 1e-10
    relative on the region means and the scalar -- three decades above what the arithmetic explains, seven below an fp32 slip."""
    from npp_amd import metrics, ops
    HW, f0, f1, lins, want = _head_case(name)
    nhwc = layout == "nhwc"
    put = (lambda f: _t(f.transpose(1, 2, 0), dev)) if nhwc else (lambda f: _t(f, dev))
    taps = [ops.lpips_tap_map(put(a), put(b), _t(l, dev), layout) for a, b, l in zip(f0, f1, lins)]
    worst = 0.0
    for k, (g, w) in enumerate(zip(taps, want["taps"])):
        assert g.dtype == torch.float64 and tuple(g.shape) == w.shape and g.is_cuda
        g = g.cpu().numpy()
        dist = float(np.abs(g - w).max())
        print(f"{name} {layout} tap {k} {w.shape}: max |GPU - restatement| = {dist:.3e}, max d = {w.max():.3e}")
        assert np.isfinite(g).all() and dist <= HEAD_BOUND * w.max(), (k, dist)
        worst = max(worst, dist / w.max())
    assert float(taps[1][0, 0]) == 0.0                                        # identical features at one position
    D = ops.lpips_compose(taps, *HW)
    assert D.dtype == torch.float64 and tuple(D.shape) == HW
    Dh = D.cpu().numpy()
    dist = float(np.abs(Dh - want["map"]).max())
    print(f"{name} {layout} map: max |GPU - restatement| = {dist:.3e}, max D = {want['map'].max():.3e}; worst tap {worst:.3e} (relative)")
    assert dist <= HEAD_BOUND * want["map"].max()
    scalar = metrics._scalar(taps)
    print(f"{name} {layout} scalar: GPU {scalar:.15g}, restatement {want['scalar']:.15g}")
    assert abs(scalar - want["scalar"]) <= HEAD_BOUND * want["scalar"]
    regions = {"all": None, "hole": MR.mask("hole", HW), "irregular": MR.mask("irregular", HW) * 0.75, "none": np.zeros(HW, np.float32)}
    totals = metrics._map_totals(D, [None if w is None else _t(w, dev) for w in regions.values()])
    for (rname, w), t in zip(regions.items(), totals):
        got, ref = metrics._mean(t), LR.region_mean(want["map"], w)
        if rname == "none":
            assert got is None and ref is None and t[0] == 0
            continue
        print(f"{name} {layout} region {rname}: GPU {got:.15g}, restatement {ref:.15g}")
        assert t[0] == (HW[0] * HW[1] if w is None else float(w.astype(np.float64).sum())) and abs(got - ref) <= HEAD_BOUND * ref


@pytest.mark.parametrize("shape", [(8, 127, 129), (8, 128, 128), (5, 129, 128)], ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}")
def test_head_at_the_threshold_between_the_two_nchw_forms(dev, shape):
    """16383 positions (the last split-channel launch), 16384 (the first with one lane per position) and 16512 (64.5 blocks of it: a
    ragged last block): the launcher's own choice and both forced forms against the restatement, same bound as above."""
    from npp_amd import metrics, ops
    f0, f1 = LR.sparse_features(shape, 7), LR.sparse_features(shape, 8)
    lin = np.abs(np.random.RandomState(9).randn(shape[0])).astype(np.float32)
    want = LR.head_on_features([f0], [f1], [lin], shape[1:])["taps"][0]
    for layout in ("nchw", "nchw_lane", "nchw_split"):
        got = ops.lpips_tap_map(_t(f0, dev), _t(f1, dev), _t(lin, dev), layout)
        dist = float(np.abs(got.cpu().numpy() - want).max())
        print(f"{shape} {layout}: max |GPU - restatement| = {dist:.3e}, max d = {want.max():.3e}")
        assert dist <= HEAD_BOUND * want.max()
        mean = metrics._mean(metrics._map_totals(got, [None])[0])
        assert abs(mean - float(want.mean())) <= HEAD_BOUND * float(want.mean())


# ---- 2. / 3. the whole metric against float64 and against the reference -----------------------------------------------------------------
_cases = {}


def _case(key):
    """Inputs, trunk state dict, lins and the restatement in float64 / float32 on the CPU, once per module (read-only).  Keys:
    (net, "golden-random"): the golden's inputs on the fixed-seed trunks of allow_random=True; (net, "small"): a 24 x 17 pair (vgg) /
    the smallest legal 31 x 31 pair (alex) on the same trunks; (net, "golden"): the golden's inputs on the golden's own trunk."""
    if key not in _cases:
        net, kind = key
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g16_lpips_image.npz"))
        if kind == "golden":
            sd = LR.vgg_state_dict(int(z["vgg_seed"])) if net == "vgg" else LR.alex_state_dict(int(z["alex_seed"]), biases=True)
            lins = [z[f"{net}_lin{k}"] for k in range(5)]
        else:
            from npp_amd import weights
            sd = LR.vgg_state_dict() if net == "vgg" else LR.alex_state_dict()
            lins = weights.lpips_lin(net)
        if kind == "small":
            a, b = LR.lattice_pair(*((24, 17) if net == "vgg" else (31, 31)), seed=5)
        else:
            a, b = z[f"{net}_in0"], z[f"{net}_in1"]
        _cases[key] = dict(a=a, b=b, sd=sd, lins=lins, f64=LR.lpips(net, sd, lins, a, b, torch.float64),
                           f32=LR.lpips(net, sd, lins, a, b, torch.float32),
                           golden={"map": z[f"{net}_val"], "taps": [z[f"{net}_tap{k}"] for k in range(5)], "scalar": float(z[f"{net}_scalar"])})
    return _cases[key]


def _arrays(r):
    return [("map", r["map"])] + [(f"tap{k}", t) for k, t in enumerate(r["taps"])] + [("scalar", np.float64(r["scalar"]))]


def _run(m, a, b):
    taps, D = m._maps(*m._pair(a, b))
    from npp_amd import metrics
    return {"map": D.cpu().numpy(), "taps": [t.cpu().numpy() for t in taps], "scalar": metrics._scalar(taps)}


def _random_metric(net, dev):
    import warnings
    from npp_amd import metrics
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return metrics.LPIPSMetric(net, device=dev, allow_random=True)


@pytest.mark.parametrize("kind", ["golden-random", "small"])
@pytest.mark.parametrize("net", ["vgg", "alex"])
def test_whole_metric_against_float64(dev, net, kind):
    """LPIPSMetric(net, allow_random=True) against the restatement in float64 and in torch fp32 on the CPU, all three on the same
    tensors: rel-L2(HIP, float64) <= 16 x rel-L2(torch fp32, float64) for the map, every tap's map and the scalar.  The trunk is the
    only fp32 stage here as in tests/test_gpu_trunk32.py::test_trunk32_vs_float64, whose factor this is (a fully sequential fp32
    accumulation lies 1.7-7 x further from float64 than torch's; 16 leaves a factor of two over that)."""
    c = _case((net, kind))
    got = _run(_random_metric(net, dev), c["a"], c["b"])
    failed = []
    for (name, g), (_, r64), (_, r32) in zip(_arrays(got), _arrays(c["f64"]), _arrays(c["f32"])):
        assert np.shape(g) == np.shape(r64)
        e_hip, e_t = LR.rel_l2(g, r64), LR.rel_l2(r32, r64)
        print(f"{net} {kind} {name} {np.shape(g)}: HIP {e_hip:.3e}  torch fp32 {e_t:.3e}  ratio {e_hip / max(e_t, 1e-300):.2f}")
        if not e_hip <= TRUNK_FACTOR * e_t:
            failed.append((name, e_hip, e_t))
    assert not failed, failed


@pytest.mark.parametrize("net", ["vgg", "alex"])
def test_whole_metric_against_the_reference(dev, net):
    """The same outputs on the golden's own trunk against g16_lpips_image.npz.  Bound per array: the reference's distance from the
    float64 restatement (what tests/test_lpips_metric_cpu.py measures; formed here on the same arrays) + test 2's bound."""
    from npp_amd import metrics
    c = _case((net, "golden"))
    m = metrics.LPIPSMetric(net, trunk_state_dict=c["sd"], lin_weights=c["lins"], device=dev)
    got = _run(m, c["a"], c["b"])
    failed = []
    for (name, g), (_, ref), (_, r64), (_, r32) in zip(_arrays(got), _arrays(c["golden"]), _arrays(c["f64"]), _arrays(c["f32"])):
        dist, bound = LR.rel_l2(g, ref), LR.rel_l2(ref, r64) + TRUNK_FACTOR * LR.rel_l2(r32, r64)
        print(f"{net} {name}: rel-L2(HIP, golden) = {dist:.3e}, bound {bound:.3e} (golden vs float64 {LR.rel_l2(ref, r64):.3e})")
        if not dist <= bound:
            failed.append((name, dist, bound))
    assert not failed, failed


# ---- 4. reproducibility and re-use -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", ["vgg", "alex"])
def test_identical_bits_and_no_memory_of_a_shape(dev, net):
    """Two runs give identical bits; one instance fed the golden's size, the small size and the golden's size again returns, each
    time, the bits of a fresh instance; after a call the trunk holds no activation buffer."""
    sizes = ["golden-random", "small", "golden-random"]
    one = _random_metric(net, dev)
    hw = _case((net, "small"))["a"].shape[:2]
    w = MR.mask("hole", hw)
    for kind in sizes:
        c = _case((net, kind))
        got, fresh = _run(one, c["a"], c["b"]), _run(_random_metric(net, dev), c["a"], c["b"])
        for (name, g), (_, f) in zip(_arrays(got), _arrays(fresh)):
            assert _bits(g) == _bits(f), (kind, name)
        if net == "vgg":
            assert one.trunk._buf == {} and one.trunk._acts == []
    c = _case((net, "small"))
    first = (one.region(c["a"], c["b"], w), one.scalar(c["a"], c["b"]), _bits(one.map(c["a"], c["b"]).cpu().numpy()))
    second = (one.region(c["a"], c["b"], w), one.scalar(c["a"], c["b"]), _bits(one.map(c["a"], c["b"]).cpu().numpy()))
    assert _bits(first[0]) == _bits(second[0]) and _bits(first[1]) == _bits(second[1]) and first[2] == second[2]
    same = _run(one, c["a"], c["a"].copy())
    assert (same["map"] == 0).all() and same["scalar"] == 0.0                 # identical images: exactly zero


def test_small_images_are_refused(dev):
    m = _random_metric("vgg", dev)
    z = np.zeros((15, 40, 3), np.float32)
    with pytest.raises(ValueError, match="at least 16"):
        m.map(z, z)
    from npp_amd import metrics
    with pytest.raises(ValueError, match="vgg16"):
        metrics.LPIPSMetric("vgg", device=dev)


# ---- 5. report and command line ----------------------------------------------------------------------------------------------------------
def _report_bits(rep):
    return tuple(None if rep[r][k] is None else np.float64(rep[r][k]).view(np.uint64).item() for r in ("all", "known", "unknown")
                 for k in ("pixels", "psnr", "ssim", "mae"))


def _parent_report(a, b, known_mask, valid_mask, dev):
    """metrics.report as it was before the lpips keyword, statement for statement, on the package's own helpers."""
    from npp_amd import metrics, ops
    dev, a, b = metrics._pair(a, b, dev)
    hw = a.shape[:2]
    m, v = metrics._region(known_mask, dev, hw, "known_mask"), metrics._region(valid_mask, dev, hw, "valid_mask")
    totals = metrics._totals(a, b, [v, m * v, (1.0 - m) * v], ops.ssim_map(a, b))
    out = {}
    for name, t in zip(("all", "known", "unknown"), totals):
        n = float(t[0])
        out[name] = {"pixels": int(n) if n == int(n) else n, "psnr": metrics._psnr(t), "ssim": metrics._ssim(t), "mae": metrics._mae(t)}
    return out


@pytest.mark.parametrize("net", ["vgg", "alex"])
def test_report_with_lpips(dev, net):
    from npp_amd import metrics
    c = _case((net, "golden-random"))
    a, b = c["a"], c["b"]
    hw = a.shape[:2]
    m = MR.mask("irregular", hw)
    v = np.ones(hw, np.float32)
    v[:, -3:] = 0
    lp = _random_metric(net, dev)
    rep = metrics.report(a, b, m, v, device=dev, lpips=lp)
    assert set(rep) == {"all", "known", "unknown", "lpips_image"} and rep["lpips_image"]["net"] == net
    D64, D32 = c["f64"]["map"], c["f32"]["map"]
    for r, w in (("all", v), ("known", m * v), ("unknown", (1 - m) * v)):
        want, fp32 = LR.region_mean(D64, w), LR.region_mean(D32, w)
        print(f"{net} {r}: lpips {rep[r]['lpips']:.9g}, float64 {want:.9g}, torch fp32 {fp32:.9g}")
        assert abs(rep[r]["lpips"] - want) <= TRUNK_FACTOR * LR.rel_l2(D32, D64) * want
    assert abs(rep["lpips_image"]["scalar"] - c["f64"]["scalar"]) <= TRUNK_FACTOR * LR.rel_l2(D32, D64) * c["f64"]["scalar"]
    parts = sum(rep[r]["lpips"] * rep[r]["pixels"] for r in ("known", "unknown"))
    whole = rep["all"]["lpips"] * rep["all"]["pixels"]
    print(f"{net}: known + unknown weighted sums {parts:.15g}, all {whole:.15g}")
    assert abs(parts - whole) <= 1e-12 * whole
    # without the metric: the parent's report, bit for bit -- and the same bits inside the extended one
    plain = metrics.report(a, b, m, v, device=dev)
    assert set(plain) == {"all", "known", "unknown"} and all(set(r) == {"pixels", "psnr", "ssim", "mae"} for r in plain.values())
    assert _report_bits(plain) == _report_bits(_parent_report(a, b, m, v, dev)) == _report_bits(rep)
    empty = metrics.report(a, b, np.ones(hw, np.float32), device=dev, lpips=lp)
    assert empty["unknown"] == {"pixels": 0, "psnr": None, "ssim": None, "mae": None, "lpips": None}


def test_evaluate_command_with_lpips(dev, tmp_path, capsys, monkeypatch):
    from npp_amd import evaluate, io as nio
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("TORCH_HOME", str(tmp_path / "torch_home"))          # (no checkpoint to be found: --random-trunks decides)
    a, b = LR.lattice_pair(40, 52)
    nio.imsave("a.png", a)
    nio.imsave("b.png", b)
    plain = evaluate.main(["--pred", "a.png", "--gt", "b.png"])
    assert "lpips" not in capsys.readouterr().out
    rep = evaluate.main(["--pred", "a.png", "--gt", "b.png", "--lpips", "vgg", "--random-trunks", "--json", "r.json"])
    printed = capsys.readouterr().out.strip()
    assert "\n" not in printed and json.loads(printed) == rep and (tmp_path / "r.json").read_text() == printed + "\n"
    assert rep["lpips_image"]["net"] == "vgg" and rep["lpips_image"]["scalar"] > 0 and rep["all"]["lpips"] > 0
    assert rep["unknown"]["lpips"] is None                                    # no --mask: everything is known
    assert {r: {k: rep[r][k] for k in plain[r]} for r in plain} == plain


def test_training_command_with_eval_lpips(dev, tmp_path, capsys, monkeypatch):
    """40 iterations on the synthetic lattice at 96^2 (the smallest size the training command's 64-pixel patches admit,
    tests/test_gpu_metrics.py): metrics.json carries the new keys, the [EVAL] line the two LPIPS figures, and evaluate reproduces the file
    as text from the two directories."""
    from npp_amd import evaluate, io as nio, train
    monkeypatch.setenv("TORCH_HOME", str(tmp_path / "torch_home"))
    img, mask = oracle.synthetic_image(96)
    angles, periods, shifts = oracle.synthetic_periodicity(96, 1)
    d = nio.write_detected_dir(str(tmp_path / "detected" / "syn"), img, mask, np.ones_like(mask), angles, periods, shifts)
    common = ["--datadir", d, "--p_topk", "1", "--random-trunks", "--N_iters", "41", "--i_testset", "40", "--i_print", "40", "--netwidth", "256",
              "--N_rand", "2048", "--rng_mode", "fast", "--basedir", str(tmp_path / "res")]
    with pytest.raises(SystemExit, match="--eval_metrics"):
        train.main(common + ["--eval_lpips", "vgg"])
    assert not (tmp_path / "res").exists()
    assert train.main(common + ["--eval_metrics", "--eval_lpips", "vgg"]) is not None
    out = capsys.readouterr().out
    res = tmp_path / "res" / "completion_top1" / "syn"
    assert sorted(os.listdir(res)) == ["metrics.json", "testset_000040"]
    rep = json.loads((res / "metrics.json").read_text())
    assert set(rep) == {"all", "known", "unknown", "iteration", "lpips_image"} and rep["iteration"] == 40
    assert rep["lpips_image"]["net"] == "vgg" and all(rep[r]["lpips"] > 0 for r in ("all", "known", "unknown"))
    line = [l for l in out.splitlines() if l.startswith("[EVAL]")][0]
    assert line.endswith(f", LPIPS known {rep['known']['lpips']:.4f} unknown {rep['unknown']['lpips']:.4f}") and ", SSIM known " in line
    again = evaluate.main(["--results", str(res), "--datadir", d, "--lpips", "vgg", "--random-trunks", "--json", str(tmp_path / "again.json")])
    assert again == rep and (tmp_path / "again.json").read_text() == (res / "metrics.json").read_text()
