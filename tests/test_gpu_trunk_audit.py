"""Trunk audit on the GPU (include/npp_hip.h "trunk audit"): the census launch against its plain C++ twin and
the NumPy restatement on planted tensors, HipTrunk.census against independent counts in torch on the exported layers, audited fits
against unaudited ones (bits) with the report recomputed from public modules, the remapping task's style term, both audits on one
iteration, and the command-line flag in child processes.  Counts are exact; the gaps are compared with an independent computation
and are not bounded."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import trunk_census_restatement as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0x5A5A5A5A5A5A5A5A
KEYS = R.FIELDS + ("exp_hist", "gate_on", "gate_flips")
# the issue's three cases, then two that take the kernel's other paths: several workgroups per chunk with images >= n behind them
# (4 chunks x 7 workgroups), and a chunk longer than one pass of its workgroups (64 chunks: 32 workgroups per chunk, 20160
# positions -> the strided loop runs twice for some lanes)
CASES = R.CASES + [(4, 3, 32, 32, 30, 33), (5, 5, 512, 512, 62, 61)]
REPORT_KEYS = {"iteration", "source", "patches", "terms", "worst", "flags"}
LAYER_KEYS = {"format", "elements", "zero", "subnormal", "at_max", "nonfinite", "exp_hist", "gate_on", "gate_flips", "feat_gap"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import npp_amd
    npp_amd.lib()
    return torch.device("cuda:0")


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float(torch.linalg.vector_norm(a - b) / torch.linalg.vector_norm(b))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_device_census_equals_the_host_twin_and_the_restatement(dev, case):
    """Planted tensors (tests/trunk_census_restatement.py: +-0, subnormals, +-65504, +-infinity, NaN, negatives, sign disagreements
    with the partner, every uncounted code poisoned): the launch's record equals the plain C++ twin word for word and the NumPy
    restatement field for field, with and without the fp32 partner, on the default stream and on another one; the guard words
    around the record come back intact."""
    from npp_amd import ops
    from npp_amd._lib import TRUNK_CENSUS_WORDS as words
    flat, ref, _ = R.planted(case, seed=11)
    act = torch.from_numpy(flat.view(np.int16)).to(dev)
    ref_d = torch.from_numpy(ref).to(dev)
    side = torch.cuda.Stream(dev)
    for with_ref in (False, True):
        want = ops.trunk16_census_host(flat, *case, ref32=ref if with_ref else None)
        restated = R.census(flat, *case, ref32=ref if with_ref else None)
        for stream in (None, side):
            buf = torch.full((words + 16,), GUARD, dtype=torch.int64, device=dev)
            if stream is None:
                ops.trunk16_census(act, *case, ref32=ref_d if with_ref else None, record=buf[8:8 + words])
            else:
                stream.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(stream):
                    ops.trunk16_census(act, *case, ref32=ref_d if with_ref else None, record=buf[8:8 + words])
                torch.cuda.current_stream(dev).wait_stream(stream)
            got = buf.cpu().numpy()
            assert (got[:8] == GUARD).all() and (got[8 + words:] == GUARD).all()
            np.testing.assert_array_equal(got[8:8 + words], want)
            dec = ops.trunk16_census_decode(got[8:8 + words])
            for f in KEYS:
                assert dec[f] == restated[f], (f, with_ref)
    assert dec["gate_flips"] > 0 and dec["at_max"] > 0 and dec["nonfinite"] > 0 and dec["subnormal"] > 0


def _torch_count(exp16, exp32=None):
    """The census of an exported layer (fp32 values that are exactly the fp16 ones), counted in torch from the fp16 bit patterns."""
    a = exp16.half().contiguous().view(torch.int16).to(torch.int32) & 0x7FFF
    e = a >> 10
    fin = e != 31
    out = {"elements": a.numel(), "zero": int((a == 0).sum()), "subnormal": int(((e == 0) & (a != 0)).sum()),
           "at_max": int((a == 0x7BFF).sum()), "nonfinite": int((~fin).sum()),
           "exp_hist": [int(((e == b) & fin).sum()) for b in range(32)], "gate_on": 0, "gate_flips": 0}
    if exp32 is not None:
        out["gate_on"] = int((exp16 > 0).sum())
        out["gate_flips"] = int(((exp16 > 0) != (exp32 > 0)).sum())
    return out


@pytest.mark.parametrize("scale", [1.0, 1e6], ids=["scale1", "scale1e6"])
def test_trunk_census_after_a_real_forward(dev, scale):
    """VGG19[0:18] with fixed-seed random weights on a 2 x 3 x 16 x 16 input (maps 16, 8 and 4 wide), at scale 1 and at 1e6 -- there
    the input itself exceeds 65504, so the fp16 input holds infinities and the layers behind it saturate.  Every layer's counts
    equal an independent count in torch on ops.trunk_export of that layer, gate_flips equals the torch count on the two trunks'
    tensors, and "saturated" is set exactly when the independent count of 65504 / non-finite values is non-zero."""
    from npp_amd import ops
    from npp_amd.losses import HipTrunk, HipTrunk32, _VGG19
    t16 = HipTrunk(_VGG19, taps=(17,), device=dev)
    t32 = HipTrunk32(_VGG19, taps=(17,), device=dev)
    x = (torch.rand((2, 3, 16, 16), generator=torch.Generator().manual_seed(3)) * scale).to(dev)
    ones, zeros = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)
    t16._forward(x, ones, zeros)
    t32._forward(x, ones, zeros)
    plain = t16.census()
    cen = t16.census(ref=t32)
    names = t16.layer_names()
    assert names == ["relu1_1", "relu1_2", "pool1", "relu2_1", "relu2_2", "pool2", "relu3_1", "relu3_2", "relu3_3", "relu3_4"]
    assert list(cen) == ["x0"] + names == list(plain)
    x0 = ops.trunk_export(t16._x0[0], 2, 2, 16, 16, 16, is_f16=True)[:, :3]
    want = {"x0": _torch_count(x0)}
    for j, (y, c, H, W) in enumerate(t16._geom):
        want[names[j]] = _torch_count(ops.trunk_export(y, 2, 2, c, H, W, is_f16=True), t32._acts[j])
    sat = 0
    for name, w in want.items():
        for f in KEYS:
            assert cen[name][f] == w[f], (name, f, cen[name][f], w[f])
            if f not in ("gate_on", "gate_flips"):
                assert plain[name][f] == w[f], (name, f)
        assert plain[name]["gate_on"] == plain[name]["gate_flips"] == 0
        sat += w["at_max"] + w["nonfinite"]
    print(f"scale {scale:g}: at_max + nonfinite {sat}, flips " + ", ".join(f"{n} {cen[n]['gate_flips']}/{cen[n]['elements']}" for n in names))
    assert ops.trunk_census_flags(cen) == (["saturated"] if sat > 0 else [])
    assert want["relu1_1"]["elements"] == 2 * 64 * 16 * 16 and want["pool2"]["elements"] == 2 * 128 * 4 * 4 and want["x0"]["elements"] == 2 * 3 * 256
    if scale > 65504:                                         # (the input's own values are out of fp16's range: reasoned, not measured)
        assert want["x0"]["at_max"] + want["x0"]["nonfinite"] > 0


def _fit(dev, graph, **kw):
    from npp_amd import synthetic as S
    from npp_amd.fit import CompletionFit
    H, K = 128, 3
    img, mask = S.synthetic_image(H)
    angles, periods, shifts = S.synthetic_periodicity(H, K)
    kw.setdefault("seed", 0)
    return CompletionFit(img, mask, angles, periods, S.SEED0_FREQS, S.init_params(K, seed=0), device=dev, N_rand=1024, shifts=shifts,
                         patch_size=64, patch_num=2, num_real_patch_per_sample=3, graph_iteration=graph, **kw)


def _same(a, b, path="state"):
    if isinstance(a, torch.Tensor):
        assert torch.equal(a, b), path
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b), path
    elif isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            _same(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{path}[{i}]")
    else:
        assert a == b, (path, a, b)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32).tolist()


def _same_fit(a, b):
    torch.cuda.synchronize()
    _same(a.state_dict(), b.state_dict())
    assert a.psnr("known") == b.psnr("known") and a.psnr("unknown") == b.psnr("unknown")
    rows = a.i_all_dev[:64 * a.W]
    assert torch.equal(a.net.render(rows), b.net.render(rows))


def _run_pair(aud, ref, n):
    sources = []
    for i in range(1, n + 1):
        assert aud.step_full() and ref.step_full(), i
        assert aud.last_source == ref.last_source, i
        assert _bits(aud.net.loss_buf) == _bits(ref.net.loss_buf), (i, aud.last_source)
        assert _bits(aud.last_patch_loss) == _bits(ref.last_patch_loss), (i, aud.last_source)
        sources.append(aud.last_source)
    return sources


def _check_report(r, terms, nk):
    assert set(r) == REPORT_KEYS and set(r["terms"]) == set(terms) and r["patches"] == nk
    sat = 0
    for name, t in r["terms"].items():
        assert set(t) == {"dx_gap", "layers", "worst_layer"}
        assert np.isfinite(t["dx_gap"]) and t["dx_gap"] > 0, (name, t["dx_gap"])
        shares = {}
        for ln, L in t["layers"].items():
            assert set(L) == LAYER_KEYS, (name, ln)
            h = L["exp_hist"]
            assert L["elements"] == L["zero"] + L["subnormal"] + sum(h[1:31]) + L["nonfinite"] and L["elements"] % nk == 0
            sat += L["at_max"] + L["nonfinite"]
            if ln != "x0":
                assert np.isfinite(L["feat_gap"]) and 0 <= L["gate_flips"] <= L["elements"] and 0 < L["gate_on"]
                shares[ln] = L["gate_flips"] / L["elements"]
        assert t["worst_layer"] in shares and shares[t["worst_layer"]] == max(shares.values())
    assert r["worst"][0] in r["terms"] and r["worst"][1] == max(t["dx_gap"] for t in r["terms"].values())
    assert r["flags"] == (["saturated"] if sat > 0 else [])


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_audited_fit_ends_with_the_bits_of_an_unaudited_one(dev, graph):
    """128^2 lattice (K = 3, W = 256, N_rand = 1024, patch 64, patch_num 2, 3 real patches, random fixed-seed trunks), 8 iterations
    of trunk_audit=2 against an unaudited twin of seed 0: every iteration's loss words, then state_dict(), psnr() and a 64-row
    render are bit-equal.  The 8 draws of seed 0, counted on the CPU (GridPatchSampler.draw on host tensors with the reference
    stream): train, train, same, val, val, same, same, val, none skipped, k = 3 / 1 for 'same' -- so the audited iterations are
    2 (train), 4 (val), 6 (same: contextual + LPIPS) and 8 (val).  Graph mode: the audited iterations count under "eager".
    dx_gap of the last audit equals rel_l2 recomputed here with a ContextualLoss(trunk_precision="fp32") of the test's own on the
    audit's batch, to 1e-12 relative (float64 norms of the same fp32 tensors; the summation order is the only freedom)."""
    from npp_amd.losses import ContextualLoss
    aud, ref = _fit(dev, graph, trunk_audit=2), _fit(dev, graph)
    sources = _run_pair(aud, ref, 8)
    assert sources == ["train", "train", "same", "val", "val", "same", "same", "val"]
    _same_fit(aud, ref)
    reps = list(aud.trunk_audits)
    assert [r["iteration"] for r in reps] == [2, 4, 6, 8] and aud.last_trunk_audit is reps[-1]
    assert ref.last_trunk_audit is None and len(ref.trunk_audits) == 0
    assert [r["source"] for r in reps] == ["train", "val", "same", "val"]
    for r in reps:
        same = r["source"] == "same"
        _check_report(r, ("contextual", "lpips") if same else ("contextual",), 2 * (1 if same else 3))
        print(f"it {r['iteration']} {r['source']}: " + ", ".join(
            f"{n} dx_gap {t['dx_gap']:.3e} worst {t['worst_layer']} {t['layers'][t['worst_layer']]['gate_flips']}/{t['layers'][t['worst_layer']]['elements']}"
            for n, t in r["terms"].items()) + f" flags {r['flags']}")
    lp_layers = list(reps[2]["terms"]["lpips"]["layers"])       # the flat input + 13 convolution layers + 4 pools of VGG16
    assert lp_layers[0] == "x0" and lp_layers[-1] == "relu5_3" and len(lp_layers) == 18 and "pool4" in lp_layers
    assert list(reps[0]["terms"]["contextual"]["layers"])[-10:] == ["relu1_1", "relu1_2", "pool1", "relu2_1", "relu2_2", "pool2", "relu3_1",
                                                                    "relu3_2", "relu3_3", "relu3_4"]
    if graph:
        st, rs = aud.graph_stats, ref.graph_stats
        assert st["eager"] >= 4 and st["eager"] + st["replayed"] == 8 and rs["eager"] + rs["replayed"] == 8
        assert st["eager"] >= rs["eager"]                     # (the four audited iterations ran launch by launch whatever their key's state)
    # the report's gap from public modules alone
    kept = aud.trunk_audit_tensors
    xy, nk = kept["xy"], reps[-1]["patches"]
    assert tuple(xy.shape) == (2 * nk, 3, 64, 64)
    buf = torch.zeros(1, dtype=torch.float32, device=dev)
    mine32 = ContextualLoss(use_vgg=True, device=dev, trunk_precision="fp32").to(dev).fused(xy, nk, aud.cx_w, buf)
    mine = rel_l2(kept["dx16"]["contextual"][:nk], mine32[:nk])
    got = reps[-1]["terms"]["contextual"]["dx_gap"]
    mine16 = ContextualLoss(use_vgg=True, device=dev).to(dev).fused(xy, nk, aud.cx_w, buf)
    print(f"dx_gap reported {got:.17g}, recomputed {mine:.17g}; a 16-bit pass of the test's own on the same batch: {rel_l2(mine16[:nk], mine32[:nk]):.17g}")
    assert abs(got - mine) <= 1e-12 * mine, (got, mine)
    # audit_trunk_next() arms one iteration of a fit that audits nothing by itself
    ref.audit_trunk_next()
    assert ref.step_full() and aud.step_full()
    assert len(ref.trunk_audits) == 1 and ref.last_trunk_audit["iteration"] == 9 and len(aud.trunk_audits) == 4
    assert ref.step_full() and aud.step_full()
    assert len(ref.trunk_audits) == 1 and len(aud.trunk_audits) == 5
    _same_fit(aud, ref)


def test_remapping_task_reports_the_style_term(dev):
    """task='remapping' with its style term (and LPIPS left on, so that a 'same' iteration adds the style gradient onto the LPIPS
    gradient in place): 4 iterations audited every time against an unaudited twin -- the style term is in every report, LPIPS
    exactly on the 'same' iterations, and the bits are unchanged.  Seed 2, counted on the CPU as in the test above (the sampler's
    mask is the clear region here): val, same, val, train."""
    from npp_amd import synthetic as S
    from npp_amd.fit import CompletionFit
    H, K = 128, 3
    img, _ = S.synthetic_image(H)
    angles, periods, shifts = S.synthetic_periodicity(H, K)
    clear = np.ones((H, H, 1), np.float32)
    clear[H // 3:H // 2] = 0.0

    def make(**kw):
        return CompletionFit(img, np.ones((H, H, 1), np.float32), angles, periods, S.SEED0_FREQS, S.init_params(K, seed=0), device=dev,
                             N_rand=1024, shifts=shifts, patch_size=64, patch_num=2, num_real_patch_per_sample=3, seed=2,
                             task="remapping", clear_mask=clear, contextual_weight=0.01, style_weight=1.0, **kw)
    aud, ref = make(trunk_audit=1), make()
    sources = _run_pair(aud, ref, 4)
    assert sources == ["val", "same", "val", "train"]
    _same_fit(aud, ref)
    reps = list(aud.trunk_audits)
    assert len(reps) == 4
    for r, src in zip(reps, sources):
        terms = ("contextual", "lpips", "style") if src == "same" else ("contextual", "style")
        _check_report(r, terms, r["patches"])
        assert list(r["terms"]["style"]["layers"])[-1] == "pool3" and "x0" in r["terms"]["style"]["layers"]
    print("sources " + str(sources) + "; style dx_gap " + ", ".join(f"{r['terms']['style']['dx_gap']:.3e}" for r in reps))


def test_both_audits_on_one_iteration(dev):
    """stash_audit=2 and trunk_audit=2: iterations 2 and 4 carry both reports, and the fit ends with the bits of an unaudited one."""
    aud, ref = _fit(dev, False, trunk_audit=2, stash_audit=2), _fit(dev, False)
    _run_pair(aud, ref, 4)
    _same_fit(aud, ref)
    assert [r["iteration"] for r in aud.trunk_audits] == [2, 4] == [r["iteration"] for r in aud.stash_audits]
    assert aud.last_stash_audit["worst"][1] > 0 and aud.last_trunk_audit["worst"][1] > 0


def test_refusals_on_the_device(dev):
    from npp_amd.losses import HipTrunk, _VGG16_STYLE
    from npp_amd.stack import StackedFit
    with pytest.raises(ValueError, match=r"trunk_precision='fp32'"):
        _fit(dev, False, trunk_audit=2, trunk_precision="fp32")
    with pytest.raises(ValueError, match=r"trunk_audit must be >= 0"):
        _fit(dev, False, trunk_audit=-1)
    with pytest.raises(ValueError, match=r"trunk_audit.*stacked fits"):
        StackedFit([_fit(dev, False, trunk_audit=2)])
    from npp_amd import synthetic as S
    from npp_amd.fit import CompletionFit
    img, mask = S.synthetic_image(128)
    angles, periods, _ = S.synthetic_periodicity(128, 3)
    with pytest.raises(ValueError, match=r"trunk_audit.*without patch losses"):
        CompletionFit(img, mask, angles, periods, S.SEED0_FREQS, S.init_params(3, seed=0), device=dev, N_rand=1024, trunk_audit=2)
    t = HipTrunk(_VGG16_STYLE, taps=(4, 9, 16), seed=777, device=dev)
    with pytest.raises(RuntimeError, match="no complete forward"):
        t.census()
    t._forward(torch.rand((2, 3, 16, 16), device=dev), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
    probe = torch.zeros(64, device=dev)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
            probe.add_(1.0)                                  # (something to record: the refusal below enqueues nothing)
            with pytest.raises(ValueError, match="stream capture"):
                t.census()
    torch.cuda.current_stream(dev).wait_stream(s)


def _cli(tmp_path, d, tag, extra):
    out = str(tmp_path / tag)
    r = subprocess.run([sys.executable, "-m", "npp_amd.train", "--datadir", d, "--basedir", out, "--p_topk", "3", "--N_iters", "6",
                        "--i_testset", "1000", "--i_print", "2", "--N_rand", "1024", "--random-trunks"] + extra,
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [re.sub(r"\([\d.]+ ms/iter", "(T ms/iter", ln).replace(out, "OUT") for ln in r.stdout.splitlines()]
    files = sorted(os.path.relpath(os.path.join(dp, f), out) for dp, _, fs in os.walk(out) for f in fs)
    return lines, files, out


def test_command_line_flag(dev, tmp_path):
    """python -m npp_amd.train in child processes on a temporary synthetic dataset: --audit_trunk 2 prints [TRUNK] lines and writes
    trunk_audit.json; the run without the flag prints the same lines (timings apart) minus the [TRUNK] ones and leaves the same
    files minus trunk_audit.json."""
    from npp_amd import io as nio, synthetic as S
    H, K = 128, 3
    img, mask = S.synthetic_image(H)
    a, p, s = S.synthetic_periodicity(H, K)
    d = nio.write_detected_dir(str(tmp_path / "detected" / "syn"), img, mask, np.ones_like(mask), a, p, s)
    plain, plain_files, _ = _cli(tmp_path, d, "plain", [])
    lines, files, out = _cli(tmp_path, d, "audited", ["--audit_trunk", "2"])
    trunk = [ln for ln in lines if ln.startswith("[TRUNK] ")]
    assert not any("TRUNK" in ln for ln in plain) and not any("trunk_audit" in f for f in plain_files)
    assert [ln for ln in lines if not ln.startswith("[TRUNK] ")] == plain
    rel = os.path.join("completion_top3", "syn", "trunk_audit.json")
    assert sorted(plain_files + [rel]) == files
    with open(os.path.join(out, rel)) as f:
        reps = json.load(f)
    assert "trunk_format" in reps[0] and "65504" in reps[0]["trunk_format"]["forward"]
    its = [r["iteration"] for r in reps[1:]]                   # (an even iteration the sampler skipped carries no audit)
    assert 1 <= len(its) == len(trunk) and set(its) <= {2, 4, 6}
    for r, ln in zip(reps[1:], trunk):
        assert set(r) == REPORT_KEYS
        assert re.fullmatch(rf"\[TRUNK\] it {r['iteration']} \({r['source']}, {r['patches']} patches\): worst gap {r['worst'][0]} "
                            r"\d\.\de[-+]\d\d, gate flips \d+\.\d\d % at (relu|pool)\w+, at_max \d+, nonfinite \d+( \[saturated\])?", ln), ln
