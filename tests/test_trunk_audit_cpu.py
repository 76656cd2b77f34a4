"""CPU checks of the trunk audit (include/npp_hip.h "trunk audit"): the census's plain C++ twin against a NumPy
restatement of the flat padded layout on planted tensors, the record's identity, the decode table, the command-line flag, the
refusals and the report's JSON form.  No GPU."""
import json

import numpy as np
import pytest

import trunk_census_restatement as R
from npp_amd import ops, train
from npp_amd._lib import CENSUS_FIELDS, CENSUS_BINS, TRUNK_CENSUS_GATE_FIELDS, TRUNK_CENSUS_WORDS, lib

KEYS = R.FIELDS + ("exp_hist", "gate_on", "gate_flips")


@pytest.mark.parametrize("case", R.CASES)
@pytest.mark.parametrize("with_ref", [False, True])
def test_host_twin_equals_the_numpy_restatement(case, with_ref):
    N_total, n, C, c_real, H, W = case
    flat, ref, counted = R.planted(case, seed=11)
    assert flat.nbytes == lib().npp_trunk_act_bytes(N_total, C, H, W)            # the restated size is the library's
    assert counted.sum() == n * c_real * H * W
    assert set(np.unique(flat[~counted])) == {0x7BFF, 0x7E00}                      # every uncounted code is poison
    want = R.census(flat, *case, ref32=ref if with_ref else None)
    rec = ops.trunk16_census_host(flat, *case, ref32=ref if with_ref else None)
    got = ops.trunk16_census_decode(rec)
    for f in KEYS:
        assert got[f] == want[f], (f, got[f], want[f])
    assert got["format"] == "fp16" and got["elements"] == n * c_real * H * W
    # the planted codes are there: +-0, subnormals, +-65504, +-infinity / NaN
    k = min(len(R.SPECIAL), got["elements"])
    sp = np.array(R.SPECIAL[:k]) & 0x7FFF
    assert got["zero"] >= (sp == 0).sum() > 0 and got["at_max"] >= (sp == 0x7BFF).sum() > 0
    assert got["subnormal"] >= ((sp >> 10 == 0) & (sp != 0)).sum() > 0 and got["nonfinite"] >= (sp >> 10 == 31).sum() > 0
    if with_ref:
        assert 0 < got["gate_flips"] < got["elements"] and 0 < got["gate_on"] < got["elements"]
        # fp16 +0 against a positive fp32 value is a flip: without it the count is one lower
        ref2 = ref.copy()
        c8, pos, j = R.index(*case)
        plus0 = flat.reshape(C // 8, -1, 8)[c8, pos, j] == 0x0000
        assert plus0.any()
        ref2[:n][plus0] = -0.25
        assert ops.trunk16_census_decode(ops.trunk16_census_host(flat, *case, ref32=ref2))["gate_flips"] == got["gate_flips"] - int(plus0.sum())
    else:
        assert got["gate_on"] == got["gate_flips"] == 0
    # the poison is uncounted: another filling of the same uncounted codes leaves the record as it is ...
    flat2 = flat.copy()
    flat2[~counted] = 0x3C00
    np.testing.assert_array_equal(ops.trunk16_census_host(flat2, *case, ref32=ref if with_ref else None), rec)
    # ... and a counted code is not: changing one moves the record
    flat2.reshape(-1)[np.flatnonzero(counted.reshape(-1))[0]] ^= 0x7FFF
    assert not np.array_equal(ops.trunk16_census_host(flat2, *case, ref32=ref if with_ref else None), rec)


@pytest.mark.parametrize("case", R.CASES)
def test_record_identity(case):
    flat, ref, _ = R.planted(case, seed=5)
    c = ops.trunk16_census_decode(ops.trunk16_census_host(flat, *case, ref32=ref))
    h = c["exp_hist"]
    assert c["elements"] == c["zero"] + c["subnormal"] + sum(h[1:31]) + c["nonfinite"]
    assert h[0] == c["zero"] + c["subnormal"] and h[31] == 0           # exponent field 31 is infinity / NaN: nonfinite
    assert 0 < c["at_max"] <= h[30]                                    # at_max lies inside bin 30


def test_decode_table_round_trips():
    assert ops.lib().npp_trunk16_census_words() == TRUNK_CENSUS_WORDS == len(CENSUS_FIELDS) + CENSUS_BINS + len(TRUNK_CENSUS_GATE_FIELDS)
    rec = np.arange(100, 100 + TRUNK_CENSUS_WORDS, dtype=np.int64)
    dec = ops.trunk16_census_decode(rec)
    assert [dec[f] for f in CENSUS_FIELDS] == [100, 101, 102, 103, 104]
    assert dec["exp_hist"] == list(range(105, 137)) and (dec["gate_on"], dec["gate_flips"]) == (137, 138)
    np.testing.assert_array_equal(ops.trunk16_census_encode(dec), rec)
    assert json.loads(json.dumps(dec)) == dec
    with pytest.raises(ValueError, match="int64 words"):
        ops.trunk16_census_decode(rec[:-1])


def test_census_refuses_bad_shapes():
    case = R.CASES[0]
    flat, ref, _ = R.planted(case, seed=1)
    N_total, n, C, c_real, H, W = case
    for bad in ((N_total, 0, C, c_real, H, W), (N_total, N_total + 1, C, c_real, H, W), (N_total, n, 24, c_real, H, W),
                (N_total, n, C, C + 1, H, W), (N_total, n, C, 0, H, W)):
        with pytest.raises(Exception, match="npp_trunk16_census_host|act: expected"):
            ops.trunk16_census_host(flat, *bad)
    with pytest.raises(ValueError, match="ref32"):
        ops.trunk16_census_host(flat, *case, ref32=ref[:, :, :-1])
    with pytest.raises(ValueError, match="act: expected"):
        ops.trunk16_census_host(flat.reshape(-1)[:-8], *case)


def test_audit_flag_parses_and_defaults_to_never():
    assert train.parse(["--datadir", "x"]).audit_trunk == 0
    assert train.parse(["--datadir", "x", "--audit_trunk", "25"]).audit_trunk == 25
    with pytest.raises(SystemExit):
        train.parse(["--datadir", "x", "--audit_trunk", "often"])


def test_refusals_name_their_switch():
    with pytest.raises(ValueError, match=r"trunk_precision='fp32'.*nothing 16-bit to audit"):
        ops.refuse_trunk_audit("fp32", capturing=False)
    with pytest.raises(SystemExit, match=r"--audit_trunk with --trunk_precision fp32"):
        train._plan(["--datadir", "x", "--audit_trunk", "2", "--trunk_precision", "fp32"])
    with pytest.raises(SystemExit, match=r"--audit_trunk N"):
        train._plan(["--datadir", "x", "--audit_trunk", "-1"])
    with pytest.raises(ValueError, match=r"trunk_audit.*stream capture"):
        ops.refuse_trunk_audit("fp16", capturing=True)
    with pytest.raises(ValueError, match=r"trunk_audit.*without patch losses \(shifts=None\)"):
        ops.refuse_trunk_audit("fp16", capturing=False, patch_losses=False)
    with pytest.raises(ValueError, match=r"trunk_audit.*stacked fits"):
        ops.refuse_trunk_audit("fp16", capturing=False, stacked=True)
    ops.refuse_trunk_audit("fp16", capturing=False)                    # the default configuration passes


def test_report_round_trips_through_json_and_prints_one_line():
    flat, ref, _ = R.planted(R.CASES[1], seed=5)
    cen = ops.trunk16_census_decode(ops.trunk16_census_host(flat, *R.CASES[1], ref32=ref))
    quiet = dict(cen, at_max=0, nonfinite=0, gate_flips=1)
    layers = {"relu1_1": dict(quiet, feat_gap=1e-3), "relu1_2": dict(cen, feat_gap=2.5e-3)}
    rep = {"iteration": 4, "source": "val", "patches": 12,
           "terms": {"contextual": {"dx_gap": 0.0811, "layers": layers, "worst_layer": "relu1_2"}},
           "worst": ["contextual", 0.0811], "flags": ["saturated"]}
    text = train.trunk_audit_dumps([rep, dict(rep, iteration=6, flags=[])], train.trunk_format())
    back = json.loads(text)
    assert "65504" in back[0]["trunk_format"]["forward"] and "bf16" in back[0]["trunk_format"]["gradients"]
    assert back[1] == rep and back[2]["iteration"] == 6 and back[2]["flags"] == []
    line = train.trunk_line(rep)
    share = 100.0 * cen["gate_flips"] / cen["elements"]
    assert line == (f"[TRUNK] it 4 (val, 12 patches): worst gap contextual 8.1e-02, gate flips {share:.2f} % at relu1_2, "
                    f"at_max {cen['at_max']}, nonfinite {cen['nonfinite']} [saturated]")


def test_closing_table_gains_a_trunk_gap_column(tmp_path, capsys):
    """npp_amd.run's closing table: a `trunk gap` column with --audit_trunk among the train arguments (worst gap over the fit's
    audits, * when one was flagged), next to `stash gap` when both audits ran, and no table at all without either flag."""
    import types
    from npp_amd import run
    for name, reps in (("one", [{"worst": ["contextual", 0.081], "flags": []}, {"worst": ["lpips", 0.03], "flags": ["saturated"]}]), ("two", [])):
        d = tmp_path / "completion_top1" / name
        d.mkdir(parents=True)
        (d / "trunk_audit.json").write_text(json.dumps([{"trunk_format": train.trunk_format()}] + reps))
        (d / "stash_audit.json").write_text(json.dumps([{"stash_format": {}}, {"worst": ["rgb_linear.bias", 0.05], "flags": []}]))
    args = types.SimpleNamespace(train_args="--audit_trunk 2", task="completion", basedir=str(tmp_path), p_topk=1)
    run.metrics_table(args, ["one", "two", "gone"])
    rows = capsys.readouterr().out.splitlines()
    assert rows[0].split() == ["image", "trunk", "gap"]
    assert rows[1].split() == ["one", "8.100e-02*"] and rows[2].split() == ["two", "n/a"] and rows[3].split() == ["gone", "-"]
    args.train_args = "--audit_stash 2 --audit_trunk 2"
    run.metrics_table(args, ["one"])
    rows = capsys.readouterr().out.splitlines()
    assert rows[0].split() == ["image", "stash", "gap", "trunk", "gap"] and rows[1].split() == ["one", "5.000e-02", "8.100e-02*"]
    args.train_args = "--audit_stash 2"
    run.metrics_table(args, ["one"])
    rows = capsys.readouterr().out.splitlines()
    assert rows[0] == f"{'image':<5}  {'stash gap':>12}" and rows[1] == f"{'one':<5}  {'5.000e-02':>12}"      # the form before this column existed
    args.train_args = ""
    run.metrics_table(args, ["one"])
    assert capsys.readouterr().out == ""
