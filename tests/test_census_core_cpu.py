"""CPU checks of what the two precision audits share (csrc/npp_census.h, npp_amd/audit.py; DESIGN.md section 6j "census core"): the
host twins of both censuses on inputs that hold every code of e4m3, e5m2 and fp16 against the NumPy restatements, the audit
schedule, and the closing table of npp_amd.run for the combinations of --eval_metrics and the audit flags.  No GPU."""
import json
import types

import census_every_code as E
import stash_census_restatement as RS
import trunk_census_restatement as RT
from npp_amd import ops, run
from npp_amd.audit import AuditSchedule


def test_stash_host_twin_counts_every_code():
    K, W, Bp, n_rows = (E.STASH[k] for k in ("K", "W", "Bp", "n_rows"))
    act, dz = E.stash_buffers(ops.train_workspace(K, Bp, 1, W))
    want, want_tiles, used_a, used_d = RS.census(act, dz, Bp, n_rows, K, W)
    assert set(act[used_a]) == set(dz[used_d]) == set(range(256))
    got, got_tiles = ops.census_decode(ops.stash8_census_host(act, dz, Bp, n_rows, K, W), K, W)
    assert list(got) == list(want)
    for name, w in want.items():
        for f in ("format",) + RS.FIELDS + ("exp_hist",):
            assert got[name][f] == w[f], (name, f, got[name][f], w[f])
        if name != "dz_rgb":                                          # (its 195 bytes cannot hold every code)
            top = 15 if w["format"] == "e4m3" else 30
            nonfinite = 2 if w["format"] == "e4m3" else 8             # +-NaN; +-infinity and three NaNs of either sign
            assert min(w[f] for f in RS.FIELDS) > 0 and all(w["exp_hist"][:top + 1]), name
            if w["elements"] % 256 == 0:                               # every code equally often
                assert w["nonfinite"] * 256 == nonfinite * w["elements"], name
    assert got_tiles == want_tiles == {"tiles": 2, "scale_min": 120, "scale_max": 131}


def test_trunk_host_twin_counts_every_code():
    flat, ref = E.trunk_tensor()
    for partner in (None, ref):
        want = RT.census(flat, *E.TRUNK, ref32=partner)
        got = ops.trunk16_census_decode(ops.trunk16_census_host(flat, *E.TRUNK, ref32=partner))
        for f in ("format",) + RT.FIELDS + ("exp_hist", "gate_on", "gate_flips"):
            assert got[f] == want[f], (f, got[f], want[f])
    # every code once: +-0, 2 x 1023 subnormals, +-65504, 2 x 1024 codes of exponent field 31, 2048 codes in each finite bin
    assert (got["elements"], got["zero"], got["subnormal"], got["at_max"], got["nonfinite"]) == (65536, 2, 2046, 2, 2048)
    assert got["exp_hist"] == [2048] * 31 + [0]
    assert got["gate_on"] == 32768 - 1 - 1023 and 0 < got["gate_flips"] < 65536      # positive, not +0, not a positive NaN


def test_audit_schedule():
    never = AuditSchedule(0, 4)
    assert not any(never.due(i) for i in range(10)) and never.last is None and len(never.reports) == 0
    third = AuditSchedule(3, 4)
    assert [i for i in range(8) if third.due(i)] == [0, 3, 6]
    never.arm()
    assert never.armed and never.due(1) and never.due(2)            # stays armed across an iteration that does not record
    rep = {"iteration": 2}
    assert never.record(rep) is rep and not never.armed and not never.due(3)
    assert never.last is rep and list(never.reports) == [rep]
    third.arm()
    assert third.due(1)
    third.record({"iteration": 1})
    assert not third.due(1) and third.due(3)                        # disarmed: the period alone decides again
    for i in range(2, 7):
        third.record({"iteration": i})
    assert [r["iteration"] for r in third.reports] == [3, 4, 5, 6] and third.last == {"iteration": 6}    # the oldest go first


METRICS = {"one": {"unknown": {"psnr": 27.125, "ssim": 0.91234, "lpips": 0.123456}},
           "two": {"unknown": {"psnr": 31.5, "ssim": None, "lpips": None}},
           "old": {"unknown": {"psnr": 9.0, "ssim": 0.5}}}
STASH = {"one": [{"worst": ["rgb_linear.bias", 0.05], "flags": []}, {"worst": ["a0.weight", 0.0125], "flags": ["saturated"]}], "two": [],
         "old": [{"worst": ["x", 1.5], "flags": []}]}
TRUNK = {"one": [{"worst": ["contextual", 0.081], "flags": []}], "two": [{"worst": ["lpips", 0.03], "flags": ["saturated"]}]}
NAMES = ["one", "two", "old", "a_long_gone_name"]
# the lines the parent of the change that merged run.metrics_table and run._table_with_stash printed for these files
TABLES = {
    "": [],
    "--eval_metrics": [
        "image             PSNR unknown  SSIM unknown",
        "one                   27.12 dB        0.9123",
        "two                   31.50 dB           n/a",
        "old                    9.00 dB        0.5000",
        "a_long_gone_name             -             -"],
    "--eval_metrics --eval_lpips vgg": [
        "image             PSNR unknown  SSIM unknown  LPIPS unknown",
        "one                   27.12 dB        0.9123         0.1235",
        "two                   31.50 dB           n/a            n/a",
        "old                    9.00 dB        0.5000            n/a",
        "a_long_gone_name             -             -              -"],
    "--eval_metrics --audit_stash 2 --audit_trunk 3": [
        "image             PSNR unknown  SSIM unknown     stash gap     trunk gap",
        "one                   27.12 dB        0.9123    5.000e-02*     8.100e-02",
        "two                   31.50 dB           n/a           n/a    3.000e-02*",
        "old                    9.00 dB        0.5000     1.500e+00             -",
        "a_long_gone_name             -             -             -             -"],
    "--eval_metrics --eval_lpips alex --audit_trunk 3": [
        "image             PSNR unknown  SSIM unknown  LPIPS unknown     trunk gap",
        "one                   27.12 dB        0.9123         0.1235     8.100e-02",
        "two                   31.50 dB           n/a            n/a    3.000e-02*",
        "old                    9.00 dB        0.5000            n/a             -",
        "a_long_gone_name             -             -              -             -"],
    "--audit_stash 2 --audit_trunk 3": [
        "image                stash gap     trunk gap",
        "one                 5.000e-02*     8.100e-02",
        "two                        n/a    3.000e-02*",
        "old                  1.500e+00             -",
        "a_long_gone_name             -             -"],
    "--eval_metrics --audit_stash 1": [
        "image             PSNR unknown  SSIM unknown     stash gap",
        "one                   27.12 dB        0.9123    5.000e-02*",
        "two                   31.50 dB           n/a           n/a",
        "old                    9.00 dB        0.5000     1.500e+00",
        "a_long_gone_name             -             -             -"],
}


def test_closing_table_for_every_combination_of_metrics_and_audits(tmp_path, capsys):
    """Hand-written metrics.json / stash_audit.json / trunk_audit.json of three fits (a fourth left nothing): a complete report, one
    with SSIM and LPIPS undefined and no stash report, one from before the LPIPS column without a trunk audit file."""
    for n in ("one", "two", "old"):
        d = tmp_path / "completion_top1" / n
        d.mkdir(parents=True)
        (d / "metrics.json").write_text(json.dumps(METRICS[n]))
        (d / "stash_audit.json").write_text(json.dumps([{"stash_format": {}}] + STASH[n]))
        if n in TRUNK:
            (d / "trunk_audit.json").write_text(json.dumps([{"trunk_format": {}}] + TRUNK[n]))
    for train_args, lines in TABLES.items():
        run.metrics_table(types.SimpleNamespace(train_args=train_args, task="completion", basedir=str(tmp_path), p_topk=1), NAMES)
        assert capsys.readouterr().out.splitlines() == lines, train_args
    run.metrics_table(types.SimpleNamespace(train_args="--eval_metrics --audit_stash 1", task="completion", basedir=str(tmp_path), p_topk=1), [])
    assert capsys.readouterr().out == ""
