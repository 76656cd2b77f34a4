"""CPU checks of the stash audit (include/npp_hip.h "stash audit"): the census's plain C++ twin against a NumPy
restatement of the W8 addressing, the record's identities, the command-line flag, the refusals and the report's JSON form.  No GPU."""
import json

import numpy as np
import pytest

import stash_census_restatement as R
from npp_amd import ops, train
from npp_amd._lib import census_layout, CENSUS_FIELDS, CENSUS_BINS, CENSUS_TILE_FIELDS

BP, N_ROWS = 128, 100          # two 64-row tiles, the second ragged (36 real rows)
CASES = [(1, 256), (3, 256), (1, 512), (3, 512)]


def _buffers(K, W, seed):
    """Uniformly random bytes in both workspace arrays (all 256 codes, every counter class), then every byte the census must NOT
    count -- rows >= N_ROWS, unused embedding slots, unused rgb features, arrays this K does not write, the 16-bit region, scale
    words of tiles without a real row -- poisoned with 0x7F (actF: NaN) / 0x7B (dzF: the largest finite code)."""
    sizes = ops.train_workspace(K, BP, 1, W)
    rng = np.random.RandomState(seed)
    act = rng.randint(0, 256, sizes[1]).astype(np.uint8)
    dz = rng.randint(0, 256, sizes[2]).astype(np.uint8)
    _, _, used_a, used_d = R.census(act, dz, BP, N_ROWS, K, W)
    act[~used_a] = 0x7F
    dz[~used_d] = 0x7B
    return act, dz, used_a, used_d


@pytest.mark.parametrize("K,W", CASES)
def test_host_twin_equals_the_numpy_restatement(K, W):
    act, dz, used_a, used_d = _buffers(K, W, seed=7 * K + W)
    want, want_tiles, _, _ = R.census(act, dz, BP, N_ROWS, K, W)
    rec = ops.stash8_census_host(act, dz, BP, N_ROWS, K, W)
    got, got_tiles = ops.census_decode(rec, K, W)
    assert list(got) == [name for name, *_ in R.table(K, W)[0]]          # the same arrays, in memory order
    for name, w in want.items():
        g = got[name]
        assert g["format"] == w["format"], name
        for f in R.FIELDS + ("exp_hist",):
            assert g[f] == w[f], (name, f, g[f], w[f])
        if name != "dz_rgb":                                          # (its 300 random bytes need not reach every class)
            assert min(g[f] for f in R.FIELDS) > 0, (name, "random bytes reach every class")
    assert got_tiles == want_tiles
    # the expected element counts, from the shapes alone
    half = W // 2
    for name, g in got.items():
        feats = 3 if name == "dz_rgb" else (R.E if name.startswith("emb") else (half if name in ("a_p", "dz_p") else W))
        assert g["features"] == feats and g["elements"] == N_ROWS * feats, name
    # the poison is uncounted: another filling of the same uncounted bytes leaves the record as it is
    act2, dz2 = act.copy(), dz.copy()
    act2[~used_a] = 0x00
    dz2[~used_d] = 0xFF
    np.testing.assert_array_equal(ops.stash8_census_host(act2, dz2, BP, N_ROWS, K, W), rec)
    # ... and a counted byte is not: flipping one moves the record
    act2[np.flatnonzero(used_a)[0]] ^= 0x7F
    assert not np.array_equal(ops.stash8_census_host(act2, dz2, BP, N_ROWS, K, W), rec)


@pytest.mark.parametrize("K,W", CASES)
def test_record_identity_names_and_size(K, W):
    table, tile_off, words = census_layout(K, W)
    names = [n for n, *_ in table]
    assert len(set(names)) == len(names)
    entry = len(CENSUS_FIELDS) + CENSUS_BINS
    assert [off for *_, off in table] == [i * entry for i in range(len(table))]
    assert tile_off == len(table) * entry and words == tile_off + len(CENSUS_TILE_FIELDS)
    assert ("a_s" in names) == ("f2" in names) == ("dz_s" in names) == ("dz_f2" in names) == (K > 1)
    assert sum(n.startswith("emb") for n in names) == K
    act, dz, _, _ = _buffers(K, W, seed=3)
    rec = ops.stash8_census_host(act, dz, BP, N_ROWS, K, W)
    assert rec.shape == (words,)
    arrays, tiles = ops.census_decode(rec, K, W)
    for name, c in arrays.items():
        h = c["exp_hist"]
        assert c["elements"] == c["zero"] + c["subnormal"] + sum(h[1:]) + c["nonfinite"], name
        assert h[0] == c["zero"] + c["subnormal"], name
        top = 15 if c["format"] == "e4m3" else 30                     # at_max lies inside its bin
        assert (name == "dz_rgb" or 0 < c["at_max"]) and c["at_max"] <= h[top], name
        if c["format"] == "e4m3":
            assert sum(h[16:]) == 0, name
        else:
            assert h[31] == 0, name                                   # exponent field 31 of e5m2 is infinity / NaN: nonfinite
    assert tiles["tiles"] == 2 and 0 <= tiles["scale_min"] <= tiles["scale_max"] <= 255


def test_census_refuses_bad_shapes():
    act, dz, _, _ = _buffers(1, 256, seed=1)
    for bp, n in ((100, 50), (128, 0), (128, 129)):
        with pytest.raises(Exception, match="npp_stash8_census_host"):
            ops.stash8_census_host(act, dz, bp, n, 1, 256)


def test_embedding_slots_restated():
    cols = sorted(R.emb_real(ks, hh, j) for ks in range(30) for hh in range(2) for j in range(8) if R.emb_real(ks, hh, j) >= 0)
    assert cols == list(range(R.E))


def test_audit_flag_parses_and_defaults_to_never():
    assert train.parse(["--datadir", "x"]).audit_stash == 0
    assert train.parse(["--datadir", "x", "--audit_stash", "25"]).audit_stash == 25
    with pytest.raises(SystemExit):
        train.parse(["--datadir", "x", "--audit_stash", "often"])


def test_refusals_name_their_switch():
    with pytest.raises(ValueError, match=r"precision='fp32'"):
        ops.refuse_stash_audit("fp32", capturing=False)
    with pytest.raises(SystemExit, match=r"--audit_stash with --precision fp32"):
        train._plan(["--datadir", "x", "--audit_stash", "2", "--precision", "fp32"])
    with pytest.raises(SystemExit, match=r"--audit_stash N"):
        train._plan(["--datadir", "x", "--audit_stash", "-1"])
    old = ops.tune("stash8", 0)
    try:
        with pytest.raises(ValueError, match=r"stash8"):
            ops.refuse_stash_audit("bf16", capturing=False)
        with pytest.raises(SystemExit, match=r"stash8"):
            train._plan(["--datadir", "x", "--audit_stash", "2"])
    finally:
        ops.tune("stash8", old)
    with pytest.raises(ValueError, match=r"stream capture"):
        ops.refuse_stash_audit("bf16", capturing=True)
    ops.refuse_stash_audit("bf16", capturing=False)                    # the default configuration passes


def test_report_round_trips_through_json():
    act, dz, _, _ = _buffers(3, 256, seed=5)
    census, tiles = ops.census_decode(ops.stash8_census_host(act, dz, BP, N_ROWS, 3, 256), 3, 256)
    gap = {"periodic_linears.0.weight": 0.03125, "rgb_linear.bias": 1.5e-3}
    rep = {"iteration": 4, "source": "val", "rows": N_ROWS, "census": census, "tile_scale": tiles, "grad_gap": gap,
           "worst": ["periodic_linears.0.weight", 0.03125], "flags": ["saturated"]}
    text = train.stash_audit_dumps([rep, dict(rep, iteration=6, flags=[])], train.stash_format(256))
    back = json.loads(text)
    assert "e4m3" in back[0]["stash_format"]["layer_inputs"] and "e5m2" in back[0]["stash_format"]["pre_activation_gradients"]
    assert back[1] == rep and back[2]["iteration"] == 6 and back[2]["flags"] == []
    line = train.stash_line(rep)
    assert line.startswith("[STASH] it 4 ") and "worst gap periodic_linears.0.weight" in line and "[saturated]" in line
    assert f"tile scale 2^{tiles['scale_min'] - 127}..2^{tiles['scale_max'] - 127}" in line
