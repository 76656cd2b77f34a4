"""The case table of the exact convolution sweep (tests/conv_cases.py) against the launcher's own plan (npp_conv3x3_plan: the struct
conv3x3_impl launches from, answered on the host) and against what the sweep has to cover; and the conditions under which equality
with a float64 convolution is the right assertion.  No GPU."""
import os

import numpy as np
import pytest

import npp_amd
from npp_amd import ops
from npp_amd._lib import NppError
import conv_cases as T

pytestmark = pytest.mark.skipif(bool(os.environ.get("NPP_CONV_TILE")), reason="NPP_CONV_TILE is set: every launch takes the forced tile")


@pytest.fixture
def tuned(request):
    """set the npp_tune values of a case; the values found at the start come back afterwards"""
    old = {k: ops.tune(k) for k in ("conv_win", "conv_wink", "conv_wstat")}
    request.addfinalizer(lambda: [ops.tune(k, v) for k, v in old.items()])

    def set_(t):
        for k, v in t.items():
            ops.tune(k, v)
    return set_


def plan_of(c, tuned, **over):
    tuned(over.pop("tune", c["tune"]))
    a = dict(N=c["N"], n=c["n"], H=c["H"], W=c["W"], cin=c["cin"], cout=c["cout"])
    a.update(over)
    return ops.conv3x3_plan(a["N"], a["n"], a["H"], a["W"], a["cin"], a["cout"], c["mode"], T.fold_of(c))


def form_of(p):
    return (p["family"], p["ct"], p["pt"], p["s"], p["npt"], p["wstat"])


def test_listed_forms_are_the_launcher_s(tuned):
    bad = []
    for c in T.all_cases():
        got = form_of(plan_of(c, tuned))
        if got != tuple(c["form"]):
            bad.append(f"{T.name(c)}: listed {c['form']}, the launcher takes {got}")
    assert not bad, "\n".join(bad)


def test_case_table_reaches_every_form_and_edge(tuned):
    seen = set()
    for c in T.all_cases():
        fam, ct, pt, s, npt, wstat = c["form"]
        km = T.MODES[T.kernel_mode(c)]
        if fam == "tile":
            seen.add(("tile", (ct, pt, s), km))
        elif fam == "win":
            seen.add(("win", km))
        else:
            seen.add(("wink", npt, km))
        if wstat:
            # the numbering, and a neighbour that just misses its condition: the same launch under the same settings with ONE more
            # image to read takes the natural numbering (the activations then outweigh half the pack; grid.y >= 8 still holds)
            side = "fwd" if km.startswith("fwd") else "grad"
            seen.add(("wstat", side))
            same = ("entry", "mode", "N", "H", "W", "cin", "cout", "tune")
            if any(all(o[k] == c[k] for k in same) and o["n"] == c["n"] + 1 and not o["form"][5] and plan_of(o, tuned)["grid_y"] >= 8
                   for o in T.all_cases()):
                seen.add(("wstat neighbour", side))
        if c["cin"] == 16:
            seen.add(("CI == 1", "image" if c.get("image") else "16 channels"))
        if c["n"] < c["N"]:
            seen.add(("n_run < N_total", "multiple of 512" if (c["n"] * (c["H"] + 2) * (c["W"] + 2)) % 512 == 0 else "not a multiple of 512"))
        if c["cout"] in (48, 96):
            seen.add(("Cout", c["cout"]))
        if c["W"] % 16:
            seen.add("W % 16 != 0")
        if c["H"] % 2:
            seen.add("odd H")
        if c["entry"] in ("pool", "dgrad_pool"):
            seen.add((c["entry"], "W", c["W"]))
        if c["entry"] == "pool" and (c["n"] * (c["H"] // 2) * ((c["W"] + 15) // 16)) % 2:
            seen.add("odd pool_tiles")
        if T.kernel_mode(c) in (0, 3):
            tap = c.get("tap")
            seen.add(("tap", "none") if not tap else ("tap", "Ctap < Cout" if tap[0] < c["cout"] and not tap[1] else "other"))
        if c.get("tap"):
            ctap, scale, y_null = c["tap"]
            if ctap == 3 and scale:
                seen.add(("tap", "Ctap = 3 scaled", T.MODES[T.kernel_mode(c)]))
            if y_null:
                seen.add(("tap", "d_y NULL"))
        if c["entry"] == "dgrad_pool":
            seen.add(("dgrad_pool", "addend" if c.get("addend") else "no addend"))
        if c.get("next_pack") and not wstat:          # (a weight-stationary launch drops the request: it would prove nothing)
            seen.add(("next_pack", fam))
            if fam == "tile":
                seen.add(("next_pack", "tile", "S > 1" if s > 1 else "S = 1"))
                seen.add(("next_pack", "tile", km))
        assert not (c.get("next_pack") and wstat), f"{T.name(c)}: d_next_pack is dropped by a weight-stationary launch"
        seen.add(("next_pack off", fam))
    want = [("tile", f, m) for f in T.TILE_FORMS for m in T.MODES]
    want += [("win", m) for m in T.MODES[:3]] + [("wink", npt, m) for npt in (1, 2) for m in T.MODES[:3]]
    want += [("wstat", "fwd"), ("wstat", "grad"), ("wstat neighbour", "fwd"), ("wstat neighbour", "grad")]
    want += [("CI == 1", "image"), ("n_run < N_total", "multiple of 512"), ("n_run < N_total", "not a multiple of 512")]
    want += [("Cout", 48), ("Cout", 96), "W % 16 != 0", "odd H", "odd pool_tiles"]
    want += [(e, "W", w) for e in ("pool", "dgrad_pool") for w in (2, 14, 16, 18)]
    want += [("tap", "none"), ("tap", "Ctap < Cout"), ("tap", "Ctap = 3 scaled", "fwd"), ("tap", "Ctap = 3 scaled", "dgrad_lin"), ("tap", "d_y NULL")]
    want += [("dgrad_pool", "addend"), ("dgrad_pool", "no addend")]
    want += [("next_pack", f) for f in ("tile", "win", "wink")] + [("next_pack off", f) for f in ("tile", "win", "wink")]
    want += [("next_pack", "tile", v) for v in ("S = 1", "S > 1", "fwd", "dgrad_mask", "fwd_pool", "dgrad_pool")]
    missing = [w for w in want if w not in seen]
    assert not missing, f"the case table does not reach: {missing}"
    big = [T.name(c) for c in T.all_cases() if T.run_range(c["n"], c["H"], c["W"]) > 8192]
    assert not big, f"more than 8192 rounded positions: {big}"


def test_launcher_rules_reach_the_tile_forms_by_shape_alone(tuned):
    """the shapes the launcher's rules give for each tile form with every window form switched off (no NPP_CONV_TILE)"""
    tuned(dict(conv_win=0, conv_wink=0, conv_wstat=0))
    for form, (cin, cout, pos) in {(2, 2, 1): (32, 512, 8192), (2, 2, 4): (64, 512, 2048), (2, 1, 4): (64, 512, 1024),
                                   (1, 1, 4): (64, 96, 1536), (1, 1, 8): (128, 32, 512), (1, 1, 1): (32, 32, 512)}.items():
        n = pos // 512                                               # 14 x 30 images: (14 + 2) (30 + 2) = 512 positions each
        p = ops.conv3x3_plan(n, n, 14, 30, cin, cout, 0, 0)
        assert (p["family"], p["ct"], p["pt"], p["s"]) == ("tile",) + form, (form, p)


def test_every_stored_value_is_an_exact_integer_and_no_sum_reaches_2_to_24():
    """Conditions on the INPUTS under which torch.equal against float64 is the right assertion (not tolerances): fp16 tensors hold
    integers |v| <= 2048, bf16 tensors |v| <= 256, every fp32 partial sum is bounded by sum |x| |w| < 2^24; and the cases are not
    degenerate: a quarter to three quarters of a forward case's pre-ReLU sums are positive, at most half of a gradient
    convolution's results are zero.  Of a data gradient + pool case that share is taken of the convolution's results, not of
    the launch's output: three of a window's four outputs are zero by construction (without the addend).  Its output is pinned
    otherwise: some routed values survive the pre-pool gate and some are gated to zero."""
    gated_somewhere = {"addend": 0, "no addend": 0}
    for c in T.all_cases():
        o, r = T.operands(c), T.reference(c)
        who = T.name(c)
        fwd = T.kernel_mode(c) in (0, 3)
        lim_in = T.F16_MAX_INT if fwd else T.BF16_MAX_INT
        for k, a in o.items():
            if k == "img":
                continue
            lim = T.F16_MAX_INT if k in ("mask", "xpre", "bias") else lim_in
            assert np.all(a == np.round(a)) and np.abs(a).max() <= lim, (who, k)
        if c.get("image") and fwd:
            s, b = np.array(T.IMG_SCALE, np.float32)[None, :, None, None], np.array(T.IMG_SHIFT, np.float32)[None, :, None, None]
            assert np.array_equal(o["img"] * s + b, o["x"]), who
        assert r["absmax_sum"] < 2 ** 24, who
        for k in ("y", "pool", "d", "dz"):
            if k in r:
                lim = T.F16_MAX_INT if fwd else T.BF16_MAX_INT
                assert np.all(r[k] == np.round(r[k])) and np.abs(r[k]).max() <= lim, (who, k, float(np.abs(r[k]).max()))
        if c.get("tap") and c["tap"][1]:
            assert all(np.log2(v) == np.round(np.log2(v)) for v in c["tap"][1]), who
        if fwd:
            share = float((r["pre"] > 0).mean())
            assert 0.25 <= share <= 0.75, (who, share)
        else:
            zeros = float((r["y" if "y" in r else "d"] == 0).mean())
            assert zeros <= 0.5, (who, zeros)
        if "xpre" in o:
            routed = r["routed"] != 0
            assert (routed & (o["xpre"] > 0)).any() and (r["dz"] != 0).any(), who
            gated = int((routed & (o["xpre"] <= 0)).sum())            # a window of four zeros, or an addend on a zero activation
            assert gated > 0 or (not c.get("addend") and routed.size < 4096), (who, gated)
            gated_somewhere["addend" if c.get("addend") else "no addend"] += gated
            # ties: some 2 x 2 window holds its maximum more than once
            x = o["xpre"]
            w4 = np.stack([x[:, :, 0::2, 0::2], x[:, :, 0::2, 1::2], x[:, :, 1::2, 0::2], x[:, :, 1::2, 1::2]])
            assert ((w4 == w4.max(0)).sum(0) > 1).mean() > 0.25, who
        if "mask" in o:
            assert (o["mask"] == 0).any() and (o["mask"] < 0).any(), who
    assert all(v > 0 for v in gated_somewhere.values()), gated_somewhere


def test_fused_pair_cases_keep_exact_integers_in_their_16_bit_intermediates():
    """the same conditions for the pair launches: the fp16 activation between conv a and conv b (it lives in LDS), both stored
    outputs, and the gated bf16 gradient between the two data gradients"""
    fwd = [(str(c), T.pair_fwd_operands(c)["x"], T.pair_fwd_reference(c)) for c in T.PAIR_FWD]
    o = T.patch_operands()
    for comp in (False, True):
        x = T.patch_composed(o, comp)
        fwd.append((f"patch comp={comp}", x, T.pair_fwd_reference_of(x, o)))
    for who, x, r in fwd:
        assert np.all(x == np.round(x)) and np.abs(x).max() <= T.F16_MAX_INT, who
        for k in ("ya", "yb", "pool"):
            assert np.all(r[k] == np.round(r[k])) and r[k].max() <= T.F16_MAX_INT, (who, k)
        assert r["absmax_sum"] < 2 ** 24, who
        for k in ("pre_a", "pre_b"):
            assert 0.25 <= float((r[k] > 0).mean()) <= 0.75, (who, k)
    for c in T.PAIR_DGRAD:
        o, r = T.pair_dgrad_operands(c), T.pair_dgrad_reference(c)
        assert all(np.all(a == np.round(a)) and np.abs(a).max() <= T.BF16_MAX_INT for a in o.values()), c
        assert np.all(r["mid"] == np.round(r["mid"])) and np.abs(r["mid"]).max() <= T.BF16_MAX_INT, c
        assert (o["ya"] == 0).any() and (o["ya"] < 0).any() and r["absmax_sum"] < 2 ** 24, c
        assert float((r["dimg"] == 0).mean()) <= 0.5, c


def test_query_errors_are_the_launcher_s():
    """bad mode, n_run > N_total, channels not a multiple of 16, W > 1021, ...: the query and the launcher of the same fold, given the
    same bad arguments (the launcher with non-null pointers: it returns before it would launch), return the same code"""
    L = npp_amd.lib()
    import ctypes as C
    out = (C.c_int32 * len(ops.CONV_PLAN_FIELDS))()
    p = C.c_void_p(64)                                                  # never dereferenced: the argument checks come first

    def launcher(a):
        g = (a["N"], a["n"], a["H"], a["W"], a["cin"], a["cout"])
        if a["fold"] == 1:
            return L.npp_conv3x3_pool(p, *g, p, p, p, p, None, 0, None, None, 0, None)
        if a["fold"] == 2:
            return L.npp_conv3x3_dgrad_pool(p, *g, p, p, None, p, None, 0, None)
        return L.npp_conv3x3(p, *g, p, p, a["mode"], p, p, None, 0, None, None)

    ok = dict(N=2, n=2, H=8, W=8, cin=32, cout=32, mode=0, fold=0)
    assert L.npp_conv3x3_plan(*ok.values(), out) == 0
    ERR_ARG = L.npp_conv3x3(None, 2, 2, 8, 8, 32, 32, None, None, 0, None, None, None, 0, None, None)      # null pointers: NPP_ERR_ARG
    assert ERR_ARG < 0
    for bad in (dict(mode=3), dict(mode=-1), dict(n=3), dict(n=0), dict(cin=24), dict(cout=40), dict(cin=528), dict(cout=8), dict(W=1022),
                dict(H=0), dict(N=0, n=0), dict(fold=1, H=7), dict(fold=1, n=3), dict(fold=1, cout=40), dict(fold=2, mode=2, cin=24),
                dict(fold=2, mode=2, n=3), dict(fold=2, mode=2, W=511)):
        a = dict(ok)
        a.update(bad)
        assert L.npp_conv3x3_plan(*a.values(), out) == ERR_ARG, bad
        assert launcher(a) == ERR_ARG, bad
        with pytest.raises(NppError):
            ops.conv3x3_plan(a["N"], a["n"], a["H"], a["W"], a["cin"], a["cout"], a["mode"], a["fold"])
    for bad in (dict(fold=3), dict(fold=-1), dict(fold=1, mode=1), dict(fold=2, mode=0)):        # the query's own arguments
        a = dict(ok)
        a.update(bad)
        assert L.npp_conv3x3_plan(*a.values(), out) == ERR_ARG, bad
    assert L.npp_conv3x3_plan(1, 1, 8, 1021, 32, 32, 0, 0, out) == 0
