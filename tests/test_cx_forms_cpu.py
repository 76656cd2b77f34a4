"""The tests of the tests of the contextual-loss core, on the CPU (no GPU, no HIP kernel): what tests/test_gpu_cx_forms.py is able
to detect with the case table, the reference and the bounds of tests/cx_reference.py.

  * coverage      the restated predicates of `cx_launch` over the table: every launch sequence and every kernel-internal path the
                  dispatch can produce occurs, and each case hits the form it names;
  * conditioning  a float64 comparison is only fair where arg-min and arg-max are stable in fp32: per case, from the reference alone;
  * noise scale   d32(case), printed, and K * d32 under the caps (1e-5 on the loss, 1e-4 relative L2 on the gradient);
  * defects       each named defect, applied to the float64 reference, moves loss or gradient by at least DETECT_FACTOR bounds.
"""
import numpy as np
import pytest
import torch

import cx_reference as R
from oracle.npp_torch_oracle import cx_loss_t

ALL = R.ALL_CASES
ids = lambda c: c.name      # noqa: E731


# ---- the restatement the defects are switched into IS the oracle ---------------------------------------------------------------
@pytest.mark.parametrize("name", ["fast_one_tile", "gen_hw63", "fast_weighted", "gen_bw0.1"])
def test_staged_restatement_equals_the_oracle_bit_for_bit(name):
    case = R.case_by_name(name)
    x, y, wt = R.inputs(case)
    out = []
    for fn in (cx_loss_t, R.cx_loss_staged):
        xt = torch.tensor(x).double().requires_grad_(True)
        loss = fn(xt, torch.tensor(y).double(), case.band_width, None if wt is None else torch.tensor(wt).double())
        loss.backward()
        out.append((loss.item(), xt.grad.numpy()))
    assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1])
    # and the grouped reference is what its definition says: independent cx_loss_t calls per group
    g = R.case_by_name("groups_gen_hw63")
    x, y, _ = R.inputs(g)
    losses, dx = R.reference(g)
    for m, (x0, nk) in enumerate(g.groups):
        if nk == 0:
            assert losses[m] == 0.0
            continue
        l1, d1 = R.cx_ref(x[x0:x0 + nk], y[x0:x0 + nk], g.band_width)
        assert l1[0] == losses[m] and np.array_equal(d1, dx[x0:x0 + nk])


# ---- coverage ------------------------------------------------------------------------------------------------------------------
def _runs():
    """Every (case, gradient wanted) the GPU test launches, with what the dispatch makes of it."""
    for c in ALL:
        N, C = c.shape[:2]
        for mode in c.modes:
            yield c, mode, R.dispatch(N, C, c.hw, mode == "grad", c.weighted)


def test_every_case_hits_the_form_it_names():
    for c, mode, d in _runs():
        want = c.form if mode == "grad" or c.value_form is None else c.value_form
        assert d["form"] == want, (c.name, mode, d)


def test_every_dispatch_outcome_occurs():
    runs = list(_runs())
    forms = {d["form"] for _, _, d in runs}
    assert forms == {"fast", "generic", "big-gradient", "big-value", "big-value-no-fit"}
    fast = [(c, m, d) for c, m, d in runs if d["fast"]]
    assert {d["loss_in_rows"] for _, _, d in fast} == {True, False}
    # loss_in_rows off for BOTH reasons: no gradient wanted, and weights with a gradient
    assert any(m == "value" for c, m, d in fast if not d["loss_in_rows"])
    assert any(m == "grad" and c.weighted for c, m, d in fast if not d["loss_in_rows"])
    assert {d["raised_lds"] for _, _, d in fast} == {True, False}
    # the generic form takes the same row pass (cx_rows_fwd32_kernel): gen_hw2047 over the default LDS limit, the small ones under
    generic = [(c, m, d) for c, m, d in runs if d["form"] == "generic"]
    assert {c.name for c, m, d in generic if d["raised_lds"]} == {"gen_hw2047"}
    assert {c.name for c, m, d in generic if not d["raised_lds"]} >= {"gen_hw2", "gen_hw63", "gen_hw65", "gen_hw120"}
    assert not any(d["raised_lds"] for _, _, d in runs if d["big"])
    assert not any(d["loss_in_rows"] for _, _, d in runs if not d["fast"])
    # cx_sim_kernel issues the row minima's atomicMin exactly where cx_rows_fwd_big_kernel follows it
    assert {d["form"] for _, _, d in runs if d["sim_atomic_min"]} == {"big-gradient", "big-value-no-fit"}
    for form in ("fast", "generic", "big-gradient"):                 # (the forms that run cx_sim_kernel on shapes of either kind)
        bodies = set().union(*[d["sim_bodies"] for _, _, d in runs if d["form"] == form])
        assert bodies == {"FULL", "non-FULL"}, (form, bodies)
    for form in ("generic", "big-gradient"):                         # (fast: hw % 32 == 0, always vector loads)
        assert {d["loads"] for _, _, d in runs if d["form"] == form} == {"vector", "scalar"}, form
    assert {d["chunks"] for _, _, d in runs} == {"one", "odd", "even"}
    assert {d["chunks"] for _, _, d in fast} == {"one", "odd", "even"}
    # weights on a fast, a generic and a big case; band widths other than 0.5 on a fast and a generic case
    assert {d["form"] for c, m, d in runs if c.weighted} >= {"fast", "generic", "big-gradient", "big-value"}
    for bw in (0.1, 1.0):
        assert {d["form"] for c, m, d in runs if c.band_width == bw} >= {"fast", "generic"}
    # groups on a fast and a generic shape, with an idle group that shares its x0 with the next, and NPP_MAX_STACK groups
    assert {d["form"] for c, m, d in runs if c.groups == R.GROUPS_7} == {"fast", "generic"}
    assert R.GROUPS_7[1][1] == 0 and R.GROUPS_7[1][0] == R.GROUPS_7[2][0] and sum(nk for _, nk in R.GROUPS_7) == 7
    assert len(R.GROUPS_16) == 16


def test_boundary_facts_by_arithmetic():
    # the block-parallel row pass takes 16 * hw * 4 bytes of dynamic LDS: 768 is the largest row at the 48 KiB default, 800 the
    # smallest multiple of 32 over it
    assert R.rows_lds_bytes(768) == 48 * 1024 and R.rows_lds_bytes(800) > 48 * 1024
    hw = {c.name: c.hw for c in ALL}
    assert hw["fast_hw768"] == 768 and hw["fast_hw800"] == 800
    assert not R.dispatch(1, 64, 768, True, False)["raised_lds"] and R.dispatch(1, 32, 800, True, False)["raised_lds"]
    # the same limit on the generic form: 767 under, 769 over; hw = 2047 needs 131 008 B, inside the limit the launch raises it to
    # (the widest row of the pass, 16 * 64 * kCxMaxCols * 4)
    assert not R.dispatch(1, 32, 767, True, False)["raised_lds"] and R.dispatch(1, 32, 769, True, False)["raised_lds"]
    assert R.dispatch(1, 32, 2047, True, False)["raised_lds"] and not R.dispatch(1, 32, 2049, True, False)["raised_lds"]
    assert R.rows_lds_bytes(2047) == 131008 <= R.CX_ROW_WAVES * 64 * R.CX_MAX_COLS * 4
    # the switch between the small and the big forms
    assert (hw["gen_hw2047"], hw["fast_hw2048"], hw["big_hw2049"], hw["big_hw2112"]) == (2047, 2048, 2049, 2112)
    assert [R.dispatch(1, 32, n, True, False)["form"] for n in (2047, 2048, 2049, 2112)] == ["generic", "fast", "big-gradient", "big-gradient"]
    assert 2112 % 32 == 0
    # big_fwd_fits at hw = 2049: C = 832 still fits, C = 864 is the smallest multiple of 32 that does not
    assert R.big_fwd_fits(1, 832, 2049) and not R.big_fwd_fits(1, 864, 2049)
    assert all(R.big_fwd_fits(1, C, 2049) for C in range(32, 864, 32))
    assert R.case_by_name("big_nofit_c864").shape == (1, 864, 3, 683)
    # the value-only big form at hw = 2049: 17 tiles of 128, one column in the last, 3 x 3 super-blocks of 8 x 8 tiles
    t = (2049 + 127) // 128
    assert t == 17 and 2049 - 16 * 128 == 1 and (t + 7) // 8 == 3
    # column chunks of the big row pass: 64 * 32 columns each, the second holds a single column
    assert 2049 - 64 * R.CX_MAX_COLS == 1
    # 9 logical blocks of cx_sim_kernel on a grid rounded up to 16
    c = R.case_by_name("fast_9_blocks")
    nb = c.shape[0] * ((c.hw + 63) // 64) ** 2
    assert nb == 9 and (nb + 7) // 8 * 8 == 16
    # hw = 2, 63, 65: below, at and across one 64-column tile
    assert (hw["gen_hw2"], hw["gen_hw63"], hw["gen_hw65"]) == (2, 63, 65)


# ---- conditioning --------------------------------------------------------------------------------------------------------------
# The one case that does NOT meet the clamp-edge condition, whatever the seed or the mix: at C = 864 and hw = 2049 (both are the
# point of the case) raw is 12 per unit dense at 0, some 95 entries lie within 1e-6 of it and together they carry 5.3e-5 of the
# gradient, 1.9 bounds.  They stay below the largest bound any case may have (GRAD_CAP), and few of them flip in practice: float32 on
# the CPU sits 3.5e-6 from float64 on this case (seeds 1 to 5: 3.2e-6 to 3.8e-6; seed 0: 1.4e-5), the kernels 1.13 times that.
EDGE_DENSE = ("big_nofit_c864",)


@pytest.mark.parametrize("case", ALL, ids=ids)
def test_conditioning(case):
    """No row whose two smallest D are closer than 1e-5 relative, no column whose two largest cx are closer than 1e-5 relative --
    over ALL rows and columns, nothing is left out.  Clamp edges: an entry of raw within 1e-6 of 0 or 1 may have its gate flipped by
    a correct fp32 evaluation.  On the small cases there is no such entry.  At hw >= 2047 and at C = 864 there always is: raw has a
    density of 2 to 12 per unit at 0, so of 4.2 M entries 10 to 100 fall inside the band whatever the seed.  What they carry is
    then measured: the part of dL/dx that flows (or would flow) through ALL of them together must stay below the case's gradient
    bound (the float32 error of raw is some 1e-7, a tenth of the band, so a correct kernel flips a few of them, not all)."""
    c = R.conditioning(case)
    _, bg = R.bounds(case)
    print(f"cx-cond  {case.name:18s} row gap {c['row_gap']:.2e} column gap {c['col_gap']:.2e} entries at a clamp edge {c['n_edge']:3d} "
          f"carrying {c['edge_grad']:.2e} of the gradient (bound {bg:.2e})")
    assert c["row_gap"] >= 1e-5
    assert c["col_gap"] >= 1e-5
    if case.hw < 2047 and case.shape[1] < 864:
        assert c["n_edge"] == 0
    if case.name in EDGE_DENSE:
        assert bg < c["edge_grad"] <= R.GRAD_CAP, "EDGE_DENSE is out of date"
    else:
        assert c["edge_grad"] <= bg


# ---- noise scale ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL, ids=ids)
def test_noise_scale_and_caps(case):
    dl, dg = R.d32(case)
    bl, bg = R.bounds(case)
    print(f"cx-d32   {case.name:18s} loss {dl:.3e} gradient {dg:.3e} -> bounds {bl:.3e} {bg:.3e}")
    assert 0 < dl and 0 < dg
    assert bl <= R.LOSS_CAP, f"K_LOSS * d32 = {bl:.3e} on the loss"
    assert bg <= R.GRAD_CAP, f"K_GRAD * d32 = {bg:.3e} on the gradient"


# ---- defect catalogue ----------------------------------------------------------------------------------------------------------
# (case, defect, mode) that the bounds do NOT separate by DETECT_FACTOR, with the case that covers the defect in that mode instead
NOT_SEPARATED = {
}


def test_scale_twice_is_linear():
    """Loss and gradient are linear in the scale: applying it twice moves both by exactly |scale - 1| relative, on every case; the
    catalogue below uses that instead of one more float64 evaluation per case."""
    case = R.case_by_name("gen_hw63")
    el, eg = R.defect_effect(case, "scale_twice", 1e-3)
    assert abs(el - 0.999) < 1e-12 and abs(eg - 0.999) < 1e-12
    assert R.defect_effect(case, "scale_twice", 1.0) == (0.0, 0.0)          # invisible at scale 1: hence the second scale everywhere


@pytest.mark.parametrize("case", ALL, ids=ids)
def test_defects_move_the_result_by_ten_bounds(case):
    """A run with a gradient sees loss and gradient: a defect counts as separated when EITHER moves by DETECT_FACTOR bounds (two of
    the defects leave the forward value alone).  A value-only run sees the loss alone, and only the defects that touch it."""
    bl, bg = R.bounds(case)
    missed = []
    for defect in R.applicable_defects(case, scale=1e-3):
        el, eg = (0.999, 0.999) if defect == "scale_twice" else R.defect_effect(case, defect)
        print(f"cx-defect {case.name:18s} {defect:14s} loss moves {el:.3e} = {el / bl:9.1f} bounds, gradient {eg:.3e} = {eg / bg:9.1f} bounds")
        for mode in case.modes:
            if mode == "value" and defect in R.GRADIENT_ONLY:
                continue
            sep = max(el / bl, eg / bg) if mode == "grad" else el / bl
            known = NOT_SEPARATED.get((case.name, defect, mode))
            if sep < R.DETECT_FACTOR and known is None:
                missed.append((defect, mode, round(sep, 2)))
            if known is not None:
                assert sep < R.DETECT_FACTOR, f"{defect} / {mode} is separated after all: drop it from NOT_SEPARATED"
                other = R.case_by_name(known)
                assert mode in other.modes and defect in R.applicable_defects(other, scale=1e-3)
                assert (other.name, defect, mode) not in NOT_SEPARATED
    assert not missed, f"{case.name}: not separated by {R.DETECT_FACTOR} bounds: {missed}"
