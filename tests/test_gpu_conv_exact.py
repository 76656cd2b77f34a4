"""The 16-bit trunk convolutions (csrc/npp_conv.hip, csrc/npp_conv_pair.hip) against a float64 convolution, EXACTLY, on every kernel form.

Operands are small integers (tests/conv_cases.py: the case table, pinned to the launcher by tests/test_conv_plan_cpu.py), so every
summation order, split, fold and fused pair has to produce the bits of the float64 result: every comparison below is torch.equal /
a raw-bit comparison (the one exception is the summation-error bound of the last test).  Operands enter through the public importers
(trunk_grad_in, conv_pack, trunk_image_in), results leave through trunk_export and the fp32 tap, AND every flat output is read back
whole as 16-bit codes: [C/8][nposp][8], position = guard + n (H+2)(W+2) + y (W+2) + x (include/npp_hip.h).

What a launch writes (read from the kernels; `range` = n_run (H+2)(W+2) rounded up to 512):
  npp_conv3x3 / _pf     every position p < range of every chunk: an interior position of an image that exists (p < N_total (H+2)(W+2))
                        gets its result -- ALSO in the images from n_run on that the rounded range happens to reach: the kernels know
                        the range, not n_run --, a border or tail position zero; the fp32 tap the same interior positions.  Guard units
                        and everything from `range` on keep what they held.
  npp_conv3x3_pool      interior positions of the images < n_run of y and of the pooled tensor; borders are not written.
  npp_conv3x3_dgrad_pool the 2 x 2 windows of the pooled interior positions p < range; the pre-pool tensor's borders are not written.
  trunk_grad_in         p < range: interior positions of images < n_run their value, every other position zero; accumulate: only
                        those interior positions.
Every output buffer is filled with a sentinel code first, so "keeps what it held" is checked, not assumed."""
import numpy as np
import pytest

import conv_cases as T

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import npp_amd
    npp_amd.lib()
    return torch.device("cuda:0")


@pytest.fixture
def tuned(request):
    """set npp_tune values; the values found at the start come back afterwards"""
    from npp_amd import ops
    old = {k: ops.tune(k) for k in ("conv_win", "conv_wink", "conv_wstat")}
    request.addfinalizer(lambda: [ops.tune(k, v) for k, v in old.items()])

    def set_(t):
        for k, v in t.items():
            ops.tune(k, v)
    return set_


# ---- buffers ------------------------------------------------------------------------------------------------------------------------
def sentinel_flat(N, C, H, W, dev):
    from npp_amd import ops
    nbytes = ops.trunk_alloc(N, C, H, W, "cpu").numel()
    assert nbytes == (C // 8) * T.nposp(N, H, W) * 16
    return torch.full((nbytes // 2,), T.SENTINEL, dtype=torch.int16, device=dev).view(torch.uint8)


def bits(buf, C, N, H, W):
    return buf.view(torch.int16).cpu().numpy().view(np.uint16).reshape(C // 8, T.nposp(N, H, W), 8)


def import_flat(a, f16, dev):
    """(N, C, H, W) fp32 NumPy -> flat fp16 / bf16 tensor through trunk_grad_in (every image: a valid convolution input)"""
    from npp_amd import ops
    N, C, H, W = a.shape
    buf = ops.trunk_alloc(N, C, H, W, dev)
    ops.trunk_grad_in(torch.from_numpy(a).to(dev), None, N, N, C, H, W, buf, as_f16=f16)
    return buf


def sentinel_tap(shape, dev):
    return torch.full(shape, T.TAP_SENTINEL, dtype=torch.float32, device=dev)


def interior_mask(written, N, H, W):
    """bool (N, H, W) from the flat positions a launch writes"""
    return written[:N * (H + 2) * (W + 2)].reshape(N, H + 2, W + 2)[:, 1:-1, 1:-1]


def assert_bits(who, what, got, want):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        c8, p, j = bad[0]
        raise AssertionError(f"{who}: {what}: {len(bad)} of {got.size} 16-bit units differ; first at chunk {c8}, unit {p} (position {p - T.GUARD}), "
                             f"element {j}: got 0x{got[c8, p, j]:04x}, want 0x{want[c8, p, j]:04x}")


def assert_equal(who, what, got, want):
    want = torch.from_numpy(np.ascontiguousarray(want)).to(torch.float32)          # the float64 reference cast once
    got = got.cpu()
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{who}: {what}: {len(bad)} of {got.numel()} values differ; first at {i}: got {float(got[i])}, want {float(want[i])}")


# ---- one case of the table -------------------------------------------------------------------------------------------------------------
def launch(c, dev, with_next_pack):
    """-> dict of raw outputs: y / pool / dz whole as 16-bit codes (NumPy), the fp32 tap and the trunk_export of each result (tensors)"""
    from npp_amd import ops
    o = T.operands(c)
    N, n, H, W, cin, cout = c["N"], c["n"], c["H"], c["W"], c["cin"], c["cout"]
    km = T.kernel_mode(c)
    fwd = km in (0, 3)
    pf, pb = ops.conv_pack(torch.from_numpy(o["w"]).to(dev), in_natural=bool(c.get("image")))
    pack = pf if fwd else pb
    nxt = pack.clone() if with_next_pack else None
    ctap, scale, y_null = c.get("tap") or (0, None, False)
    tap = sentinel_tap((N, ctap, H, W), dev) if ctap else None
    out = {}
    if fwd:
        if c.get("image"):
            x = ops.trunk_alloc(N, 16, H, W, dev)
            ops.trunk_image_in(torch.from_numpy(o["img"]).to(dev), T.IMG_SCALE, T.IMG_SHIFT, x)
        else:
            x = import_flat(o["x"], True, dev)
        bias = torch.from_numpy(o["bias"]).to(dev)
        y = None if y_null else sentinel_flat(N, cout, H, W, dev)
        if km == 0:
            ops.conv3x3(x, N, n, H, W, cin, cout, pack, bias, 0, None, y, tap, ctap, scale, next_pack=nxt)
        else:
            yp = sentinel_flat(N, cout, H // 2, W // 2, dev)
            ops.conv3x3_pool(x, N, n, H, W, cin, cout, pack, bias, y, yp, tap, ctap, scale, next_pack=nxt)
            out["pool"] = bits(yp, cout, N, H // 2, W // 2)
            out["pool_export"] = ops.trunk_export(yp, N, n, cout, H // 2, W // 2, is_f16=True)
    else:
        g = import_flat(o["g"], False, dev)
        if km == 4:
            xpre = import_flat(o["xpre"], True, dev)
            add = import_flat(o["addend"], False, dev) if "addend" in o else None
            dz = sentinel_flat(N, cout, 2 * H, 2 * W, dev)
            ops.conv3x3_dgrad_pool(g, N, n, H, W, cin, cout, pack, xpre, add, dz, next_pack=nxt)
            out["dz"] = bits(dz, cout, N, 2 * H, 2 * W)
            out["dz_export"] = ops.trunk_export(dz, N, N, cout, 2 * H, 2 * W)
            y = None
        else:
            mask = import_flat(o["mask"], True, dev) if km == 1 else None
            y = None if y_null else sentinel_flat(N, cout, H, W, dev)
            ops.conv3x3(g, N, n, H, W, cin, cout, pack, None, km, mask, y, tap, ctap, scale, next_pack=nxt)
    if y is not None:
        out["y"] = bits(y, cout, N, H, W)
        out["export"] = ops.trunk_export(y, N, n, cout, H, W, is_f16=fwd)
    if tap is not None:
        out["tap"] = tap
    torch.cuda.synchronize()
    return out


def check(c, out):
    who = T.name(c)
    r = T.reference(c)
    N, n, H, W, cout = c["N"], c["n"], c["H"], c["W"], c["cout"]
    km = T.kernel_mode(c)
    fwd = km in (0, 3)
    rng_ = T.run_range(n, H, W)
    ctap, scale, y_null = c.get("tap") or (0, None, False)
    if km == 4:
        wp, _ = T.written_positions(N, H, W, rng_, True)
        wpre = np.zeros((N, 2 * H + 2, 2 * W + 2), bool)
        wpre[:, 1:-1, 1:-1] = np.repeat(np.repeat(interior_mask(wp, N, H, W), 2, 1), 2, 2)
        written = np.zeros(T.npos_round(N, 2 * H, 2 * W), bool)
        written[:wpre.size] = wpre.reshape(-1)
        assert written.sum() == 4 * wp.sum()
        assert_bits(who, "pre-pool gradient, whole buffer", out["dz"], T.flat_expect(r["dz"], N, cout, 2 * H, 2 * W, written, False))
        full = wpre[:, 1:-1, 1:-1].reshape(N, -1).all(1)                      # images whose every window was routed
        assert_equal(who, "pre-pool gradient (trunk_export)", out["dz_export"].cpu()[torch.from_numpy(full)], r["dz"][full])
        return
    ref = r["y"]
    if ref.shape[1] < cout:                                                   # the image gradient: 3 real channels of 16
        ref = np.concatenate([ref, np.zeros((N, cout - ref.shape[1], H, W))], 1)
    written, _ = T.written_positions(N, H, W, rng_, km == 3, n if km == 3 else None)
    if not y_null:
        assert_bits(who, "flat output, whole buffer", out["y"], T.flat_expect(ref, N, cout, H, W, written, fwd))
        assert_equal(who, "trunk_export", out["export"], ref[:n])
    if ctap:
        m = interior_mask(T.written_positions(N, H, W, rng_, True, n if km == 3 else None)[0], N, H, W)
        s = np.array([(scale[co & 3] if scale else 1.0) for co in range(ctap)])[None, :, None, None]
        want = np.where(m[:, None], ref[:, :ctap] * s, T.TAP_SENTINEL)
        assert_equal(who, "fp32 tap", out["tap"], want)
    if km == 3:
        Ho, Wo = H // 2, W // 2
        wpool, _ = T.written_positions(N, Ho, Wo, T.npos_round(N, Ho, Wo), True, n)
        assert_bits(who, "pooled tensor, whole buffer", out["pool"], T.flat_expect(r["pool"], N, cout, Ho, Wo, wpool, True))
        assert_equal(who, "pooled tensor (trunk_export)", out["pool_export"], r["pool"][:n])


def run_cases(cases, dev, tuned):
    assert cases, "the table lists no case for this form"
    failures = []
    for c in cases:
        tuned(c["tune"])
        try:
            out = launch(c, dev, False)
            check(c, out)
            if c.get("next_pack"):                                            # the same launch requesting a pack into L2: equal bits
                again = launch(c, dev, True)
                for k, v in out.items():
                    same = torch.equal(v, again[k]) if torch.is_tensor(v) else np.array_equal(v, again[k])
                    assert same, f"{T.name(c)}: {k} differs with d_next_pack"
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, f"{len(failures)} of {len(cases)} cases differ from the float64 reference:\n" + "\n".join(failures)


@pytest.mark.parametrize("form", T.TILE_FORMS, ids=lambda f: "x".join(map(str, f)))
def test_tile_forms_equal_the_float64_convolution(dev, tuned, form):
    run_cases([c for c in T.all_cases() if c["form"][0] == "tile" and tuple(c["form"][1:4]) == form], dev, tuned)


def test_window_form_equals_the_float64_convolution(dev, tuned):
    run_cases([c for c in T.all_cases() if c["form"][0] == "win"], dev, tuned)


@pytest.mark.parametrize("npt", [1, 2])
def test_group_split_window_form_equals_the_float64_convolution(dev, tuned, npt):
    run_cases([c for c in T.all_cases() if c["form"][0] == "wink" and c["form"][4] == npt], dev, tuned)


# ---- the fused pair launches ------------------------------------------------------------------------------------------------------------
def _pair_inputs(o, first, dev):
    from npp_amd import ops
    if first:
        N, _, H, W = o["x"].shape
        x = ops.trunk_alloc(N, 16, H, W, dev)
        ops.trunk_image_in(torch.from_numpy(o["img"]).to(dev), T.IMG_SCALE, T.IMG_SHIFT, x)
    else:
        x = import_flat(o["x"], True, dev)
    pa, _ = ops.conv_pack(torch.from_numpy(o["wa"]).to(dev), in_natural=first)
    pb, _ = ops.conv_pack(torch.from_numpy(o["wb"]).to(dev))
    return x, pa, torch.from_numpy(o["ba"]).to(dev), pb, torch.from_numpy(o["bb"]).to(dev)


def _check_pair_outputs(who, r, N, n, n_keep, cmid, cout, H, W, ya, yb, yp, tap):
    keep, _ = T.written_positions(N, H, W, T.npos_round(N, H, W), True, min(n_keep, n))
    assert_bits(who, "y_a, whole buffer", bits(ya, cmid, N, H, W), T.flat_expect(r["ya"], N, cmid, H, W, keep, True))
    assert_bits(who, "y_b, whole buffer", bits(yb, cout, N, H, W), T.flat_expect(r["yb"], N, cout, H, W, keep, True))
    Ho, Wo = H // 2, W // 2
    wpool, _ = T.written_positions(N, Ho, Wo, T.npos_round(N, Ho, Wo), True, n)
    assert_bits(who, "y_pool, whole buffer", bits(yp, cout, N, Ho, Wo), T.flat_expect(r["pool"], N, cout, Ho, Wo, wpool, True))
    if tap is not None:
        m = np.arange(N) < n
        assert_equal(who, "tap_b", tap, np.where(m[:, None, None, None], r["yb"], T.TAP_SENTINEL))


@pytest.mark.parametrize("case", T.PAIR_FWD, ids=lambda c: f"{c[0]}to{c[1]}to{c[2]}-{c[3]}x{c[4]}")
def test_fused_pair_forward_equals_the_float64_chain(dev, case):
    """relu(conv a) -> relu(conv b) -> pool: y_a / y_b for the images < n_keep (interior only), the pooled tensor and the fp32 tap for
    the images < n_run; every other unit of the three flat outputs keeps its sentinel."""
    from npp_amd import ops
    cin, cmid, cout, H, W, N, n, _ = case
    assert ops.conv_pair_fwd_ok(H, W, cin, cmid, cout)
    o, r = T.pair_fwd_operands(case), T.pair_fwd_reference(case)
    for k in ("ya", "yb"):
        assert np.all(r[k] == np.round(r[k])) and r[k].max() <= T.F16_MAX_INT and r["absmax_sum"] < 2 ** 24
    x, pa, ba, pb, bb = _pair_inputs(o, cin == 16, dev)
    for n_keep, with_tap in ((0, True), (1, False), (n, True)):
        ya, yb, yp = sentinel_flat(N, cmid, H, W, dev), sentinel_flat(N, cout, H, W, dev), sentinel_flat(N, cout, H // 2, W // 2, dev)
        tap = sentinel_tap((N, cout, H, W), dev) if with_tap else None
        ops.conv_pair_fwd(x, N, n, n_keep, H, W, cin, cmid, cout, pa, ba, pb, bb, ya, yb, yp, tap)
        _check_pair_outputs(f"pair {case} n_keep={n_keep}", r, N, n, n_keep, cmid, cout, H, W, ya, yb, yp, tap)


@pytest.mark.parametrize("comp", [False, True])
def test_fused_pair_with_patch_plumbing_equals_the_pair_on_the_composed_input(dev, comp):
    """npp_conv_pair_fwd_patch (loss NULL) = npp_conv_pair_fwd on the batch [x | y] the crops compose: both against the float64 chain
    on that batch, integer crops, 0 / 1 masks, power-of-two scale and shift."""
    from npp_amd import ops
    n_p, k, P = T.PATCH["n_p"], T.PATCH["k"], T.PATCH["P"]
    N = 2 * n_p * k
    o = T.patch_operands()
    xin = T.patch_composed(o, comp)
    r = T.pair_fwd_reference_of(xin, o)
    assert np.all(xin == np.round(xin)) and np.all(r["yb"] == np.round(r["yb"])) and r["yb"].max() <= T.F16_MAX_INT
    pa, _ = ops.conv_pack(torch.from_numpy(o["wa"]).to(dev), in_natural=True)
    pb, _ = ops.conv_pack(torch.from_numpy(o["wb"]).to(dev))
    ba, bb = torch.from_numpy(o["ba"]).to(dev), torch.from_numpy(o["bb"]).to(dev)
    t = {key: torch.from_numpy(o[key]).to(dev) for key in ("pred", "fake", "fmask", "real", "rmask")}
    zero = torch.ones(4, dtype=torch.float32, device=dev)
    outs = []
    for fused in (True, False):
        ya, yb, yp = sentinel_flat(N, 64, P, P, dev), sentinel_flat(N, 64, P, P, dev), sentinel_flat(N, 64, P // 2, P // 2, dev)
        tap = sentinel_tap((N, 64, P, P), dev)
        if fused:
            ops.conv_pair_fwd_patch(t["pred"], t["fake"], t["fmask"], t["real"], t["rmask"], n_p, k, P, comp, T.PATCH["scale"], T.PATCH["shift"],
                                    zero, None, N, 64, 64, pa, ba, pb, bb, ya, yb, yp, tap)
            assert float(zero.abs().max()) == 0.0
        else:
            x0 = ops.trunk_alloc(N, 16, P, P, dev)
            ops.trunk_patch_in(t["pred"], t["fake"], t["fmask"], t["real"], t["rmask"], n_p, k, P, comp, T.PATCH["scale"], T.PATCH["shift"], x0)
            ops.conv_pair_fwd(x0, N, N, N, P, P, 16, 64, 64, pa, ba, pb, bb, ya, yb, yp, tap)
        _check_pair_outputs(f"patch pair comp={comp} fused={fused}", r, N, N, N, 64, 64, P, P, ya, yb, yp, tap)
        outs.append((ya.clone(), yb.clone(), yp.clone(), tap.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*outs))


@pytest.mark.parametrize("case", T.PAIR_DGRAD, ids=lambda c: f"{c[0]}x{c[1]}")
def test_fused_pair_data_gradient_equals_the_float64_chain(dev, case):
    """conv b's data gradient -> gate by y_a > 0 -> conv a's data gradient -> times scale; images from n_run on are untouched"""
    from npp_amd import ops
    H, W, N, n, _ = case
    assert ops.lib().npp_conv_pair_dgrad_ok(H, W, 64)
    o, r = T.pair_dgrad_operands(case), T.pair_dgrad_reference(case)
    assert np.all(r["mid"] == np.round(r["mid"])) and np.abs(r["mid"]).max() <= T.BF16_MAX_INT and r["absmax_sum"] < 2 ** 24
    _, pbb = ops.conv_pack(torch.from_numpy(o["wb"]).to(dev))
    _, pab = ops.conv_pack(torch.from_numpy(o["wa"]).to(dev), in_natural=True)
    dz, ya = import_flat(o["dz"], False, dev), import_flat(o["ya"], True, dev)
    dimg = sentinel_tap((N, 3, H, W), dev)
    ops.conv_pair_dgrad(dz, N, n, H, W, 64, pbb, ya, pab, dimg, T.GRAD_SCALE)
    m = np.arange(N) < n
    assert_equal(f"pair dgrad {case}", "d_dimg", dimg, np.where(m[:, None, None, None], r["dimg"], T.TAP_SENTINEL))


# ---- importers and exporters ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,H,W", [(48, 9, 13), (16, 9, 13), (48, 1, 1), (16, 1, 1)])
def test_importers_and_exporters_round_trip_exactly(dev, C, H, W):
    from npp_amd import ops
    N, n = 3, 2
    rng = np.random.RandomState(C + H)
    rng_ = T.run_range(n, H, W)
    for f16 in (True, False):
        for gated in (False, True):
            v = rng.randint(-9, 10, (n, C, H, W)).astype(np.float32)
            old = rng.randint(-9, 10, (N, C, H, W)).astype(np.float32)
            gate = rng.choice((-1, 0, 1, 2), (N, C, H, W)).astype(np.float32)
            gflat = import_flat(gate, True, dev) if gated else None
            want = np.where(gate[:n] > 0, v, 0.0) if gated else v
            who = f"trunk_grad_in C={C} {H}x{W} as_f16={f16} gate={gated}"
            # plain: every position below `range` is written (images from n_run on and all borders: zero), nothing from `range` on
            buf = sentinel_flat(N, C, H, W, dev)
            ops.trunk_grad_in(torch.from_numpy(v).to(dev), gflat, N, n, C, H, W, buf, as_f16=f16)
            full = np.zeros((N, C, H, W), np.float32)
            full[:n] = want
            written, _ = T.written_positions(N, H, W, rng_, False)
            assert_bits(who, "whole buffer", bits(buf, C, N, H, W), T.flat_expect(full, N, C, H, W, written, f16))
            assert_equal(who, "trunk_export", ops.trunk_export(buf, N, n, C, H, W, is_f16=f16), want)
            # accumulate onto a whole tensor: only the interior positions of the images < n_run change
            buf = sentinel_flat(N, C, H, W, dev)
            ops.trunk_grad_in(torch.from_numpy(old).to(dev), None, N, N, C, H, W, buf, as_f16=f16)
            all_pos, _ = T.written_positions(N, H, W, T.npos_round(N, H, W), False)
            base = T.flat_expect(old, N, C, H, W, all_pos, f16)
            assert_bits(who, "whole buffer before accumulate", bits(buf, C, N, H, W), base)
            ops.trunk_grad_in(torch.from_numpy(v).to(dev), gflat, N, n, C, H, W, buf, as_f16=f16, accumulate=True)
            acc = old.copy()
            acc[:n] += want
            inner, _ = T.written_positions(N, H, W, rng_, True, n)
            assert_bits(who, "whole buffer after accumulate", bits(buf, C, N, H, W), T.flat_expect(acc, N, C, H, W, inner, f16, base=base))
            assert_equal(who, "trunk_export after accumulate", ops.trunk_export(buf, N, N, C, H, W, is_f16=f16), acc)
    # the image importer: img * scale + shift into channels 0..2 of a 16-channel tensor, zero elsewhere, the whole rounded range
    if C == 16:
        x = rng.randint(0, 4, (N, 3, H, W)).astype(np.float32)
        s, b = np.array(T.IMG_SCALE, np.float32)[None, :, None, None], np.array(T.IMG_SHIFT, np.float32)[None, :, None, None]
        buf = sentinel_flat(N, 16, H, W, dev)
        ops.trunk_image_in(torch.from_numpy((x - b) / s).to(dev), T.IMG_SCALE, T.IMG_SHIFT, buf)
        full = np.zeros((N, 16, H, W), np.float32)
        full[:, :3] = x
        all_pos, _ = T.written_positions(N, H, W, T.npos_round(N, H, W), False)
        assert_bits("trunk_image_in", "whole buffer", bits(buf, 16, N, H, W), T.flat_expect(full, N, 16, H, W, all_pos, True))
        assert_equal("trunk_image_in", "trunk_export", ops.trunk_export(buf, N, N, 16, H, W, is_f16=True), full)


# ---- saturation -------------------------------------------------------------------------------------------------------------------------
def test_forward_saturates_at_65504_exactly(dev, tuned):
    """16 channels of 0 / 32 against weights of 32 (output channels 0..7) and 1 (8..15): sums of 1024 k; from k = 64 on they exceed the
    fp16 range and must be stored as exactly 65504, in the flat tensor and in the tap; below, 1024 k and 32 k are fp16 numbers."""
    from npp_amd import ops
    tuned(dict(conv_win=0, conv_wink=0, conv_wstat=0))
    N, H, W = 2, 9, 13
    rng = np.random.RandomState(7)
    x = (32 * (rng.rand(N, 16, H, W) < 0.6)).astype(np.float32)
    w = np.ones((16, 16, 3, 3), np.float32)
    w[:8] = 32
    bias = np.zeros(16, np.float32)
    t = lambda a: torch.from_numpy(a).double()
    exact = torch.nn.functional.conv2d(t(x), t(w), padding=1)
    want = exact.clamp(0, 65504).numpy()
    assert (exact > 65504).any() and (exact[:, :8] < 65504).any() and exact.max() < 2 ** 24
    pf, _ = ops.conv_pack(torch.from_numpy(w).to(dev))
    y, tap = sentinel_flat(N, 16, H, W, dev), sentinel_tap((N, 16, H, W), dev)
    ops.conv3x3(import_flat(x, True, dev), N, N, H, W, 16, 16, pf, torch.from_numpy(bias).to(dev), 0, None, y, tap, 16, None)
    assert_equal("saturation", "trunk_export", ops.trunk_export(y, N, N, 16, H, W, is_f16=True), want)
    assert_equal("saturation", "fp32 tap", tap, want)
    written, _ = T.written_positions(N, H, W, T.npos_round(N, H, W), False)
    assert_bits("saturation", "whole buffer", bits(y, 16, N, H, W), T.flat_expect(want, N, 16, H, W, written, True))


# ---- summation error of each family, through the fp32 tap ----------------------------------------------------------------------------------
SUM_CASES = [("tile S=1", (2, 2, 62, 62, 128, 512), (0, 0, 0), ("tile", 2, 2, 1, 0)),
             ("tile S=4", (1, 1, 40, 46, 128, 512), (0, 0, 0), ("tile", 2, 2, 4, 0)),
             ("tile S=8", (1, 1, 14, 30, 128, 32), (0, 0, 0), ("tile", 1, 1, 8, 0)),
             ("win", (2, 2, 15, 17, 128, 64), (2, 0, 0), ("win", 2, 8, 1, 0)),
             ("wink npt=1", (2, 2, 15, 17, 128, 64), (0, 2, 0), ("wink", 2, 4, 2, 1)),
             ("wink npt=2", (3, 3, 44, 44, 128, 512), (0, 2, 0), ("wink", 2, 8, 2, 2))]


@pytest.mark.parametrize("tag,shape,tune,form", SUM_CASES, ids=[s[0].replace(" ", "_") for s in SUM_CASES])
def test_summation_error_of_each_family_through_the_fp32_tap(dev, tuned, tag, shape, tune, form):
    """Gaussian operands rounded to fp16 beforehand, zero bias, the tap over all Cout channels (the unrounded accumulator after the
    ReLU): its largest distance from the float64 convolution of the same operands may be at most 4 x the distance of the CPU's
    float32 conv2d (only should that distance be zero: 1e-6 of the largest result instead) -- the margin tests/test_gpu_dense_gemm.py
    gives another summation order.  Cin = 128 throughout.  Measured on the MI355X (tap / fp32-CPU, largest absolute distance):
    tile S=1 3.5e-6 / 1.4e-6, S=4 8.1e-7 / 1.5e-6, S=8 5.0e-7 / 9.8e-7, win 1.6e-6 / 9.9e-7, wink npt=1 1.0e-6 / 9.8e-7,
    npt=2 1.4e-6 / 1.5e-6: the split forms sum shorter chains and sit below the CPU, the unsplit ones 1.6 - 2.5 x above it."""
    from npp_amd import ops
    N, n, H, W, cin, cout = shape
    tuned(T.tune_of(*tune))
    p = ops.conv3x3_plan(N, n, H, W, cin, cout, 0, 0)
    assert (p["family"], p["ct"], p["pt"], p["s"], p["npt"]) == form, p
    rng = np.random.RandomState(len(tag))
    x = torch.from_numpy(rng.randn(N, cin, H, W).astype(np.float32)).half().float()
    w = torch.from_numpy((rng.randn(cout, cin, 3, 3) / np.sqrt(9 * cin)).astype(np.float32)).half().float()
    F = torch.nn.functional
    r64 = torch.relu(F.conv2d(x.double(), w.double(), padding=1))
    r32 = torch.relu(F.conv2d(x, w, padding=1))
    pf, _ = ops.conv_pack(w.to(dev))
    tap = sentinel_tap((N, cout, H, W), dev)
    ops.conv3x3(import_flat(x.numpy(), True, dev), N, n, H, W, cin, cout, pf, torch.zeros(cout, device=dev), 0, None, None, tap, cout, None)
    d_gpu = float((tap.cpu().double() - r64).abs().max())
    d_cpu = float((r32.double() - r64).abs().max())
    lim = 4.0 * d_cpu if d_cpu > 0.0 else 1e-6 * float(r64.abs().max())      # the floor ONLY when the CPU distance is zero
    print(f"summation error, {tag} ({cin} -> {cout}, {N} x {H} x {W}): tap {d_gpu:.3g}  fp32-CPU {d_cpu:.3g}  bound {lim:.3g}")
    assert d_gpu <= lim, (tag, d_gpu, d_cpu, lim)
