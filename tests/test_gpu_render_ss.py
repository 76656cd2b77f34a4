"""Supersampled renders on the GPU (npp_mlp_fwd_grid_ss / _view_ss and their fp32 forms, NPPNet.render_grid / render_view with
supersample=S): against the point-sampled launches, against render_at of the restatement's sample positions averaged on the CPU,
against the parent's dense grid launch (nesting), all bit for bit; the inside bytes, the chunking, the stores of a launch and the
render command's --supersample.  Fit 24 x 40, canvas 37 x 53 (no multiple of a tile), chunks that start mid-pixel-row."""
import re

import numpy as np
import pytest

import oracle
import render_ss_restatement as S
import view_restatement as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIT = (24, 40)
KW = [(1, 256), (3, 256), (1, 512), (3, 512)]
PRECISIONS = ("bf16", "fp32")
SSS = (2, 4, 8)
TOTAL = R.CANVAS[0] * R.CANVAS[1]
VIEWS = {"AFFINE": R.AFFINE, "PROJECTIVE": R.PROJECTIVE, "SS_HORIZON": S.SS_HORIZON}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import npp_amd
    npp_amd.lib()
    return torch.device("cuda:0")


_NETS = {}


def _net(dev, K, W, out_act=1):
    if (K, W, out_act) not in _NETS:
        from npp_amd.model import NPPNet
        angles, periods, _ = oracle.synthetic_periodicity(64, K)
        P = oracle.init_params(K, W=W, seed=7 * K + W)
        net = NPPNet(angles, periods, oracle.SEED0_FREQS, FIT, params=P, device=dev, ksplit=1, width=W)
        net.out_act = out_act
        _NETS[(K, W, out_act)] = net
    return _NETS[(K, W, out_act)]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ubits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. ss = 1 is the point-sampled launch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,W", KW)
def test_supersample_1_is_the_point_launch(dev, K, W):
    net = _net(dev, K, W)
    for prec in PRECISIONS:
        g = net.render_grid(R.CANVAS, origin=S.GRID_ORIGIN, scale=S.GRID_SCALE, precision=prec)
        g1 = net.render_grid(R.CANVAS, origin=S.GRID_ORIGIN, scale=S.GRID_SCALE, precision=prec, supersample=1)
        assert torch.equal(_bits(g1), _bits(g)), prec
        for name, M in VIEWS.items():
            v, vin = net.render_view(R.CANVAS, M, precision=prec, return_inside=True)
            v1, vin1 = net.render_view(R.CANVAS, M, precision=prec, return_inside=True, supersample=1)
            assert torch.equal(_bits(v1), _bits(v)) and torch.equal(vin1, vin), (prec, name)


# ---- 2. / 3. the launch is render_at of the rule's sample positions, averaged by the rule ------------------------------------------
@pytest.mark.parametrize("ss", SSS)
@pytest.mark.parametrize("out_act", [0, 1, 2])
def test_grid_equals_render_at_of_the_samples_averaged_on_the_cpu(dev, ss, out_act):
    net = _net(dev, 3, 256, out_act)
    yx = S.grid_samples(R.CANVAS, S.GRID_ORIGIN, S.GRID_SCALE, ss)
    for prec in PRECISIONS:
        at = net.render_at(torch.from_numpy(yx), precision=prec).cpu().numpy().reshape(TOTAL, ss * ss, 3)
        want, count = S.average(at)
        assert (count == ss * ss).all()
        got = net.render_grid(R.CANVAS, origin=S.GRID_ORIGIN, scale=S.GRID_SCALE, precision=prec, supersample=ss)
        assert got.shape == R.CANVAS + (3,) and got.dtype == torch.float32
        assert np.array_equal(_ubits(got.cpu().numpy().reshape(TOTAL, 3)), _ubits(want)), prec


@pytest.mark.parametrize("ss", SSS)
@pytest.mark.parametrize("out_act", [0, 1, 2])
@pytest.mark.parametrize("name", list(VIEWS))
def test_view_equals_render_at_of_the_samples_averaged_on_the_cpu(dev, ss, out_act, name):
    net = _net(dev, 3, 256, out_act)
    M = VIEWS[name]
    yx, counts, inside = S.view_samples(M, R.CANVAS, FIT, ss)
    _, centre = R.view_coords(M, R.CANVAS, FIT)
    c = counts.reshape(TOTAL, ss * ss)
    if name == "SS_HORIZON":                     # all three kinds of pixel occur: a changed constant cannot empty the case
        assert c.all(1).any() and (c.any(1) & ~c.all(1) & (centre != 0)).any() and (c.any(1) & (centre == 0)).any()
        assert not ((centre != 0) & ~c.any(1)).any()
    else:
        assert c.all()
    for prec in PRECISIONS:
        at = net.render_at(torch.from_numpy(yx), precision=prec).cpu().numpy().reshape(TOTAL, ss * ss, 3)
        want = S.pixel_colours(at, c, inside)
        got, gin = net.render_view(R.CANVAS, M, precision=prec, return_inside=True, supersample=ss)
        assert np.array_equal(gin.cpu().numpy().reshape(-1), inside), prec
        assert np.array_equal(_ubits(got.cpu().numpy().reshape(TOTAL, 3)), _ubits(want)), prec


# ---- 4. inside bytes do not depend on ss -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,W", KW)
def test_inside_bytes_are_those_of_the_point_launch(dev, K, W):
    net = _net(dev, K, W)
    for prec in PRECISIONS:
        for name, M in VIEWS.items():
            _, in1 = net.render_view(R.CANVAS, M, precision=prec, return_inside=True)
            assert (name == "SS_HORIZON") == bool((in1 == 0).any())
            for ss in SSS:
                out, ins = net.render_view(R.CANVAS, M, precision=prec, return_inside=True, supersample=ss)
                assert torch.equal(ins, in1), (prec, name, ss)
                assert bool((_bits(out)[ins == 0] == 0).all())                     # exactly +0.0
                assert bool(torch.isfinite(out).all())
                assert bool((out[ins != 0] != 0).any())


# ---- 5. nesting against the point-sampled dense grid: the offset convention, independently -----------------------------------------
def _block_mean(dense, Hc, Wc, ss):
    """The ordered ss x ss block mean of a (ss Hc, ss Wc, 3) canvas by the rule: sample a ss + b is dense pixel (ss i + a, ss j + b)."""
    o = dense.cpu().numpy().reshape(Hc, ss, Wc, ss, 3).transpose(0, 2, 1, 3, 4).reshape(Hc * Wc, ss * ss, 3)
    return S.average(o)[0]


@pytest.mark.parametrize("ss", SSS)
def test_nesting_positions_are_exact_and_equal(ss):
    Hc, Wc = R.CANVAS
    o = 1.0 / (2 * ss) - 0.5
    i, j = np.divmod(np.arange(ss * Hc * ss * Wc), ss * Wc)
    dense = np.stack([np.float32(o) + i.astype(np.float32) / np.float32(ss), np.float32(o) + j.astype(np.float32) / np.float32(ss)], 1)
    exact = np.stack([o + i / ss, o + j / ss], 1)                                    # float64: dyadic numbers, no rounding at this size
    assert np.array_equal(dense.astype(np.float64), exact)
    ours = S.grid_samples(R.CANVAS, (0.0, 0.0), (1.0, 1.0), ss).reshape(Hc, Wc, ss, ss, 2)
    ours = ours.transpose(0, 2, 1, 3, 4).reshape(-1, 2)                              # (i, a, j, b) = the dense canvas in row-major order
    assert np.array_equal(ours, dense.astype(np.float32))


@pytest.mark.parametrize("K,W", KW)
def test_supersampled_grid_is_the_block_mean_of_the_dense_point_grid(dev, K, W):
    net = _net(dev, K, W)
    Hc, Wc = R.CANVAS
    for prec in PRECISIONS:
        for ss in SSS:
            o = 1.0 / (2 * ss) - 0.5
            dense = net.render_grid((ss * Hc, ss * Wc), origin=(o, o), scale=float(ss), precision=prec)
            got = net.render_grid(R.CANVAS, precision=prec, supersample=ss)
            assert np.array_equal(_ubits(got.cpu().numpy().reshape(TOTAL, 3)), _ubits(_block_mean(dense, Hc, Wc, ss))), (prec, ss)


# ---- 6. power-of-two affine views are the grid launch ------------------------------------------------------------------------------
@pytest.mark.parametrize("K,W", KW)
def test_power_of_two_affine_views_are_the_supersampled_grid(dev, K, W):
    net = _net(dev, K, W)
    for prec in PRECISIONS:
        for ss in SSS:
            for sy, sx, y0, x0 in R.POW2_VIEWS:
                g = net.render_grid(R.CANVAS, origin=(y0, x0), scale=(sy, sx), precision=prec, supersample=ss)
                v, ins = net.render_view(R.CANVAS, R.affine(sy, sx, y0, x0), precision=prec, supersample=ss, return_inside=True)
                assert torch.equal(_bits(v), _bits(g)) and bool((ins != 0).all()), (prec, ss, sy, sx, y0, x0)


# ---- 7. chunking and what a launch stores ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,W", [(3, 256), (1, 512)])
def test_chunking_gives_the_bits_of_one_launch(dev, K, W):
    net = _net(dev, K, W)
    for prec in PRECISIONS:
        for ss in SSS:
            one = net.render_grid(R.CANVAS, origin=S.GRID_ORIGIN, scale=S.GRID_SCALE, precision=prec, supersample=ss)
            v1, i1 = net.render_view(R.CANVAS, S.SS_HORIZON, precision=prec, supersample=ss, return_inside=True)
            for chunk in (777, 64 * 37 + 17):
                g = net.render_grid(R.CANVAS, origin=S.GRID_ORIGIN, scale=S.GRID_SCALE, precision=prec, supersample=ss, chunk_rows=chunk)
                assert torch.equal(_bits(g), _bits(one)), (prec, ss, chunk)
                v, i = net.render_view(R.CANVAS, S.SS_HORIZON, precision=prec, supersample=ss, return_inside=True, chunk_rows=chunk)
                assert torch.equal(_bits(v), _bits(v1)) and torch.equal(i, i1), (prec, ss, chunk)


@pytest.mark.parametrize("K,W", [(3, 256), (1, 512)])
def test_a_launch_stores_exactly_n_rows(dev, K, W):
    from npp_amd import ops
    net = _net(dev, K, W)
    for w, prec in ((net._wf_pack(), "bf16"), (net._w32_pack(), "fp32")):
        for ss in SSS:
            whole, win = net.render_view(R.CANVAS, S.SS_HORIZON, precision=prec, supersample=ss, return_inside=True)
            whole, win = whole.reshape(-1, 3), win.reshape(-1)
            gwhole = net.render_grid(R.CANVAS, origin=S.GRID_ORIGIN, scale=S.GRID_SCALE, precision=prec, supersample=ss).reshape(-1, 3)
            for s0, n in ((0, 1), (777, 300), (TOTAL - 17, 17)):
                out = torch.full((n + 70, 3), -7.0, dtype=torch.float32, device=dev)
                inside = torch.full((n + 70,), 9, dtype=torch.uint8, device=dev)
                ops.render(ops.view_arg(s0, n, R.CANVAS[1], S.SS_HORIZON), net.cfg, w, net.params, precision=prec, out=out, inside=inside,
                           out_act=1, width=W, supersample=ss)
                assert torch.equal(_bits(out[:n]), _bits(whole[s0:s0 + n])) and torch.equal(inside[:n], win[s0:s0 + n]), (prec, ss, s0, n)
                assert bool((out[n:] == -7.0).all()) and bool((inside[n:] == 9).all())
                out.fill_(-7.0)
                ops.render(ops.grid_arg(s0, n, R.CANVAS[1], S.GRID_ORIGIN, S.GRID_SCALE), net.cfg, w, net.params, precision=prec, out=out,
                           out_act=1, width=W, supersample=ss)
                assert torch.equal(_bits(out[:n]), _bits(gwhole[s0:s0 + n])) and bool((out[n:] == -7.0).all()), (prec, ss, s0, n)
            out = torch.full((4, 3), -7.0, dtype=torch.float32, device=dev)
            inside = torch.full((4,), 9, dtype=torch.uint8, device=dev)
            ops.render(ops.view_arg(5, 0, R.CANVAS[1], S.SS_HORIZON), net.cfg, w, net.params, precision=prec, out=out, inside=inside, width=W,
                       supersample=ss)                                               # n = 0: nothing launched
            ops.render(ops.grid_arg(5, 0, R.CANVAS[1]), net.cfg, w, net.params, precision=prec, out=out, width=W, supersample=ss)
            assert bool((out == -7.0).all()) and bool((inside == 9).all())


def test_launchers_refuse_bad_supersampling(dev):
    from npp_amd import ops, NppError, lib
    net = _net(dev, 1, 256)
    for prec, w in (("bf16", net._wf_pack()), ("fp32", net._w32_pack())):
        out = torch.full((64, 3), 5.0, dtype=torch.float32, device=dev)
        for src in (ops.grid_arg((1 << 20) * 16, 1, 16), ops.view_arg(0, 4, (1 << 20) + 1, np.eye(3))):
            with pytest.raises(NppError, match=r"failed \(-1\).*2\^20"):
                ops.render(src, net.cfg, w, net.params, precision=prec, out=out, width=256, supersample=2)
        with pytest.raises(ValueError, match="supersample 3"):
            ops.render(ops.grid_arg(0, 4, 16), net.cfg, w, net.params, precision=prec, out=out, width=256, supersample=3)
        with pytest.raises(ValueError, match="tensor of positions"):
            ops.render(torch.zeros((64, 2), dtype=torch.float32, device=dev), net.cfg, w, net.params, precision=prec, supersample=2)
        g = ops.grid_arg(0, 4, 16)
        fn = lib(256).npp_mlp_fwd_grid_ss if prec == "bf16" else lib(256).npp_mlp_fwd32_grid_ss
        for ss in (3, 0):                                                            # the library's own refusal
            with pytest.raises(NppError, match=r"failed \(-1\).*ss=%d must be 1, 2, 4 or 8" % ss):
                ops.check(fn(ops.C.byref(g), ss, ops.C.byref(net.cfg), 256, ops._p(w), ops._p(net.params), ops._p(out), 1, None), "grid_ss")
        torch.cuda.synchronize()
        assert bool((out == 5.0).all())                                              # nothing was launched
    with pytest.raises(ValueError, match="supersample"):
        net.render_grid(R.CANVAS, supersample=3)
    with pytest.raises(ValueError, match="supersample"):
        net.render_view(R.CANVAS, np.eye(3), supersample=0)


# ---- 8. the render command -----------------------------------------------------------------------------------------------------------
def test_render_command_supersamples(dev, tmp_path, capsys):
    from npp_amd import render, view
    net = _net(dev, 3, 256)
    model = str(tmp_path / "model.npz")
    net.save(model)
    npy = str(tmp_path / "half.npy")
    r = render.main(["--model", model, "--out", str(tmp_path / "half.png"), "--scale", "0.5", "--supersample", "2", "--npy", npy])
    want = net.render_grid((12, 20), scale=0.5, supersample=2).cpu().numpy()
    assert np.array_equal(_ubits(r), _ubits(want)) and np.array_equal(_ubits(np.load(npy)), _ubits(want))
    assert re.search(r"2 x 2 samples per pixel -> ", capsys.readouterr().out)
    r = render.main(["--model", model, "--out", str(tmp_path / "auto.png"), "--scale", "0.25", "--supersample", "auto"])
    assert np.array_equal(_ubits(r), _ubits(net.render_grid((6, 10), scale=0.25, supersample=4).cpu().numpy()))
    assert re.search(r"4 x 4 samples per pixel \(auto\) -> ", capsys.readouterr().out)
    render.main(["--model", model, "--out", str(tmp_path / "plain.png"), "--scale", "0.5"])
    assert "samples per pixel" not in capsys.readouterr().out                      # without the flag: the closing line of before

    size = (48, 64)
    quad = np.array([[20.5, 9.25], [22.0, 52.5], [38.25, 60.0], [33.0, 2.75]])      # a receding rectangle: the far end minifies
    r2p, p2r = view.quad_to_rect(quad, FIT)
    vj = view.write(str(tmp_path / "view.json"), size, FIT, quad, r2p, p2r)
    ss = view.supersample_for(p2r, size)
    assert ss > 1
    r = render.main(["--model", model, "--view", vj, "--out", str(tmp_path / "view.png"), "--supersample", "auto"])
    out = capsys.readouterr().out
    assert re.search(r"%d x %d samples per pixel \(auto\)" % (ss, ss), out.strip().split("\n")[-1])
    assert f"{ss} x {ss} samples per canvas pixel" in out.split("\n")[0]
    assert np.array_equal(_ubits(r), _ubits(net.render_view(size, p2r, supersample=ss).cpu().numpy()))
