"""Adaptive supersampling on the GPU (npp_view_ss_classes, npp_mlp_fwd_view_list / npp_mlp_fwd32_view_list, NPPNet.render_view with
supersample="adaptive"): the class launch against its host twin and the NumPy restatement, and the definition itself -- every pixel
of an adaptive render is, bit for bit, the pixel of the uniform render at that pixel's own S -- with what a listed launch stores,
the chunking, the degenerate maps, canvases that change per call and the render command.  Fit 24 x 40, canvas 37 x 53."""
import re

import numpy as np
import pytest

import oracle
import render_adaptive_restatement as A
import render_ss_restatement as S
import view_restatement as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIT = (24, 40)
KW = [(1, 256), (3, 256), (1, 512), (3, 512)]
PRECISIONS = ("bf16", "fp32")
SSS = (1, 2, 4, 8)
TOTAL = R.CANVAS[0] * R.CANVAS[1]
VIEWS = {"ADAPT_VIEW": A.ADAPT_VIEW, "AFFINE": R.AFFINE, "PROJECTIVE": R.PROJECTIVE, "HORIZON": R.HORIZON, "SS_HORIZON": S.SS_HORIZON}
POISON = 0x7FA12345                 # a NaN payload no kernel writes: a touched word shows as changed bits


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import npp_amd
    npp_amd.lib()
    return torch.device("cuda:0")


_NETS = {}


def _net(dev, K, W, out_act=1):                  # the nets of test_gpu_render_ss.py
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


_UNIFORM = {}


def _uniform(net, key, M, size, prec, ss):
    """render_view(supersample=ss) of the whole canvas -> (colours (n, 3), inside (n,)): computed once per case and left unchanged."""
    k = (key, tuple(size), prec, ss)
    if k not in _UNIFORM:
        out, ins = net.render_view(size, M, precision=prec, return_inside=True, supersample=ss)
        _UNIFORM[k] = (out.reshape(-1, 3), ins.reshape(-1))
    return _UNIFORM[k]


def _by_definition(net, key, M, size, prec, dev):
    """The adaptive render by its definition: per pixel the uniform launch selected by the restatement's class map; +0 and byte 0
    where the class is 0."""
    cls = torch.from_numpy(A.classes(M, size, FIT)[0]).to(dev)
    out = torch.zeros((cls.shape[0], 3), dtype=torch.float32, device=dev)
    ins = torch.zeros(cls.shape[0], dtype=torch.uint8, device=dev)
    for ss in SSS:
        u, ui = _uniform(net, key, M, size, prec, ss)
        out[cls == ss] = u[cls == ss]
        ins[cls == ss] = ui[cls == ss]
    return out, ins, cls


def _assert_adaptive(got, want, what):
    (out, ins, cls), (wout, wins, wcls) = got, want
    assert out.shape == cls.shape + (3,) and out.dtype == torch.float32 and ins.dtype == cls.dtype == torch.uint8
    assert torch.equal(cls.reshape(-1), wcls), what
    assert torch.equal(ins.reshape(-1), wins), what
    assert torch.equal(_bits(out.reshape(-1, 3)), _bits(wout)), what
    zero = cls.reshape(-1) == 0
    assert bool((_bits(out.reshape(-1, 3))[zero] == 0).all()) and bool((ins.reshape(-1)[zero] == 0).all()), what      # exactly +0.0


# ---- 1. the class launch -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(VIEWS))
def test_class_launch_equals_the_host_twin_and_the_restatement(dev, name):
    from npp_amd import ops
    M = VIEWS[name]
    for start, n in ((0, TOTAL), (777, 300), (TOTAL - 17, 17)):
        v = ops.view_arg(start, n, R.CANVAS[1], M)
        cls = torch.full((n + 70,), 99, dtype=torch.uint8, device=dev)
        ins = torch.full((n + 70,), 9, dtype=torch.uint8, device=dev)
        assert ops.view_ss_classes(v, FIT, cls, ins) is cls
        hcls, hin = ops.view_ss_classes_host(v, FIT)
        want, win, _ = A.classes(M, R.CANVAS, FIT, start, n)
        assert np.array_equal(hcls, want) and np.array_equal(hin, win)
        assert np.array_equal(cls[:n].cpu().numpy(), want) and np.array_equal(ins[:n].cpu().numpy(), win), (name, start, n)
        assert bool((cls[n:] == 99).all()) and bool((ins[n:] == 9).all())          # exactly n bytes each
        only = ops.view_ss_classes(v, FIT, torch.full((n,), 99, dtype=torch.uint8, device=dev))       # no inside buffer
        assert torch.equal(only, cls[:n])
    point = _net(dev, 1, 256).render_view(R.CANVAS, M, return_inside=True)[1].reshape(-1)
    whole = torch.empty(TOTAL, dtype=torch.uint8, device=dev)
    wins = torch.empty(TOTAL, dtype=torch.uint8, device=dev)
    ops.view_ss_classes(ops.view_arg(0, TOTAL, R.CANVAS[1], M), FIT, whole, wins)
    assert torch.equal(wins, point) and torch.equal(whole == 0, point == 0)        # the point launch's bytes
    if name == "ADAPT_VIEW":
        assert {k: int((whole == k).sum()) for k in (0, 1, 2, 4, 8)} == A.ADAPT_COUNTS


# ---- 2. the definition -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,W", KW)
def test_adaptive_is_per_pixel_the_uniform_launch_of_its_class(dev, K, W):
    """Fails on a tree without the feature, where render_view refuses supersample="adaptive"."""
    net = _net(dev, K, W)
    for prec in PRECISIONS:
        got = net.render_view(R.CANVAS, A.ADAPT_VIEW, precision=prec, supersample="adaptive", return_inside=True, return_classes=True)
        want = _by_definition(net, ("ADAPT", K, W, 1), A.ADAPT_VIEW, R.CANVAS, prec, dev)
        assert {k: int((want[2] == k).sum()) for k in (0, 1, 2, 4, 8)} == A.ADAPT_COUNTS
        _assert_adaptive(got, want, (K, W, prec))
        assert bool(torch.isfinite(got[0]).all()) and bool((got[0][got[2] != 0] != 0).any())
        alone = net.render_view(R.CANVAS, A.ADAPT_VIEW, precision=prec, supersample="adaptive")
        assert torch.equal(_bits(alone), _bits(got[0]))


@pytest.mark.parametrize("out_act", [0, 1, 2])
def test_adaptive_definition_with_every_output_nonlinearity(dev, out_act):
    net = _net(dev, 3, 256, out_act)
    for prec in PRECISIONS:
        got = net.render_view(R.CANVAS, A.ADAPT_VIEW, precision=prec, supersample="adaptive", return_inside=True, return_classes=True)
        _assert_adaptive(got, _by_definition(net, ("ADAPT", 3, 256, out_act), A.ADAPT_VIEW, R.CANVAS, prec, dev), (out_act, prec))


# ---- 3. the listed launch alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ss", SSS)
@pytest.mark.parametrize("K,W", [(3, 256), (1, 512)])
def test_listed_launch_stores_the_listed_pixels_and_nothing_else(dev, ss, K, W):
    from npp_amd import ops
    net = _net(dev, K, W)
    s0, n, pad = 53 * 5 + 17, 300, 70                                              # a window that starts and ends mid-row, across the horizon
    inside_w = list(range(s0, s0 + n, 3)) + [s0 + n - 1]
    assert inside_w[-2] < inside_w[-1] and len(inside_w) % 64 != 0
    pix = torch.tensor([s0 - 5] + inside_w + [s0 + n + 2], dtype=torch.int64, device=dev)      # one index below, one above the window
    listed = torch.zeros(n, dtype=torch.bool, device=dev)
    listed[torch.tensor(inside_w, device=dev) - s0] = True
    for prec, w in (("bf16", net._wf_pack()), ("fp32", net._w32_pack())):
        u, ui = _uniform(net, ("HORIZON", K, W, 1), S.SS_HORIZON, R.CANVAS, prec, ss)
        big = torch.full((n + 2 * pad, 3), POISON, dtype=torch.int32, device=dev).view(torch.float32)
        bigin = torch.full((n + 2 * pad,), 9, dtype=torch.uint8, device=dev)
        ops.render(ops.view_arg(s0, n, R.CANVAS[1], S.SS_HORIZON), net.cfg, w, net.params, precision=prec, out=big[pad:pad + n],
                   inside=bigin[pad:pad + n], out_act=1, width=W, supersample=ss, pixels=pix)
        got, gin = _bits(big[pad:pad + n]), bigin[pad:pad + n]
        assert torch.equal(got[listed], _bits(u[s0:s0 + n])[listed]) and torch.equal(gin[listed], ui[s0:s0 + n][listed]), (prec, ss)
        assert bool((got[~listed] == POISON).all()) and bool((gin[~listed] == 9).all()), (prec, ss)      # unlisted pixels of the window
        for part in (_bits(big[:pad]), _bits(big[pad + n:])):                      # ... and every word outside it
            assert bool((part == POISON).all()), (prec, ss)
        assert bool((bigin[:pad] == 9).all()) and bool((bigin[pad + n:] == 9).all()), (prec, ss)
        assert bool((ui[s0:s0 + n][listed] == 0).any()) and bool((ui[s0:s0 + n][listed] != 0).any())     # pixels behind the horizon too
        ops.render(ops.view_arg(s0, n, R.CANVAS[1], S.SS_HORIZON), net.cfg, w, net.params, precision=prec, out=big[pad:pad + n],
                   out_act=1, width=W, supersample=ss, pixels=pix[:0])             # an empty list, no inside buffer: a no-op
        assert torch.equal(_bits(big[pad:pad + n]), got)


# ---- 4. chunking ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,W", [(3, 256), (1, 512)])
def test_adaptive_does_not_depend_on_chunk_rows(dev, K, W):
    net = _net(dev, K, W)
    for prec in PRECISIONS:
        one = net.render_view(R.CANVAS, A.ADAPT_VIEW, precision=prec, supersample="adaptive", return_inside=True, return_classes=True)
        for chunk in (64, 1000):
            got = net.render_view(R.CANVAS, A.ADAPT_VIEW, precision=prec, supersample="adaptive", return_inside=True,
                                  return_classes=True, chunk_rows=chunk)
            assert all(torch.equal(_bits(a) if a.dtype == torch.float32 else a, _bits(b) if b.dtype == torch.float32 else b)
                       for a, b in zip(got, one)), (prec, chunk)


# ---- 5. degenerate maps ------------------------------------------------------------------------------------------------------------------------
def test_one_class_maps_are_the_uniform_launch_and_an_empty_view_launches_nothing(dev, monkeypatch):
    from npp_amd import ops
    net = _net(dev, 3, 256)
    for prec in PRECISIONS:
        for M, ss in ((R.AFFINE, 1), (A.QUARTER, 4)):
            out, ins, cls = net.render_view(R.CANVAS, M, precision=prec, supersample="adaptive", return_inside=True, return_classes=True)
            want, win = net.render_view(R.CANVAS, M, precision=prec, supersample=ss, return_inside=True)
            assert bool((cls == ss).all()) and torch.equal(_bits(out), _bits(want)) and torch.equal(ins, win), (prec, ss)
        assert torch.equal(_bits(net.render_view(R.CANVAS, R.AFFINE, precision=prec, supersample="adaptive")),
                           _bits(net.render_view(R.CANVAS, R.AFFINE, precision=prec)))                   # all class 1: the point launch
    calls = []
    real = ops.render
    monkeypatch.setattr(ops, "render", lambda *a, **k: (calls.append(k.get("supersample")), real(*a, **k))[1])
    for prec in PRECISIONS:
        out, ins, cls = net.render_view(R.CANVAS, A.BEHIND, precision=prec, supersample="adaptive", return_inside=True, return_classes=True)
        assert not calls                                                           # wholly behind the horizon: no listed launch
        assert bool((_bits(out) == 0).all()) and not bool(ins.any()) and not bool(cls.any())
    net.render_view(R.CANVAS, R.AFFINE, supersample="adaptive")
    assert calls == [1]                                                            # one class: one listed launch


# ---- 6. shapes that change per call ----------------------------------------------------------------------------------------------------------------
def test_canvases_that_change_per_call(dev):
    net = _net(dev, 3, 256)
    big = (64, 80)
    for prec in PRECISIONS:
        for size, key in ((big, "big"), (R.CANVAS, "ADAPT"), (big, "big")):
            got = net.render_view(size, A.ADAPT_VIEW, precision=prec, supersample="adaptive", return_inside=True, return_classes=True)
            _assert_adaptive(got, _by_definition(net, (key, 3, 256, 1), A.ADAPT_VIEW, size, prec, dev), (prec, size))


# ---- 7. the command ------------------------------------------------------------------------------------------------------------------------------------
def test_render_command_adaptive(dev, tmp_path, capsys):
    from npp_amd import render, view, io as nio
    net = _net(dev, 3, 256)
    model = str(tmp_path / "model.npz")
    net.save(model)
    size = (48, 64)
    quad = np.array([[20.5, 9.25], [22.0, 52.5], [38.25, 60.0], [33.0, 2.75]])      # a receding rectangle: the far end minifies
    r2p, p2r = view.quad_to_rect(quad, FIT)
    vj = view.write(str(tmp_path / "view.json"), size, FIT, quad, r2p, p2r)
    cls = view.supersample_classes(p2r, size, FIT)
    assert len(set(np.unique(cls)) - {0}) > 1                                      # more than one class: there is something to adapt
    r = render.main(["--model", model, "--view", vj, "--out", str(tmp_path / "a.png"), "--supersample", "adaptive"])
    out = capsys.readouterr().out.strip().split("\n")
    want, wcls = net.render_view(size, p2r, supersample="adaptive", return_classes=True)
    assert np.array_equal(wcls.cpu().numpy(), cls)
    assert np.array_equal(np.ascontiguousarray(r).view(np.uint32), want.cpu().numpy().view(np.uint32))
    nio.imsave(str(tmp_path / "py.png"), want.cpu().numpy())
    assert open(str(tmp_path / "a.png"), "rb").read() == open(str(tmp_path / "py.png"), "rb").read()
    note = view.adaptive_note(cls, auto=view.supersample_for(p2r, size))
    assert note in out[-1] and note in out[0] and re.search(r"\d x \d on \d+\.\d % of the pixels in view; \d+ chain rows, 0\.\d+ of uniform", out[-1])
    r = render.main(["--model", model, "--out", str(tmp_path / "g.png"), "--scale", "0.25", "--supersample", "adaptive"])
    assert np.array_equal(np.ascontiguousarray(r).view(np.uint32), net.render_grid((6, 10), scale=0.25, supersample=4).cpu().numpy().view(np.uint32))
    assert "4 x 4 samples per pixel (adaptive" in capsys.readouterr().out
    assert torch.equal(_bits(net.render_grid((6, 10), scale=0.25, supersample="adaptive")), _bits(net.render_grid((6, 10), scale=0.25, supersample=4)))
