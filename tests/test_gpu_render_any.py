"""Rendering a fitted NPP-Net at any scale and beyond its border, on the GPU: the grid launches (npp_mlp_fwd_grid /
npp_mlp_fwd32_grid), the fp32-position launches (npp_mlp_fwd_coordf / npp_mlp_fwd32_coordf / npp_warp_fwd_coordf), the model file
and the render command line.  Non-square fit frames (res = (211, 325)) and canvases throughout."""
import os

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

RES = (211, 325)
KW = [(1, 256), (3, 256), (5, 256), (1, 512), (3, 512), (5, 512)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import npp_amd
    npp_amd.lib()
    return torch.device("cuda:0")


_NETS = {}


def _net(dev, K, W, out_act=1):
    key = (K, W, out_act)
    if key not in _NETS:
        from npp_amd.model import NPPNet
        angles, periods, _ = oracle.synthetic_periodicity(RES[0], K)
        P = oracle.init_params(K, W=W, seed=10 * K + W)
        _NETS[key] = (NPPNet(angles, periods, oracle.SEED0_FREQS, RES, params=P, device=dev, ksplit=1, width=W, out_act=out_act),
                      P, angles, periods)
    return _NETS[key]


def _int_grid(H, W, dev):
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.int32), torch.arange(W, dtype=torch.int32), indexing="ij")
    return torch.stack([yy.reshape(-1), xx.reshape(-1)], 1).contiguous().to(dev)


@pytest.mark.parametrize("K,W", KW)
def test_scale_one_is_todays_render_and_integer_upscales_nest(dev, K, W):
    """(1) scale 1 at origin 0 == render() / render_fp32() of the int32 full grid; (2) at S = 2, 3, 4 the canvas pixel (S i, S j)
    is pixel (i, j) of scale 1, bit for bit (the division form is exact for S = 3 too)."""
    net, *_ = _net(dev, K, W)
    H, Wd = RES
    grid = _int_grid(H, Wd, dev)
    ref = {"bf16": net.render(grid).reshape(H, Wd, 3), "fp32": net.render_fp32(grid).reshape(H, Wd, 3)}
    for prec, r in ref.items():
        one = net.render_grid(RES, precision=prec)
        assert one.shape == (H, Wd, 3) and one.dtype == torch.float32
        assert torch.equal(one, r), prec
        for S in (2, 3, 4):
            up = net.render_grid((S * H, S * Wd), scale=S, precision=prec)
            assert torch.equal(up[::S, ::S], r), (prec, S)


def _built_widths():
    import npp_amd
    return list(npp_amd.FUSED_WIDTHS)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("W", _built_widths())
@pytest.mark.parametrize("K", [1, 3])
def test_every_source_kind_through_the_one_path(dev, K, W, precision):
    """ops.render on the four kinds of coordinate source -- int32 indices, the same integers as float32, the grid and the identity
    view -- over the 13 x 11 = 143 pixels of a 13 x 11 fit (three 64-row tiles, the last one ragged): the same bits on the 143 rows,
    inside bytes all 3, and the grid and view launches leave rows 143..191 of a prefilled 192-row output alone."""
    from npp_amd import ops
    from npp_amd.model import NPPNet
    H, Wd = 13, 11
    n, bp = H * Wd, 192
    angles, periods, _ = oracle.synthetic_periodicity(RES[0], K)      # (periods of a larger image: every period + offset stays > 0)
    net = NPPNet(angles, periods, oracle.SEED0_FREQS, (H, Wd), params=oracle.init_params(K, W=W, seed=7 * K + W), device=dev, ksplit=1,
                 width=W)
    pack = net._w32_pack() if precision == "fp32" else net._wf_pack()
    idx = torch.cat([_int_grid(H, Wd, dev), torch.zeros((bp - n, 2), dtype=torch.int32, device=dev)], 0).contiguous()

    def run(src, **kw):
        out = torch.full((bp, 3), 5.0, dtype=torch.float32, device=dev)
        ops.render(src, net.cfg, pack, net.params, precision=precision, out=out, width=W, **kw)
        return out
    ref = run(idx)
    assert bool(torch.isfinite(ref).all()) and float(ref[:n].std()) > 0.0
    assert torch.equal(run(idx.to(torch.float32))[:n], ref[:n])
    inside = torch.full((bp,), 9, dtype=torch.uint8, device=dev)
    for src, kw in ((ops.grid_arg(0, n, Wd), {}), (ops.view_arg(0, n, Wd, np.eye(3)), {"inside": inside})):
        out = run(src, **kw)
        assert torch.equal(out[:n], ref[:n]), type(src).__name__
        assert bool((out[n:] == 5.0).all()), type(src).__name__
    assert bool((inside[:n] == 3).all()) and bool((inside[n:] == 9).all())


@pytest.mark.parametrize("K,W", KW)
def test_float_positions_equal_the_grid_form(dev, K, W):
    """(3) the same positions built on the host in fp32 (model.canvas_coords) and passed to render_at == render_grid, bitwise."""
    from npp_amd.model import canvas_coords
    net, *_ = _net(dev, K, W)
    for size, origin, scale in (((300, 410), (-17.25, 40.5), (2.5, 2.5)), ((97, 131), (3.0, -9.0), (3.0, 1.75))):
        c = canvas_coords(size, origin, scale)
        for prec in ("bf16", "fp32"):
            g = net.render_grid(size, origin=origin, scale=scale, precision=prec).reshape(-1, 3)
            a = net.render_at(torch.from_numpy(c), precision=prec)
            assert torch.equal(a, g), (size, prec)
            assert bool(torch.isfinite(g).all())


@pytest.mark.parametrize("K,W", [(1, 256), (3, 512), (5, 256)])
def test_chunked_and_ragged_launches_write_exactly_n_rows(dev, K, W):
    """(4) launches of 64 k + 17 rows and chunk_rows that is not a multiple of the canvas width == one launch, bitwise; nothing is
    written past row n of the output (guard-filled buffer)."""
    from npp_amd import ops
    net, *_ = _net(dev, K, W)
    size, origin, scale = (150, 233), (-4.5, 7.25), (1.5, 2.0)
    total = size[0] * size[1]
    for prec, w in (("bf16", net.wf), ("fp32", net._w32_pack())):
        whole = net.render_grid(size, origin=origin, scale=scale, precision=prec).reshape(-1, 3)
        assert torch.equal(net.render_grid(size, origin=origin, scale=scale, precision=prec, chunk_rows=64 * 37 + 17).reshape(-1, 3), whole)
        assert torch.equal(net.render_grid(size, origin=origin, scale=scale, precision=prec, chunk_rows=size[1] + 1).reshape(-1, 3), whole)
        s0 = 0
        for k in (0, 1, 5, 40):
            n = 64 * k + 17
            out = torch.full((n + 200, 3), 12345.0, dtype=torch.float32, device=dev)
            ops.render(ops.grid_arg(s0, n, size[1], origin, scale), net.cfg, w, net.params, precision=prec, out=out, out_act=1, width=W)
            assert torch.equal(out[:n], whole[s0:s0 + n]), (prec, k)
            assert bool((out[n:] == 12345.0).all()), (prec, k)          # the clamped tail rows are not stored
            s0 += n
        # the very last pixel of the canvas, as the last row of a ragged launch
        out = torch.full((64 + 1, 3), -7.0, dtype=torch.float32, device=dev)
        ops.render(ops.grid_arg(total - 17, 17, size[1], origin, scale), net.cfg, w, net.params, precision=prec, out=out, out_act=1, width=W)
        assert torch.equal(out[:17], whole[total - 17:]) and bool((out[17:] == -7.0).all())


@pytest.mark.parametrize("K,W", KW)
def test_subpixel_and_extension_window_matches_the_oracle(dev, K, W):
    """(5) a 2.5x non-square window at origin (-17.25, 40.5) that reaches past the border (negative rows, columns past W, rows
    past H): a row sample with the corners against the oracle, with the bounds of the integer-grid tests."""
    from npp_amd.model import canvas_coords
    net, P, angles, periods = _net(dev, K, W)
    size, origin, scale = (600, 900), (-17.25, 40.5), 2.5
    c_all = canvas_coords(size, origin, scale)
    assert c_all[:, 0].min() < 0 and c_all[:, 0].max() > RES[0] and c_all[:, 1].max() > RES[1]
    n = c_all.shape[0]
    rng = np.random.RandomState(K + W)
    idx = np.concatenate([[0, size[1] - 1, n - size[1], n - 1], rng.randint(0, n, 508)])
    c = c_all[idx]
    emb = oracle.embed(c, angles, periods, oracle.SEED0_FREQS, RES)
    raw_f, _ = oracle.mlp_forward(P, emb, K)
    raw_b, _ = oracle.mlp_forward(P, emb, K, emulate_bf16=True)
    pf, pb = oracle.sigmoid(raw_f), oracle.sigmoid(raw_b)
    t = torch.from_numpy(idx).to(dev)
    g32 = net.render_grid(size, origin=origin, scale=scale, precision="fp32").reshape(-1, 3)[t].cpu().numpy()
    g16 = net.render_grid(size, origin=origin, scale=scale, precision="bf16").reshape(-1, 3)[t].cpu().numpy()
    assert np.abs(g32 - pf).max() < 5e-5
    assert np.abs(g16 - pb).max() < 4e-3
    assert np.abs(g16 - pf).max() < 2e-2
    assert np.linalg.norm(g16 - pf) / np.linalg.norm(pf) < 5e-3


def test_against_the_reference_at_subpixel_and_outside_positions(dev):
    """(6) tests/golden/g15_subpixel.npz (the reference's own embedder and NPP_Net, CPU fp32): reference_api's Embedder_periodic
    on float positions, render_at in both chains; integer-valued float input keeps the int32 path bit for bit."""
    from npp_amd import ops, reference_api
    from npp_amd.model import NPPNet
    g = np.load(os.path.join(GOLDEN, "g15_subpixel.npz"))
    c, res, angles, periods, freqs = g["coords"], tuple(int(v) for v in g["res"]), g["angles"], g["periods"], g["freqs"]
    ct = torch.from_numpy(c).to(dev)
    for k in range(3):
        ep, d = reference_api.get_embedder(10, 0, res, selected_angles=angles[k], selected_periods=periods[k], freq_scales=[1],
                                           freq_offsets=[0, -1, 1, 0.5, -0.5], angle_offsets=[0])
        assert d == 22
        v = ep.embed(ct.clone())
        assert float((v.cpu() - torch.from_numpy(g["warp"][k])).abs().max()) < 2e-5
        ci = torch.from_numpy(np.round(c)).to(dev)                                     # integer-valued floats
        assert torch.equal(ep.embed(ci.clone()), ops.warp_fwd(ci.to(torch.int32).contiguous(), ep.cfg))
        assert torch.equal(ops.warp_fwd(ci.contiguous(), ep.cfg), ops.warp_fwd(ci.to(torch.int32).contiguous(), ep.cfg))
    P = oracle.init_params(3, W=256, seed=int(g["param_seed"]))
    net = NPPNet(angles, periods, freqs, res, params=P, device=dev, ksplit=1, width=256)
    f32 = net.render_at(ct, precision="fp32").cpu().numpy()
    b16 = net.render_at(ct, precision="bf16").cpu().numpy()
    assert np.abs(f32 - g["pred"]).max() < 1e-4
    assert np.abs(b16 - g["pred"]).max() < 2e-2
    # the stand-alone embedder on float positions against the reference's embedding
    e = ops.embed_fwd(ct[:64].contiguous(), net.cfg, torch.float32, precise=True).cpu().numpy()
    assert np.abs(e - g["emb64"]).max() < 1e-4


def test_save_load_render(dev, tmp_path):
    """(7) a fit trained 30 iterations, saved and loaded into a fresh NPPNet: render_grid at scale 1 == fit.render_image(), bit for
    bit; the tanh output (out_act 2) survives a save -> load round trip of a net built from oracle.init_params."""
    from npp_amd.fit import CompletionFit
    from npp_amd.model import NPPNet
    H = 256
    img, mask = oracle.synthetic_image(H)
    a2, p2, s2 = oracle.synthetic_periodicity(H, 3)
    fit = CompletionFit(img, mask, a2, p2, oracle.SEED0_FREQS, oracle.init_params(3, seed=1), device=dev, N_rand=2048, shifts=s2,
                        rng_mode="fast")
    for _ in range(30):
        fit.step_full()
    path = str(tmp_path / "fit.npz")
    fit.save_model(path, image="syn")
    net = NPPNet.load(path, device=dev)
    assert net.meta["task"] == "completion" and net.meta["image"] == "syn" and net.K == 3 and net.width == 256
    assert torch.equal(net.latents, fit.net.latents) and torch.equal(net.params, fit.net.params)
    assert torch.equal(net.render_grid((H, H)), fit.render_image())
    fit.close()
    t, P, *_ = _net(dev, 3, 256, out_act=2)
    t.save(str(tmp_path / "tanh.npz"))
    t2 = NPPNet.load(str(tmp_path / "tanh.npz"), device=dev)
    assert t2.out_act == 2
    grid = _int_grid(*RES, dev)
    r = t.render(grid).reshape(*RES, 3)
    assert float(r.min()) < 0.0                                          # tanh range
    assert torch.equal(t2.render_grid(RES), r) and torch.equal(t2.render_grid(RES, precision="fp32"), t.render_fp32(grid).reshape(*RES, 3))


def test_cli_end_to_end(dev, tmp_path):
    """(8) python -m npp_amd.train --save_model on the driver test's 256^2 synthetic, then python -m npp_amd.render (in-process)."""
    from PIL import Image
    from npp_amd import io as nio, render, train
    H, K = 256, 3
    img, mask = oracle.synthetic_image(H)
    a, p, s = oracle.synthetic_periodicity(H, K)
    d = nio.write_detected_dir(str(tmp_path / "detected" / "syn"), img, mask, np.ones_like(mask), a, p, s)
    fit = train.main(["--datadir", d, "--basedir", str(tmp_path / "results"), "--p_topk", "3", "--N_iters", "121", "--i_testset", "60",
                      "--i_print", "60", "--rng_mode", "fast", "--random-trunks", "--save_model"])
    out = tmp_path / "results" / "completion_top3" / "syn"
    assert sorted(os.listdir(out)) == ["model.npz", "testset_000060", "testset_000120"]
    model = str(out / "model.npz")
    dumped = np.asarray(Image.open(out / "testset_000120" / "pred_rgb_img.png"))
    r1 = render.main(["--model", model, "--out", str(tmp_path / "s1.png"), "--scale", "1", "--npy", str(tmp_path / "s1.npy")])
    assert r1.shape == (H, H, 3)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "s1.png")), dumped)          # valid mask is all ones here
    assert np.array_equal(r1, fit.render_image().cpu().numpy())
    r2 = render.main(["--model", model, "--out", str(tmp_path / "s2.png"), "--scale", "2"])
    png2 = np.asarray(Image.open(tmp_path / "s2.png"))
    assert png2.shape == (2 * H, 2 * H, 3) and np.array_equal(png2[::2, ::2], dumped) and np.array_equal(r2[::2, ::2], r1)
    r3 = render.main(["--model", model, "--out", str(tmp_path / "ext.png"), "--origin", "-64", "-64", "--size", "384", "384",
                      "--precision", "bf16"])
    assert r3.shape == (384, 384, 3) and bool(np.isfinite(r3).all())
    assert np.array_equal(r3[64:320, 64:320], r1)
    assert np.load(str(tmp_path / "s1.npy")).dtype == np.float32


def test_abi_argument_errors(dev):
    """(9) zero / negative / non-finite scale, canvas width 0, an index >= 2^24: NPP_ERR_ARG with a message; n = 0 is a no-op."""
    from npp_amd import ops, NppError
    net, *_ = _net(dev, 1, 256)
    for prec, w in (("bf16", net.wf), ("fp32", net._w32_pack())):
        def call(start, n, cw, origin=(0.0, 0.0), scale=(1.0, 1.0)):
            out = torch.full((max(n, 1), 3), 5.0, dtype=torch.float32, device=dev)
            ops.render(ops.grid_arg(start, n, cw, origin, scale), net.cfg, w, net.params, precision=prec, out=out, width=256)
            return out
        for scale in ((0.0, 1.0), (1.0, -2.0), (float("nan"), 1.0), (1.0, float("inf"))):
            with pytest.raises(NppError, match=r"failed \(-1\).*scale"):
                call(0, 64, 16, scale=scale)
        with pytest.raises(NppError, match=r"failed \(-1\).*canvas width 0"):
            call(0, 64, 0)
        with pytest.raises(NppError, match=r"failed \(-1\).*2\^24"):
            call((1 << 24) * 16, 1, 16)
        with pytest.raises(NppError, match=r"failed \(-1\).*2\^24"):
            call(0, 64, (1 << 24) + 1)
        with pytest.raises(NppError, match=r"failed \(-1\).*>= 0"):
            call(-1, 64, 16)
        assert bool((call(0, 0, 16) == 5.0).all())                                       # n = 0: nothing launched, nothing written
        assert call((1 << 24) * 16 - 1, 1, 16).shape == (1, 3)                            # the last representable row is fine
    torch.cuda.synchronize()
