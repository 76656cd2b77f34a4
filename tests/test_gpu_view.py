"""Perspective views on the GPU: the projective render (npp_mlp_fwd_view / npp_mlp_fwd32_view, NPPNet.render_view) against the grid
launches, the fp32-position launches and the NumPy restatement, bit for bit; the image warp kernel against its host twin; the render
command's --view / --into path.  Canvas 37 x 53 (no multiple of the 64-row tile), chunks of 777 pixels (they start mid-row)."""
import numpy as np
import pytest

import oracle
import view_restatement as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIT = (24, 40)             # the fit's image size: smaller than what the views reach, so the inside bytes 0, 1 and 3 all occur
KW = [(1, 256), (3, 256), (1, 512), (3, 512)]
CHUNK = 777
PRECISIONS = ("bf16", "fp32")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import npp_amd
    npp_amd.lib()
    return torch.device("cuda:0")


_NETS = {}


def _net(dev, K, W):
    if (K, W) not in _NETS:
        from npp_amd.model import NPPNet
        angles, periods, _ = oracle.synthetic_periodicity(64, K)
        P = oracle.init_params(K, W=W, seed=7 * K + W)
        _NETS[(K, W)] = NPPNet(angles, periods, oracle.SEED0_FREQS, FIT, params=P, device=dev, ksplit=1, width=W)
    return _NETS[(K, W)]


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("K,W", KW)
def test_power_of_two_affine_views_are_the_grid_launch(dev, K, W):
    net = _net(dev, K, W)
    for prec in PRECISIONS:
        for sy, sx, y0, x0 in R.POW2_VIEWS:
            g = net.render_grid(R.CANVAS, origin=(y0, x0), scale=(sy, sx), precision=prec, chunk_rows=CHUNK)
            v = net.render_view(R.CANVAS, R.affine(sy, sx, y0, x0), precision=prec, chunk_rows=CHUNK)
            assert v.shape == R.CANVAS + (3,) and v.dtype == torch.float32
            assert torch.equal(_bits(v), _bits(g)), (prec, sy, sx, y0, x0)


@pytest.mark.parametrize("K,W", KW)
@pytest.mark.parametrize("name", ["AFFINE", "PROJECTIVE", "HORIZON"])
def test_views_equal_render_at_of_their_positions(dev, K, W, name):
    from npp_amd import view
    net = _net(dev, K, W)
    M = getattr(R, name)
    ryx, rin = R.view_coords(M, R.CANVAS, FIT)
    yx = view.canvas_coords(M, R.CANVAS, res=FIT)
    assert np.array_equal(yx.view(np.uint32), ryx.view(np.uint32))
    seen = torch.from_numpy(rin != 0).to(dev)
    assert (name == "HORIZON") == bool((rin == 0).any())
    for prec in PRECISIONS:
        out, inside = net.render_view(R.CANVAS, M, precision=prec, chunk_rows=CHUNK, return_inside=True)
        assert inside.shape == R.CANVAS and inside.dtype == torch.uint8
        assert np.array_equal(inside.cpu().numpy().reshape(-1), rin), prec
        at = net.render_at(torch.from_numpy(yx), precision=prec)
        out = out.reshape(-1, 3)
        assert torch.equal(_bits(out[seen]), _bits(at[seen])), prec
        assert bool((_bits(out[~seen]) == 0).all()), prec                      # exactly +0.0, not the network at (0, 0)
        assert bool(torch.isfinite(out).all())
        # the default chunk (one launch) and chunks of 777 give identical bits
        one, inside1 = net.render_view(R.CANVAS, M, precision=prec, return_inside=True)
        assert torch.equal(_bits(one.reshape(-1, 3)), _bits(out)) and torch.equal(inside1, inside)
        assert torch.equal(net.render_view(R.CANVAS, M, precision=prec, chunk_rows=CHUNK), out.view(*R.CANVAS, 3))


@pytest.mark.parametrize("K,W", [(3, 256), (1, 512)])
def test_a_launch_stores_exactly_n_rows(dev, K, W):
    from npp_amd import ops
    net = _net(dev, K, W)
    total = R.CANVAS[0] * R.CANVAS[1]
    for w, prec in ((net._wf_pack(), "bf16"), (net._w32_pack(), "fp32")):
        whole = net.render_view(R.CANVAS, R.HORIZON, precision=prec).reshape(-1, 3)
        for s0, n in ((0, 1), (CHUNK, 777), (total - 17, 17)):
            out = torch.full((n + 70, 3), -7.0, dtype=torch.float32, device=dev)
            inside = torch.full((n + 70,), 9, dtype=torch.uint8, device=dev)
            ops.render(ops.view_arg(s0, n, R.CANVAS[1], R.HORIZON), net.cfg, w, net.params, precision=prec, out=out, inside=inside, out_act=1, width=W)
            assert torch.equal(_bits(out[:n]), _bits(whole[s0:s0 + n])), (prec, s0, n)
            assert bool((out[n:] == -7.0).all()) and bool((inside[n:] == 9).all()) and bool((inside[:n] != 9).all())
        out = torch.full((4, 3), -7.0, dtype=torch.float32, device=dev)
        ops.render(ops.view_arg(5, 0, R.CANVAS[1], R.HORIZON), net.cfg, w, net.params, precision=prec, out=out, width=W)     # n = 0: nothing launched
        assert bool((out == -7.0).all())


def test_launchers_refuse_bad_views(dev):
    from npp_amd import ops, NppError
    net = _net(dev, 1, 256)
    bad = np.eye(3)
    bad[2, 1] = np.nan
    for prec, w in (("bf16", net._wf_pack()), ("fp32", net._w32_pack())):
        out = torch.full((64, 3), 5.0, dtype=torch.float32, device=dev)

        def call(start, n, cw, M=np.eye(3)):
            ops.render(ops.view_arg(start, n, cw, M), net.cfg, w, net.params, precision=prec, out=out, width=256)
        for args, msg in (((0, 64, 16, bad), r"m\[7\].*not finite"), ((0, 64, 0), "canvas width 0"), ((-1, 64, 16), ">= 0"),
                          (((1 << 24) * 16, 1, 16), r"2\^24"), ((0, 64, (1 << 24) + 1), r"2\^24")):
            with pytest.raises(NppError, match=r"failed \(-1\).*" + msg):
                call(*args)
        torch.cuda.synchronize()
        assert bool((out == 5.0).all())                                            # nothing was launched
    for M, msg in ((np.array([[1.0, 2, 3], [2, 4, 6], [0, 0, 1]]), "singular"), (bad, "non-finite")):
        with pytest.raises(ValueError, match=msg):
            net.render_view(R.CANVAS, M)


@pytest.mark.parametrize("mode", ["nearest", "bilinear"])
@pytest.mark.parametrize("C", [1, 3, 4])
def test_warp_kernel_equals_its_host_twin(dev, mode, C):
    from npp_amd import view
    src = R.warp_source(C)
    for name, M in R.WARP_MAPS.items():
        want, win = view.warp_image(src, M, R.WARP_CANVAS, mode)
        got, gin = view.warp_image(torch.from_numpy(src).to(dev), M, R.WARP_CANVAS, mode, device=dev)
        assert got.is_cuda and got.dtype == torch.uint8 and gin.shape == R.WARP_CANVAS
        assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(gin.cpu().numpy(), win), name


def test_render_command_puts_the_fit_into_the_photograph(dev, tmp_path):
    from PIL import Image
    from npp_amd import io as nio, render, view
    net = _net(dev, 3, 256)
    model = str(tmp_path / "model.npz")
    net.save(model)
    size = (48, 64)
    rng = np.random.RandomState(11)
    photo = rng.randint(0, 256, size + (3,)).astype(np.uint8)
    mask = np.where(rng.rand(*size) < 0.5, 0, 255).astype(np.uint8)
    Image.fromarray(photo).save(tmp_path / "photo.png")
    Image.fromarray(mask).save(tmp_path / "mask.png")
    quad = np.array([[6.5, 9.25], [10.0, 52.5], [38.25, 47.0], [33.0, 5.75]])          # the fit's rectangle, well inside the photograph
    r2p, p2r = view.quad_to_rect(quad, FIT)
    vj = view.write(str(tmp_path / "view.json"), size, FIT, quad, r2p, p2r)
    want, inside = net.render_view(size, p2r, return_inside=True)
    inside = inside.cpu().numpy()
    assert 0 < (inside == 3).mean() < 1 and (inside != 0).all() and (inside == 1).any()
    nio.imsave(str(tmp_path / "want.png"), want.cpu().numpy())
    w8 = np.asarray(Image.open(tmp_path / "want.png"))                                   # imsave's conversion of render_view
    base = ["--model", model, "--view", vj, "--chunk_rows", str(CHUNK)]

    def run(name, *extra):
        r = render.main(base + ["--out", str(tmp_path / name)] + list(extra))
        assert np.array_equal(r, want.cpu().numpy())
        return np.asarray(Image.open(tmp_path / name))
    into = ["--into", str(tmp_path / "photo.png")]
    assert np.array_equal(run("plain.png"), w8)
    got = run("into.png", *into)
    assert np.array_equal(got, np.where((inside == 3)[..., None], w8, photo))
    got = run("into_mask.png", *into, "--mask", str(tmp_path / "mask.png"))
    assert np.array_equal(got, np.where(((inside == 3) & (mask == 0))[..., None], w8, photo))
    got = run("into_beyond.png", *into, "--beyond")
    assert np.array_equal(got, w8)                                                       # the whole photograph sees the plane
    got = run("into_both.png", *into, "--beyond", "--mask", str(tmp_path / "mask.png"))
    assert np.array_equal(got, np.where((mask == 0)[..., None], w8, photo))


def test_rectify_on_the_device_writes_the_cpu_folder(dev, tmp_path):
    from PIL import Image
    from npp_amd import rectify
    rng = np.random.RandomState(3)
    Image.fromarray(rng.randint(0, 256, (48, 64, 3)).astype(np.uint8)).save(tmp_path / "photo.png")
    Image.fromarray(np.where(rng.rand(48, 64) < 0.3, 0, 255).astype(np.uint8)).save(tmp_path / "mask.png")
    argv = ["--photo", str(tmp_path / "photo.png"), "--quad", "-6", "3.25", "9", "57.5", "40.25", "70", "44", "7.75", "--size", "33", "41",
            "--mask", str(tmp_path / "mask.png")]
    a = rectify.main(argv + ["--outdir", str(tmp_path / "gpu"), "--device", "cuda:0"])
    b = rectify.main(argv + ["--outdir", str(tmp_path / "cpu"), "--device", "cpu"])
    for name in ("gt_img.png", "valid_mask.png", "unknown_mask.png", "masked_img.png"):
        assert np.array_equal(np.asarray(Image.open(f"{a}/{name}")), np.asarray(Image.open(f"{b}/{name}"))), name
    assert open(f"{a}/view.json").read() == open(f"{b}/view.json").read()
