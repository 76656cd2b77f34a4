"""The antialiased image warp on the GPU: the kernel of npp_warp_image_u8_ss against its host twin bit for bit on the grid of cases
of test_warp_ss_cpu.py (the 40 x 29 canvas is 1160 pixels: no multiple of the 256-thread block), one sample against the point
kernel, the cases whose result follows without a restatement, changing shapes on one stream and the rectify command."""
import ctypes as C
import functools

import numpy as np
import pytest

import warp_ss_restatement as W

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CANVAS = W.WARP_CANVAS
MODES = ("nearest", "bilinear")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import npp_amd
    npp_amd.lib()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _host(name, mode, ss, Cn, reduce):
    """The host twin's (out, inside) of a case of the grid, computed once."""
    from npp_amd import ops
    return ops.warp_image_u8_host(W.warp_source(Cn), W.WARP_MAPS[name], CANVAS, mode, ss, reduce)


def _launch(dev, src, M, size, mode, ss, reduce, with_inside=True):
    """npp_warp_image_u8_ss itself on buffers pre-filled with 0xA5 -> (out, inside or None) as NumPy arrays."""
    import npp_amd
    from npp_amd import ops
    t = torch.from_numpy(np.ascontiguousarray(src)).to(dev)
    out = torch.full(tuple(size) + tuple(t.shape[2:]), 0xA5, dtype=torch.uint8, device=dev)
    inside = torch.full(tuple(size), 0xA5, dtype=torch.uint8, device=dev) if with_inside else None
    m = (C.c_double * 9)(*np.asarray(M, np.float64).reshape(9))
    rc = npp_amd.lib().npp_warp_image_u8_ss(ops._p(t), t.shape[0], t.shape[1], 1 if t.dim() == 2 else t.shape[2], size[0], size[1], m,
                                            MODES.index(mode), ss, W.REDUCES.index(reduce), ops._p(out), ops._p(inside), ops._stream())
    assert rc == 0, npp_amd.lib().npp_last_error_string()
    return out.cpu().numpy(), None if inside is None else inside.cpu().numpy()


@pytest.mark.parametrize("reduce", W.REDUCES)
@pytest.mark.parametrize("ss", (2, 4, 8))
@pytest.mark.parametrize("mode", MODES)
def test_kernel_equals_its_host_twin_and_writes_every_byte(dev, mode, ss, reduce):
    for Cn in (1, 3, 4):
        src = W.warp_source(Cn)
        for name, M in W.WARP_MAPS.items():
            want, win = _host(name, mode, ss, Cn, reduce)
            got, gin = _launch(dev, src, M, CANVAS, mode, ss, reduce)
            assert np.array_equal(got, want), (name, Cn)           # a byte left at 0xA5 would differ: the twin writes 0 outside
            assert np.array_equal(gin, win), (name, Cn)
            assert set(np.unique(gin)) <= {0, 255}


def test_kernel_without_an_inside_array(dev):
    for mode in MODES:
        want, _ = _host("projective", mode, 4, 3, "mean")
        got, none = _launch(dev, W.warp_source(3), W.WARP_MAPS["projective"], CANVAS, mode, 4, "mean", with_inside=False)
        assert none is None and np.array_equal(got, want), mode


@pytest.mark.parametrize("mode", MODES)
def test_one_sample_is_the_point_kernel_byte_for_byte(dev, mode):
    from npp_amd import ops
    for Cn in (1, 3, 4):
        src = W.warp_source(Cn)
        for name, M in W.WARP_MAPS.items():
            want, win = ops.warp_image_u8(torch.from_numpy(src).to(dev), M, CANVAS, mode)            # npp_warp_image_u8
            for reduce in W.REDUCES:
                got, gin = _launch(dev, src, M, CANVAS, mode, 1, reduce)
                assert np.array_equal(got, want.cpu().numpy()) and np.array_equal(gin, win.cpu().numpy()), (name, Cn, reduce)


def test_block_means_stripes_and_darkest_samples_on_the_device(dev):
    from npp_amd import view
    for S in (2, 4, 8):
        src, M, size, want = W.block_mean_case(S)
        bsrc, _, _, mean = W.block_min_case(S)
        for mode in MODES:
            out, inside = view.warp_image(src, M, size, mode, device=dev, supersample=S)
            assert out.is_cuda and np.array_equal(out.cpu().numpy(), want) and bool((inside == 255).all()), (S, mode)
            out, inside = view.warp_image(bsrc, M, size, mode, device=dev, supersample=S, reduce="min")
            assert bool((out == 0).all()) and bool((inside == 255).all()), (S, mode)
            out, inside = view.warp_image(bsrc, M, size, mode, device=dev, supersample=S, reduce="mean")
            assert bool((out == mean).all()) and bool((inside == 255).all()), (S, mode)
    src, M, size = W.stripe_case()
    out, inside = view.warp_image(src, M, size, "bilinear", device=dev)
    assert bool((out == 0).all()) and bool((inside == 255).all())
    out, inside = view.warp_image(src, M, size, "bilinear", device=dev, supersample=4)
    assert bool((out == 128).all()) and bool((inside == 255).all())
    one_high = np.arange(20, 200, 20, dtype=np.uint8).reshape(1, 9)
    out, inside = view.warp_image(one_high, np.eye(3), (1, 9), "bilinear", device=dev, supersample=2)
    assert not bool(out.any()) and not bool(inside.any())


def test_changing_shapes_on_one_stream(dev):
    from npp_amd import view
    rng = np.random.RandomState(17)
    a = (rng.randint(0, 256, (23, 31, 3)).astype(np.uint8), W.WARP_MAPS["projective"], (40, 29), 8)
    b = (rng.randint(0, 256, (301, 277, 3)).astype(np.uint8), np.array([[7.3, 0.4, -3.0], [-0.2, 9.1, 2.5], [0.002, 0.001, 1.0]]), (33, 41), 2)
    got = [view.warp_image(torch.from_numpy(src).to(dev), M, size, "bilinear", device=dev, supersample=ss) for src, M, size, ss in (a, b, a)]
    for (src, M, size, ss), (out, inside) in zip((a, b, a), got):                     # compared after all three were enqueued
        want, win = view.warp_image(src, M, size, "bilinear", supersample=ss)
        assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(inside.cpu().numpy(), win), (size, ss)
        assert 0 < (win == 255).mean() < 1


def test_device_entry_refuses_bad_arguments_and_launches_nothing(dev):
    import npp_amd
    from npp_amd import ops
    L = npp_amd.lib()
    t = torch.from_numpy(W.warp_source(3)).to(dev)
    out = torch.full(CANVAS + (3,), 0xA5, dtype=torch.uint8, device=dev)
    m = (C.c_double * 9)(*np.eye(3).reshape(9))
    for ss, reduce, msg in ((3, 0, b"ss=3"), (16, 0, b"ss=16"), (2, 2, b"reduce=2")):
        assert L.npp_warp_image_u8_ss(ops._p(t), 23, 31, 3, CANVAS[0], CANVAS[1], m, 1, ss, reduce, ops._p(out), None, ops._stream()) == -1
        assert msg in L.npp_last_error_string() and b"npp_warp_image_u8_ss" in L.npp_last_error_string()
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())


def test_rectify_supersampled_on_the_device_writes_the_cpu_folder(dev, tmp_path):
    from PIL import Image
    from npp_amd import rectify
    _, _, argv = W.rectify_inputs(tmp_path)
    a = rectify.main(argv + ["--outdir", str(tmp_path / "gpu"), "--device", "cuda:0", "--supersample", "4"])
    b = rectify.main(argv + ["--outdir", str(tmp_path / "cpu"), "--device", "cpu", "--supersample", "4"])
    for name in ("gt_img.png", "valid_mask.png", "unknown_mask.png", "masked_img.png"):
        assert np.array_equal(np.asarray(Image.open(f"{a}/{name}")), np.asarray(Image.open(f"{b}/{name}"))), name
