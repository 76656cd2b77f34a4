"""Rendering a fitted NPP-Net at any scale and beyond its border -- the parts that need no GPU: the model file (NumPy reader /
writer), the host form of the canvas mapping, the command lines' argument checks, and the oracle against the reference's own
embedder and network at non-integer, negative and out-of-canvas positions (tests/golden/g15_subpixel.npz)."""
import os
import subprocess
import sys
import zipfile

import numpy as np
import pytest

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _write(path, K, W, **meta):
    from npp_amd import modelfile
    P = oracle.init_params(K, W=W, seed=K + W)
    angles, periods, _ = oracle.synthetic_periodicity(256, K)
    lat = np.array([0.1, -0.2, 0.3, -0.4, 0.5, -0.6], np.float32)
    modelfile.write(path, P, lat, angles, periods, oracle.SEED0_FREQS, (211, 325), W, out_act=1, **meta)
    return P, lat, angles, periods


@pytest.mark.parametrize("K,W", [(1, 256), (3, 256), (1, 512), (3, 512)])
def test_model_file_round_trip(tmp_path, K, W):
    from npp_amd import modelfile
    path = str(tmp_path / "model.npz")
    P, lat, angles, periods = _write(path, K, W, task="completion", image="syn", iterations=120)
    d = modelfile.read(path)
    shapes = oracle.param_shapes(K, W=W)
    assert list(d["params"]) == list(shapes)                          # the reference's names, in the blob's order
    for name, shp in shapes.items():
        assert d["params"][name].shape == tuple(shp)
        assert d["params"][name].dtype == np.float32
        assert np.array_equal(d["params"][name].view(np.uint32), P[name].view(np.uint32))      # bit for bit
    assert np.array_equal(d["latents"], lat) and np.array_equal(d["angles_deg"], angles) and np.array_equal(d["periods"], periods)
    assert np.array_equal(d["freqs"], np.asarray(oracle.SEED0_FREQS, np.float32))
    assert np.array_equal(d["freq_offsets"], np.array([0.0, -1.0, 1.0, 0.5, -0.5], np.float32))
    assert d["res"] == (211, 325) and d["K"] == K and d["width"] == W and d["out_act"] == 1 and d["format_version"] == 1
    assert d["meta"] == {"task": "completion", "image": "syn", "iterations": "120"}
    with np.load(path, allow_pickle=False) as f:                      # a plain archive: no pickled objects anywhere
        assert set(modelfile.state_dict({k: f[k] for k in f.files})) == set(shapes)


def test_model_file_rejects_damaged_or_foreign_files(tmp_path):
    from npp_amd import modelfile
    path = str(tmp_path / "model.npz")
    _write(path, 3, 256)
    blob = open(path, "rb").read()
    cut = str(tmp_path / "cut.npz")
    open(cut, "wb").write(blob[:len(blob) // 2])
    with pytest.raises(ValueError, match="not a readable model file"):
        modelfile.read(cut)
    with np.load(path, allow_pickle=False) as f:
        arrays = {k: f[k] for k in f.files}

    def variant(name, **change):
        a = dict(arrays)
        for k, v in change.items():
            if v is None:
                a.pop(k)
            else:
                a[k] = v
        p = str(tmp_path / f"{name}.npz")
        np.savez(p, **a)
        return p
    with pytest.raises(ValueError, match="format_version 2 unknown"):
        modelfile.read(variant("v2", **{"npp/format_version": np.asarray(2, np.int64)}))
    with pytest.raises(ValueError, match="rgb_linear.bias missing"):
        modelfile.read(variant("missing", **{"rgb_linear.bias": None}))
    with pytest.raises(ValueError, match=r"scale_linears.0.weight has shape \(256, 256\)"):
        modelfile.read(variant("shape", **{"scale_linears.0.weight": np.zeros((256, 256), np.float32)}))
    with pytest.raises(ValueError, match="npp/latents missing"):
        modelfile.read(variant("nolat", **{"npp/latents": None}))
    with pytest.raises(ValueError, match="not an NPP-Net model file"):
        modelfile.read(variant("foreign", **{"npp/format_version": None}))
    z = str(tmp_path / "notzip.npz")
    open(z, "wb").write(b"not a zip archive at all")
    with pytest.raises(ValueError):
        modelfile.read(z)
    assert zipfile.is_zipfile(path)


@pytest.mark.parametrize("S", [2, 3, 4])
def test_canvas_mapping_is_exact_at_multiples_of_an_integer_scale(S):
    """The fp32 positions y0 + i / sy the grid launches form (and render_at is fed with in the GPU tests): at scale S the canvas
    pixel (S i, S j) lands exactly on the integer fit pixel (i, j) -- S = 3 included, where 1 / 3 is not a binary fraction."""
    from npp_amd.model import canvas_coords
    H, W = 37, 53
    c = canvas_coords((S * H, S * W), scale=S)
    assert c.dtype == np.float32 and c.shape == (S * H * S * W, 2)
    grid = c.reshape(S * H, S * W, 2)[::S, ::S]
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    assert np.array_equal(grid[..., 0], yy.astype(np.float32)) and np.array_equal(grid[..., 1], xx.astype(np.float32))
    # a shifted origin by a whole pixel keeps it exact; the partial form equals the full one
    p0 = 3 * S * (S * W) + 1                                            # canvas row 3 S, column 1
    c2 = canvas_coords((S * H, S * W), origin=(-5, 7), scale=(S, S), start=p0, n=1000)
    assert np.array_equal(c2, canvas_coords((S * H, S * W), origin=(-5, 7), scale=S)[p0:p0 + 1000])
    assert np.array_equal(c2[S - 1], np.array([-5 + 3, 7 + 1], np.float32))     # canvas (3 S, S) -> fit (3, 1), shifted


def test_train_flag_and_render_cli_arguments(tmp_path):
    from npp_amd import train
    assert train.parse(["--datadir", "x", "--save_model"]).save_model is True
    assert train.parse(["--datadir", "x"]).save_model is False
    model = str(tmp_path / "model.npz")
    _write(model, 1, 256)
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")

    def run(*args):
        return subprocess.run([sys.executable, "-m", "npp_amd.render", *args], cwd=ROOT, env=env, capture_output=True, text=True,
                              timeout=120)
    out = str(tmp_path / "x.png")
    for args, msg in ((["--model", model, "--out", out, "--scale", "0"], "--scale"),
                      (["--model", model, "--out", out, "--scale", "2", "-1"], "--scale"),
                      (["--model", model, "--out", out, "--size", "-4", "16"], "--size"),
                      (["--model", str(tmp_path / "none.npz"), "--out", out], "no such file"),
                      (["--model", model, "--out", out, "--chunk_rows", "0"], "--chunk_rows")):
        r = run(*args)
        assert r.returncode != 0 and msg in r.stderr, (args, r.returncode, r.stderr[-500:])
        assert not os.path.exists(out)


def test_oracle_reproduces_the_reference_at_subpixel_and_outside_positions():
    g = np.load(os.path.join(GOLDEN, "g15_subpixel.npz"))
    c, res, angles, periods, freqs = g["coords"], tuple(int(v) for v in g["res"]), g["angles"], g["periods"], g["freqs"]
    assert c.dtype == np.float32 and (c != np.round(c)).any() and (c < 0).any()
    assert (c[:, 0] >= res[0]).any() and (c[:, 1] >= res[1]).any()    # past the bottom and the right border too
    for k in range(3):
        w = oracle.periodic_warp(c, angles[k], periods[k], res)
        assert np.abs(w - g["warp"][k]).max() < 2e-5
    P = oracle.init_params(3, W=256, seed=int(g["param_seed"]))
    ck = [sum(float(np.asarray(v, np.float64).sum()) for v in P.values()), sum(float(np.abs(np.asarray(v, np.float64)).sum()) for v in P.values())]
    assert np.allclose(ck, g["param_checksum"], rtol=0, atol=1e-6)
    emb = oracle.embed(c, angles, periods, freqs, res)
    assert np.abs(emb[:64] - g["emb64"]).max() < 5e-5
    raw, _ = oracle.mlp_forward(P, emb, 3)
    np.testing.assert_allclose(raw, g["raw"], rtol=1e-4, atol=2e-5)
    assert np.abs(oracle.sigmoid(raw) - g["pred"]).max() < 1e-5
