"""Stash audit on the GPU (include/npp_hip.h "stash audit"): the census launch against its plain C++ twin and
a NumPy decode of the copied-back bytes, the gradient gap against nets stepped under either stash format, audited fits against
unaudited ones (bits), the stacked census and the command-line flag."""
import json
import os

import numpy as np
import pytest

import oracle
import stash_census_restatement as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import npp_amd
    npp_amd.lib()
    return torch.device("cuda:0")


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _net(dev, K, width=256, ksplit=3, H=256, params=None):
    from npp_amd.model import NPPNet
    angles, periods, _ = oracle.synthetic_periodicity(H, K)
    P = oracle.init_params(K, W=width, seed=0) if params is None else params
    return NPPNet(angles, periods, oracle.SEED0_FREQS, (H, H), params=P, device=dev, ksplit=ksplit, width=width), P


def _iteration(net, dev, n, H=256):
    """One real iteration up to (not including) the optimiser step, the inputs of test_fused_training_step_gradients: n random rows
    (seed 5) padded to a multiple of 64, random colours (seed 2).  -> Bp, the padded coordinates on the device."""
    rng = np.random.RandomState(5)
    c = np.stack([rng.randint(0, H, n), rng.randint(0, H, n)], 1).astype(np.int32)
    Bp = (n + 63) // 64 * 64
    cp = np.zeros((Bp, 2), np.int32)
    cp[:n] = c
    gt = np.random.RandomState(2).rand(n, 3).astype(np.float32)
    coords = torch.from_numpy(cp).to(dev)
    net.zero_grad()
    net.forward_train(coords)
    net.workspace(Bp)["dpred"].zero_()
    net.pixel_loss(Bp, n, torch.from_numpy(gt).to(dev))
    net.backward(Bp)
    return Bp, coords


def _host_bytes(net, Bp):
    ws = net.workspace(Bp)
    torch.cuda.synchronize()
    return ws["actT"].cpu().numpy(), ws["dzT"].cpu().numpy()


@pytest.mark.parametrize("K,W", [(3, 256), (1, 256), (3, 512)])
def test_device_census_equals_the_host_twin(dev, K, W):
    """n = 100 real rows in Bp = 128 (two tiles, the second ragged; several workgroups per array) after one real iteration: the
    launch's record equals the plain C++ twin on the copied-back bytes, on the default stream and on another one, and the guard
    words around the record come back intact."""
    from npp_amd import ops
    from npp_amd._lib import census_layout
    n = 100
    net, _ = _net(dev, K, W)
    Bp, _ = _iteration(net, dev, n)
    assert Bp == 128
    act, dz = _host_bytes(net, Bp)
    want = ops.stash8_census_host(act, dz, Bp, n, K, W)
    words = census_layout(K, W)[2]
    ws = net.workspace(Bp)
    side = torch.cuda.Stream(dev)
    for stream in (None, side):
        buf = torch.full((words + 16,), GUARD, dtype=torch.int64, device=dev)
        if stream is None:
            ops.stash8_census(ws["actT"], ws["dzT"], Bp, n, K, buf[8:8 + words], W)
        else:
            stream.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(stream):
                ops.stash8_census(ws["actT"], ws["dzT"], Bp, n, K, buf[8:8 + words], W)
            torch.cuda.current_stream(dev).wait_stream(stream)
        got = buf.cpu().numpy()
        assert (got[:8] == GUARD).all() and (got[8 + words:] == GUARD).all()
        np.testing.assert_array_equal(got[8:8 + words], want)
    # the Python form, and the restatement's decode of the same bytes
    arrays = net.stash_census(Bp, n)
    ref, ref_tiles, _, _ = R.census(act, dz, Bp, n, K, W)
    assert list(arrays) == list(ref)
    for name in ref:
        for f in R.FIELDS + ("exp_hist",):
            assert arrays[name][f] == ref[name][f], (name, f)
    assert net.last_tile_scale == ref_tiles
    # a real iteration leaves no non-finite code behind, and a_p / the embeddings hold values (not all zero)
    assert all(c["nonfinite"] == 0 for c in arrays.values())
    assert arrays["emb0"]["zero"] < arrays["emb0"]["elements"] and arrays["dz_rgb"]["elements"] == 3 * n


@pytest.mark.parametrize("K,W", [(3, 256), (1, 512)])
def test_device_census_on_random_bytes(dev, K, W):
    """Uniformly random bytes in both arrays (every code, every class, non-finite ones included -- a real iteration leaves none), three
    tiles: one real row, a ragged tile, every row.  The launch equals the plain C++ twin word for word."""
    from npp_amd import ops
    Bp = 192
    sizes = ops.train_workspace(K, Bp, 1, W)
    g = torch.Generator(device=dev).manual_seed(K + W)
    act = torch.randint(0, 256, (sizes[1],), dtype=torch.uint8, device=dev, generator=g)
    dz = torch.randint(0, 256, (sizes[2],), dtype=torch.uint8, device=dev, generator=g)
    act_h, dz_h = act.cpu().numpy(), dz.cpu().numpy()
    for n in (1, 100, Bp):
        got = ops.stash8_census(act, dz, Bp, n, K, None, W).cpu().numpy()
        np.testing.assert_array_equal(got, ops.stash8_census_host(act_h, dz_h, Bp, n, K, W))
    arrays, _ = ops.census_decode(got, K, W)
    assert all(c["nonfinite"] > 0 and c["at_max"] > 0 and c["zero"] > 0 for name, c in arrays.items() if name != "dz_rgb")


def _limits(net, Bp, n, K, W):
    act, dz = _host_bytes(net, Bp)
    arrays = net.stash_census(Bp, n)
    ref = R.census(act, dz, Bp, n, K, W)[0]
    for name in ref:                                       # equal to the NumPy decode of the bytes, whatever they are
        for f in R.FIELDS:
            assert arrays[name][f] == ref[name][f], (name, f)
    return arrays


def test_forced_limits_are_counted(dev):
    """(a) dz outgrows its tile's lift: the f1 columns of the two layers that read f1 (pos_linears.0, scale_linears.0) scaled UP by
    s = 65536, feature_linear1 scaled down by the same power of two -- every forward value is unchanged (power-of-two scalings are
    exact in bf16 and fp32), dL/df1 = W^T dz grows by s: from about 0.014 x the tile's max |dL/draw| (the initialisation's scales:
    |W_rgb| <= 0.09, |W_p| <= 0.044 over 128 terms) to several hundred times it, where bf8 saturates above 14-28 x.  The factor is
    reasoned; 65536 is the value used (measured with it: 25183 of 25600 dz_f1 codes at the limit, the unscaled control none).  (b) periodic_linears.3.bias = 1000:
    snake(z_3) > 448 in the forward stash.  Counts > 0 and equal to the NumPy decode; the unscaled control is printed."""
    K, W, n = 3, 256, 100
    net, P = _net(dev, K, W)
    Bp, _ = _iteration(net, dev, n)
    ctl = _limits(net, Bp, n, K, W)
    print("control: at_max " + ", ".join(f"{k} {v['at_max']}" for k, v in ctl.items() if v["at_max"]) + " | nonfinite "
          + str(sum(v["nonfinite"] for v in ctl.values())))
    s = 65536.0
    Pa = {k: np.array(v, np.float32, copy=True) for k, v in P.items()}
    Pa["feature_linear1.weight"] /= s
    Pa["feature_linear1.bias"] /= s
    Pa["pos_linears.0.weight"][:, :W] *= s
    Pa["scale_linears.0.weight"][:, :W] *= s
    net_a, _ = _net(dev, K, W, params=Pa)
    Bp, _ = _iteration(net_a, dev, n)
    a = _limits(net_a, Bp, n, K, W)
    print(f"(a) s = {s:g}: dz_f1 at_max {a['dz_f1']['at_max']} of {a['dz_f1']['elements']}")
    assert a["dz_f1"]["at_max"] > 0
    np.testing.assert_array_equal(net_a.workspace(Bp)["pred"].cpu().numpy(), net.workspace(Bp)["pred"].cpu().numpy())   # same forward
    Pb = {k: np.array(v, np.float32, copy=True) for k, v in P.items()}
    Pb["periodic_linears.3.bias"][:] = 1000.0
    net_b, _ = _net(dev, K, W, params=Pb)
    Bp, _ = _iteration(net_b, dev, n)
    b = _limits(net_b, Bp, n, K, W)
    print(f"(b) bias 1000: a3 at_max {b['a3']['at_max']} of {b['a3']['elements']}")
    assert b["a3"]["at_max"] > 0


def test_gradient_gap_is_the_distance_between_the_two_stashes(dev):
    """On the inputs of test_fused_training_step_gradients (n = 677, K = 3, W = 256, ksplit = 3): the 8-bit leg is the iteration's own
    slabs (stash_gap leaves them, pred and dpred as they were: bits), the 16-bit leg equals grads() of an identical net stepped
    under stash8 = 0 (bits), the reported gap is NumPy's rel_l2 of the two to 1e-6, and 0 < worst < 0.13 -- the sum of the 9e-2 and
    4e-2 that test grants the two formats against the same fp32 oracle (triangle inequality; these inputs only).
    Measured on an MI355X: worst periodic_linears.1.weight 5.652e-02, median 4.479e-02."""
    from npp_amd import ops
    K, W, n = 3, 256, 677
    net, _ = _net(dev, K, W)
    Bp, coords = _iteration(net, dev, n)
    ws = net.workspace(Bp)
    G8 = net.grads()
    before = {k: ws[k].clone() for k in ("gslabs", "pred", "dpred")}
    loss_before = net._loss_bufs.clone()
    gap = net.stash_gap(Bp, coords)
    torch.cuda.synchronize()
    assert ops.tune("stash8") == 1                                   # flipped back
    for k, t in before.items():
        assert torch.equal(ws[k], t), k
    assert torch.equal(net._loss_bufs, loss_before)
    G8_after = net.grads()
    for name in G8:
        assert np.array_equal(G8[name], G8_after[name]), name
    old = ops.tune("stash8", 0)
    try:
        net16, _ = _net(dev, K, W)
        _iteration(net16, dev, n)
        torch.cuda.synchronize()
        G16 = net16.grads()
    finally:
        ops.tune("stash8", old)
    leg16 = net.stash_gap_grads16()
    assert set(leg16) == set(G16) == set(gap)
    for name in G16:
        assert np.array_equal(leg16[name], G16[name]), name
        assert abs(gap[name] - rel_l2(G8[name], G16[name])) < 1e-6, (name, gap[name])
    worst = max(gap, key=gap.get)
    print(f"gradient gap stash8 vs stash16: worst {worst} {gap[worst]:.3e}, median {float(np.median(list(gap.values()))):.3e}")
    assert 0 < gap[worst] < 0.13, (worst, gap[worst])


def _fit(dev, graph, **kw):
    from npp_amd import synthetic as S
    from npp_amd.fit import CompletionFit
    H, K = 128, 3
    img, mask = S.synthetic_image(H)
    angles, periods, shifts = S.synthetic_periodicity(H, K)
    return CompletionFit(img, mask, angles, periods, S.SEED0_FREQS, S.init_params(K, seed=0), device=dev, N_rand=1024, shifts=shifts,
                         patch_size=64, patch_num=2, num_real_patch_per_sample=3, graph_iteration=graph, seed=0, **kw)


def _same(a, b, path="state"):
    if isinstance(a, torch.Tensor):
        assert torch.equal(a, b), path
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b), path
    elif isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            _same(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{path}[{i}]")
    else:
        assert a == b, (path, a, b)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_audited_fit_ends_with_the_bits_of_an_unaudited_one(dev, graph):
    """128^2 lattice, N_rand = 1024, 6 iterations audited every iteration against an unaudited twin: state_dict() bit-identical;
    6 reports with rows = the batch's n and patch-carrying sources; graph mode: the audited iterations count as eager."""
    it = 6
    aud, ref = _fit(dev, graph, stash_audit=1), _fit(dev, graph)
    n_rows = 1024 + 2 * 64 * 64
    for i in range(it):
        assert aud.step_full() and ref.step_full()
        assert aud.last_source == ref.last_source
        assert aud.last_stash_audit["iteration"] == i + 1
    torch.cuda.synchronize()
    _same(aud.state_dict(), ref.state_dict())
    reps = list(aud.stash_audits)
    assert len(reps) == it and ref.last_stash_audit is None and len(ref.stash_audits) == 0
    for r in reps:
        assert set(r) == {"iteration", "source", "rows", "census", "tile_scale", "grad_gap", "worst", "flags"}
        assert r["rows"] == n_rows and r["source"] in ("val", "train", "same")
        assert r["tile_scale"]["tiles"] == (n_rows + 63) // 64
        assert r["worst"][1] == max(r["grad_gap"].values()) > 0
        sat = sum(c["at_max"] + c["nonfinite"] for c in r["census"].values()) > 0
        assert r["flags"] == (["saturated"] if sat else [])
    print("worst gaps: " + ", ".join(f"{r['source']} {r['worst'][0]} {r['worst'][1]:.3e}" for r in reps))
    if graph:
        assert aud.graph_stats == {"captured": 0, "replayed": 0, "eager": it}
        assert ref.graph_stats["eager"] + ref.graph_stats["replayed"] == it
    # audit_next() arms one iteration of a fit that audits nothing by itself
    ref.audit_next()
    assert ref.step_full() and aud.step_full()
    assert len(ref.stash_audits) == 1 and ref.last_stash_audit["iteration"] == it + 1
    assert ref.step_full() and aud.step_full()
    assert len(ref.stash_audits) == 1
    torch.cuda.synchronize()
    _same(aud.state_dict(), ref.state_dict())


def test_refusals_on_the_device(dev):
    from npp_amd import ops
    with pytest.raises(ValueError, match="precision='fp32'"):
        _fit(dev, False, stash_audit=2, precision="fp32")
    old = ops.tune("stash8", 0)
    try:
        with pytest.raises(ValueError, match="stash8"):
            _fit(dev, False, stash_audit=2)
    finally:
        ops.tune("stash8", old)
    net, _ = _net(dev, 1)
    Bp, coords = _iteration(net, dev, 64)
    probe = torch.zeros(64, device=dev)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
            probe.add_(1.0)                                  # (something to record: the refusals below enqueue nothing)
            with pytest.raises(ValueError, match="stream capture"):
                net.stash_census(Bp, 64)
            with pytest.raises(ValueError, match="stream capture"):
                net.stash_gap(Bp, coords)
    torch.cuda.current_stream(dev).wait_stream(s)


def test_stacked_census_per_image(dev):
    """A two-image stack after step_full(): each image's census equals the host twin on its rows of the stacked workspace."""
    from npp_amd import ops
    from npp_amd.fit import CompletionFit
    from npp_amd.stack import StackedFit
    H, K = 128, 1
    angles, periods, shifts = oracle.synthetic_periodicity(H, K)
    fits = []
    for i in range(2):
        img, mask = oracle.synthetic_image(H, seed=i)
        fits.append(CompletionFit(img, mask, np.asarray(angles, np.float64) + 0.3 * i, periods, oracle.SEED0_FREQS,
                                  oracle.init_params(K, seed=i), device=dev, N_rand=1024, shifts=shifts, seed=10 + i, patch_size=64, patch_num=2))
    st = StackedFit(fits)
    try:
        took = 0
        for _ in range(3):                                   # (an image may sit an iteration out: stop at the first both took)
            took = st.step_full()
            if took == 2:
                break
        assert took >= 1
        census = st.stash_census()
        torch.cuda.synchronize()
        assert len(census) == 2 and sum(c is not None for c in census) == took
        for m, c in enumerate(census):
            if c is None:
                continue
            rec = ops.stash8_census_host(st.actF[m].cpu().numpy(), st.dzF[m].cpu().numpy(), st.Bp, st.n, K, st.width)
            want, tiles = ops.census_decode(rec, K, st.width)
            assert c == want and st.last_tile_scales[m] == tiles
            assert c["a0"]["elements"] == st.n * 256
    finally:
        st.close()


def test_command_line_flag(dev, tmp_path, capsys):
    """python -m npp_amd.train --audit_stash 2 (in-process) on a temporary synthetic dataset: [STASH] lines and stash_audit.json."""
    from npp_amd import io as nio, synthetic as S, train
    H, K = 128, 3
    img, mask = S.synthetic_image(H)
    a, p, s = S.synthetic_periodicity(H, K)
    d = nio.write_detected_dir(str(tmp_path / "detected" / "syn"), img, mask, np.ones_like(mask), a, p, s)
    fit = train.main(["--datadir", d, "--basedir", str(tmp_path / "out"), "--p_topk", "3", "--N_iters", "7", "--i_testset", "1000",
                      "--i_print", "1000", "--N_rand", "1024", "--random-trunks", "--audit_stash", "2"])
    out = capsys.readouterr().out
    with open(os.path.join(str(tmp_path / "out"), "completion_top3", "syn", "stash_audit.json")) as f:
        reps = json.load(f)
    assert "stash_format" in reps[0] and len(reps) - 1 == len(fit.stash_audits) >= 1
    its = [r["iteration"] for r in reps[1:]]
    assert its == [r["iteration"] for r in fit.stash_audits] and all(i % 2 == 0 for i in its)
    assert out.count("[STASH] it ") == len(reps) - 1
    assert set(reps[1]["grad_gap"]) == set(fit.net.state_dict())
