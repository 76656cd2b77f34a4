"""CompletionFit(graph_iteration=True): the device side of an iteration replayed as one captured HIP graph per iteration shape.
Every test runs the graph-mode fit next to an eager twin of the same seed and compares BITS (torch.equal / np.array_equal, no
tolerance): the eager loop is bit-reproducible (ops.DETERMINISTIC) and a graph replays the same launches.

Shared setup, the smallest at which every branch still exists: a 128 x 128 lattice (npp_amd.synthetic) with its centred hole,
K = 3, W = 256, N_rand = 1024, patch size 64 with patch_num = 2 and 3 real patches per sample, fixed-seed random trunks.  At this
size the sampler (host code: GridPatchSampler.draw; tests/dev_sampler_restatement.py for rng_mode='device') returns k = 3 for
the 'val' and 'train' sources and k = 1 for 'same', and no draw with k == 0, for the seed used here -- counted on the CPU."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEED = 0
# Iterations of the shared run.  Counted on the CPU for SEED: the 60 draws of the reference stream are 'val' x 24, 'train' x 21,
# 'same' x 15 (device stream: 29 / 17 / 14), none skipped; a key is (source, k, loss accumulator, buffer set) with the last two
# alternating in step, so 3 sources x 2 = 6 keys, each launch by launch for its first two uses: 12 eager iterations, 48 replayed.
N = 60


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import npp_amd
    npp_amd.lib()
    return torch.device("cuda:0")


def _fit(dev, graph, **kw):
    from npp_amd import synthetic as S
    from npp_amd.fit import CompletionFit
    H, K = 128, 3
    img, mask = S.synthetic_image(H)
    angles, periods, shifts = S.synthetic_periodicity(H, K)
    kw.setdefault("seed", SEED)
    return CompletionFit(img, mask, angles, periods, S.SEED0_FREQS, S.init_params(K, seed=0), device=dev, N_rand=1024, shifts=shifts,
                         patch_size=64, patch_num=2, num_real_patch_per_sample=3, graph_iteration=graph, **kw)


def _same(a, b, path="state"):
    """Bit equality of two state_dict()-like structures."""
    if isinstance(a, torch.Tensor):
        assert isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b), path
    elif isinstance(a, np.ndarray):
        assert a.dtype == np.asarray(b).dtype and np.array_equal(a, b), path
    elif isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            _same(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{path}[{i}]")
    else:
        assert type(a) is type(b) and a == b, (path, a, b)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32).tolist()


def _run_pair(g, e, n, each=None):
    """n iterations of step_full() of the graph-mode fit g and its eager twin e, side by side: the same iterations run / are
    skipped, and after every one the pixel loss and last_patch_loss are equal as bits.  -> the sources of the executed ones."""
    sources = []
    for i in range(1, n + 1):
        rg, re = g.step_full(), e.step_full()
        assert rg == re, i
        if rg:
            assert g.last_source == e.last_source, i
            assert _bits(g.net.loss_buf) == _bits(e.net.loss_buf), (i, g.last_source)
            assert _bits(g.last_patch_loss) == _bits(e.last_patch_loss), (i, g.last_source)
            sources.append(g.last_source)
        if each is not None:
            each(i)
    return sources


def _same_fit(g, e):
    _same(g.state_dict(), e.state_dict())
    assert g.psnr("known") == e.psnr("known") and g.psnr("unknown") == e.psnr("unknown")
    rows = g.i_all_dev[:64 * g.W]
    assert torch.equal(g.net.render(rows), e.net.render(rows))


_RUNS = {}


def _shared(dev, mode):
    """The N-iteration twin run of one rng_mode, once per module (tests 1, 2, 5 and 6 read it; nobody steps these fits again)."""
    if mode not in _RUNS:
        g, e = _fit(dev, True, rng_mode=mode), _fit(dev, False, rng_mode=mode)
        try:
            sources = _run_pair(g, e, N)
            err = None
        except AssertionError as ex:                              # reported by every test that reads the run
            sources, err = None, ex
        _RUNS[mode] = (g, e, sources, err)
    g, e, sources, err = _RUNS[mode]
    if err is not None:
        raise err
    return g, e, sources


@pytest.mark.parametrize("mode", ["reference", "device"])
def test_graph_iterations_are_the_eager_iterations_bit_for_bit(dev, mode):
    """Test 1: prefetch = 0 with the reference stream, and the device draws.  Pixel loss and patch loss after every iteration (in
    the shared run), then state_dict() -- params, m, v, pixel latents and moments, LPIPS latents and moments, every step counter,
    lr --, psnr() and a render of 64 rows."""
    g, e, _ = _shared(dev, mode)
    assert g.graph_iteration and not e.graph_iteration
    _same_fit(g, e)
    assert (g.net.lr, g.net.global_step, g.net.opt_step, g.percepLoss.lat_step, g.percepLoss.touched, g.last_source, g.net._clean) == (
        e.net.lr, e.net.global_step, e.net.opt_step, e.percepLoss.lat_step, e.percepLoss.touched, e.last_source, e.net._clean)


@pytest.mark.parametrize("mode", ["reference", "device"])
def test_the_iterations_really_were_replayed(dev, mode):
    """Test 2: at least half of the executed iterations are graph replays (the capture policy leaves 12 of the 60 eager, see N),
    and every patch source that occurred has a captured graph."""
    g, e, sources = _shared(dev, mode)
    st = g.graph_stats
    assert set(st) == {"captured", "replayed", "eager"}
    assert st["replayed"] + st["eager"] == len(sources) == N - g.skipped
    assert st["replayed"] >= len(sources) / 2, st
    assert set(sources) == {"val", "train", "same"}
    live = {key[2] for key, ent in g._it_graphs.items() if ent[0] is not None}
    assert live == set(sources) and st["captured"] >= 3, (st, live)
    assert e.graph_stats == {"captured": 0, "replayed": 0, "eager": 0}


def test_patch_size_decay_inside_the_run(dev):
    """Test 3: patch_size_decay = 40 puts one decay (64 -> 32, patch_num 2 -> 4) into 70 iterations.  Identical to the eager twin;
    the graphs of the old shape are gone; replays resume in the new shape (31 iterations there, 12 of them eager)."""
    g, e = _fit(dev, True, patch_size_decay=40), _fit(dev, False, patch_size_decay=40)
    seen = {}

    def each(i):
        if i in (39, 40):
            seen[i] = (g.graph_stats, {key[0] for key in g._it_graphs})
    _run_pair(g, e, 70, each)
    assert (g.patch_size, g.patch_num) == (e.patch_size, e.patch_num) == (32, 4)
    _same_fit(g, e)
    assert seen[39][1] == {(64, 2)} and seen[39][0]["replayed"] > 0
    assert seen[40][1] == {(32, 4)}                                # the first iteration of the new shape dropped the old graphs
    assert {key[0] for key in g._it_graphs} == {(32, 4)} and len(g._it_graphs) <= g.MAX_ITER_GRAPHS
    assert g.graph_stats["replayed"] > seen[40][0]["replayed"] and g.graph_stats["captured"] > seen[40][0]["captured"]


def test_producer_thread_path(dev):
    """Test 4: prefetch = 8 with the reference stream (the command line's default path: draws on the producer thread, the device
    half of the sampler an iteration ahead on its own stream, two sets of batch buffers).  Both state_dict() after close().  How
    far a producer thread had drawn ahead when it was stopped is host timing in either fit, so the position of the random stream
    ('rng', 'draw_iter') is the one part of the state that is not compared; everything the fits computed is."""
    g, e = _fit(dev, True, prefetch=8), _fit(dev, False, prefetch=8)
    try:
        _run_pair(g, e, N)
    finally:
        g.close()
        e.close()
    sg, se = g.state_dict(), e.state_dict()
    for sd in (sg, se):
        del sd["rng"], sd["draw_iter"]
    _same(sg, se)
    assert g.graph_stats["replayed"] >= (N - g.skipped) / 2
    assert {key[5] for key in g._it_graphs} == {0, 1}              # both buffer sets were captured


def test_skipped_iterations_agree(dev):
    """Test 5: no draw of the shared runs has k == 0 (the CPU count for SEED says so for both streams), so none is constructed by
    force: what is asserted is that the two modes agree on it, and the counters that a skipped iteration must not move."""
    for mode in ("reference", "device"):
        g, e, sources = _shared(dev, mode)
        assert g.skipped == e.skipped == N - len(sources)
        assert g.iteration == e.iteration == N and g.net.opt_step == e.net.opt_step == len(sources)


@pytest.mark.parametrize("resume_graph", [True, False])
def test_resume_from_a_graph_mode_state(dev, resume_graph):
    """Test 6: 30 graph iterations, state_dict(), loaded into a fresh fit of either mode, 30 more: the 60 uninterrupted eager
    iterations of the shared run."""
    _, e60, _ = _shared(dev, "reference")
    g = _fit(dev, True)
    for _ in range(30):
        g.step_full()
    sd = g.state_dict()
    r = _fit(dev, resume_graph)
    r.load_state_dict(sd)
    for _ in range(30):
        r.step_full()
    _same(r.state_dict(), e60.state_dict())
    assert r.psnr("unknown") == e60.psnr("unknown")
    if resume_graph:
        assert r.graph_stats["replayed"] > 0


def test_segmentation_task(dev):
    """Test 7: task='segmentation' (no LPIPS, contextual weight 0.005, the LR clock standing still), 40 iterations."""
    kw = dict(task="segmentation", use_perceptual_loss=False, contextual_weight=0.005)
    g, e = _fit(dev, True, **kw), _fit(dev, False, **kw)
    _run_pair(g, e, 40)
    _same_fit(g, e)
    assert g.net.global_step == 0 and g.percepLoss.lat_step == 0
    assert g.graph_stats["replayed"] >= 20


def test_a_runtime_that_cannot_capture_falls_back(dev, monkeypatch):
    """Test 8: torch.cuda.graph raising on entry: one warning, no graph, the eager bits."""
    class _NoCapture:
        def __init__(self, *a, **k):
            pass

        def __enter__(self):
            raise RuntimeError("stream capture is not available")

        def __exit__(self, *a):
            return False
    monkeypatch.setattr(torch.cuda, "graph", _NoCapture)
    g, e = _fit(dev, True), _fit(dev, False)
    e.lp_graph = False                                             # (the twin's LPIPS-branch graph would meet the same patch)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        _run_pair(g, e, 20)
    mine = [w for w in rec if "captured as a HIP graph" in str(w.message)]   # (of the iteration or of its LPIPS branch: one in all)
    assert len(mine) == 1, [str(w.message) for w in rec]
    st = g.graph_stats
    assert st["captured"] == 0 and st["replayed"] == 0 and st["eager"] == 20 - g.skipped
    _same_fit(g, e)


def test_refusals_name_the_switch(dev):
    """Test 9."""
    from npp_amd.stack import StackedFit
    for kw, name in ((dict(precision="fp32"), "precision='fp32'"), (dict(trunk_precision="fp32"), "trunk_precision='fp32'"),
                     (dict(task="remapping"), "task='remapping'")):
        with pytest.raises(ValueError) as ex:
            _fit(dev, True, **kw)
        assert name in str(ex.value) and "graph_iteration" in str(ex.value)
    with pytest.raises(ValueError) as ex:
        StackedFit([_fit(dev, True), _fit(dev, True, seed=1)])
    assert "graph_iteration" in str(ex.value)


@pytest.mark.parametrize("step", [1, 2, 1000])
def test_device_word_adam_equals_the_argument_form(dev, step):
    """Test 10: the scalar record.  The fused Adam + re-pack + loss-partials launch takes a NETWORK's blob only (its scatter walks
    the layer table), so the 4 096-element blob with 2 slabs goes through the plain device-word form the LPIPS latents use
    (npp_adam_step_dev against npp_adam_step), and the new entry (npp_adam_step_net_pack_dev against npp_adam_step_net_pack) is
    run on the smallest network blob (K = 1), 2 slabs, with the pixel-loss latents, the idle accumulator's clear and both packs.
    The words are the host's (ops.adam_words): the learning rate is not computed on the device, so there is no device schedule to
    compare -- the rule stays the host's double pow."""
    from npp_amd import ops, synthetic as S
    from npp_amd.model import NPPNet
    gen = torch.Generator(device="cpu").manual_seed(1234 + step)

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=gen) * scale).to(dev)
    lr = 5e-4 * 0.1 ** (step / 50000)
    hp = torch.from_numpy(np.array(ops.adam_words(lr, step), np.float32)).to(dev)
    # ---- 4 096 elements, 2 slabs
    p0, m0, v0, gs = rnd(4096), rnd(4096, scale=1e-2), rnd(4096, scale=1e-2).abs(), rnd(2, 4096, scale=1e-2)
    a, b = [t.clone() for t in (p0, m0, v0)], [t.clone() for t in (p0, m0, v0)]
    ops.adam_step(*a, gs, 2, 4096, lr, step)
    ops.adam_step_dev(*b, gs, 2, 4096, hp)
    for x, y, name in zip(a, b, ("p", "m", "v")):
        assert torch.equal(x, y), name
    assert not torch.equal(a[0], p0)
    # ---- the fused launch on a network blob
    H = 64
    angles, periods, _ = S.synthetic_periodicity(H, 1)
    nets = [NPPNet(angles, periods, S.SEED0_FREQS, (H, H), params=S.init_params(1, seed=0), device=dev, ksplit=2, lrate=lr) for _ in range(2)]
    n_par = nets[0].n_params
    m1, v1 = rnd(n_par, scale=1e-3), rnd(n_par, scale=1e-3).abs()
    lm, lv, dl = rnd(6, scale=1e-3), rnd(6, scale=1e-3).abs(), rnd(6, scale=1e-2)
    ws0 = nets[0].workspace(64)
    g1 = rnd(ws0["gslabs"].numel(), scale=1e-3)
    for net in nets:
        ws = net.workspace(64)
        assert net.ksplit == 2 and ws["gslabs"].numel() == g1.numel()
        ws["gslabs"].copy_(g1)
        net.m.copy_(m1), net.v.copy_(v1), net.lat_m.copy_(lm), net.lat_v.copy_(lv), net.dlatent.copy_(dl)
        net._loss_bufs.copy_(torch.tensor([0.25, 0.75], device=dev))
        net.opt_step, net.lr = step - 1, lr
    a, b = nets
    before = a.params.clone(), a.wf.clone()
    a.optimizer_step(64)
    words = torch.from_numpy(np.array(b.step_words(), np.float32)).to(dev)
    assert torch.equal(words, hp)
    b.optimizer_launch_dev(64, words)
    b.optimizer_advance()
    for name in ("params", "m", "v", "latents", "lat_m", "lat_v", "dlatent", "wf", "wb", "_loss_bufs"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert (a.opt_step, a.lr, a.global_step, a._clean) == (b.opt_step, b.lr, b.global_step, b._clean)
    assert not torch.equal(a.params, before[0]) and not torch.equal(a.wf, before[1])
    assert float(a._loss_bufs[1]) == 0.0 and float(a._loss_bufs[0]) == 0.25     # the idle accumulator cleared, the current one kept


def test_command_line_flag(dev, tmp_path, capsys):
    """python -m npp_amd.train --graph_iteration (in-process; the default path: reference stream, producer thread, the loop on a
    stream of its own) against the same command without the flag: the fitted network and the written model equal as bits, the
    counts printed once."""
    from npp_amd import io as nio, synthetic as S, train
    H, K = 128, 3
    img, mask = S.synthetic_image(H)
    a, p, s = S.synthetic_periodicity(H, K)
    d = nio.write_detected_dir(str(tmp_path / "detected" / "syn"), img, mask, np.ones_like(mask), a, p, s)
    fits = {}
    for name, flag in (("graph", ["--graph_iteration"]), ("eager", [])):
        fits[name] = train.main(["--datadir", d, "--basedir", str(tmp_path / name), "--p_topk", "3", "--N_iters", "61", "--i_testset", "60",
                                 "--i_print", "60", "--N_rand", "1024", "--random-trunks", "--save_model"] + flag)
    out = capsys.readouterr().out
    assert out.count("[GRAPH]") == 1
    g, e = fits["graph"], fits["eager"]
    assert g.graph_iteration and g.graph_stats["replayed"] > 0 and g.graph_stats["replayed"] + g.graph_stats["eager"] == 60 - g.skipped
    for name in ("params", "m", "v", "latents"):
        assert torch.equal(getattr(g.net, name), getattr(e.net, name)), name
    assert torch.equal(g.percepLoss._lat, e.percepLoss._lat) and g.percepLoss.lat_step == e.percepLoss.lat_step
    assert (g.net.opt_step, g.net.lr, g.skipped) == (e.net.opt_step, e.net.lr, e.skipped)
    ma, mb = (np.load(str(tmp_path / n / "completion_top3" / "syn" / "model.npz")) for n in ("graph", "eager"))
    assert set(ma.files) == set(mb.files)
    for k in ma.files:
        if k != "meta":
            assert np.array_equal(ma[k], mb[k]), k
