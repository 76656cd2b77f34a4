"""rng_mode="device" without a GPU: the definition of the draws (tests/dev_sampler_restatement.py: Philox4x32-10, the
cycle-walking Feistel permutation, the lattice half) checked on its own, against the project's NumPy GridPatchSampler.draw(), and
against the host twins of the two launches (npp_dev_sampler_*_host: the kernels' arithmetic through the C ABI)."""
import numpy as np
import pytest

import dev_sampler_restatement as R

SEED = 20261018
KAT = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    from npp_amd import dev_sampler
    assert _hex(R.philox4x32_10(ctr, key)) == want
    assert _hex(dev_sampler.philox4x32_10(ctr, key)) == want


@pytest.mark.parametrize("N", [1, 2, 3, 5, 17, 1000, 1024, 1025, 4097, 245000])
def test_permutation_maps_the_range_onto_itself(N):
    from npp_amd import dev_sampler
    p = R.perm(N, N, 7, 1, SEED)
    assert np.array_equal(np.sort(p), np.arange(N))
    np.testing.assert_array_equal(dev_sampler.perm_host(SEED, 7, 1, N, N), p)
    if N > 1:
        assert not np.array_equal(p, R.perm(N, N, 8, 1, SEED)) or N < 4       # another draw index, another permutation


def test_uniformity_of_the_permutation_draws():
    """N = 1000, n = 100, draws t = 0..19999 of stream 1, seed 2024: inclusion counts (chi^2 / (1 - n/N): the inclusion indicator
    of a without-replacement draw has variance p (1 - p)), the element at position 0, and pair co-inclusion over elements 0..49.
    Measured with this definition: z = +0.87, -0.92, max |z| = 3.37 (binomial variance; 3.35 with T p) (four Feistel rounds instead of eight: +2.37 on the first)."""
    N, n, T = 1000, 100, 20000
    s = R.perm(N, n, np.arange(T), 1, 2024)
    assert s.shape == (T, n)
    df = N - 1
    inc = np.bincount(s.reshape(-1), minlength=N).astype(np.float64)
    e = T * n / N
    z_inc = (((inc - e) ** 2 / e).sum() / (1 - n / N) - df) / np.sqrt(2 * df)
    first = np.bincount(s[:, 0], minlength=N).astype(np.float64)
    e0 = T / N
    z_first = (((first - e0) ** 2 / e0).sum() - df) / np.sqrt(2 * df)
    member = np.zeros((T, 50), np.float64)
    rows, cols = np.nonzero(s < 50)
    member[rows, s[rows, cols]] = 1.0
    co = member.T @ member
    p2 = n * (n - 1) / (N * (N - 1))
    zz = (co - T * p2) / np.sqrt(T * p2 * (1 - p2))
    z_pair = np.abs(zz[np.triu_indices(50, 1)]).max()
    print(f"inclusion z {z_inc:+.2f}, position-0 z {z_first:+.2f}, pair max |z| {z_pair:.2f}")
    assert abs(z_inc) <= 4 and abs(z_first) <= 4 and z_pair <= 4.5


# ---- the lattice half ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case():
    c = R.case_image()
    assert (len(c["pool_train"]), len(c["pool_val"])) == (3782, 862)
    return c


class _StubRng:
    """np.random's two calls as GridPatchSampler.draw() makes them, answered with the device mode's values for draw t."""

    def __init__(self, seed, t):
        self.seed, self.t = seed, t

    def uniform(self, lo, hi):
        return R.uniform(self.seed, self.t)

    def choice(self, N, size, replace):
        assert replace is False
        return R.perm(N, int(np.prod(size)), self.t, 1, self.seed)


def _sampler(c, n_p):
    import torch
    from npp_amd.sampler import GridPatchSampler
    return GridPatchSampler(img=torch.from_numpy(c["img"])[None], mask=torch.from_numpy(c["mask"])[None, ..., None], N_samples=n_p,
                            patch_size=c["P"], height=c["H"], width=c["W"], pool_train=c["known"], pool_val=c["unknown"],
                            selected_shifts=[[list(s) for s in R.SHIFTS_DXDY]], rng=_StubRng(SEED, 0))


def _host_image(c, ratio, seed, keep):
    from npp_amd import dev_sampler
    arrs = [np.ascontiguousarray(c[k], np.int32) for k in ("sat", "pool_val", "pool_train")]
    keep.extend(arrs)
    return dev_sampler.make_image(arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[2].ctypes.data, len(c["pool_val"]), len(c["pool_train"]),
                                  len(c["known"]), c["shifts_dydx"], ratio, seed, c["H"], c["W"], c["P"])


def assert_same_draw(got, want, n_p):
    """got: a draw in GridPatchSampler.draw()'s form (real_cen float64 positions or None), want: the restatement's."""
    assert (got["source"], got["k"]) == (want["source"], want["k"])
    np.testing.assert_array_equal(np.asarray(got["cen"], np.int64), want["cen"])
    if want["real"] is None:
        assert got["real_cen"] is None
    else:
        np.testing.assert_array_equal(np.rint(got["real_cen"]).astype(np.int32), want["real"])
    if want["weights"] is None:
        assert got["weights"] is None
    else:
        assert got["weights"].dtype == np.float32 and np.array_equal(got["weights"], want["weights"])


@pytest.mark.parametrize("n_p", [2, 4])
@pytest.mark.parametrize("ratio", [0.3, 0.035, 0.0])
def test_lattice_half_equals_the_numpy_sampler_and_the_host_twin(case, n_p, ratio):
    """64 draws: the restatement, GridPatchSampler.draw() fed the restatement's uniform / choice values, and the decision
    launch's host twin agree on every field; the inputs reach every branch (all sources; every k the ratio can give)."""
    from npp_amd import dev_sampler
    topk, ts = 3, list(range(64))
    want = R.case_draws(case, n_p, topk, ratio, SEED, ts)
    smp = _sampler(case, n_p)
    keep = []
    im = _host_image(case, ratio, SEED, keep)
    for t, w in zip(ts, want):
        smp.rng = _StubRng(SEED, t)
        assert_same_draw(smp.draw(topk, ratio), w, n_p)
        rec = dev_sampler.decide_host([im], [t], n_p, topk)
        assert_same_draw(dev_sampler.parse_record(rec[0], topk), w, n_p)
        assert rec[0, 3] == t and rec[0, 2] == n_p
    src = [w["source"] for w in want]
    assert (src.count("val"), src.count("train"), src.count("same")) == (27, 25, 12)
    ks = {w["k"] for w in want if w["source"] != "same"}
    if ratio == 0.3:
        assert ks == {3}
    elif ratio == 0.035:
        assert ks == ({0, 1, 2, 3} if n_p == 2 else {0, 1, 2})
    else:
        assert ks == {0}


def test_host_twin_serves_several_images_at_once(case):
    """M = 3 images of different sizes, seeds and draw indices in one call: each record is that image's own draw."""
    from npp_amd import dev_sampler
    cases = [case, R.case_image(64, 64, ((10, 30, 12, 40),), 6), R.case_image(40, 136, ((8, 30, 50, 90),), 7)]
    seeds, ts, keep = [SEED, 3, 2 ** 40 + 5], [5, 0, 77], []
    for t0 in range(8):
        tt = [t + t0 for t in ts]
        rec = dev_sampler.decide_host([_host_image(c, 0.3, s, keep) for c, s in zip(cases, seeds)], tt, 2, 3)
        for i, c in enumerate(cases):
            assert_same_draw(dev_sampler.parse_record(rec[i], 3), R.case_draws(c, 2, 3, 0.3, seeds[i], [tt[i]])[0], 2)


@pytest.mark.parametrize("N,n", R.PIXEL_CASES)
def test_pixel_rows_host_twin(case, N, n):
    from npp_amd import dev_sampler
    keep = []
    im = _host_image(case, 0.3, SEED, keep)
    im.n_train = N
    for t in (0, 1, 4000000000):
        np.testing.assert_array_equal(dev_sampler.pixels_host([im], [t], n)[0], R.pixels(N, n, SEED, t))


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_sampling_more_than_the_population_raises(case):
    from npp_amd import dev_sampler
    with pytest.raises(ValueError):
        R.perm(5, 6, 0, 1, SEED)
    with pytest.raises(ValueError):
        dev_sampler.perm_host(SEED, 0, 2, 5, 6)
    keep = []
    im = _host_image(case, 0.3, SEED, keep)
    im.n_train = 10
    with pytest.raises(ValueError):
        dev_sampler.pixels_host([im], [0], 11)
    im.n_pool_val = im.n_pool_train = 1                       # fewer centres than fake patches: k = -1 in the record
    rec = dev_sampler.decide_host([im], [0], 2, 3)
    assert rec[0, 1] == -1
    with pytest.raises(ValueError, match="larger sample than population"):
        dev_sampler.parse_record(rec[0], 3)


def _fit_kw():
    import oracle
    img, mask = oracle.synthetic_image(64)
    a, p, s = oracle.synthetic_periodicity(64, 1)
    return dict(img=img, mask=mask, angles_deg=a, periods=p, freqs=oracle.SEED0_FREQS, params=oracle.init_params(1, seed=0),
                device="cpu", shifts=s)


def test_refusals_by_name():
    """The mode's refusals come before any device work, so they show without a GPU."""
    from npp_amd.fit import CompletionFit
    kw = _fit_kw()
    with pytest.raises(ValueError, match="prefetch"):
        CompletionFit(rng_mode="device", prefetch=2, **kw)
    with pytest.raises(ValueError, match="no_reg_sampling"):
        CompletionFit(rng_mode="device", no_reg_sampling=True, **kw)
    with pytest.raises(ValueError) as e:
        CompletionFit(rng_mode="nope", **kw)
    for mode in ("reference", "numpy", "fast", "device"):
        assert repr(mode) in str(e.value)


def test_mixed_modes_in_one_stack_are_refused():
    from types import SimpleNamespace
    from npp_amd.stack import StackedFit
    net = SimpleNamespace(precision="bf16")
    with pytest.raises(ValueError, match="rng_mode='device' for every image"):
        StackedFit([SimpleNamespace(net=net, rng_mode="device"), SimpleNamespace(net=net, rng_mode="reference")])


def test_train_cli_takes_the_mode():
    from npp_amd.train import parse
    assert parse(["--datadir", ".", "--rng_mode", "device"]).rng_mode == "device"
