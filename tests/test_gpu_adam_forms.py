"""Every form of the Adam step on the same inputs, compared as BITS (torch.equal, no tolerance): the update, the slab sum and the
host's scalar rule are each written once (csrc/npp_adam.h: adam_update, slab_sum / adam_quad, adam_words), and the
forms below are what calls them -- the flat blob forms (argument, device-word, with the latent tail; vector and scalar kernel),
the fused Adam + re-pack launch (argument, device-word, against Adam followed by pack), its stacked form, and the latent group
of the patch losses (losses.LatentGroup).

NPP_ADAM_FORMS_DIGESTS=<file>: additionally writes the sha256 of the raw bytes of every output tensor of every case there (JSON),
for comparing two builds of the library (NPP_LIB_PATH / NPP_LIB_PATH_W512)."""
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

_DIGESTS = {}
_DIGEST_FILE = os.environ.get("NPP_ADAM_FORMS_DIGESTS")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import npp_amd
    for w in npp_amd.FUSED_WIDTHS:
        npp_amd.lib(w)
    yield torch.device("cuda:0")
    if _DIGEST_FILE:
        with open(_DIGEST_FILE, "w") as f:
            json.dump(_DIGESTS, f, indent=0, sort_keys=True)


def _record(case, **tensors):
    if _DIGEST_FILE:
        for name, t in tensors.items():
            _DIGESTS[f"{case}/{name}"] = hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _same(a, b, names, what):
    for x, y, name in zip(a, b, names):
        assert x.shape == y.shape and torch.equal(x, y), (what, name)


class _Rnd:
    def __init__(self, dev, seed):
        self.dev, self.gen = dev, torch.Generator(device="cpu").manual_seed(seed)

    def __call__(self, *shape, scale=1.0, off=0):
        """off = 1: the tensor starts one float into its allocation (4 bytes past a 16-byte boundary)."""
        n = int(np.prod(shape))
        t = torch.empty(n + off, dtype=torch.float32, device=self.dev)[off:]
        t.copy_(torch.randn(n, generator=self.gen) * scale)          # the same values at either offset
        return t.view(*shape)


def _words(ops, lr, step, dev):
    return torch.from_numpy(np.array(ops.adam_words(lr, step), np.float32)).to(dev)


def _lr(step):
    return 5e-4 * 0.1 ** ((step - 1) / 50000)


FLAT_N = (1, 4, 5, 1023, 1024, 1025, 1029)        # a block is 256 threads x 4: n % 4 in {0, 1, 3}, one full block, a second block
FLAT_SLABS = (1, 3, 4, 5, 9)                      # holding only a scalar-tail thread; the four-way unroll, its remainder, both
TAIL = ("lat", "lat_m", "lat_v", "dlat", "zero")


def _flat_forms(dev, ops, n, n_slabs, step, off, seed):
    """The three flat forms from one state -> {form: (p, m, v)}, and the tail (lat, lat_m, lat_v, dlat, zero) the net form stepped,
    next to the same six latents stepped as a blob of their own."""
    rnd = _Rnd(dev, seed)
    stride = (n + 3) // 4 * 4
    p0, m0, v0 = rnd(n, off=off), rnd(n, scale=1e-2, off=off), rnd(n, scale=1e-2, off=off).abs_()
    g = rnd(n_slabs * stride, scale=1e-2, off=off)
    lat0, lm0, lv0, dl0 = rnd(6), rnd(6, scale=1e-3), rnd(6, scale=1e-3).abs(), rnd(6, scale=1e-2)
    assert all((t.data_ptr() % 16 == 4) == bool(off) for t in (p0, m0, v0, g))
    lr = _lr(step)

    def state():                                   # clones keep the offset of the originals
        out = []
        for t in (p0, m0, v0):
            c = torch.empty(n + off, dtype=torch.float32, device=dev)[off:]
            c.copy_(t)
            out.append(c)
        return out
    out = {}
    a = state()
    ops.adam_step(*a, g, n_slabs, stride, lr, step)
    out["arg"] = a
    b = state()
    ops.adam_step_dev(*b, g, n_slabs, stride, _words(ops, lr, step, dev))
    out["dev"] = b
    c = state()
    tail = [lat0.clone(), lm0.clone(), lv0.clone(), dl0.clone(), torch.full((2,), 0.5, device=dev)]
    ops.adam_step_net(*c, g, n_slabs, stride, *tail, lr, step)
    out["net"] = c
    alone = [lat0.clone(), lm0.clone(), lv0.clone()]
    ops.adam_step(*alone, dl0, 1, 6, lr, step)
    return out, tail, alone, (p0, m0, v0)


@pytest.mark.parametrize("step", [1, 1000])
def test_flat_forms_agree_in_the_vector_and_the_scalar_kernel(dev, step):
    """npp_adam_step, npp_adam_step_dev (words from ops.adam_words) and npp_adam_step_net (6-element tail, 2-word zero) on the same
    blob, at every n / n_slabs where the kernel's paths switch; once with 16-byte aligned tensors and a slab stride of n rounded up
    to 4 (adam_kernel<4>), once with every tensor one float into its allocation (adam_kernel<1>).  The two kernels add the slabs
    in the same order and share the update, so they agree too; so does the tail with the six latents stepped as a blob."""
    from npp_amd import ops
    for n in FLAT_N:
        for n_slabs in FLAT_SLABS:
            seed = 1000 * n + 10 * n_slabs + step
            per_kernel = {}
            for off in (0, 1):
                forms, tail, alone, init = _flat_forms(dev, ops, n, n_slabs, step, off, seed)
                case = f"flat/n{n}/s{n_slabs}/t{step}/off{off}"
                for f in ("dev", "net"):
                    _same(forms["arg"], forms[f], "pmv", (case, f))
                assert not torch.equal(forms["arg"][0], init[0]), case
                _same(tail[:3], alone, TAIL, (case, "tail"))
                assert float(tail[3].abs().max()) == 0.0 and float(tail[4].abs().max()) == 0.0, case
                for f, (p, m, v) in forms.items():
                    _record(f"{case}/{f}", p=p, m=m, v=v)
                _record(f"{case}/tail", **dict(zip(TAIL, tail)))
                per_kernel[off] = forms["arg"], tail
            _same(per_kernel[0][0], per_kernel[1][0], "pmv", (n, n_slabs, step, "vector against scalar kernel"))
            _same(per_kernel[0][1], per_kernel[1][1], TAIL, (n, n_slabs, step, "tail, vector against scalar kernel"))


NET = ("p", "m", "v", "lat", "lat_m", "lat_v", "dlat", "zero", "wf", "wb")


def _net_state(dev, K, width, ksplit, seed):
    from npp_amd import ops
    from npp_amd.model import param_layout
    _, n = param_layout(K, width)
    assert n % 4                                   # the parameter count is odd: the last thread takes the cnt < 4 branch
    rnd = _Rnd(dev, seed)
    stride = (n + 3) // 4 * 4
    p = rnd(n, scale=0.1)
    st = dict(p=p, m=rnd(n, scale=1e-3), v=rnd(n, scale=1e-3).abs(), lat=rnd(6), lat_m=rnd(6, scale=1e-3), lat_v=rnd(6, scale=1e-3).abs(),
              dlat=rnd(6, scale=1e-2), zero=torch.full((2,), 0.5, device=dev))
    st["wf"], st["wb"] = ops.pack_weights(p, K, None, None, width)
    return n, stride, st, rnd(ksplit * stride, scale=1e-3)


def _fused_forms(dev, K, width, ksplit, step, seed=77):
    """-> ({form: [p, m, v, lat, lat_m, lat_v, dlat, zero, wf, wb]}, the initial state, (n, stride, g, lr))"""
    from npp_amd import ops
    n, stride, st0, g = _net_state(dev, K, width, ksplit, seed)
    lr = _lr(step)
    out = {}
    for form in ("pack", "pack_dev", "net_then_pack"):
        s = [st0[k].clone() for k in NET]
        blobs, tail, (wf, wb) = s[:3], s[3:8], s[8:]
        if form == "pack":
            ops.adam_step_net_pack(*blobs, g, ksplit, stride, *tail, lr, step, K, wf, wb, width)
        elif form == "pack_dev":
            ops.adam_step_net_pack_dev(*blobs, g, ksplit, stride, *tail, _words(ops, lr, step, dev), K, wf, wb, width)
        else:
            ops.adam_step_net(*blobs, g, ksplit, stride, *tail, lr, step)
            ops.pack_weights(blobs[0], K, wf, wb, width)
        out[form] = s
    return out, st0, (n, stride, g, lr)


@pytest.mark.parametrize("K,width,ksplit,step", [(1, 256, 1, 1), (1, 256, 5, 1), (1, 256, 5, 1000), (3, 512, 5, 1000)])
def test_fused_forms_agree(dev, K, width, ksplit, step):
    """adam_step_net_pack, adam_step_net_pack_dev and adam_step_net + pack_weights from one state: blobs, latents, the cleared
    gradient and zero words and both packs."""
    forms, st0, _ = _fused_forms(dev, K, width, ksplit, step)
    case = f"fused/K{K}/w{width}/s{ksplit}/t{step}"
    for f in ("pack_dev", "net_then_pack"):
        _same(forms["pack"], forms[f], NET, (case, f))
    a = dict(zip(NET, forms["pack"]))
    assert not torch.equal(a["p"], st0["p"]) and not torch.equal(a["wf"], st0["wf"]) and not torch.equal(a["wb"], st0["wb"])
    assert float(a["dlat"].abs().max()) == 0.0 and float(a["zero"].abs().max()) == 0.0
    for f, s in forms.items():
        _record(f"{case}/{f}", **dict(zip(NET, s)))


def test_stacked_form_steps_the_active_image_like_the_single_launch(dev):
    """npp_adam_step_net_pack_stack, M = 2 with image 1 sitting the iteration out (a hand-made npp_stack_iter record): image 0's
    blobs, latents and packs are the single fused launch's bits, image 1's are untouched."""
    from npp_amd import ops
    from npp_amd._lib import StackIter
    K, width, ksplit, step, M = 1, 256, 5, 1000, 2
    forms, st0, (n, stride, g, lr) = _fused_forms(dev, K, width, ksplit, step)
    single = dict(zip(NET, forms["pack"]))

    def rows(t, cols=None):                        # (M, cols) with both rows = t
        r = torch.zeros((M, cols or t.numel()), dtype=t.dtype, device=dev)
        r[:, :t.numel()] = t
        return r
    s = {k: rows(st0[k], stride if k in ("p", "m", "v") else None) for k in NET}
    before = {k: t.clone() for k, t in s.items()}
    it = (StackIter * M)()
    it[0].active = 1
    it[0].step_size, it[0].inv_sqrt_bc2 = map(float, ops.adam_words(lr, step))
    it_dev = torch.from_numpy(np.frombuffer(bytes(it), np.uint8).copy()).to(dev)
    pl = torch.zeros((M, ops.PIXEL_LOSS_SCRATCH), dtype=torch.float32, device=dev)      # count word 0: no partial sums to add
    cur = torch.full((M, 2), 0.25, device=dev)
    ops.adam_step_net_pack_stack(s["p"], s["m"], s["v"], n, rows(g), ksplit, stride, s["lat"], s["lat_m"], s["lat_v"], s["dlat"], 6,
                                 s["zero"], M, K, s["wf"], s["wb"], it_dev, pl, cur, width)
    for k in NET:
        assert torch.equal(s[k][0, :single[k].numel()], single[k]), ("image 0", k)
        assert torch.equal(s[k][1], before[k][1]), ("image 1", k)
    assert float((cur - 0.25).abs().max()) == 0.0 and float(pl.abs().max()) == 0.0
    _record("stack/K1/w256/s5/t1000", **s)


def test_latent_group_step_equals_words_launch_advance(dev):
    """losses.LatentGroup (what LPIPS and StyleLoss keep their latents in): adam_step(lr) against step_words + adam_launch_dev +
    adam_advance from the same state, two steps; a 64-element group of two taps, no trunk."""
    from npp_amd.losses import LPIPS, LatentGroup, StyleLoss
    assert issubclass(LPIPS, LatentGroup) and issubclass(StyleLoss, LatentGroup)
    rnd = _Rnd(dev, 5)
    inits = [rnd(40), rnd(24)]
    m0, v0 = rnd(64, scale=1e-3), rnd(64, scale=1e-3).abs()
    a, b = LatentGroup(inits, dev), LatentGroup(inits, dev)
    assert a._lat.numel() == 64 and [t.numel() for t in a.latents] == [40, 24] and a.latents[1].data_ptr() == a._lat.data_ptr() + 160
    for grp in (a, b):
        grp._lat_m.copy_(m0), grp._lat_v.copy_(v0)
        grp.lat_step = 4
    lr = 3e-4
    for i in range(2):
        d = rnd(64, scale=1e-2)
        for grp in (a, b):
            grp.zero_latent_grads()
            assert float(grp._dlat.abs().max()) == 0.0
            grp.dlatents[0].add_(d[:40]), grp.dlatents[1].add_(d[40:])
        a.adam_step(lr)
        hp = torch.from_numpy(np.array(b.step_words(lr), np.float32)).to(dev)
        b.adam_launch_dev(hp)
        b.adam_advance()
        _same((a._lat, a._lat_m, a._lat_v), (b._lat, b._lat_m, b._lat_v), ("lat", "lat_m", "lat_v"), ("latent group", i))
        assert a.lat_step == b.lat_step == 5 + i
        _record(f"latent_group/{i}", lat=a._lat, lat_m=a._lat_m, lat_v=a._lat_v)
    assert not torch.equal(a._lat, torch.cat(inits))
