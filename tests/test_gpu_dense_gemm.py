"""The fp32 dense-layer GEMM (csrc/npp_linear.hip: one kernel body behind the npp_linear_* / npp_gram_* entry points) on every
operand form, load path and split path, against references that no HIP kernel takes part in.

Exact sweep.  Operands are integer-valued fp32 in [-3, 3], biases and the prior contents of accumulated outputs integers in [-8, 8]:
every product and every partial sum, in any order, is an integer below 2^24 (tests/test_gemm_plan_cpu.py checks that for every
case), so the fp32 MFMA gives the true value and so does a float atomicAdd in any arrival order.  The reference is the int64 matmul
on the CPU and the assertion is equality -- a dropped or doubled k element of a ragged range, a bias added by two ranges, an edge
clamp one element off all change an integer.  Every matrix sits inside a wider buffer filled with a sentinel (also between its rows
where it has a leading dimension); the whole buffer is compared, so a store outside the matrix fails too, and a load outside it
brings the sentinel into the sums.  The cases (tests/gemm_plan_restatement.py) list the path they are there for; each asserts, from
the arguments it is about to pass, that the restated launcher takes that path.

Rounding tests.  Gaussian data against the float64 evaluation of the same formula by relative L2; bound: 4 x the distance of the
float32 CPU evaluation from the float64 one on the test's own inputs, floor 1e-6 (the convention of tests/test_gpu_scratch_reuse.py)."""
import ctypes as C

import numpy as np
import pytest

import gemm_plan_restatement as R

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(R.fill_overridden(), reason="NPP_GEMM_BATCH_FILL is set: the restated plan holds the default fills")]

SENTINEL = -7777.25


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import npp_amd
    npp_amd.lib()
    return torch.device("cuda:0")


def _L():
    from npp_amd._lib import lib
    return lib()


def _s():
    from npp_amd import ops
    return ops._stream()


def _ok(rc, c):
    assert rc == 0, f"{R.name(c)}: rc {rc}: {_L().npp_last_error_string()}"


class Buf:
    """A flat sentinel-filled buffer that holds one or more matrices (R.Lay); `h` is the host's picture of what the device buffer
    has to hold: the inputs as uploaded (up()), the outputs once put() has written the reference into it after the launch."""

    def __init__(self, dev, *lays):
        self.dev, self.h, self.d = dev, torch.full((max(l.size for l in lays),), SENTINEL), None

    def hv(self, lay):
        v = self.h.as_strided(lay.shape, lay.strides, lay.start)
        return v[0] if lay.nb is not None and lay.sb == 0 else v           # one matrix shared by the batches

    def put(self, lay, vals):
        self.hv(lay).copy_(vals.to(torch.float32))
        return self

    def up(self):
        self.d = self.h.to(self.dev)
        assert self.d.data_ptr() % 16 == 0
        return self

    def ptr(self, lay):
        return C.c_void_p(self.d.data_ptr() + 4 * lay.start)

    def addr16(self, lay):
        return (self.d.data_ptr() + 4 * lay.start) % 16

    def dv(self, lay):
        return self.d.as_strided(lay.shape, lay.strides, lay.start)

    def bad(self, skip=None):
        """'' when the device buffer holds exactly the host's picture (values and sentinels; `skip`: a matrix whose values are
        judged elsewhere -- only its surroundings are compared)."""
        got = self.d.cpu()
        if skip is not None:
            self.hv(skip).copy_(got.as_strided(skip.shape, skip.strides, skip.start))
        if torch.equal(got, self.h):
            return ""
        idx = torch.nonzero(got != self.h).flatten()
        i = int(idx[0])
        return f"{idx.numel()} of {got.numel()} floats differ, first at flat index {i}: {float(got[i])!r} for {float(self.h[i])!r}"


def _gen(tag, i):
    return torch.Generator().manual_seed(1000003 * (sum(map(ord, tag)) % 997) + i)


def _ints(g, shape, m=R.OPERAND_MAX):
    return torch.randint(-m, m + 1, tuple(shape), generator=g, dtype=torch.int64)


def _pick(g, shape, values):
    return torch.tensor(values, dtype=torch.float64)[torch.randint(0, len(values), tuple(shape), generator=g)]


def _path(c, *plans):
    """The plan restated from the arguments about to be passed is the table's plan, and shows the path the case is listed for."""
    assert tuple(plans) == tuple(R.case_plans(c)), f"{R.name(c)}: plan from the tensors {plans} is not the table's {R.case_plans(c)}"
    m = R.path_mismatch(c, plans)
    assert not m, f"{R.name(c)}: {m}"
    return f"{R.name(c)} | " + " ; ".join(f"{p.form} splits={p.splits} kchunk={p.kchunk} vec_a={p.vec_a} vec_b={p.vec_b} grid={p.grid} {p.mode}"
                                          for p in plans)


def _cases(fam):
    return [(i, c) for i, c in enumerate(R.all_cases()) if c["fam"] == fam]


# ---- exact sweep ---------------------------------------------------------------------------------------------------------------
def test_forward_exact(dev):
    """npp_linear_fwd: act 0 / 1 / 2, with and without z and bias, x and y dense or column blocks; the split contraction (the bias
    arrives once) and the same shapes through a wider y (one range) give the same integers."""
    L = _L()
    for i, c in _cases("fwd"):
        B, cin, cout, act = c["B"], c["cin"], c["cout"], c["act"]
        lay, g = R.fwd_lays(c), _gen("fwd", i)
        x, w = _ints(g, (B, cin)), _ints(g, (cout, cin))
        b = _ints(g, (cout,), R.PRIOR_MAX) if c["bias"] else None
        bx, bw, by, bz = Buf(dev, lay["x"]).put(lay["x"], x).up(), Buf(dev, lay["w"]).put(lay["w"], w).up(), Buf(dev, lay["y"]).up(), Buf(dev, lay["z"]).up()
        bb = Buf(dev, R.Lay(1, cout)).put(R.Lay(1, cout), b).up() if c["bias"] else None
        what = _path(c, R.plan_linear_fwd(B, cin, cout, act, lay["x"].ld, lay["y"].ld, c["z"], bx.addr16(lay["x"]), bw.addr16(lay["w"])))
        _ok(L.npp_linear_fwd(bx.ptr(lay["x"]), lay["x"].ld, bw.ptr(lay["w"]), bb.ptr(R.Lay(1, cout)) if bb else None, B, cin, cout, act,
                             by.ptr(lay["y"]), lay["y"].ld, bz.ptr(lay["z"]) if c["z"] else None, lay["z"].ld if c["z"] else 0, _s()), c)
        z = x @ w.T + (b if b is not None else 0)
        if act != 1:
            by.put(lay["y"], z.clamp(min=0) if act == 2 else z)
        if c["z"]:
            bz.put(lay["z"], z)
        for nm, buf, skip in (("y", by, lay["y"] if act == 1 else None), ("z", bz, None), ("x", bx, None), ("w", bw, None)):
            m = buf.bad(skip)
            assert not m, f"{what}: {nm}: {m}"


def test_data_gradient_exact(dev):
    """npp_linear_bwd_data: in_used columns of w taken from column 0 / 1 / 4 of a wider matrix, accumulate on and off, the split
    contraction with dense dx."""
    L = _L()
    for i, c in _cases("bwd_data"):
        B, cout, used = c["B"], c["cout"], c["used"]
        lay, g = R.bwd_data_lays(c), _gen("bwd_data", i)
        dz, w, prior = _ints(g, (B, cout)), _ints(g, (cout, c["cin"])), _ints(g, (B, used), R.PRIOR_MAX)
        bdz, bw, bdx = Buf(dev, lay["dz"]).put(lay["dz"], dz).up(), Buf(dev, lay["w"]).put(lay["w"], w).up(), Buf(dev, lay["dx"])
        if c["acc"]:
            bdx.put(lay["dx"], prior)
        bdx.up()
        what = _path(c, R.plan_linear_bwd_data(B, lay["w"].ld, cout, used, lay["dz"].ld, lay["dx"].ld, c["acc"], bdz.addr16(lay["dz"]),
                                               bw.addr16(lay["w"])))
        _ok(L.npp_linear_bwd_data(bdz.ptr(lay["dz"]), lay["dz"].ld, bw.ptr(lay["w"]), B, lay["w"].ld, cout, bdx.ptr(lay["dx"]), lay["dx"].ld,
                                  used, int(c["acc"]), _s()), c)
        bdx.put(lay["dx"], dz @ w[:, :used] + (prior if c["acc"] else 0))
        for nm, buf in (("dx", bdx), ("dz", bdz), ("w", bw)):
            m = buf.bad()
            assert not m, f"{what}: {nm}: {m}"


def test_weight_gradient_exact(dev):
    """npp_linear_bwd_weight: dw and db (or no db), accumulate on and off, dz and x dense or column blocks, one to 32 k ranges."""
    L = _L()
    for i, c in _cases("bwd_weight"):
        B, cin, cout = c["B"], c["cin"], c["cout"]
        lay, g = R.bwd_weight_lays(c), _gen("bwd_weight", i)
        dz, x = _ints(g, (B, cout)), _ints(g, (B, cin))
        pw, pb = _ints(g, (cout, cin), R.PRIOR_MAX), _ints(g, (1, cout), R.PRIOR_MAX)
        bdz, bx = Buf(dev, lay["dz"]).put(lay["dz"], dz).up(), Buf(dev, lay["x"]).put(lay["x"], x).up()
        bdw, bdb = Buf(dev, lay["dw"]), Buf(dev, lay["db"])
        if c["acc"]:
            bdw.put(lay["dw"], pw)
            bdb.put(lay["db"], pb)
        bdw.up()
        bdb.up()
        what = _path(c, R.plan_linear_bwd_weight(B, cin, cout, lay["dz"].ld, lay["x"].ld, c["acc"], bdz.addr16(lay["dz"]), bx.addr16(lay["x"])))
        _ok(L.npp_linear_bwd_weight(bdz.ptr(lay["dz"]), lay["dz"].ld, bx.ptr(lay["x"]), lay["x"].ld, B, cin, cout, bdw.ptr(lay["dw"]),
                                    bdb.ptr(lay["db"]) if c["db"] else None, int(c["acc"]), _s()), c)
        bdw.put(lay["dw"], dz.T @ x + (pw if c["acc"] else 0))
        if c["db"]:
            bdb.put(lay["db"], dz.sum(0, keepdim=True) + (pb if c["acc"] else 0))
        for nm, buf in (("dw", bdw), ("db", bdb), ("dz", bdz), ("x", bx)):
            m = buf.bad()
            assert not m, f"{what}: {nm}: {m}"


_ZY = {4: [-1.0, 0.0, 1.0], 2: [0.0, 0.5, 1.0], 3: [-1.0, -0.5, 0.0, 0.5, 1.0]}


def _deriv(zy, kind):
    return (zy > 0).to(torch.float64) if kind == 4 else (zy * (1 - zy) if kind == 2 else 1 - zy * zy)


def test_batched_forms_exact(dev):
    """npp_linear_fwd_batched / _bwd_data_batched / _bwd_weight_batched over 1, 2 and 5 problems: weights and biases as rows of one
    blob (row length a multiple of 4, and odd), x shared with batch stride 0, in_used < in, the folded activation derivatives
    (kinds 2 / 3 / 4 at inputs where they are dyadic) against float64 AND against npp_act_bwd on the unfolded product, the weight
    gradient called twice = twice the gradient."""
    L = _L()
    for fam in ("fwd_b", "bwd_data_b", "bwd_weight_b"):
        for i, c in _cases(fam):
            nb, B, cin, cout = c["nb"], c["B"], c["cin"], c["cout"]
            lay, g = R.batched_lays(c), _gen(fam, i)
            if fam == "bwd_weight_b":
                dz, x = _ints(g, (nb, B, cout)), _ints(g, (nb, B, cin))
                bdz, bx = Buf(dev, lay["dz"]).put(lay["dz"], dz).up(), Buf(dev, lay["x"]).put(lay["x"], x).up()
                shared = c["where"] != "dense"
                bdw = Buf(dev, lay["dw"], lay["db"]) if shared else Buf(dev, lay["dw"])
                bdb = bdw if shared else Buf(dev, lay["db"])
                pw, pb = _ints(g, (nb, cout, cin), R.PRIOR_MAX), _ints(g, (nb, 1, cout), R.PRIOR_MAX)
                bdw.put(lay["dw"], pw)
                bdb.put(lay["db"], pb)
                bdw.up()
                if not shared:
                    bdb.up()
                what = _path(c, R.plan_linear_bwd_weight(B, cin, cout, lay["dz"].ld, lay["x"].ld, True, bdz.addr16(lay["dz"]), bx.addr16(lay["x"]),
                                                         nb, lay["dz"].sb, lay["x"].sb, lay["dw"].sb))
                for rep in (1, 2):
                    _ok(L.npp_linear_bwd_weight_batched(bdz.ptr(lay["dz"]), lay["dz"].ld, lay["dz"].sb, bx.ptr(lay["x"]), lay["x"].ld, lay["x"].sb,
                                                        nb, B, cin, cout, bdw.ptr(lay["dw"]), lay["dw"].sb, bdb.ptr(lay["db"]), lay["db"].sb, _s()), c)
                    bdw.put(lay["dw"], pw + rep * (dz.transpose(1, 2) @ x))
                    bdb.put(lay["db"], pb + rep * dz.sum(1, keepdim=True))
                    for nm, buf in (("dw", bdw), ("db", bdb), ("dz", bdz), ("x", bx)):
                        m = buf.bad()
                        assert not m, f"{what}: call {rep}: {nm}: {m}"
                continue
            w, b = _ints(g, (nb, cout, cin)), _ints(g, (nb, 1, cout), R.PRIOR_MAX)
            blob = Buf(dev, lay["w"], lay["b"]).put(lay["w"], w).put(lay["b"], b).up()
            if fam == "fwd_b":
                x = _ints(g, (B, cin)) if c["shared"] else _ints(g, (nb, B, cin))
                bx, by, bz = Buf(dev, lay["x"]).put(lay["x"], x).up(), Buf(dev, lay["y"]).up(), Buf(dev, lay["z"]).up()
                what = _path(c, R.plan_linear_fwd(B, cin, cout, c["act"], lay["x"].ld, lay["y"].ld, c["z"], bx.addr16(lay["x"]),
                                                  blob.addr16(lay["w"]), nb, lay["x"].sb, lay["w"].sb, lay["y"].sb))
                _ok(L.npp_linear_fwd_batched(bx.ptr(lay["x"]), lay["x"].ld, lay["x"].sb, blob.ptr(lay["w"]), lay["w"].sb, blob.ptr(lay["b"]),
                                             lay["b"].sb, nb, B, cin, cout, c["act"], by.ptr(lay["y"]), lay["y"].ld, lay["y"].sb,
                                             bz.ptr(lay["z"]) if c["z"] else None, lay["z"].ld if c["z"] else 0, lay["z"].sb if c["z"] else 0,
                                             _s()), c)
                z = x @ w.transpose(1, 2) + b
                by.put(lay["y"], z.clamp(min=0) if c["act"] == 2 else z)
                if c["z"]:
                    bz.put(lay["z"], z)
                bufs = (("y", by), ("z", bz), ("x", bx), ("blob", blob))
            else:
                used, kind = c["used"], c["dact"]
                dz, prior = _ints(g, (nb, B, cout)), _ints(g, (nb, B, used), R.PRIOR_MAX)
                bdz, bdx, bzy = Buf(dev, lay["dz"]).put(lay["dz"], dz).up(), Buf(dev, lay["dx"]), Buf(dev, lay["zy"])
                zy = _pick(g, (nb, B, used), _ZY[kind]) if kind else None
                if kind:
                    bzy.put(lay["zy"], zy)
                if c["acc"]:
                    bdx.put(lay["dx"], prior)
                bdx.up()
                bzy.up()
                what = _path(c, R.plan_linear_bwd_data(B, cin, cout, used, lay["dz"].ld, lay["dx"].ld, c["acc"], bdz.addr16(lay["dz"]),
                                                       blob.addr16(lay["w"]), nb, lay["dz"].sb, lay["w"].sb, lay["dx"].sb, dact=kind != 0))

                def call(zy_ptr, k):
                    _ok(L.npp_linear_bwd_data_batched(bdz.ptr(lay["dz"]), lay["dz"].ld, lay["dz"].sb, blob.ptr(lay["w"]), lay["w"].sb, nb, B, cin,
                                                      cout, bdx.ptr(lay["dx"]), lay["dx"].ld, lay["dx"].sb, used, int(c["acc"]), zy_ptr,
                                                      lay["zy"].ld if k else 0, lay["zy"].sb if k else 0, k, _s()), c)
                prod = (dz @ w[:, :, :used]).to(torch.float64)
                if kind:                                    # the unfolded product through npp_act_bwd, on the same data
                    call(None, 0)
                    two = torch.empty(nb, B, used, device=dev)
                    for q in range(nb):
                        _ok(L.npp_act_bwd(C.c_void_p(bdx.dv(lay["dx"])[q].data_ptr()), lay["dx"].ld, C.c_void_p(bzy.dv(lay["zy"])[q].data_ptr()),
                                          lay["zy"].ld, B, used, kind, C.c_void_p(two[q].data_ptr()), used, _s()), c)
                    bdx.put(lay["dx"], prod)
                    m = bdx.bad()
                    assert not m, f"{what}: unfolded product: {m}"
                    call(bzy.ptr(lay["zy"]), kind)
                    assert torch.equal(bdx.dv(lay["dx"]), two), f"{what}: folded derivative differs from npp_act_bwd on the product"
                    bdx.put(lay["dx"], prod * _deriv(zy, kind))
                else:
                    call(None, 0)
                    bdx.put(lay["dx"], prod + (prior if c["acc"] else 0))
                bufs = (("dx", bdx), ("dz", bdz), ("zy", bzy), ("blob", blob))
            for nm, buf in bufs:
                m = buf.bad()
                assert not m, f"{what}: {nm}: {m}"


def test_strided_weight_gradient_exact(dev):
    """npp_linear_bwd_weight_strided (x_snake off): the four row-major / feature-major combinations of dz and x, x with more features
    than the layer reads, dw with ld == in (split from 256 rows on) and ld > in (one range), 1 and 3 problems; it accumulates."""
    L = _L()
    for i, c in _cases("strided"):
        nb, B, cin, cout = c["nb"], c["B"], c["cin"], c["cout"]
        lay, g = R.strided_lays(c), _gen("strided", i)
        dz, x = _ints(g, (nb, B, cout)), _ints(g, (nb, B, cin + 3))
        pw, pb = _ints(g, (nb, cout, cin), R.PRIOR_MAX), _ints(g, (nb, 1, cout), R.PRIOR_MAX)
        bdz = Buf(dev, lay["dz"]).put(lay["dz"], dz.transpose(1, 2) if c["fm_dz"] else dz).up()
        bx = Buf(dev, lay["x"]).put(lay["x"], x.transpose(1, 2) if c["fm_x"] else x).up()
        bdw, bdb = Buf(dev, lay["dw"]).put(lay["dw"], pw).up(), Buf(dev, lay["db"]).put(lay["db"], pb).up()
        dz_sr, dz_so = (1, lay["dz"].ld) if c["fm_dz"] else (lay["dz"].ld, 1)
        x_sr, x_si = (1, lay["x"].ld) if c["fm_x"] else (lay["x"].ld, 1)
        what = _path(c, R.plan_linear_bwd_weight_strided(B, cin, cout, dz_sr, dz_so, lay["dz"].sb, x_sr, x_si, lay["x"].sb, nb, lay["dw"].ld,
                                                         lay["dw"].sb, bdz.addr16(lay["dz"]), bx.addr16(lay["x"])))
        _ok(L.npp_linear_bwd_weight_strided(bdz.ptr(lay["dz"]), dz_sr, dz_so, lay["dz"].sb, bx.ptr(lay["x"]), x_sr, x_si, lay["x"].sb, 0, nb, B,
                                            cin, cout, bdw.ptr(lay["dw"]), lay["dw"].ld, lay["dw"].sb, bdb.ptr(lay["db"]), lay["db"].sb, _s()), c)
        bdw.put(lay["dw"], pw + dz.transpose(1, 2) @ x[:, :, :cin])
        bdb.put(lay["db"], pb + dz.sum(1, keepdim=True))
        for nm, buf in (("dw", bdw), ("db", bdb), ("dz", bdz), ("x", bx)):
            m = buf.bad()
            assert not m, f"{what}: {nm}: {m}"


def _gram_scratch(N, Cc, hw, dev):
    n = int(_L().npp_gram_fwd_det_scratch_bytes(N, Cc, hw))
    return torch.full((n,), 255, dtype=torch.uint8, device=dev), n          # 0xFF bytes: "no initial content required"


def test_gram_exact(dev):
    """npp_gram_fwd (atomic split) and npp_gram_fwd_det (two-pass split, its scratch filled with 0xFF bytes) against F F^T;
    npp_gram_bwd (two launches, split only for one sample) against (dG + dG^T) F."""
    L = _L()
    for i, c in _cases("gram_fwd") + _cases("gram_bwd"):
        N, Cc, hw = c["N"], c["C"], c["hw"]
        lf, lg, g = R.Lay(Cc, hw, nb=N), R.Lay(Cc, Cc, nb=N), _gen("gram", i)
        f = _ints(g, (N, Cc, hw))
        bf = Buf(dev, lf).put(lf, f).up()
        if c["fam"] == "gram_fwd":
            bg = Buf(dev, lg).up()
            what = _path(c, R.plan_gram_fwd(N, Cc, hw, bf.addr16(lf), det=c["det"]))
            if c["det"]:
                ws, n = _gram_scratch(N, Cc, hw, dev)
                _ok(L.npp_gram_fwd_det(bf.ptr(lf), N, Cc, hw, bg.ptr(lg), C.c_void_p(ws.data_ptr()), n, _s()), c)
            else:
                _ok(L.npp_gram_fwd(bf.ptr(lf), N, Cc, hw, bg.ptr(lg), _s()), c)
            bg.put(lg, f @ f.transpose(1, 2))
            bufs = (("G", bg), ("F", bf))
        else:
            dg = _ints(g, (N, Cc, Cc))
            bdg, bdf = Buf(dev, lg).put(lg, dg).up(), Buf(dev, lf).up()
            what = _path(c, *R.plan_gram_bwd(N, Cc, hw, bdg.addr16(lg), bf.addr16(lf)))
            _ok(L.npp_gram_bwd(bdg.ptr(lg), bf.ptr(lf), N, Cc, hw, bdf.ptr(lf), _s()), c)
            bdf.put(lf, (dg + dg.transpose(1, 2)) @ f)
            bufs = (("dF", bdf), ("dG", bdg), ("F", bf))
        for nm, buf in bufs:
            m = buf.bad()
            assert not m, f"{what}: {nm}: {m}"


# ---- rounding tests ------------------------------------------------------------------------------------------------------------
def _rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _np(t):
    return t.detach().cpu().numpy()


def _judge(tag, got, f, *inputs, bound=None):
    """f evaluated on the float64 and the float32 inputs (CPU): the kernel's distance from the float64 value within 4 x the float32
    evaluation's (floor 1e-6), or within `bound` where one is given."""
    r64, r32 = f(*[t.double() for t in inputs]), f(*[t.float() for t in inputs])
    d32, err = _rel_l2(_np(r32), _np(r64)), _rel_l2(_np(got), _np(r64))
    lim = max(4.0 * d32, 1e-6) if bound is None else bound
    print(f"{tag}: kernel {err:.3g}  fp32-CPU {d32:.3g}  bound {lim:.3g}")
    assert err <= lim, (tag, err, d32, lim)


def _snake(z):
    return z + torch.sin(z) ** 2


def _randn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def _twice(run):
    a = run().clone()
    b = run().clone()
    torch.cuda.synchronize()
    return a, torch.equal(a, b)


def test_forward_and_data_gradient_rounding(dev):
    """The largest contractions of the sweep, split and in one range (the one-range forms twice: same bits); the snake epilogue
    against z + sin^2 z and the folded snake derivative (kind 1) against 1 + sin 2z, both in float64."""
    from npp_amd import ops
    g = torch.Generator().manual_seed(11)
    B, cin, cout = 5, 2052, 64
    x, w, b = _randn(g, B, cin), _randn(g, cout, cin, scale=cin ** -0.5), _randn(g, cout)
    xd, wd, bd = x.to(dev), w.to(dev), b.to(dev)
    lin = lambda x, w, b: x @ w.T + b                                                     # noqa: E731
    assert R.plan_linear_fwd(B, cin, cout, 0, cin, cout, False, 0, 0).splits == 22
    _judge("fwd split", ops.linear_fwd(xd, wd, bd, 0, torch.empty(B, cout, device=dev)), lin, x, w, b)
    wide = torch.empty(B, cout + 3, device=dev)
    y, same = _twice(lambda: ops.linear_fwd(xd, wd, bd, 0, wide[:, :cout]))
    assert same, "npp_linear_fwd in one range does not repeat its bits"
    _judge("fwd one range", y, lin, x, w, b)
    z = torch.empty(B, cout, device=dev)
    y, same = _twice(lambda: ops.linear_fwd(xd, wd, bd, 1, torch.empty(B, cout, device=dev), z))
    assert same, "npp_linear_fwd with snake does not repeat its bits"
    _judge("fwd snake y", y, lambda x, w, b: _snake(lin(x, w, b)), x, w, b)
    _judge("fwd snake z", z, lin, x, w, b)
    B, cin, cout = 10, 128, 2050
    dz, w = _randn(g, B, cout), _randn(g, cout, cin, scale=cin ** -0.5)
    dzd, wd = dz.to(dev), w.to(dev)
    assert R.plan_linear_bwd_data(B, cin, cout, cin, cout, cin, False, 0, 0).splits == 22
    _judge("bwd_data split", ops.linear_bwd_data(dzd, wd, torch.empty(B, cin, device=dev)), lambda dz, w: dz @ w, dz, w)
    wide = torch.empty(B, cin + 4, device=dev)
    dx, same = _twice(lambda: ops.linear_bwd_data(dzd, wd, wide[:, :cin]))
    assert same, "npp_linear_bwd_data in one range does not repeat its bits"
    _judge("bwd_data one range", dx, lambda dz, w: dz @ w, dz, w)
    nb = 2
    dz, w, zy = _randn(g, nb, B, cout), _randn(g, nb, cout, cin, scale=cin ** -0.5), _randn(g, nb, B, cin)
    dzd, wd, zyd = dz.to(dev), w.to(dev), zy.to(dev)
    dx, same = _twice(lambda: ops.linear_bwd_data_batched(dzd, wd, torch.empty(nb, B, cin, device=dev), zy=zyd, act=1))
    assert same, "npp_linear_bwd_data_batched does not repeat its bits"
    _judge("bwd_data batched, snake derivative folded", dx, lambda dz, w, zy: (dz @ w) * (1 + torch.sin(2 * zy)), dz, w, zy)
    x, w, b = _randn(g, nb, B, cout), _randn(g, nb, cin, cout, scale=cout ** -0.5), _randn(g, nb, cin)
    y, same = _twice(lambda: ops.linear_fwd_batched(x.to(dev), w.to(dev), b.to(dev), 1, torch.empty(nb, B, cin, device=dev)))
    assert same, "npp_linear_fwd_batched does not repeat its bits"
    _judge("fwd batched snake", y, lambda x, w, b: _snake(x @ w.transpose(1, 2) + b[:, None, :]), x, w, b)


def test_weight_gradient_rounding(dev):
    """npp_linear_bwd_weight at 2100 rows (22 ranges), the batched form at 2048 (32 ranges), the strided form at 2048 rows split
    (ld == in) and in one range (ld > in, twice: same bits)."""
    from npp_amd import ops
    g = torch.Generator().manual_seed(12)
    B, cin, cout = 2100, 33, 1
    dz, x = _randn(g, B, cout), _randn(g, B, cin)
    dw, db = torch.empty(cout, cin, device=dev), torch.empty(cout, device=dev)
    assert R.plan_linear_bwd_weight(B, cin, cout, cout, cin, False, 0, 0).splits == 22
    ops.linear_bwd_weight(dz.to(dev), x.to(dev), dw, db)
    _judge("bwd_weight split dw", dw, lambda dz, x: dz.T @ x, dz, x)
    _judge("bwd_weight split db", db, lambda dz: dz.sum(0), dz)
    nb, B, cin, cout = 2, 2048, 64, 64
    dz, x = _randn(g, nb, B, cout), _randn(g, nb, B, cin + 3)
    dzd, xd = dz.to(dev), x.to(dev)
    wgrad = lambda dz, x: dz.transpose(1, 2) @ x[:, :, :cin]                               # noqa: E731
    dw, db = torch.zeros(nb, cout, cin, device=dev), torch.zeros(nb, cout, device=dev)
    ops.linear_bwd_weight_batched(dzd, xd[:, :, :cin], dw, db)
    _judge("bwd_weight batched split dw", dw, wgrad, dz, x)
    _judge("bwd_weight batched split db", db, lambda dz: dz.sum(1), dz)
    dw.zero_()
    db.zero_()
    ops.linear_bwd_weight_strided(dzd, xd, dw, db, False, False)
    _judge("strided split dw", dw, wgrad, dz, x)
    _judge("strided split db", db, lambda dz: dz.sum(1), dz)

    def one_range():
        wide, db1 = torch.zeros(nb, cout, cin + 2, device=dev), torch.zeros(nb, cout, device=dev)
        ops.linear_bwd_weight_strided(dzd.transpose(1, 2).contiguous(), xd.transpose(1, 2).contiguous(), wide[:, :, :cin], db1, True, True)
        return torch.cat([wide[:, :, :cin], db1[:, :, None]], 2)
    got, same = _twice(one_range)
    assert same, "npp_linear_bwd_weight_strided in one range does not repeat its bits"
    _judge("strided one range dw", got[:, :, :cin], wgrad, dz, x)
    _judge("strided one range db", got[:, :, cin], lambda dz: dz.sum(1), dz)


def test_strided_weight_gradient_with_snake_on_the_operand(dev):
    """x_snake=True: x holds pre-activations z and the layer input is snake(z), evaluated with the hardware sine on the way into LDS.
    Bound: rel_l2 < 2e-5, the project's bound for hardware sine against precise sinf (test_gpu_light.py, fused chains against the
    layer-by-layer path), with z drawn from a standard normal.  Nobody has measured the range of the stashed pre-activations of real
    ranking fits against this bound: outside a few units the hardware sine's argument reduction may cost more than it does here."""
    from npp_amd import ops
    g = torch.Generator().manual_seed(13)
    nb, B, cin, cout = 2, 2048, 64, 64
    dz, z = _randn(g, nb, B, cout), _randn(g, nb, B, cin)
    f = lambda dz, z: dz.transpose(1, 2) @ _snake(z)                                       # noqa: E731
    for fm in (False, True):
        dw, db = torch.zeros(nb, cout, cin, device=dev), torch.zeros(nb, cout, device=dev)
        zd = z.transpose(1, 2).contiguous().to(dev) if fm else z.to(dev)
        ops.linear_bwd_weight_strided(dz.to(dev), zd, dw, db, False, fm, x_snake=True)
        _judge(f"strided x_snake feature_major_x={fm}", dw, f, dz, z, bound=2e-5)


def test_gram_rounding(dev):
    """npp_gram_fwd / _det at (1, 128, 2050) (22 ranges; the two-pass form twice: same bits -- the atomic form is documented as
    order-dependent), npp_gram_bwd split (1, 512, 9) and in one range (2, 256, 36; twice: same bits)."""
    L = _L()
    g = torch.Generator().manual_seed(14)
    N, Cc, hw = 1, 128, 2050
    f = _randn(g, N, Cc, hw)
    fd, G = f.to(dev), torch.empty(N, Cc, Cc, device=dev)
    gram = lambda f: f @ f.transpose(1, 2)                                                 # noqa: E731
    assert L.npp_gram_fwd(C.c_void_p(fd.data_ptr()), N, Cc, hw, C.c_void_p(G.data_ptr()), _s()) == 0
    _judge("gram_fwd atomic", G, gram, f)

    def det():
        ws, n = _gram_scratch(N, Cc, hw, dev)
        assert L.npp_gram_fwd_det(C.c_void_p(fd.data_ptr()), N, Cc, hw, C.c_void_p(G.data_ptr()), C.c_void_p(ws.data_ptr()), n, _s()) == 0
        return G
    got, same = _twice(det)
    assert same, "npp_gram_fwd_det does not repeat its bits"
    _judge("gram_fwd two-pass", got, gram, f)
    for (N, Cc, hw), split in (((1, 512, 9), True), ((2, 256, 36), False)):
        assert all((p.splits > 1) == split for p in R.plan_gram_bwd(N, Cc, hw))
        f, dg = _randn(g, N, Cc, hw), _randn(g, N, Cc, Cc)
        fd, dgd, df = f.to(dev), dg.to(dev), torch.empty(N, Cc, hw, device=dev)

        def bwd():
            assert L.npp_gram_bwd(C.c_void_p(dgd.data_ptr()), C.c_void_p(fd.data_ptr()), N, Cc, hw, C.c_void_p(df.data_ptr()), _s()) == 0
            return df
        got, same = _twice(bwd)
        assert split or same, "npp_gram_bwd in one range does not repeat its bits"
        _judge(f"gram_bwd {'split' if split else 'one range'}", got, lambda dg, f: (dg + dg.transpose(1, 2)) @ f, dg, f)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_act_fwd_rounding(dev, n):
    """npp_act_fwd: identity, sigmoid, tanh against float64 at sizes around one block."""
    from npp_amd import ops
    x = _randn(torch.Generator().manual_seed(n), n, scale=2.0)
    for kind, f in ((0, lambda x: x), (2, torch.sigmoid), (3, torch.tanh)):
        buf = torch.full((n + 8,), SENTINEL, device=dev)
        ops.act_fwd(x.to(dev), kind, buf[4:4 + n])
        assert float(buf[:4].max()) == SENTINEL == float(buf[4 + n:].min()), f"kind {kind}: wrote outside its {n} elements"
        _judge(f"act_fwd kind {kind} n={n}", buf[4:4 + n], f, x)
