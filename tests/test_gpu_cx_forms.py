"""The contextual-loss core (csrc/npp_cx.hip) on every launch form of `cx_launch`, against float64.

Reference, case table and bounds live in tests/cx_reference.py (checked without a GPU by tests/test_cx_forms_cpu.py: which form each
case hits, that arg-min / arg-max of every case are stable in fp32, and that each named defect moves the float64 result by at least
ten bounds).  Here the kernels run:

  a. ops.cx_fwd_bwd over the table: loss and dL/dx against cx_ref, the value-only call, scale = 1e-3 next to 1;
  c. ops.cx_fwd_bwd_groups directly, on a group table built from StackIter as stack.py builds it: X = 7 samples in M = 4 groups with
     an idle one in the middle, loss_stride = 3 on a pre-filled buffer, and M = 16 groups of one sample each;
  d. ops.cx_fwd_bwd_flat: the gated bf16 gradient in the trunk's flat layout, with and without groups, N_total > N;
  e. run-to-run bits, one case per form.

Bound (b): K_LOSS * d32(case) relative on the loss, K_GRAD * d32(case) relative L2 on the gradient, d32 = the distance of the SAME
formula in float32 on the CPU from float64 on the case's own inputs (computed at test time, printed with every figure).

Measured on an MI355X, worst (kernel error / d32) per case over every figure the tests below print for it (both scales, value-only
calls, every group; d32 of the loss is floored at 2^-24, see cx_reference.LOSS_D32_FLOOR):

  case                d32 loss  worst ratio   d32 gradient  worst ratio
  fast_one_tile      5.96e-08     1.85       6.15e-07     1.10
  fast_hw32_c96      1.01e-07     0.14       8.10e-07     0.91
  fast_hw96_c128     2.14e-07     0.33       1.53e-06     0.77
  fast_9_blocks      6.89e-08     2.12       7.48e-07     1.09
  fast_hw768         9.27e-08     1.82       2.10e-06     0.87
  fast_hw800         7.64e-08     0.86       1.71e-06     0.86
  fast_hw2048        9.08e-08     1.19       1.84e-06     1.06
  gen_hw2            7.32e-08     0.66       1.03e-07     1.75
  gen_hw63           1.27e-07     1.17       7.77e-07     1.27
  gen_hw65           5.96e-08     3.06       7.04e-07     0.91
  gen_hw120          5.96e-08     0.58       1.12e-06     1.01
  gen_hw2047         7.13e-08     1.83       1.76e-06     1.16
  big_hw2049         1.15e-07     2.20       1.86e-06     1.09
  big_hw2112         8.25e-08     2.83       1.87e-06     1.07
  big_nofit_c864     1.77e-07     1.49       3.38e-06     1.13
  fast_bw0.1         9.85e-08     0.80       7.02e-07     1.03
  fast_bw1.0         5.96e-08     2.45       7.57e-07     1.49
  gen_bw0.1          1.60e-07     1.00       8.10e-07     0.91
  gen_bw1.0          5.96e-08     2.67       1.06e-06     1.42
  fast_weighted      7.27e-08     1.55       6.10e-07     1.11
  gen_weighted       5.96e-08     1.72       7.76e-07     1.27
  big_weighted       6.36e-08     1.70       1.65e-06     1.11
  groups_fast_hw64   1.13e-07     4.38       7.66e-07     1.15
  groups_gen_hw63    1.85e-07     4.72       7.96e-07     0.95
  groups_16_singles  2.76e-07     1.62       6.52e-07     1.56

Worst ratio on the loss 4.72, on the gradient 1.75.  K = the smallest power of two at or above 4 x the worst ratio:
K_LOSS = 32, K_GRAD = 8.  With them K * d32 is at most 8.8e-6 on the loss (cap 1e-5) and 3.0e-5 relative L2 on the gradient (cap 1e-4),
and every defect of the catalogue moves loss or gradient by at least 10 bounds on every case it applies to.
"""
import numpy as np
import pytest

import cx_reference as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import npp_amd
    npp_amd.lib()          # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _on(case, dev):
    x, y, wt = R.inputs(case)
    return (torch.from_numpy(np.array(x)).to(dev), torch.from_numpy(np.array(y)).to(dev),
            None if wt is None else torch.from_numpy(np.array(wt)).to(dev))


class _Figures:
    """Every figure is printed (error, d32, their ratio, the bound) before anything is asserted; the assertion comes last and names
    all that missed."""

    def __init__(self, case):
        self.case, self.missed = case, []
        self.dl, self.dg = R.d32(case)
        self.bl, self.bg = R.bounds(case)

    def loss(self, what, err):
        print(f"cx-ratio {self.case.name:18s} {what:28s} loss err {err:.3e} d32 {self.dl:.3e} ratio {err / self.dl:7.2f} bound {self.bl:.3e}")
        if not err <= self.bl:
            self.missed.append(f"{what}: loss error {err:.3e} > {self.bl:.3e}")

    def grad(self, what, err):
        print(f"cx-ratio {self.case.name:18s} {what:28s} grad err {err:.3e} d32 {self.dg:.3e} ratio {err / self.dg:7.2f} bound {self.bg:.3e}")
        if not err <= self.bg:
            self.missed.append(f"{what}: gradient error {err:.3e} > {self.bg:.3e}")

    def done(self):
        assert not self.missed, f"{self.case.name} ({self.case.pins}): " + "; ".join(self.missed)


# ---- a. ops.cx_fwd_bwd over the table ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_cx_fwd_bwd_against_float64(dev, case):
    """Loss and dL/dx of ops.cx_fwd_bwd against the float64 reference, the value-only call against the reference and against the
    call with a gradient, at scale 1 and 1e-3 (loss and gradient are linear in it)."""
    from npp_amd import ops
    x, y, wt = _on(case, dev)
    ref_l, ref_dx = R.reference(case)
    ref_l = float(ref_l[0])
    fig = _Figures(case)
    for scale in (1.0, 1e-3):
        tag = f"scale {scale:g}"
        loss, dx = ops.cx_fwd_bwd(x, y, case.band_width, wt, scale=scale)
        loss_v, none = ops.cx_fwd_bwd(x, y, case.band_width, wt, scale=scale, want_grad=False)
        torch.cuda.synchronize()
        assert none is None and dx.shape == x.shape
        assert np.isfinite(loss.item()) and bool(torch.isfinite(dx).all())
        fig.loss(f"{tag} with gradient", abs(loss.item() - scale * ref_l) / abs(scale * ref_l))
        fig.grad(f"{tag} with gradient", R.rel_l2(_np(dx), scale * ref_dx))
        fig.loss(f"{tag} value only", abs(loss_v.item() - scale * ref_l) / abs(scale * ref_l))
        fig.loss(f"{tag} value - gradient call", abs(loss_v.item() - loss.item()) / abs(scale * ref_l))
    fig.done()


# ---- c. ops.cx_fwd_bwd_groups --------------------------------------------------------------------------------------------------
def _iter_table(groups, dev):
    """The per-image table of a stacked launch, as StackedFit.step_from fills it (stack.py): one StackIter per group, idle groups
    keep their zero-initialised entry but for the running x0."""
    from npp_amd import ops
    from npp_amd._lib import StackIter
    M = len(groups)
    it = (StackIter * M)()
    for e, (x0, nk) in zip(it, groups):
        e.x0, e.nk, e.active, e.k = x0, nk, int(nk > 0), 1
    return ops.h2d(np.frombuffer(bytes(it), np.uint8).copy(), dev), M


def _prefill(M, stride, dev):
    """Known non-zero words, all different, exact in float32 and small next to the losses (the kernel ADDS to the active slots)."""
    return torch.arange(1, M * stride + 1, dtype=torch.float32, device=dev) / 1024.0


def _check_group_losses(fig, what, before, after, ref_l, stride):
    """Active slots grew by the group's reference loss; the idle slots and every padding word kept their bits."""
    b, a = before.cpu().numpy(), after.cpu().numpy()
    grown = a.astype(np.float64) - b.astype(np.float64)
    for m, rl in enumerate(ref_l):
        if rl == 0.0:
            assert a[m * stride].tobytes() == b[m * stride].tobytes(), f"{what}: idle group {m}'s loss slot changed"
        else:
            fig.loss(f"{what} group {m}", abs(grown[m * stride] - rl) / abs(rl))
    pad = np.ones(a.shape, bool)
    pad[::stride] = False
    assert a[pad].tobytes() == b[pad].tobytes(), f"{what}: padding words of the loss buffer changed"


@pytest.mark.parametrize("name", ["groups_fast_hw64", "groups_gen_hw63"])
def test_cx_groups_with_an_idle_group(dev, name):
    """X = 7 samples, M = 4 groups (0,2), (2,0), (2,1), (3,4): an idle group in the middle that shares its x0 with the next one;
    the groups' y differ in scale and offset, so a mean or a 1 / N over the wrong samples shows (tests/test_cx_forms_cpu.py)."""
    from npp_amd import ops
    case = R.case_by_name(name)
    x, y, _ = _on(case, dev)
    ref_l, ref_dx = R.reference(case)
    it_dev, M = _iter_table(case.groups, dev)
    fig = _Figures(case)
    for scale in (1.0, 1e-3):
        loss = _prefill(M, 3, dev)
        before = loss.clone()
        dx = ops.cx_fwd_bwd_groups(x, y, it_dev, M, case.band_width, scale, loss, 3)
        torch.cuda.synchronize()
        _check_group_losses(fig, f"scale {scale:g}", before, loss, scale * ref_l, 3)
        fig.grad(f"scale {scale:g}", R.rel_l2(_np(dx), scale * ref_dx))
        for m, (x0, nk) in enumerate(case.groups):
            if nk:
                fig.grad(f"scale {scale:g} group {m}", R.rel_l2(_np(dx[x0:x0 + nk]), scale * ref_dx[x0:x0 + nk]))
    fig.done()


def test_cx_groups_sixteen_single_sample_groups(dev):
    """M = 16 = NPP_MAX_STACK groups of one sample each at (16, 32, 4, 8): every sample against the float64 reference of its own
    group AND against the kernels' own N = 1 call on that sample."""
    from npp_amd import ops
    case = R.case_by_name("groups_16_singles")
    x, y, _ = _on(case, dev)
    ref_l, ref_dx = R.reference(case)
    it_dev, M = _iter_table(case.groups, dev)
    fig = _Figures(case)
    loss = _prefill(M, 3, dev)
    before = loss.clone()
    dx = ops.cx_fwd_bwd_groups(x, y, it_dev, M, case.band_width, 1.0, loss, 3)
    torch.cuda.synchronize()
    _check_group_losses(fig, "16 singles", before, loss, ref_l, 3)
    fig.grad("16 singles", R.rel_l2(_np(dx), ref_dx))
    grown = (loss.double() - before.double()).cpu().numpy()[::3]
    for n in range(16):
        l1, dx1 = ops.cx_fwd_bwd(x[n:n + 1].contiguous(), y[n:n + 1].contiguous(), case.band_width)
        fig.loss(f"sample {n} - its N = 1 call", abs(grown[n] - l1.item()) / abs(ref_l[n]))
        fig.grad(f"sample {n} - its N = 1 call", float(np.linalg.norm(_np(dx[n]) - _np(dx1[0])) / np.linalg.norm(ref_dx[n])))
        fig.grad(f"sample {n}", R.rel_l2(_np(dx[n]), ref_dx[n]))
    fig.done()


# ---- d. ops.cx_fwd_bwd_flat ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fast_one_tile", "gen_hw63", "groups_fast_hw64", "groups_gen_hw63"])
def test_cx_flat_output(dev, name):
    """dL/dx written into the trunk's flat bf16 gradient tensor, gated by [yact > 0] (yact: the features themselves as fp16, set up as
    tests/test_gpu_scratch_reuse.py does), N_total = N + 3 images in the tensor.  Per element
    |got - ref gate| <= 2^-8 |ref| + K_GRAD d32 rms(ref) (one bf16 rounding is 2^-9 relative; the factor two covers a value that sits
    on a rounding boundary), exactly zero where the gate is closed, and the images beyond N keep what they held."""
    from npp_amd import ops
    case = R.case_by_name(name)
    x, y, _ = _on(case, dev)
    N, C, h, w = case.shape
    N_total = N + 3
    ref_l, ref_dx = R.reference(case)
    fig = _Figures(case)
    rng = np.random.RandomState(7)
    feats = torch.cat([x, torch.from_numpy(np.maximum(rng.randn(3, C, h, w), 0).astype(np.float32)).to(dev)])
    held = torch.from_numpy((1.0 + rng.rand(N_total, C, h, w)).astype(np.float32)).to(dev)      # non-zero everywhere
    yact, dz = ops.trunk_alloc(N_total, C, h, w, dev), ops.trunk_alloc(N_total, C, h, w, dev)
    ops.trunk_grad_in(feats, None, N_total, N_total, C, h, w, yact, as_f16=True)
    ops.trunk_grad_in(held, None, N_total, N_total, C, h, w, dz)
    before = ops.trunk_export(dz, N_total, N_total, C, h, w)
    assert bool((before != 0).all())
    if case.groups is None:
        it_dev, M, stride = None, 0, 1
        loss = _prefill(1, 1, dev)
    else:
        (it_dev, M), stride = _iter_table(case.groups, dev), 3
        loss = _prefill(M, 3, dev)
    lb = loss.clone()
    ops.cx_fwd_bwd_flat(x, y, yact, dz, N_total, case.band_width, 1.0, loss, stride, it_dev, M)
    after = ops.trunk_export(dz, N_total, N_total, C, h, w)
    torch.cuda.synchronize()
    _check_group_losses(fig, "flat", lb, loss, ref_l, stride)
    got = _np(after[:N])
    gate = _np(x.to(torch.float16) > 0)
    want = ref_dx * gate
    rms = float(np.sqrt(np.mean(ref_dx ** 2)))
    excess = np.abs(got - want) - (2.0 ** -8 * np.abs(ref_dx) + fig.bg * rms)
    worst = np.unravel_index(np.argmax(excess), excess.shape)
    print(f"cx-flat  {case.name:18s} worst element {worst}: got {got[worst]:.6e} want {want[worst]:.6e}, "
          f"largest (|got - want| - 2^-8 |ref|) / rms(ref) = {float(np.max(np.abs(got - want) - 2.0 ** -8 * np.abs(ref_dx))) / rms:.3e} "
          f"(allowed {fig.bg:.3e})")
    assert np.all(got[gate == 0] == 0.0), "gradient behind a closed gate"
    assert excess[worst] <= 0, f"element {worst}: {got[worst]} against {want[worst]}"
    assert torch.equal(after[N:], before[N:]), "images of dz beyond N were written"
    fig.done()


# ---- e. run-to-run bits --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,grad", [("fast_hw96_c128", True), ("fast_weighted", True), ("gen_hw65", True), ("big_hw2049", True),
                                       ("big_hw2049", False), ("big_nofit_c864", False), ("groups_gen_hw63", True)])
def test_cx_run_to_run_bits(dev, name, grad):
    """The kernels claim order-independent sums: two calls, identical loss and gradient bits.  One case per form."""
    from npp_amd import ops
    case = R.case_by_name(name)
    x, y, wt = _on(case, dev)

    def call():
        if case.groups is not None:
            it_dev, M = _iter_table(case.groups, dev)
            loss = _prefill(M, 3, dev)
            return loss, ops.cx_fwd_bwd_groups(x, y, it_dev, M, case.band_width, 1.0, loss, 3)
        return ops.cx_fwd_bwd(x, y, case.band_width, wt, want_grad=grad)
    l1, d1 = call()
    l2, d2 = call()
    torch.cuda.synchronize()
    assert torch.equal(l1.view(torch.int32), l2.view(torch.int32))
    if grad:
        assert torch.equal(d1.view(torch.int32), d2.view(torch.int32))
