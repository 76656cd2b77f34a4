"""The census core on the GPU (csrc/npp_census.h; DESIGN.md section 6j "census core"): both census launches on the inputs of
tests/test_census_core_cpu.py -- every code of e4m3, e5m2 and fp16 among the counted elements -- against their plain C++ twins, word
for word, with the guard words around the record intact."""
import numpy as np
import pytest

import census_every_code as E

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


def _guarded(dev, words, launch):
    buf = torch.full((words + 16,), GUARD, dtype=torch.int64, device=dev)
    launch(buf[8:8 + words])
    got = buf.cpu().numpy()
    assert (got[:8] == GUARD).all() and (got[8 + words:] == GUARD).all()
    return got[8:8 + words]


def test_stash_census_counts_every_code(dev):
    from npp_amd import ops
    from npp_amd._lib import census_layout
    K, W, Bp, n_rows = (E.STASH[k] for k in ("K", "W", "Bp", "n_rows"))
    act, dz = E.stash_buffers(ops.train_workspace(K, Bp, 1, W))
    want = ops.stash8_census_host(act, dz, Bp, n_rows, K, W)
    act_d, dz_d = torch.from_numpy(act).to(dev), torch.from_numpy(dz).to(dev)
    got = _guarded(dev, census_layout(K, W)[2], lambda rec: ops.stash8_census(act_d, dz_d, Bp, n_rows, K, rec, W))
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("with_ref", [False, True])
def test_trunk_census_counts_every_code(dev, with_ref):
    from npp_amd import ops
    from npp_amd._lib import TRUNK_CENSUS_WORDS
    flat, ref = E.trunk_tensor()
    want = ops.trunk16_census_host(flat, *E.TRUNK, ref32=ref if with_ref else None)
    act_d = torch.from_numpy(flat.view(np.int16)).to(dev)
    ref_d = torch.from_numpy(ref).to(dev) if with_ref else None
    got = _guarded(dev, TRUNK_CENSUS_WORDS, lambda rec: ops.trunk16_census(act_d, *E.TRUNK, ref32=ref_d, record=rec))
    np.testing.assert_array_equal(got, want)
