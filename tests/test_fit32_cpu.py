"""Host-side checks of the exact-fp32 fit: the command line switch, the binding of every new C entry, StackedFit's refusal."""
import os
import re
import types

import pytest

import npp_amd
from npp_amd import ops, train
from npp_amd._lib import SYMBOLS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_train_precision_flag():
    assert train.parse(["--datadir", "x"]).precision == "bf16"
    assert train.parse(["--datadir", "x", "--precision", "fp32"]).precision == "fp32"
    assert train.parse(["--datadir", "x", "--task", "remapping", "--precision", "fp32"]).precision == "fp32"
    with pytest.raises(SystemExit):
        train.parse(["--datadir", "x", "--precision", "fp16"])


def test_every_fp32_training_entry_is_bound():
    hdr = open(os.path.join(ROOT, "include", "npp_hip.h")).read()
    declared = set(re.findall(r"\b(npp_[a-z0-9_]*32[a-z0-9_]*)\s*\(", hdr))
    new = {"npp_train_workspace32", "npp_pack32_bwd_bytes", "npp_pack_weights32_bwd", "npp_mlp_fwd32_train", "npp_mlp_bwd32",
           "npp_mlp_wgrad32"}
    assert new <= declared, new - declared
    ops_src = open(ops.__file__).read()
    for name in sorted(declared):
        assert name in SYMBOLS, name                          # ctypes signature (_lib)
        assert re.search(r"\." + name + r"\(", ops_src), name   # a wrapper in ops calls it
        for width in npp_amd.FUSED_WIDTHS:
            assert hasattr(npp_amd.lib(width), name), (name, width)
    for fn in ("train_workspace32", "pack_weights32_bwd", "mlp_fwd32_train", "mlp_bwd32", "mlp_wgrad32"):
        assert callable(getattr(ops, fn))


def test_workspace32_sizes_and_argument_checks():
    import ctypes as C
    L = npp_amd.lib()
    sizes = (C.c_int64 * 4)()
    assert L.npp_train_workspace32(3, 256, 100, 4, sizes) < 0          # Bp not a multiple of 64
    assert L.npp_train_workspace32(3, 256, 128, 4, sizes) == 0
    ref = (C.c_int64 * 4)()
    assert L.npp_train_workspace(3, 256, 128, 4, ref) == 0
    assert sizes[3] == ref[3]                                           # the slab layout and stride of the bf16 chain
    assert sizes[1] == (11 * 256 + 128 + 22 * 3) * 128 * 4 and sizes[2] == (11 * 256 + 128 + 4) * 128 * 4
    L.npp_pack32_bwd_bytes.restype = C.c_int64
    assert L.npp_pack32_bwd_bytes(1, 256) == (16 + 8 * 32) * 8 * 64 * 16      # W_p^T (16 k-step groups) + feature_linear1 and layers 7..1 (32 each)
    L512 = npp_amd.lib(512)
    assert L512.npp_train_workspace32(3, 512, 128, 4, sizes) == 0 and L.npp_train_workspace32(3, 512, 128, 4, sizes) < 0


def test_nppnet_rejects_unknown_precision_by_name():
    import inspect
    from npp_amd.model import NPPNet
    from npp_amd.fit import CompletionFit
    assert inspect.signature(NPPNet.__init__).parameters["precision"].default == "bf16"
    assert inspect.signature(CompletionFit.__init__).parameters["precision"].default == "bf16"
    with pytest.raises(ValueError, match="precision"):             # (checked before any device work)
        NPPNet([[0.0, 90.0]], [[10.0, 10.0]], [1.0] * 10, (64, 64), device="cpu", precision="fp16")


def test_stackedfit_refuses_fp32_fits_by_name():
    from npp_amd.stack import StackedFit
    fake = types.SimpleNamespace(net=types.SimpleNamespace(precision="fp32"))
    with pytest.raises(ValueError, match="precision"):
        StackedFit([fake])
