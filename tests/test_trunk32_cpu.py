"""Host-side checks of the exact-fp32 trunks (trunk_precision="fp32"): the command line switch, the new C entries and their
argument checks, the defaults of the public classes, StackedFit's refusal.  No GPU calls."""
import inspect
import os
import re
import types

import pytest

import npp_amd
from npp_amd import ops, train
from npp_amd._lib import SYMBOLS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("npp_conv32_pack_bytes", "npp_conv32_pack", "npp_conv32", "npp_maxpool2_fwd32", "npp_maxpool2_bwd32")


def test_train_trunk_precision_flag():
    assert train.parse(["--datadir", "x"]).trunk_precision == "fp16"
    a = train.parse(["--datadir", "x", "--trunk_precision", "fp32"])
    assert a.trunk_precision == "fp32" and a.precision == "bf16"                 # independent of --precision
    a = train.parse(["--datadir", "x", "--task", "remapping", "--precision", "fp32", "--trunk_precision", "fp32"])
    assert (a.precision, a.trunk_precision) == ("fp32", "fp32")
    with pytest.raises(SystemExit):
        train.parse(["--datadir", "x", "--trunk_precision", "bf16"])


def test_run_passes_trunk_precision_through_train_args():
    import shlex
    a = train.parse(["--datadir", "."] + shlex.split("--trunk_precision fp32 --precision fp32"))
    assert a.trunk_precision == "fp32"


def test_library_exports_the_fp32_trunk_entries():
    hdr = open(os.path.join(ROOT, "include", "npp_hip.h")).read()
    declared = set(re.findall(r"\b(npp_[a-z0-9_]+)\s*\(", hdr))
    ops_src = open(ops.__file__).read()
    for name in NEW:
        assert name in declared and name in SYMBOLS, name
        assert re.search(r"\." + name + r"\(", ops_src), name                   # a wrapper in ops calls it
        for width in npp_amd.FUSED_WIDTHS:
            assert hasattr(npp_amd.lib(width), name), (name, width)
    for fn in ("conv32_pack", "conv32", "maxpool2_fwd32", "maxpool2_bwd32"):
        assert callable(getattr(ops, fn))
    assert os.path.exists(os.path.join(os.path.dirname(ops.__file__), "csrc", "npp_conv32.hip"))


def test_conv32_pack_sizes_and_argument_checks():
    L = npp_amd.lib()
    # [32-channel output tiles][8-channel input chunks][9 taps][4 channel pairs][2][32] floats, zero padded
    assert L.npp_conv32_pack_bytes(3, 64, 0) == 2 * 1 * 9 * 256 * 4             # image layer: Cin 3 padded to one chunk of 8
    assert L.npp_conv32_pack_bytes(3, 64, 1) == 1 * 8 * 9 * 256 * 4             # its data gradient: 3 outputs padded to one tile of 32
    assert L.npp_conv32_pack_bytes(256, 512, 0) == 16 * 32 * 9 * 256 * 4 == L.npp_conv32_pack_bytes(512, 256, 1)
    assert L.npp_conv32_pack_bytes(48, 64, 0) < 0 and L.npp_conv32_pack_bytes(64, 3, 0) < 0 and L.npp_conv32_pack_bytes(64, 64, 2) < 0
    # argument checks come before any launch: null pointers / unsupported channel counts / n_run > N_total are refused
    assert L.npp_conv32(None, 1, 1, 8, 8, 64, 64, None, 0, None, None, None, None, None, None, None, None, None) < 0
    assert L.npp_maxpool2_fwd32(None, 1, 1, 8, 8, 64, None, None) < 0
    assert L.npp_maxpool2_bwd32(None, None, None, 1, 2, 8, 8, 64, 1, None, None) < 0
    assert b"npp_maxpool2_bwd32" in L.npp_last_error_string()


def test_trunk_precision_defaults_and_values():
    from npp_amd.fit import CompletionFit
    from npp_amd.losses import ContextualLoss, LPIPS, StyleLoss, HipTrunk, HipTrunk32, _trunk_class
    for cls in (CompletionFit, ContextualLoss, LPIPS, StyleLoss):
        assert inspect.signature(cls.__init__).parameters["trunk_precision"].default == "fp16", cls
    assert _trunk_class("fp16") is HipTrunk and _trunk_class("fp32") is HipTrunk32
    assert list(inspect.signature(HipTrunk32.__init__).parameters) == list(inspect.signature(HipTrunk.__init__).parameters)
    with pytest.raises(ValueError, match="trunk_precision"):
        _trunk_class("bf16")
    with pytest.raises(ValueError, match="trunk_precision"):                     # (checked before any device work)
        ContextualLoss(use_vgg=True, device="cpu", trunk_precision="tf32")


def test_stackedfit_refuses_fp32_trunk_fits_by_name():
    from npp_amd.stack import StackedFit
    fake = types.SimpleNamespace(net=types.SimpleNamespace(precision="bf16"), trunk_precision="fp32")
    with pytest.raises(ValueError, match="trunk_precision"):
        StackedFit([fake])
