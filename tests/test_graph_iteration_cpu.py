"""Host-side checks of the captured iteration (CompletionFit(graph_iteration=True)): the command line switch, the refusals by
name as far as they can be reached without a device, the new C entry and its argument check, the host arithmetic of the scalar
record.  No GPU calls."""
import math
import os
import re

import numpy as np
import pytest

import npp_amd
from npp_amd import ops, train
from npp_amd._lib import SYMBOLS
from npp_amd.fit import refuse_graph_iteration

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_train_graph_iteration_flag():
    assert train.parse(["--datadir", "x"]).graph_iteration is False
    a = train.parse(["--datadir", "x", "--graph_iteration"])
    assert a.graph_iteration is True and (a.precision, a.trunk_precision) == ("bf16", "fp16")


def test_run_passes_graph_iteration_through_train_args():
    import shlex
    assert train.parse(["--datadir", "."] + shlex.split("--graph_iteration --rng_mode device")).graph_iteration is True


@pytest.mark.parametrize("flags,name", [(["--precision", "fp32"], "--precision fp32"),
                                        (["--trunk_precision", "fp32"], "--trunk_precision fp32"),
                                        (["--task", "remapping"], "--task remapping")])
def test_the_command_line_refuses_by_name(flags, name):
    """_plan refuses before it touches weights, data or the device."""
    with pytest.raises(SystemExit) as e:
        train._plan(["--datadir", "does-not-exist", "--graph_iteration"] + flags)
    assert name in str(e.value) and "--graph_iteration" in str(e.value)


@pytest.mark.parametrize("kw,name", [(dict(precision="fp32"), "precision='fp32'"), (dict(trunk_precision="fp32"), "trunk_precision='fp32'"),
                                     (dict(task="remapping"), "task='remapping'"), (dict(style_weight=1.0), "style_weight=1.0")])
def test_the_constructor_refusal_names_the_switch(kw, name):
    a = dict(precision="bf16", trunk_precision="fp16", task="completion", style_weight=None)
    refuse_graph_iteration(a["precision"], a["trunk_precision"], a["task"], a["style_weight"], ValueError)       # the built mode passes
    refuse_graph_iteration("bf16", "fp16", "segmentation", None, ValueError)
    a.update(kw)
    with pytest.raises(ValueError) as e:
        refuse_graph_iteration(a["precision"], a["trunk_precision"], a["task"], a["style_weight"], ValueError)
    assert name in str(e.value) and "graph_iteration=True" in str(e.value)


def test_stack_key_keeps_graph_fits_out_of_a_stack():
    src = open(train.__file__).read()
    body = src[src.index("def stack_key(job):"):src.index("def plan_key(plan):")]
    assert "f.graph_iteration" in body                                          # as trunk_precision: such a fit runs the plain loop


def test_library_exports_the_device_word_adam_pack_entry():
    hdr = open(os.path.join(ROOT, "include", "npp_hip.h")).read()
    declared = set(re.findall(r"\b(npp_[a-z0-9_]+)\s*\(", hdr))
    name = "npp_adam_step_net_pack_dev"
    assert name in declared and name in SYMBOLS
    assert re.search(r"\." + name + r"\(", open(ops.__file__).read())
    for w in npp_amd.FUSED_WIDTHS:
        L = npp_amd.lib(w)
        # no record pointer / no blobs: reported on the host, nothing launched
        rc = L.npp_adam_step_net_pack_dev(None, None, None, None, 0, 1, 0, None, None, None, None, 0, None, 0, 0.9, 0.999, 1e-8, None, 3, w,
                                          None, None, None, None, None)
        assert rc < 0 and b"npp_adam_step_net_pack_dev" in L.npp_last_error_string()


def test_adam_words_are_the_argument_forms_host_arithmetic():
    """npp_adam_step / npp_adam_step_net_pack: float arguments widened to double, pow / sqrt in double, results rounded to float."""
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
    for lr in (5e-4, 5e-4 * 0.1 ** (1234 / 50000), 1.0):
        for step in (1, 2, 1000, 2800):
            ss, inv = ops.adam_words(lr, step)
            assert ss.dtype == np.float32 and inv.dtype == np.float32
            assert ss == np.float32(float(np.float32(lr)) / (1.0 - b1 ** step))
            assert inv == np.float32(1.0 / math.sqrt(1.0 - b2 ** step))
