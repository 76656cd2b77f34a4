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


_WORD_LRS = (5e-4, 5e-4 * 0.1 ** (1234 / 50000), 1.0, 1e-7)
_WORD_STEPS = tuple(range(1, 3001)) + (10000, 50000)


@pytest.mark.parametrize("width", npp_amd.FUSED_WIDTHS)
def test_adam_words_equal_the_librarys_rule_as_bits(width):
    """ops.adam_words is the Python statement of the one C rule (adam_words in csrc/npp_adam.h, exported as npp_adam_words, which
    every argument-form Adam entry calls): equal as bits over the fits' whole step range, in both libraries."""
    import ctypes
    L = npp_amd.lib(width)
    out = (ctypes.c_float * 2)()
    for lr in _WORD_LRS:
        got = np.empty((len(_WORD_STEPS), 2), np.float32)
        want = np.empty_like(got)
        for i, step in enumerate(_WORD_STEPS):
            assert L.npp_adam_words(lr, 0.9, 0.999, step, out) == 0
            got[i] = out[0], out[1]
            want[i] = ops.adam_words(lr, step)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), lr


@pytest.mark.parametrize("width", npp_amd.FUSED_WIDTHS)
def test_adam_words_entry_checks_its_arguments(width):
    import ctypes
    L = npp_amd.lib(width)
    assert "npp_adam_words" in SYMBOLS
    out = (ctypes.c_float * 2)()
    for args in ((5e-4, 0.9, 0.999, 0, out), (5e-4, 0.9, 0.999, -3, out), (5e-4, 0.9, 0.999, 1, None)):
        assert L.npp_adam_words(*args) == -1                     # NPP_ERR_ARG (include/npp_hip.h)
        assert b"npp_adam_words" in L.npp_last_error_string()


def test_light_adam_scalars_are_adam_words_along_the_clock():
    """NPPNetLight.adam_scalars (the word table a graphed candidate fit replays) is the sequence "ops.adam_words(net.lr, net.opt_step + 1),
    then advance the clock" -- the eager loop's own values -- and leaves the clock where it was.  The two methods read plain
    attributes only, so no device is needed."""
    from npp_amd.light import NPPNetLight
    net = object.__new__(NPPNetLight)
    net.lrate, net.lrate_decay, net.lr, net.global_step, net.opt_step = 5e-4, 500, 5e-4, 0, 0
    for _ in range(7):                                   # a clock that has run: lr is no longer lrate
        net.opt_step += 1
        net.advance_clock()
    before = (net.lr, net.global_step, net.opt_step)
    n = 3000
    tab = net.adam_scalars(n)
    assert tab.dtype == np.float32 and tab.shape == (n, 2) and (net.lr, net.global_step, net.opt_step) == before
    want = np.empty_like(tab)
    for i in range(n):
        want[i] = ops.adam_words(net.lr, net.opt_step + 1)
        net.opt_step += 1
        net.advance_clock()
    assert np.array_equal(tab.view(np.uint32), want.view(np.uint32))


def test_lr_rule_is_the_reference_schedule():
    assert ops.lr_rule(5e-4, 500, 0) == 5e-4
    assert ops.lr_rule(5e-4, 500, 1234) == 5e-4 * (0.1 ** (1234 / (500 * 100)))


@pytest.mark.parametrize("width", npp_amd.FUSED_WIDTHS)
def test_fused_adam_entries_keep_their_own_checks_and_texts(width):
    """The three forms of the fused Adam + re-pack launch share a launcher (adam_pack_go) but each reports its own rule under its own
    name, on the host, before anything is launched: step < 1 only in the argument form, the device words only in the device-word
    form, M / the strides only in the stacked form; what they share (blobs, parameter count, alignment) names the caller."""
    L = npp_amd.lib(width)
    N = None

    def pack(step):
        return L.npp_adam_step_net_pack(N, N, N, N, 0, 1, 0, N, N, N, N, 0, N, 0, 5e-4, 0.9, 0.999, 1e-8, step, 3, width, N, N, N, N, N)

    def pack_dev(hp):
        return L.npp_adam_step_net_pack_dev(N, N, N, N, 0, 1, 0, N, N, N, N, 0, N, 0, 0.9, 0.999, 1e-8, hp, 3, width, N, N, N, N, N)

    def pack_stack(M, it):
        return L.npp_adam_step_net_pack_stack(N, N, N, 0, N, 0, 1, 0, 0, N, N, N, N, 0, 6, N, 0, 1, 0.9, 0.999, 1e-8, M, 3, width, N, 0, N, 0,
                                              N, 0, N, it, N)
    words = (__import__("ctypes").c_float * 4)()
    for call, name, text in ((lambda: pack(0), "npp_adam_step_net_pack:", "step < 1"),
                             (lambda: pack(1), "npp_adam_step_net_pack:", "16-byte aligned blobs"),
                             (lambda: pack_dev(None), "npp_adam_step_net_pack_dev:", "device words"),
                             (lambda: pack_dev(words), "npp_adam_step_net_pack_dev:", "16-byte aligned blobs"),
                             (lambda: pack_stack(0, words), "npp_adam_step_net_pack_stack:", "per-image strides"),
                             (lambda: pack_stack(2, None), "npp_adam_step_net_pack_stack:", "per-image strides"),
                             (lambda: pack_stack(2, words), "npp_adam_step_net_pack_stack:", "16-byte aligned blobs and strides")):
        assert call() == -1                          # NPP_ERR_ARG
        msg = L.npp_last_error_string().decode()
        assert msg.startswith(name) and text in msg, msg
