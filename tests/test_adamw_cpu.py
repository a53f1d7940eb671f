"""CPU-only: cris_adamw_step (per-tensor weight decay, coupled or decoupled, in the fused Adam update) is declared the same way in
include/cris_hip.h and in cris/pytorch_amd/hip.py (the regex approach of tests/test_lr_schedule_cpu.py), it was added without
moving the ABI version or the Adam descriptor, every host-side argument check refuses what it should and says why, the ready-made
no_decay rules exempt what the reference's group_weight (utils/misc.py:168-189) exempts - derived here from the module types - and
ops.AdamTable.set_decay / NativeTrainer validate the decay settings before they touch a device."""
import ctypes as C
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cris.pytorch_amd import hip  # noqa: E402
from header_decls import HEADER, ctype_of, prototypes  # noqa: E402

NAME = "cris_adamw_step"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return hip.load()


def test_signature_matches_the_prototype():
    protos = prototypes(open(HEADER).read())
    assert NAME in protos and NAME in hip._SIGS and NAME in hip.EXPORTS
    ret, params = protos[NAME]
    res, args = hip._SIGS[NAME]
    assert ret == "int" and res is C.c_int
    assert list(args) == [ctype_of(p) for p in params.split(",")]
    assert [p.split()[-1].lstrip("*") for p in params.split(",")] == [
        "dev_table", "n_desc", "total_blocks", "beta1", "beta2", "eps", "decay_of", "decoupled", "bias_corr1", "bias_corr2", "grad_scale",
        "step_dev", "loss_scale_dev", "skip_dev", "pack_taps", "stream"]
    # cris_adam_step_amp with the scalar replaced by (decay_of, decoupled): every other parameter as there, in its order
    amp = [p.split()[-1].lstrip("*") for p in protos["cris_adam_step_amp"][1].split(",")]
    assert [x for x in amp if x != "weight_decay"] == [p.split()[-1].lstrip("*") for p in params.split(",") if p.split()[-1].lstrip("*")
                                                       not in ("decay_of", "decoupled")]
    assert "const cris_adam_desc*" in params.split(",")[0] and "const float*" in params.split(",")[6]      # both tables are read only


def test_descriptor_and_abi_version_did_not_move(lib):
    assert lib.cris_sizeof(b"cris_adam_desc") == C.sizeof(hip.AdamDesc) == 112
    src = open(HEADER).read()
    assert int(re.search(r"#define CRIS_ABI_VERSION (\d+)", src).group(1)) == hip.ABI_VERSION == lib.cris_abi_version() == 8
    comment = re.search(r"/\* CRIS_ABI_VERSION moves.*?\*/", src, flags=re.S).group(0)
    tail = comment[comment.index(NAME):]
    assert "without moving it" in tail
    # the sentences before it are still there
    assert "cris_ema_advance" in comment and "WITHOUT moving it" in comment
    assert "cris_adam_schedule_lrs" in comment and comment.index("cris_adam_schedule_lrs") < comment.index(NAME)
    assert comment.count("without moving it") >= 2


def test_argument_checks_without_a_gpu(lib):
    """every check returns before anything is launched: the pointers below are never dereferenced"""
    tab, dec, step, scale, skip = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    good = [tab, 4, 7, 0.9, 0.999, 1e-8, dec, 1, 1.0, 1.0, 1.0, step, scale, skip, 1]

    def bad(i, v):
        a = list(good)
        a[i] = v
        return tuple(a)
    for args, msg in ((bad(0, None), b"null dev_table"), (bad(6, None), b"null decay_of"),
                      (bad(1, 0), b"n_desc must be >= 1"), (bad(1, -3), b"n_desc must be >= 1"),
                      (bad(2, 0), b"total_blocks must be >= 1"), (bad(2, -1), b"total_blocks must be >= 1"),
                      (bad(14, 0), b"pack_taps must be 1 or 9"), (bad(14, 3), b"pack_taps must be 1 or 9"), (bad(14, -9), b"pack_taps must be 1 or 9"),
                      (bad(7, 2), b"decoupled must be 0 or 1"), (bad(7, -1), b"decoupled must be 0 or 1")):
        assert lib.cris_adamw_step(*args, None) != 0, args
        err = lib.cris_last_error()
        assert NAME.encode() in err and msg in err, (args, err)


# ---- the ready-made no_decay rules against the module types ------------------------------------------------------------------
def expected_exempt():
    """{parameter name: exempt?} of the tiny spec, from the TYPE of the module that owns each parameter: everything a BatchNorm /
    LayerNorm owns and every bias is exempt (group_weight's weight_decay=0 group); every weight of a Conv / Linear / Embedding /
    MultiheadAttention and every bare projection or positional matrix is decayed.  The one scalar (logit_scale, which the trainer
    never updates) has no decay either."""
    import torch.nn as nn
    from cris.pytorch_amd import arch
    clip, head = arch.specs_by_name("tiny")
    tree = arch.build_param_tree(clip, head)
    norms = (nn.modules.batchnorm._BatchNorm, nn.LayerNorm)
    out, kinds = {}, set()
    for mname, mod in tree.named_modules():
        for pname, p in mod.named_parameters(recurse=False):
            full = (mname + "." if mname else "") + pname
            if isinstance(mod, norms):
                out[full] = True
                kinds.add("norm")
            elif pname in ("bias", "in_proj_bias"):
                out[full] = True
                kinds.add("bias")
            elif full == "backbone.logit_scale":
                out[full] = True
            else:
                assert isinstance(mod, (nn.Conv2d, nn.Linear, nn.Embedding, nn.MultiheadAttention)) or pname in ("positional_embedding", "text_projection"), full
                out[full] = False
                kinds.add(type(mod).__name__ if pname in ("weight", "in_proj_weight") else pname)
    assert set(out) == {n for n, _ in tree.named_parameters()}
    assert {"norm", "bias", "Conv2d", "Linear", "Embedding", "MultiheadAttention", "positional_embedding", "text_projection"} <= kinds
    return tree, out


def test_no_decay_rules_match_the_module_types():
    from cris.pytorch_amd.trainer import no_decay_1d, no_decay_1d_and_positional
    tree, want = expected_exempt()
    params = dict(tree.named_parameters())
    got = {n: no_decay_1d(n, p) for n, p in params.items()}
    assert all(isinstance(v, bool) for v in got.values())
    assert got == want, [n for n in want if got[n] != want[n]][:5]
    assert 0 < sum(want.values()) < len(want)
    for n in ("backbone.token_embedding.weight", "backbone.positional_embedding", "backbone.visual.attnpool.positional_embedding",
              "backbone.text_projection", "backbone.visual.conv1.weight", "proj.txt.weight"):
        assert got[n] is False, n
    for n in ("backbone.visual.bn1.weight", "backbone.ln_final.weight", "backbone.ln_final.bias", "proj.txt.bias",
              "backbone.transformer.resblocks.0.attn.in_proj_bias"):
        assert got[n] is True, n
    got2 = {n: no_decay_1d_and_positional(n, p) for n, p in params.items()}
    assert all(isinstance(v, bool) for v in got2.values())
    extra = {n for n in params if got2[n] != got[n]}
    assert extra == {n for n in params if "positional_embedding" in n} and len(extra) == 2
    assert all(got2[n] for n in extra)


# ---- validation before a device is touched -----------------------------------------------------------------------------------
BAD_DECAYS = (-0.01, float("nan"), float("inf"), -float("inf"), "0.1", None, [0.1], True)


def test_adam_table_validates_decays_without_a_gpu():
    from cris.pytorch_amd import ops
    tab = object.__new__(ops.AdamTable)                  # no constructor: no device, no library
    tab.params = [None, None, None]
    for bad in BAD_DECAYS:
        with pytest.raises(ValueError):
            tab.set_decay([0.0, bad, 0.1], True)
        with pytest.raises(ValueError):
            ops.AdamTable.checked_decay("w", bad)
    for bad in (0.1, [0.1, 0.2], [0.1] * 4, "abc"):      # not a sequence, or not one value per tensor
        with pytest.raises(ValueError):
            tab.set_decay(bad, False)
    with pytest.raises(ValueError):
        tab.set_decay([0.0, 0.0, 0.0], 1)                # decoupled is a bool
    assert not hasattr(tab, "decays")                    # nothing was stored by a refused call
    assert ops.AdamTable.checked_decays([0, 0.5, 1e-2], 3) == [0.0, 0.5, 0.01]
    tab.decays, tab.decoupled = [0.0] * 3, True
    with pytest.raises(ValueError, match="weight_decay"):
        tab.step(weight_decay=0.01)                      # next to a list: refused before the library is looked at
    tab.set_decay(None)
    assert tab.decays is None and tab.decoupled is False


def test_trainer_validates_weight_decay_settings_without_a_gpu():
    from cris.pytorch_amd import arch
    from cris.pytorch_amd.trainer import NativeTrainer, no_decay_1d
    for bad in BAD_DECAYS:
        with pytest.raises(ValueError, match="weight_decay"):
            NativeTrainer(None, None, None, "cpu", weight_decay=bad)         # before the state dict or the device is looked at
        with pytest.raises(ValueError, match="weight_decay"):
            NativeTrainer(None, None, None, "cpu", weight_decay=bad, decoupled_weight_decay=True, no_decay=no_decay_1d)
    for bad in (0, 1.5, "bias", [no_decay_1d]):
        with pytest.raises(ValueError, match="no_decay"):
            NativeTrainer(None, None, None, "cpu", weight_decay=0.01, no_decay=bad)
    # a rule that does not answer with a bool: refused on the tensors of the state dict as given, before the engine is built
    # (clip / head are None: building it would fail with another exception)
    clip, head = arch.specs_by_name("tiny")
    sd = arch.synthetic_state_dict(clip, head, 0)
    for answer in (1, 0, None, "yes", 0.0):
        with pytest.raises(ValueError, match="no_decay"):
            NativeTrainer(None, None, sd, "cpu", weight_decay=0.01, no_decay=lambda n, t: answer)
    import torch
    with pytest.raises(ValueError, match="no_decay"):
        NativeTrainer(None, None, sd, "cpu", weight_decay=0.01, no_decay=lambda n, t: torch.tensor(t.dim() <= 1))
    assert NativeTrainer._checked_weight_decay(0, 0, None) == (0.0, False, None)
    assert NativeTrainer._exempt(no_decay_1d, [("a.weight", sd["proj.txt.weight"]), ("a.bias", sd["proj.txt.bias"])]) == {"a.bias"}
