"""CPU-only: the configurable segmentation loss (weighted BCE + soft Dice: cris_seg_loss_fwd / cris_seg_loss_bwd /
cris_seg_loss_ws_floats) is declared the same way in include/cris_hip.h and in cris/pytorch_amd/hip.py (the regex approach of
tests/test_adamw_cpu.py), it was added without moving the ABI version, every host-side argument check refuses what it should and
says why, ops.SegLoss and NativeTrainer validate the settings before they touch a device, the default spec is no spec, and the
drop-in CRIS module reads the four optional cfg keys."""
import ctypes as C
import os
import re
import sys
from types import SimpleNamespace as NS

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cris.pytorch_amd import hip, ops  # noqa: E402
from cris.pytorch_amd.ops import SegLoss  # noqa: E402
from header_decls import HEADER, ctype_of, prototypes  # noqa: E402

NAMES = ("cris_seg_loss_fwd", "cris_seg_loss_bwd", "cris_seg_loss_ws_floats")
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return hip.load()


# ---- ops.SegLoss ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [
    dict(bce_weight=-0.1), dict(dice_weight=-1.0), dict(bce_weight=0.0, dice_weight=0.0), dict(bce_weight=0), dict(pos_weight=0.0),
    dict(pos_weight=-2.0), dict(dice_smooth=0.0), dict(dice_smooth=-1e-3),
    dict(bce_weight=NAN), dict(dice_weight=NAN), dict(pos_weight=NAN), dict(dice_smooth=NAN),
    dict(bce_weight=INF), dict(dice_weight=INF), dict(pos_weight=INF), dict(dice_smooth=INF), dict(dice_weight=-INF),
    dict(dice_weight="1.0"), dict(pos_weight=None), dict(dice_smooth=[1.0]), dict(bce_weight=True)])
def test_seg_loss_refuses_bad_values(kw):
    with pytest.raises(ValueError):
        SegLoss(**kw)


def test_seg_loss_fields_defaults_and_normalisation():
    d = SegLoss()
    assert (d.bce_weight, d.dice_weight, d.pos_weight, d.dice_smooth) == (1.0, 0.0, 1.0, 1.0) == d.scalars
    with pytest.raises(Exception):                       # frozen
        d.dice_weight = 1.0
    assert SegLoss.normalized(None) is None
    assert SegLoss.normalized(SegLoss()) is None
    assert SegLoss.normalized(SegLoss(1, 0, 1, 1)) is None               # integers are the same numbers
    assert SegLoss.normalized(SegLoss(bce_weight=1.0, dice_weight=0.0, pos_weight=1.0, dice_smooth=1.0)) is None
    for spec in (SegLoss(dice_weight=1.0), SegLoss(pos_weight=2.5), SegLoss(bce_weight=0.5), SegLoss(bce_weight=0.0, dice_weight=1.0),
                 SegLoss(dice_weight=1.0, dice_smooth=1e-3)):
        assert SegLoss.normalized(spec) is spec
    s = SegLoss(bce_weight=0, dice_weight=2, pos_weight=3, dice_smooth=1e-3)
    assert s.scalars == (0.0, 2.0, 3.0, 1e-3) and all(type(v) is float for v in s.scalars)
    for bad in (1.0, "dice", {"dice_weight": 1.0}, (1.0, 1.0, 1.0, 1.0)):
        with pytest.raises(ValueError):
            SegLoss.normalized(bad)


def test_trainer_validates_the_loss_without_a_gpu():
    from cris.pytorch_amd.trainer import NativeTrainer
    for bad in (1.0, "dice", {"dice_weight": 1.0}):
        with pytest.raises(ValueError, match="loss"):
            NativeTrainer(None, None, None, "cpu", loss=bad)             # before the state dict or the device is looked at


# ---- the C interface --------------------------------------------------------------------------------------------------------
def test_signatures_match_the_prototypes():
    protos = prototypes(open(HEADER).read())
    for name in NAMES:
        assert name in protos and name in hip._SIGS and name in hip.EXPORTS, name
        ret, params = protos[name]
        res, args = hip._SIGS[name]
        assert {"int": C.c_int, "long": C.c_long}[ret] is res, name
        assert list(args) == [ctype_of(p) for p in params.split(",")], name
    names = lambda n: [p.split()[-1].lstrip("*") for p in protos[n][1].split(",")]           # noqa: E731
    assert names("cris_seg_loss_fwd") == ["logits", "target", "Bn", "HW", "w_bce", "w_dice", "pw", "s", "loss", "terms", "coef", "ws", "stream"]
    assert names("cris_seg_loss_bwd") == ["logits", "target", "Bn", "HW", "w_bce", "w_dice", "pw", "s", "coef", "gscale", "dlogits", "stream"]
    assert names("cris_seg_loss_ws_floats") == ["Bn"]
    # the four scalars travel as plain floats
    for n in ("cris_seg_loss_fwd", "cris_seg_loss_bwd"):
        assert [p.strip() for p in protos[n][1].split(",")][4:8] == ["float w_bce", "float w_dice", "float pw", "float s"]
    # the BCE entry points are still what they were
    assert hip._SIGS["cris_bce_fwd"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p])
    assert hip._SIGS["cris_bce_bwd"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p])


def test_abi_version_did_not_move_and_the_header_says_why(lib):
    src = open(HEADER).read()
    assert int(re.search(r"#define CRIS_ABI_VERSION (\d+)", src).group(1)) == hip.ABI_VERSION == lib.cris_abi_version() == 8
    comment = re.search(r"/\* CRIS_ABI_VERSION moves.*?\*/", src, flags=re.S).group(0)
    assert all(n in comment for n in NAMES)
    tail = comment[comment.index("cris_seg_loss_fwd"):]
    assert "without moving it" in tail
    # the sentences before it are still there, in their order
    assert "cris_ema_advance" in comment and "WITHOUT moving it" in comment
    order = [comment.index(n) for n in ("cris_step_advance took", "cris_eval_iou_batch", "cris_grad_sumsq", "cris_grad_accumulate", "cris_ema_advance",
                                        "cris_adam_schedule_lrs", "cris_adamw_step", "cris_seg_loss_fwd")]
    assert order == sorted(order)
    assert comment.count("without moving it") >= 3


def test_workspace_size(lib):
    assert lib.cris_seg_loss_ws_floats(1) > 0
    assert lib.cris_seg_loss_ws_floats(8) == 8 * lib.cris_seg_loss_ws_floats(1)          # a fixed slice count per sample
    assert lib.cris_seg_loss_ws_floats(1) % 4 == 0
    assert lib.cris_seg_loss_ws_floats(0) == 0


def test_argument_checks_without_a_gpu(lib):
    """every check returns before anything is launched: the pointers below are never dereferenced"""
    x, t, loss, terms, coef, ws, gs, dx = (0x1000 * (i + 1) for i in range(8))
    fwd = [x, t, 2, 5, 1.0, 1.0, 1.0, 1.0, loss, terms, coef, ws]
    bwd = [x, t, 2, 5, 1.0, 1.0, 1.0, 1.0, coef, gs, dx]

    def bad(good, i, v):
        a = list(good)
        a[i] = v
        return a
    scalars = [((4, -1.0), b">= 0"), ((5, -0.5), b">= 0"), ((6, 0.0), b"pw must be > 0"), ((6, -1.0), b"pw must be > 0"),
               ((7, 0.0), b"s must be > 0"), ((7, -1.0), b"s must be > 0"), ((4, NAN), b"finite"), ((5, INF), b"finite"),
               ((6, NAN), b"finite"), ((7, INF), b"finite")]
    sizes = [((2, 0), b"Bn must be >= 1"), ((2, -3), b"Bn must be >= 1"), ((3, 0), b"HW must be >= 1"), ((3, -1), b"HW must be >= 1")]
    for fn, good, nulls in ((lib.cris_seg_loss_fwd, fwd, (0, 1, 8, 9, 10, 11)), (lib.cris_seg_loss_bwd, bwd, (0, 1, 8, 10))):
        name = fn.__name__.encode()
        cases = [(bad(good, i, None), b"null operand") for i in nulls] + [(bad(good, i, v), msg) for (i, v), msg in scalars + sizes]
        both = list(good)
        both[4] = both[5] = 0.0
        cases.append((both, b"must not both be 0"))
        for args, msg in cases:
            assert fn(*args, None) != 0, (name, args)
            err = lib.cris_last_error()
            assert name in err and msg in err, (name, args, err)
    # gscale may be null (no scale factor), as for cris_bce_bwd; an operand off a 16-byte boundary is refused by the forward
    assert lib.cris_seg_loss_fwd(*bad(fwd, 0, x + 4), None) != 0 and b"16-byte aligned" in lib.cris_last_error()
    assert lib.cris_seg_loss_fwd(*bad(fwd, 11, ws + 8), None) != 0 and b"16-byte aligned" in lib.cris_last_error()


# ---- the drop-in module -----------------------------------------------------------------------------------------------------
TINY = dict(clip_pretrain="synthetic:tiny", word_len=9, fpn_in=[128, 256, 128], fpn_out=[64, 128, 256], num_layers=2,
            vis_dim=128, num_head=2, dim_ffn=256, dropout=0.1, intermediate=False, word_dim=128, base_lr=1e-4, lr_multi=0.1)


def test_cris_reads_the_loss_keys_of_the_cfg():
    from cris.pytorch_amd.model import CRIS
    from cris.pytorch_amd.model.segmenter import seg_loss_from_cfg
    assert CRIS(NS(**TINY)).loss_spec is None                            # every shipped yaml
    assert CRIS(dict(TINY)).loss_spec is None
    m = CRIS(NS(loss_dice_weight=1.0, **TINY))
    assert m.loss_spec == SegLoss(dice_weight=1.0)
    m = CRIS(dict(TINY, loss_bce_weight=0.5, loss_dice_weight=2, loss_pos_weight=3.0, loss_dice_smooth=1e-3))
    assert m.loss_spec == SegLoss(0.5, 2.0, 3.0, 1e-3)
    assert CRIS(NS(loss_bce_weight=1.0, loss_dice_weight=0.0, **TINY)).loss_spec is None          # the defaults, spelled out
    assert seg_loss_from_cfg(NS(loss_pos_weight=2.0)) == SegLoss(pos_weight=2.0)
    with pytest.raises(ValueError):
        CRIS(NS(loss_dice_weight=-1.0, **TINY))
    with pytest.raises(ValueError):
        seg_loss_from_cfg(dict(loss_bce_weight=0.0))


def test_shipped_configs_have_no_loss_keys():
    import glob
    yamls = glob.glob(os.path.join(ROOT, "**", "*.yaml"), recursive=True)
    for y in yamls:
        assert "loss_" not in open(y).read(), y


def test_engine_set_loss_normalises_without_a_device():
    from cris.pytorch_amd.engine import Engine
    e = object.__new__(Engine)                           # no constructor: no device, no library
    e.set_loss(SegLoss())
    assert e.loss_spec is None and e.loss_terms is None
    e.set_loss(SegLoss(dice_weight=1.0))
    assert e.loss_spec == SegLoss(dice_weight=1.0) and e.loss_terms is None
    e.set_loss(None)
    assert e.loss_spec is None
    with pytest.raises(ValueError):
        e.set_loss("dice")
    assert ops.SegLoss is SegLoss
