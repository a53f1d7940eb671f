"""CPU-only: the entry points and the descriptor of the weight average (csrc/ema.hip) are declared the same way in
include/cris_hip.h and in cris/pytorch_amd/hip.py (the regex approach of tests/test_grad_accum_cpu.py), they were added
without moving the ABI version, every host-side argument check refuses what it should and says why, the host mirror of the
warm-up weight equals its closed form, and NativeTrainer validates the new arguments before it touches a device."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cris.pytorch_amd import hip  # noqa: E402
from header_decls import HEADER, ctype_of, prototypes  # noqa: E402

NEW = ("cris_ema_advance", "cris_ema_update", "cris_ema_blocks")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return hip.load()


def test_new_signatures_match_the_prototypes():
    protos = prototypes(open(HEADER).read())
    for name in NEW:
        assert name in protos, name
        assert name in hip._SIGS and name in hip.EXPORTS, name
        ret, params = protos[name]
        res, args = hip._SIGS[name]
        assert res is {"int": C.c_int, "long": C.c_long}[ret], name
        want = [ctype_of(p) for p in params.split(",")]
        assert list(args) == want, (name, args, want)
    assert [p.split()[-1] for p in protos["cris_ema_advance"][1].split(",")] == ["step_dev", "every", "decay", "warmup", "state", "stream"]
    assert [p.split()[-1] for p in protos["cris_ema_update"][1].split(",")] == ["dev_table", "n_desc", "total_blocks", "state", "stream"]


def test_descriptor_mirror(lib):
    assert [f for f, _ in hip.EmaDesc._fields_] == ["p", "ema", "n", "row_live", "row_len", "block_start"]
    assert hip.STRUCTS["cris_ema_desc"] is hip.EmaDesc
    assert lib.cris_sizeof(b"cris_ema_desc") == C.sizeof(hip.EmaDesc) == 40
    # the Adam descriptor did not grow for this
    assert lib.cris_sizeof(b"cris_adam_desc") == C.sizeof(hip.AdamDesc) == 112
    assert "ema" not in [f for f, _ in hip.AdamDesc._fields_]


def test_abi_version_did_not_move(lib):
    src = open(HEADER).read()
    assert int(re.search(r"#define CRIS_ABI_VERSION (\d+)", src).group(1)) == hip.ABI_VERSION == lib.cris_abi_version() == 8
    comment = re.search(r"/\* CRIS_ABI_VERSION moves.*?\*/", src, flags=re.S).group(0)
    assert "cris_ema_advance" in comment and "WITHOUT moving it" in comment          # the header says so, and why


def desc(**kw):
    d = hip.EmaDesc()
    d.p, d.ema, d.n = 0x10000, 0x20000, 100
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_argument_checks_without_a_gpu(lib):
    """every check returns before anything is launched: the pointers below are never dereferenced"""
    step, state = 0x1000, 0x2000
    for args, msg in (((None, 1, 0.9, 0, state), b"null"),
                      ((step, 1, 0.9, 0, None), b"null"),
                      ((step, 0, 0.9, 0, state), b"every must be >= 1"),
                      ((step, -3, 0.9, 0, state), b"every must be >= 1"),
                      ((step, 1, 0.0, 0, state), b"decay must lie in (0, 1)"),
                      ((step, 1, 1.0, 1, state), b"decay must lie in (0, 1)"),
                      ((step, 1, -0.5, 0, state), b"decay must lie in (0, 1)"),
                      ((step, 1, float("nan"), 0, state), b"decay must lie in (0, 1)"),
                      ((step, 1, 0.9, 0, state + 4), b"16-byte aligned")):
        assert lib.cris_ema_advance(*args, None) != 0, args
        err = lib.cris_last_error()
        assert b"cris_ema_advance" in err and msg in err, (args, err)
    table = 0x3000
    for args, msg in (((None, 1, 1, state), b"null"),
                      ((table, 1, 1, None), b"null"),
                      ((table, 0, 1, state), b"empty table"),
                      ((table, 2, 1, state), b"empty table"),
                      ((table, 1, 1, state + 8), b"16-byte aligned")):
        assert lib.cris_ema_update(*args, None) != 0, args
        err = lib.cris_last_error()
        assert b"cris_ema_update" in err and msg in err, (args, err)
    for d, msg in ((desc(p=None), b"null"),
                   (desc(ema=None), b"null"),
                   (desc(n=0), b"n must be > 0"),
                   (desc(n=-4), b"n must be > 0"),
                   (desc(ema=0x20004), b"ema must be 16-byte aligned"),
                   (desc(ema=0x20008), b"ema must be 16-byte aligned"),
                   (desc(row_live=0x30000), b"row_live needs row_len > 0"),
                   (desc(row_live=0x30000, row_len=-1), b"row_live needs row_len > 0")):
        assert lib.cris_ema_blocks(C.byref(d)) < 0
        err = lib.cris_last_error()
        assert b"cris_ema_blocks" in err and msg in err, err
    assert lib.cris_ema_blocks(None) < 0
    # good descriptors: the Adam kernels' partition; p may sit at any 4-byte offset
    be = lib.cris_adam_block_elems()
    assert [lib.cris_ema_blocks(C.byref(desc(n=n))) for n in (1, be - 1, be, be + 1, 2 * be + 3)] == [1, 1, 1, 2, 3]
    assert lib.cris_ema_blocks(C.byref(desc(p=0x10004, row_live=0x30000, row_len=7, n=35))) == 1


def test_host_mirror_of_the_weight():
    from cris.pytorch_amd import ops
    f = np.float32
    for decay in (0.9, 0.9999):
        for t in (0, 1, 9, 10, 1000):
            plain = ops.ema_weight(t, decay, False)
            assert isinstance(plain, np.float32) and plain == f(1) - f(decay)
            warm = ops.ema_weight(t, decay, True)
            ramp = f(1 + t) / f(10 + t)                                   # (1 + t and 10 + t are exact in fp32)
            assert isinstance(warm, np.float32) and warm == f(1) - min(f(decay), ramp)
            assert float(warm) == pytest.approx(1.0 - min(decay, (1.0 + t) / (10.0 + t)), rel=1e-6 / (1.0 - decay))
    # the ramp crosses decay = 0.9 between t = 80 ((81/90) = 0.9 exactly in the reals) and stays there
    assert ops.ema_weight(79, 0.9, True) > ops.ema_weight(1000, 0.9, True) == ops.ema_weight(1000, 0.9, False)
    assert ops.ema_weight(0, 0.9999, True) == f(1) - f(1) / f(10)


def test_trainer_validates_the_arguments():
    """raised before the state dict or the device is looked at"""
    from cris.pytorch_amd.trainer import NativeTrainer
    for kw in ({"ema_decay": 0.0}, {"ema_decay": 1.0}, {"ema_decay": -0.1}, {"ema_decay": 1.5}, {"ema_decay": "0.9"},
               {"ema_decay": True}, {"ema_decay": float("nan")},
               {"ema_decay": 0.9, "ema_every": 0}, {"ema_decay": 0.9, "ema_every": -2}, {"ema_decay": 0.9, "ema_every": 1.5},
               {"ema_decay": 0.9, "ema_every": True}, {"ema_every": 0}):
        with pytest.raises(ValueError, match="ema_"):
            NativeTrainer(None, None, None, "cpu", **kw)
    assert NativeTrainer._checked_ema(None, 1, False) == (None, 1, False)
    assert NativeTrainer._checked_ema(0.5, 3, 1) == (0.5, 3, True)
