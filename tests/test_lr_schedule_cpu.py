"""CPU-only: the entry point of the per-step learning-rate schedule (csrc/lr.hip) is declared the same way in include/cris_hip.h and
in cris/pytorch_amd/hip.py (the regex approach of tests/test_ema_cpu.py), it was added without moving the ABI version or the Adam
descriptor, every host-side argument check refuses what it should and says why, the tables of cris.pytorch_amd.lr equal torch's
schedulers stepped on the CPU, and ops.LrSchedule / NativeTrainer validate a table before they touch a device."""
import ctypes as C
import os
import re
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cris.pytorch_amd import hip, lr  # noqa: E402
from header_decls import HEADER, ctype_of, prototypes  # noqa: E402

NAME = "cris_adam_schedule_lrs"
BASE = [1e-5, 1e-4]                 # two groups
N = 12


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
    assert [p.split()[-1].lstrip("*") for p in params.split(",")] == ["dev_table", "n_desc", "group_of", "step_dev", "lr_table", "n_rows",
                                                                     "n_groups", "lr_out", "stream"]
    assert "cris_adam_desc*" in params.split(",")[0] and "const" not in params.split(",")[0]      # the one table that is written


def test_descriptor_and_abi_version_did_not_move(lib):
    assert lib.cris_sizeof(b"cris_adam_desc") == C.sizeof(hip.AdamDesc) == 112
    assert hip.AdamDesc.lr.offset == 40 and hip.AdamDesc.lr.size == 4
    src = open(HEADER).read()
    assert int(re.search(r"#define CRIS_ABI_VERSION (\d+)", src).group(1)) == hip.ABI_VERSION == lib.cris_abi_version() == 8
    comment = re.search(r"/\* CRIS_ABI_VERSION moves.*?\*/", src, flags=re.S).group(0)
    assert NAME in comment and "without moving it" in comment
    assert "cris_ema_advance" in comment and "WITHOUT moving it" in comment          # (the sentence before it is still there)


def test_argument_checks_without_a_gpu(lib):
    """every check returns before anything is launched: the pointers below are never dereferenced"""
    tab, grp, step, lrs, out = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    good = [tab, 4, grp, step, lrs, 5, 2, out]

    def bad(i, v):
        a = list(good)
        a[i] = v
        return tuple(a)
    for args, msg in ((bad(0, None), b"null"), (bad(2, None), b"null"), (bad(3, None), b"null"), (bad(4, None), b"null"),
                      (bad(1, 0), b"n_desc must be >= 1"), (bad(1, -7), b"n_desc must be >= 1"),
                      (bad(5, 0), b"n_rows must be >= 1"), (bad(5, -1), b"n_rows must be >= 1"),
                      (bad(6, 0), b"n_groups must lie in [1, 255]"), (bad(6, -2), b"n_groups must lie in [1, 255]"),
                      (bad(6, 256), b"n_groups must lie in [1, 255]")):
        assert lib.cris_adam_schedule_lrs(*args, None) != 0, args
        err = lib.cris_last_error()
        assert NAME.encode() in err and msg in err, (args, err)


# ---- cris.pytorch_amd.lr against torch's schedulers ------------------------------------------------------------------------
def f32(rows):
    return np.asarray(rows, dtype=np.float64).astype(np.float32)


def stepped(make, n=N, base=BASE):
    """float32-rounded get_last_lr() before each of n `optimizer.step(); scheduler.step()` on a two-group SGD on the CPU"""
    import torch
    opt = torch.optim.SGD([{"params": [torch.zeros(1, requires_grad=True)], "lr": x} for x in base], lr=base[0])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sched = make(opt)
        rows = []
        for _ in range(n):
            rows.append(list(sched.get_last_lr()))
            opt.step()
            sched.step()
    return f32(rows)


def same_bits(a, b):
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    assert np.array_equal(a.view(np.int32), b.view(np.int32)), (a, b)


def test_reference_epochs_is_epoch_group_lrs_row_by_row():
    from cris.pytorch_amd.trainer import epoch_group_lrs
    base_lr, multi, ms, gamma = 1e-4, 0.1, (2, 3), 0.1
    t = lr.reference_epochs(base_lr, multi, ms, gamma, steps_per_epoch=3, epochs=5)
    assert t.shape == (15, 2) and t.dtype == np.float32
    for i in range(15):
        same_bits(t[i], f32(epoch_group_lrs(i // 3, base_lr, multi, ms, gamma)))
    same_bits(t[:3], f32([[base_lr, base_lr]] * 3))                          # epoch 0: both groups at base_lr
    same_bits(t[3], f32([multi * base_lr, base_lr]))                        # epoch 1: the backbone multiplier, no milestone yet
    same_bits(t[6], f32([multi * base_lr * gamma, base_lr * gamma]))        # epoch 2: first milestone
    same_bits(t[9], f32([multi * base_lr * gamma ** 2, base_lr * gamma ** 2]))
    same_bits(t[12], t[9])
    assert len({t[i].tobytes() for i in range(15)}) == 4


def test_closed_forms_equal_the_torch_schedulers():
    from torch.optim import lr_scheduler as S
    same_bits(lr.constant(BASE, N), f32([BASE] * N))
    assert lr.constant(BASE).shape == (1, 2)
    same_bits(lr.multistep(BASE, (3, 7), 0.1, N), stepped(lambda o: S.MultiStepLR(o, [3, 7], 0.1)))
    same_bits(lr.cosine(BASE, N), stepped(lambda o: S.CosineAnnealingLR(o, T_max=N)))
    same_bits(lr.cosine(BASE, N, eta_min=1e-6), stepped(lambda o: S.CosineAnnealingLR(o, T_max=N, eta_min=1e-6)))
    same_bits(lr.poly(BASE, N, 2.0), stepped(lambda o: S.PolynomialLR(o, total_iters=N, power=2.0)))
    same_bits(lr.poly(BASE, N, 0.9), stepped(lambda o: S.PolynomialLR(o, total_iters=N, power=0.9)))
    # the schedules move, and end where they should
    c = lr.cosine(BASE, N)
    assert np.all(np.diff(c, axis=0) < 0) and np.array_equal(c[0], f32(BASE))


def test_warmup_equals_linearlr():
    from torch.optim import lr_scheduler as S
    # on a constant schedule the closed form is LinearLR's own sequence, exactly
    w = lr.with_warmup(lr.constant(BASE, N), 4, 0.1)
    same_bits(w, stepped(lambda o: S.LinearLR(o, start_factor=0.1, end_factor=1.0, total_iters=4)))
    same_bits(w, lr.from_torch(lambda o: S.ChainedScheduler([S.LinearLR(o, 0.1, 1.0, 4)]), BASE, N))
    same_bits(w[4:], f32([BASE] * (N - 4)))
    same_bits(w[0], f32(np.asarray(BASE) * 0.1))
    # chained onto a moving schedule, torch's ChainedScheduler multiplies each scheduler's RECURSIVE factor into the running
    # value (lr *= f_t / f_{t-1}, in float64), which differs from the product of the two closed forms in the last bits of the
    # float64 and so, now and then, in the last bit of the float32: compared against from_torch with 1 ulp of float32 allowed
    got = lr.with_warmup(lr.cosine(BASE, N), 4, 0.1)
    want = lr.from_torch(lambda o: S.ChainedScheduler([S.LinearLR(o, 0.1, 1.0, 4), S.CosineAnnealingLR(o, T_max=N)]), BASE, N)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape == (N, 2)
    ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    print("with_warmup(cosine) against ChainedScheduler: max %d ulp" % ulps.max())
    assert ulps.max() <= 1
    same_bits(got[4:], lr.cosine(BASE, N)[4:])                               # rows past the warm-up are untouched
    same_bits(lr.with_warmup(lr.cosine(BASE, N), 0, 0.5), lr.cosine(BASE, N))
    for kw in (dict(warmup_steps=-1, start_factor=0.5), dict(warmup_steps=2, start_factor=0.0), dict(warmup_steps=2, start_factor=1.5),
               dict(warmup_steps=1.5, start_factor=0.5)):
        with pytest.raises(ValueError):
            lr.with_warmup(lr.constant(BASE, N), **kw)


def test_from_torch_reproduces_onecycle():
    from torch.optim import lr_scheduler as S

    def make(o):
        return S.OneCycleLR(o, max_lr=[1e-4, 1e-3], total_steps=N)
    t = lr.from_torch(make, BASE, N)
    same_bits(t, stepped(make))
    assert t.shape == (N, 2) and t[:, 1].argmax() not in (0, N - 1)          # up, then down


def test_tables_are_validated_without_a_gpu():
    from cris.pytorch_amd import ops
    from cris.pytorch_amd.trainer import NativeTrainer
    ok = lr.cosine(BASE, N)
    checked = ops.LrSchedule.checked_table(ok.astype(np.float64).tolist())
    same_bits(checked, ok)
    assert checked.flags["C_CONTIGUOUS"]
    assert ops.LrSchedule.checked_table(np.zeros((1, 3))).shape == (1, 3)    # zero is a rate; any number of groups up to 255
    for bad in ([1e-4, 1e-5],                                                # 1-d
                np.zeros((2, 2, 2)),
                np.zeros((0, 2)),                                            # no row
                np.zeros((3, 0)), np.zeros((1, 256)),
                [[1e-4, -1e-5]],                                             # negative
                [[1e-4, float("nan")]], [[float("inf"), 1e-4]],
                "abc"):
        with pytest.raises(ValueError):
            ops.LrSchedule.checked_table(bad)
        with pytest.raises(ValueError):
            ops.LrSchedule(None, [0, 1], bad)                                # refused before the Adam table is looked at
        with pytest.raises(ValueError, match="lr_schedule"):
            NativeTrainer(None, None, None, "cpu", lr_schedule=bad)          # before the state dict or the device is looked at
    with pytest.raises(ValueError, match="lr_schedule"):
        NativeTrainer(None, None, None, "cpu", lr_schedule=np.full((4, 3), 1e-4))        # three columns: the trainer has two groups
    with pytest.raises(ValueError, match="lr_schedule"):
        NativeTrainer(None, None, None, "cpu", lr_schedule=np.full((4, 1), 1e-4))
    with pytest.raises(ValueError):
        ops.LrSchedule(None, [0, 2], ok)                                     # a group index outside the table's columns
    with pytest.raises(ValueError):
        ops.LrSchedule(None, [0, -1], ok)
    assert NativeTrainer._checked_schedule(None) is None
    same_bits(NativeTrainer._checked_schedule(ok.tolist()), ok)
