"""The per-step learning-rate schedule of the native trainer (csrc/lr.hip, ops.LrSchedule, NativeTrainer(lr_schedule=...)).  The
kernel copies floats, so every comparison is bit for bit: the kernel on tables of fake descriptors against the table entry it must
have copied (and against the uploaded bytes everywhere else), the trainer against the host path that existed before - a second
trainer without a schedule that calls set_group_lrs before every step.  Tiny spec, 64 x 64, batch 2."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)

pytestmark = pytest.mark.gpu

from cris.pytorch_amd import hip, lr  # noqa: E402
from trainer_cases import MICRO, batch, make_trainer, recorded  # noqa: E402

DEV = "cuda"
BASE = 1e-4
# six distinct rows (backbone, rest), none of them the constructor's (BASE, BASE)
T6 = np.array([[2e-5, 3e-4], [5e-5, 2.5e-4], [8e-5, 2e-4], [6e-5, 1.5e-4], [4e-5, 5e-5], [1e-5, 2e-5]], dtype=np.float32)
T3 = T6[:3].copy()


# ---- the kernel -------------------------------------------------------------------------------------------------------------
LR_OFF, DESC = hip.AdamDesc.lr.offset, C.sizeof(hip.AdamDesc)


def fake_table(n):
    """n descriptors with fake (never dereferenced) pointers and a different recognisable value in every field"""
    arr = (hip.AdamDesc * n)()
    for i in range(n):
        for k, (name, ct) in enumerate(hip.AdamDesc._fields_):
            if ct is C.c_float:
                v = 1000.0 * (k + 1) + i + 0.25
            elif ct is C.c_void_p:
                v = 0x7F0000000000 + (k << 32) + 16 * i
            else:
                v = 0x01010000 * (k + 1) + i
            setattr(arr[i], name, v)
    return arr


@pytest.mark.parametrize("n_groups", [1, 2, 3])
@pytest.mark.parametrize("n_desc", [1, 255, 256, 257, 449])
def test_kernel_copies_the_row_and_nothing_else(n_desc, n_groups):
    assert (LR_OFF, DESC) == (40, 112)
    n_rows = 5
    rng = np.random.default_rng(100 * n_desc + n_groups)
    # distinct values, 0.0 and a float32 subnormal among them
    table = (np.arange(1, n_rows * n_groups + 1, dtype=np.float32) * np.float32(1.0009765625e-5)).reshape(n_rows, n_groups)
    table[2, 0] = 0.0                                                                  # (rows 0, 2 and 4 are the ones selected below)
    table[4, n_groups - 1] = np.float32(1e-41)
    assert 0 < table[4, n_groups - 1] < np.finfo(np.float32).tiny and len(set(table.ravel().tolist())) == table.size
    group_of = rng.permutation(np.arange(n_desc) % n_groups).astype(np.uint8)          # shuffled, every group used when it can be
    upload = np.frombuffer(bytes(fake_table(n_desc)), dtype=np.uint8).reshape(n_desc, DESC).copy()
    tab = torch.from_numpy(upload.copy()).to(DEV)
    grp, tbl = torch.from_numpy(group_of).to(DEV), torch.from_numpy(table).to(DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = torch.full((n_groups + 2,), -1.0, device=DEV)                                # two floats behind lr_out stay as they are
    for s, row in ((0, 0), (1, 0), (3, 2), (5, 4), (9, 4)):          # clamped below, first, interior, last, clamped past the end
        step.fill_(s)
        for lr_out in (out, None):
            tab.copy_(torch.from_numpy(upload))
            out.fill_(-1.0)
            hip.call("cris_adam_schedule_lrs", tab.data_ptr(), n_desc, grp.data_ptr(), step.data_ptr(), tbl.data_ptr(), n_rows, n_groups,
                     hip.ptr(lr_out), None)
            got = tab.cpu().numpy()
            got_lr = got[:, LR_OFF:LR_OFF + 4].copy().view(np.uint32).ravel()
            want_lr = table[row][group_of].view(np.uint32)
            assert np.array_equal(got_lr, want_lr), (s, np.flatnonzero(got_lr != want_lr)[:5])
            got[:, LR_OFF:LR_OFF + 4] = upload[:, LR_OFF:LR_OFF + 4]
            assert np.array_equal(got, upload), s                                      # every other byte of the table
            o = out.cpu().numpy()
            if lr_out is None:
                assert np.all(o == -1.0)
            else:
                assert np.array_equal(o[:n_groups].view(np.uint32), table[row].view(np.uint32)) and np.all(o[n_groups:] == -1.0), (s, o)
        assert int(step) == s
    assert np.array_equal(grp.cpu().numpy(), group_of) and np.array_equal(tbl.cpu().numpy().view(np.uint32), table.view(np.uint32))


# ---- the trainer ------------------------------------------------------------------------------------------------------------
def rates(table, t):
    return tuple(float(x) for x in table[min(t, len(table) - 1)])


def train(tr, head, first, steps, out=None, host_table=None):
    """`steps` optimizer steps on batches first, first + 1, ...; host_table: the path that existed before the schedule -
    set_group_lrs with the step's row (the last one past the end) in front of every step"""
    out = out if out is not None else dict(losses=[], metrics=[], lrs=[], handles=[])
    for t in range(first, first + steps):
        if host_table is not None:
            tr.set_group_lrs(*rates(host_table, t))
        loss, metric = tr.train_step(*batch(tr.accum_steps * MICRO, head, t))
        out["losses"].append(float(loss))
        out["metrics"].append(metric.cpu().tolist())
        if tr._lr is not None:
            out["lrs"].append(tr.current_lrs.cpu().numpy().copy())
        out["handles"].append(tr._graph if tr._graph is not None else tr._cmds)
    return out


def finish(tr, out):
    torch.cuda.synchronize()
    out["final"] = tr.model_state_dict()
    out["m"] = [t.detach().cpu().clone() for t in tr.adam.m]
    out["v"] = [t.detach().cpu().clone() for t in tr.adam.v]
    return out


_RUNS = {}


def run(steps, launch="eager", table=None, host_table=None, **kw):
    """computed once per configuration, read-only afterwards.  table: the trainer follows it on the device (lr_schedule);
    host_table: the oracle, a trainer without a schedule driven by set_group_lrs"""
    key = (steps, launch, None if table is None else table.tobytes(), None if host_table is None else host_table.tobytes(),
           tuple(sorted(kw.items())))
    if key not in _RUNS:
        sched = {} if table is None else {"lr_schedule": table}
        tr, head = make_trainer(launch=launch, **sched, **kw)
        out = train(tr, head, 0, steps, host_table=host_table)
        out.update(tr=tr, head=head)
        _RUNS[key] = finish(tr, out)
    return _RUNS[key]


def same_run(a, b):
    assert a["losses"] == b["losses"] and a["metrics"] == b["metrics"], (a["losses"], b["losses"])
    same_state(a, b)


def same_state(a, b):
    """final parameters, BatchNorm statistics and Adam moments"""
    keys = [k for k, v in a["final"].items() if v.is_floating_point()]
    assert keys and list(a["final"].keys()) == list(b["final"].keys())
    bad = [k for k in keys if not torch.equal(a["final"][k], b["final"][k])]
    assert not bad, (len(bad), bad[:5])
    assert all(torch.equal(x, y) for x, y in zip(a["m"], b["m"])) and all(torch.equal(x, y) for x, y in zip(a["v"], b["v"]))


def differs(a, b):
    return any(not torch.equal(a["final"][k], b["final"][k]) for k in a["final"])


def same_rows(lrs, table, first=0):
    assert len(lrs) > 0
    for i, got in enumerate(lrs):
        want = table[min(first + i, len(table) - 1)]
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (first + i, got, want)


def test_trainer_equals_the_host_path():
    dev, host, const = run(6, table=T6), run(6, host_table=T6), run(6)
    assert dev["tr"]._lr is not None and host["tr"]._lr is None and const["tr"]._lr is None
    same_run(dev, host)
    same_rows(dev["lrs"], T6)
    assert differs(dev, const) and dev["losses"] != const["losses"]          # the schedule did something
    assert dev["losses"][0] == const["losses"][0]                            # (the first loss is taken before the first update)
    with pytest.raises(RuntimeError):
        const["tr"].current_lrs


def test_reference_recipe_equals_set_epoch_at_the_boundaries():
    milestones, gamma, multi = (2,), 0.1, 0.1
    table = lr.reference_epochs(BASE, multi, milestones, gamma, steps_per_epoch=2, epochs=3)
    assert table.shape == (6, 2) and len({r.tobytes() for r in table}) == 3
    dev = run(6, table=table, lr_multi=multi)
    tr, head = make_trainer(launch="eager", lr_multi=multi)
    out = None
    for epoch in range(3):
        tr.set_epoch(epoch, milestones=milestones, gamma=gamma)
        out = train(tr, head, 2 * epoch, 2, out)
    same_run(dev, finish(tr, out))
    same_rows(dev["lrs"], table)


@pytest.mark.parametrize("launch", ["graph", "cmdlist"])
def test_replay_follows_the_table_from_device_state(launch):
    e, r = run(5, table=T6), run(5, launch=launch, table=T6)
    tr = r["tr"]
    assert tr.launch == launch, tr.graph_error
    same_run(r, e)
    same_rows(r["lrs"], T6)
    # one capture / recording: step 0 ran eagerly, step 1 built it, and it is the same object ever after
    h = r["handles"]
    assert h[0] is None and h[1] is not None and all(x is h[1] for x in h[2:])
    assert (tr._graph if launch == "graph" else tr._cmds) is h[1]


def test_switched_off_it_issues_the_launches_of_a_trainer_without_the_argument():
    a, cmds_a = recorded(lr_schedule=None)
    b, cmds_b = recorded()
    assert a._lr is None and b._lr is None
    assert cmds_a == cmds_b and len(cmds_a) > 100
    assert not any(name == "cris_adam_schedule_lrs" for name, _ in cmds_a)
    c, cmds_c = recorded(lr_schedule=T6)
    names = [name for name, _ in cmds_c]
    tables = sum(1 for t in c.adam.tables.values() if t.n)
    assert tables >= 1 and names.count("cris_adam_schedule_lrs") == tables
    first = names.index("cris_adam_step_amp")
    assert names[first - tables:first] == ["cris_adam_schedule_lrs"] * tables          # directly in front of the update
    assert [x for x in cmds_c if x[0] != "cris_adam_schedule_lrs"] == cmds_a


def table_lrs(tr):
    """the `lr` fields of the trainer's device tables, in AdamTable order -> {group: set of values}"""
    seen = {0: set(), 1: set()}
    for taps, idx in tr.adam.index.items():
        t = tr.adam.tables[taps]
        if t.n:
            raw = t.dev.cpu().numpy().reshape(t.n, DESC)[:, LR_OFF:LR_OFF + 4].copy().view(np.float32).ravel()
            for j, i in enumerate(idx):
                seen[tr.group[tr.names[i]]].add(float(raw[j]))
    return seen


def test_switching_off_restores_the_host_rates():
    tr, head = make_trainer(launch="graph", lr_schedule=T3)
    out = train(tr, head, 0, 3)
    assert tr._graph is not None and table_lrs(tr) == {0: {float(T3[2, 0])}, 1: {float(T3[2, 1])}}
    tr.set_lr_schedule(None)
    assert tr._lr is None and tr._graph is None
    assert table_lrs(tr) == {0: {float(np.float32(BASE))}, 1: {float(np.float32(BASE))}}                          # what the constructor set, not the last row
    with pytest.raises(RuntimeError):
        tr.current_lrs
    train(tr, head, 3, 1, out)
    # the plain trainer: the same three rows through set_group_lrs, then the constructor's rates
    plain, _ = make_trainer(launch="eager")
    want = train(plain, head, 0, 3, host_table=T3)
    plain.set_group_lrs(BASE, BASE)
    train(plain, head, 3, 1, want)
    same_run(finish(tr, out), finish(plain, want))
    # set_group_lrs under a schedule lasts until the next step overwrites it
    tr.set_lr_schedule(T3)
    tr.set_group_lrs(7e-3, 7e-3)
    assert table_lrs(tr) == {0: {float(np.float32(7e-3))}, 1: {float(np.float32(7e-3))}}
    tr.train_step(*batch(MICRO, head, 4))
    torch.cuda.synchronize()
    assert table_lrs(tr) == {0: {float(T3[2, 0])}, 1: {float(T3[2, 1])}}
    with pytest.raises(ValueError, match="lr_schedule"):
        tr.set_lr_schedule(np.zeros((3, 3), dtype=np.float32))


def test_one_row_per_optimizer_step_under_accumulation():
    dev, host = run(3, table=T6, accum_steps=2), run(3, host_table=T6, accum_steps=2)
    assert dev["tr"].step_idx == 3
    same_run(dev, host)
    same_rows(dev["lrs"], T6)                                               # row t at optimizer step t, not at micro-batch t
    assert differs(dev, run(3, accum_steps=2))


def test_with_clipping():
    dev, host = run(3, table=T6, max_norm=1e-3), run(3, host_table=T6, max_norm=1e-3)
    assert float(dev["tr"].grad_norm) > 1e-3                               # (it does clip)
    same_run(dev, host)
    same_rows(dev["lrs"], T6)


def test_past_the_end_and_resume():
    whole = run(5, table=T3)
    same_run(whole, run(5, host_table=T3))                                  # (the oracle repeats the last row)
    same_rows(whole["lrs"], T3)
    assert all(np.array_equal(x, T3[2]) for x in whole["lrs"][2:])
    assert differs(whole, run(5, host_table=T6[:5].copy()))                 # staying on row 2 is not going on to rows 3 and 4
    a, head = make_trainer(launch="eager", lr_schedule=T3)
    groups = a.optimizer_state_dict()["param_groups"]
    assert [g["lr"] for g in groups] == [float(T3[0, 0]), float(T3[0, 1])]  # before the first step: row 0 comes next
    train(a, head, 0, 2)
    saved = dict(model=a.model_state_dict(), opt=a.optimizer_state_dict())
    assert [g["lr"] for g in saved["opt"]["param_groups"]] == [float(T3[2, 0]), float(T3[2, 1])]          # the NEXT step's row
    assert "lr_schedule" not in saved["opt"] and set(saved["opt"]) == {"state", "param_groups"}           # configuration, not state
    b, _ = make_trainer(launch="eager")
    b.load_model_state_dict(saved["model"])
    b.load_optimizer_state_dict(saved["opt"])
    b.set_lr_schedule(T3)
    assert b.step_idx == 2
    out = train(b, head, 2, 3)
    assert out["losses"] == whole["losses"][2:]
    same_rows(out["lrs"], T3, first=2)
    assert out["metrics"] == whole["metrics"][2:]
    same_state(finish(b, out), whole)
    assert [g["lr"] for g in b.optimizer_state_dict()["param_groups"]] == [float(T3[2, 0]), float(T3[2, 1])]
