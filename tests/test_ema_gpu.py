"""The weight average of the native trainer (csrc/ema.hip, ops.EmaTable, NativeTrainer(ema_decay=...)) against its definition in
torch fp32 on the host: ema.add_((p - ema) * w), three roundings, bit for bit - the kernels on a table of awkward sizes, the
trainer against the recurrence replayed from per-step parameter snapshots.  Tiny spec, 64 x 64, batch 2."""
import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)

pytestmark = pytest.mark.gpu

from cris.pytorch_amd import arch, hip, ops  # noqa: E402
from cris.pytorch_amd.infer import InferenceRunner  # noqa: E402
from trainer_cases import MICRO, batch, make_trainer, recorded, same_floats  # noqa: E402

DEV = "cuda"
EMBED = "backbone.token_embedding.weight"
SENTINEL = 12345.0


# ---- the kernels ----------------------------------------------------------------------------------------------------
def state_of(st):
    """(updates, weight, active) of a 16-byte state record"""
    h = st.cpu()
    return int(h[0]), h[1:2].view(torch.float32)[0].numpy().copy()[()], int(h[2])


@pytest.mark.parametrize("warmup", [False, True])
@pytest.mark.parametrize("every", [1, 2, 3])
def test_advance(every, warmup):
    for decay in (0.9, 0.9999):
        step = torch.zeros(1, dtype=torch.int32, device=DEV)
        st = torch.zeros(4, dtype=torch.int32, device=DEV)
        updates, weight = 0, np.float32(0.0)
        for s in range(1, 13):
            step.fill_(s)
            hip.call("cris_ema_advance", step.data_ptr(), every, decay, int(warmup), st.data_ptr(), None)
            active = int(s % every == 0)
            if active:
                weight = ops.ema_weight(updates, decay, warmup)
                updates += 1
            got = state_of(st)
            assert got[0] == updates and got[2] == active, (s, got)
            assert got[1].dtype == np.float32 and got[1] == weight, (s, got, weight)          # exactly
            assert int(st[3]) == 0 and int(step) == s
        assert updates == 12 // every


def kernel_case():
    """the table of the issue: (name, parameter tensor, row_live or None); parameters are views into larger buffers so that
    some start 4 and 8 bytes off a 16-byte boundary"""
    B = hip.load().cris_adam_block_elems()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    big = (8 * cus + 3) * B + 5                      # more block trips than the grid has blocks: a second grid-stride trip
    g = torch.Generator(device="cpu").manual_seed(7)
    named, live = [], {}
    for i, n in enumerate([1, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, B - 1, B, B + 1, 2 * B + 3, big]):
        named.append(("t%d_%d" % (i, n), torch.randn(n, generator=g)))
    for off, n in ((1, 1025), (2, 2 * B + 3), (1, 6), (2, 4), (3, B + 2)):
        named.append(("off%d_%d" % (off, n), (off, torch.randn(n + off, generator=g))))
    named.append(("rows5x7", torch.randn(5, 7, generator=g)))
    live["rows5x7"] = torch.tensor([1, 0, 1, 0, 0], dtype=torch.uint8)
    named.append(("rows6x512", torch.randn(6, 512, generator=g)))
    live["rows6x512"] = torch.tensor([0, 1, 1, 0, 1, 0], dtype=torch.uint8)
    return named, live


def test_kernel_equals_the_torch_formula_bit_for_bit():
    named, live_h = kernel_case()
    gen = torch.Generator(device="cpu").manual_seed(11)
    for scale in (1.0, 1e6):                                               # second run: operands six orders of magnitude apart
        bufs, params, host_p = [], [], {}
        for name, t in named:
            off = 0
            if isinstance(t, tuple):
                off, t = t
            d = (t * scale).to(DEV)
            bufs.append((d, d.clone()))
            params.append((name, d[off:] if off else d))
            host_p[name] = (t * scale)[off:]
            assert params[-1][1].data_ptr() % 16 == 4 * off
        live = {k: v.to(DEV) for k, v in live_h.items()}
        tab = ops.EmaTable(params, row_live=live, guard=4)
        tab.flat.fill_(SENTINEL)
        host_e = {}
        for name, p in params:
            e = torch.randn(p.shape, generator=gen)
            if name in live_h:
                e[live_h[name] == 0] = SENTINEL                                # skipped rows: must stay untouched
            host_e[name] = e
            tab.views[name].copy_(e)
        assert all(v.data_ptr() % 16 == 0 for v in tab.views.values())
        flat0 = tab.flat.clone()
        step = torch.tensor([1], dtype=torch.int32, device=DEV)
        # not an EMA step (1 % 2 != 0): nothing moves, the count and the weight included
        tab.state.copy_(torch.tensor([5, 0, 0, 0], dtype=torch.int32))
        tab.state[1:2].view(torch.float32).fill_(0.25)
        tab.update(step, every=2, decay=0.9)
        assert torch.equal(tab.flat, flat0)
        assert state_of(tab.state) == (5, np.float32(0.25), 0)
        # an EMA step
        tab.update(step, every=1, decay=0.9, warmup=True)
        upd, w, active = state_of(tab.state)
        assert (upd, active) == (6, 1) and w == ops.ema_weight(5, 0.9, True)
        got = tab.flat.cpu()
        covered = torch.zeros(got.numel(), dtype=torch.bool)
        for name, p in params:
            want = host_e[name].clone()
            want.add_((host_p[name] - want) * float(w))
            if name in live_h:
                dead = live_h[name] == 0
                want[dead] = SENTINEL
                assert bool((want[~dead] != SENTINEL).all())
            o, n = tab.offsets[name], p.numel()
            assert torch.equal(got[o:o + n].view(p.shape), want), (name, scale)
            assert not torch.equal(want, host_e[name])                     # (it did move)
            assert bool((got[o - 4:o] == SENTINEL).all()) and bool((got[o + n:o + n + 4] == SENTINEL).all()), name      # guards
            covered[o:o + n] = True
        assert bool((got[~covered] == SENTINEL).all())                      # every float outside the slices
        assert all(torch.equal(d, d0) for d, d0 in bufs)                    # p unchanged
        del tab, bufs, params
    lib = hip.load()
    assert lib.cris_ema_update(None, 1, 1, None, None) != 0 and b"cris_ema_update" in lib.cris_last_error()


# ---- the trainer ------------------------------------------------------------------------------------------------------
def train(tr, head, first, steps, out=None):
    out = out if out is not None else dict(losses=[], metrics=[], snaps=[])
    for t in range(first, first + steps):
        loss, metric = tr.train_step(*batch(tr.accum_steps * MICRO, head, t))
        out["losses"].append(float(loss))
        out["metrics"].append(metric.cpu().tolist())
        out["snaps"].append(tr.model_state_dict())
    return out


_RUNS = {}


def run(steps, launch="eager", **kw):
    """computed once per configuration, read-only afterwards: `steps` optimizer steps; the model snapshot before the first and
    after every step, losses, metrics, Adam moments, and (with ema_decay) the averaged state dict and its update count"""
    key = (steps, launch, tuple(sorted(kw.items())))
    if key in _RUNS:
        return _RUNS[key]
    tr, head = make_trainer(launch=launch, **kw)
    out = dict(tr=tr, head=head, losses=[], metrics=[], snaps=[tr.model_state_dict()])
    train(tr, head, 0, steps, out)
    torch.cuda.synchronize()
    out["m"] = [t.detach().cpu().clone() for t in tr.adam.m]
    out["v"] = [t.detach().cpu().clone() for t in tr.adam.v]
    if tr.ema_decay is not None:
        out["ema"], out["updates"] = tr.ema_state_dict(), tr.ema_num_updates
    _RUNS[key] = out
    return out


def host_ema(snaps, decay, every=1, warmup=False, start=None, updates=0, first_step=1):
    """the recurrence on the CPU, from the snapshot before the first step and the one after every optimizer step"""
    e = {k: v.clone() for k, v in (start if start is not None else snaps[0]).items() if v.is_floating_point()}
    for i, sd in enumerate(snaps[1:]):
        if (first_step + i) % every:
            continue
        w = float(ops.ema_weight(updates, decay, warmup))
        for k in e:
            e[k].add_((sd[k] - e[k]) * w)
        updates += 1
    return e, updates


def test_trainer_equals_the_host_recurrence():
    r = run(5, ema_decay=0.9)
    tr = r["tr"]
    want, updates = host_ema(r["snaps"], 0.9)
    assert r["updates"] == updates == 5
    same_floats(r["ema"], want)
    live = tr.model_state_dict()
    assert list(r["ema"].keys()) == list(live.keys())
    assert [k for k in live if k.startswith("module.")] == [] and all(k.startswith("module.") for k in tr.ema_state_dict(ddp_prefix=True))
    tracked = [k for k in live if k.endswith("num_batches_tracked")]
    assert tracked and all(int(r["ema"][k]) == int(live[k]) == 5 for k in tracked)
    stats = [k for k in live if k.endswith(("running_mean", "running_var"))]
    assert stats and "backbone.logit_scale" in want
    moved = [k for k in want if not torch.equal(want[k], live[k])]
    assert len(moved) > len(want) // 2 and any(k in moved for k in stats)          # the average is not the last iterate
    assert tr._ema.num_elements == sum(v.numel() for v in want.values())           # one more fp32 copy, nothing else


def test_the_average_only_reads_the_model():
    on, off = run(4, ema_decay=0.9), run(4)
    assert off["tr"]._ema is None and off["tr"].ema_decay is None
    assert on["losses"] == off["losses"] and on["metrics"] == off["metrics"]
    same_floats(on["snaps"][-1], off["snaps"][-1])
    assert all(torch.equal(a, b) for a, b in zip(on["m"], off["m"])) and all(torch.equal(a, b) for a, b in zip(on["v"], off["v"]))


def test_switched_off_it_issues_the_launches_of_a_trainer_without_the_argument():
    a, cmds_a = recorded(ema_decay=None)
    b, cmds_b = recorded()
    assert a._ema is None and b._ema is None
    assert cmds_a == cmds_b and len(cmds_a) > 100
    assert not any(name.startswith("cris_ema") for name, _ in cmds_a)
    c, cmds_c = recorded(ema_decay=0.9)
    assert [name for name, _ in cmds_c if name.startswith("cris_ema")] == ["cris_ema_advance", "cris_ema_update"]
    assert [x for x in cmds_c if not x[0].startswith("cris_ema")] == cmds_a and cmds_c[-1][0] == "cris_ema_update"
    assert all(torch.equal(a.engine.P[k], c.engine.P[k]) for k in a.engine.P)


@pytest.mark.parametrize("launch", ["graph", "cmdlist"])
def test_replay_gates_and_warms_up_from_device_state(launch):
    kw = dict(ema_decay=0.9, ema_every=2, ema_warmup=True)
    e, r = run(5, **kw), run(5, launch=launch, **kw)
    tr = r["tr"]
    assert tr.launch == launch and (tr._graph is not None or tr._cmds is not None), tr.graph_error
    assert e["losses"] == r["losses"]
    same_floats(r["snaps"][-1], e["snaps"][-1])
    assert r["updates"] == e["updates"] == 2                               # steps 2 and 4
    same_floats(r["ema"], e["ema"])
    want, _ = host_ema(e["snaps"], 0.9, every=2, warmup=True)
    same_floats(e["ema"], want)
    plain, _ = host_ema(e["snaps"], 0.9, every=2, warmup=False)
    assert any(not torch.equal(plain[k], want[k]) for k in want)           # (warm-up does change the weights used)


def test_one_update_per_optimizer_step_under_accumulation():
    r = run(3, accum_steps=2, ema_decay=0.9, ema_warmup=True)
    want, updates = host_ema(r["snaps"], 0.9, warmup=True)
    assert r["updates"] == updates == 3 and r["tr"].step_idx == 3
    same_floats(r["ema"], want)


def test_with_clipping():
    r = run(3, ema_decay=0.9, max_norm=1e-3)
    assert float(r["tr"].grad_norm) > 1e-3                                 # (it does clip)
    want, _ = host_ema(r["snaps"], 0.9)
    same_floats(r["ema"], want)


def test_skipping_untouched_embedding_rows_changes_no_bit(monkeypatch):
    skip = run(5, ema_decay=0.9)
    live = skip["tr"].engine.embed_live
    assert live is not None and skip["tr"]._ema.row_live[EMBED] is live
    assert 0 < int(live.sum()) < live.numel()                              # rows that never had a gradient exist, and live ones
    monkeypatch.setenv("CRIS_ADAM_ROW_SKIP", "0")
    dense = run(5, ema_decay=0.9, base_lr=1e-4)                            # (another cache key: built under the variable)
    assert dense["tr"].engine.embed_live is None and dense["tr"]._ema.row_live == {}
    same_floats(dense["ema"], skip["ema"])
    same_floats(dense["snaps"][-1], skip["snaps"][-1])


def test_resume():
    kw = dict(ema_decay=0.9, ema_every=2, ema_warmup=True)
    whole = run(5, **kw)
    a, head = make_trainer(launch="eager", **kw)
    train(a, head, 0, 3)
    saved = dict(model=a.model_state_dict(ddp_prefix=True), opt=a.optimizer_state_dict(), ema=a.ema_state_dict(ddp_prefix=True),
                 n=a.ema_num_updates)
    assert saved["n"] == 1
    b, _ = make_trainer(launch="eager", **kw)
    b.load_model_state_dict(saved["model"])
    # loading the model alone restarts the average from the loaded weights
    assert b.ema_num_updates == 0
    same_floats(b.ema_state_dict(), a.model_state_dict())
    b.load_optimizer_state_dict(saved["opt"])
    b.load_ema_state_dict(saved["ema"], saved["n"])
    assert b.ema_num_updates == 1 and b.step_idx == 3
    assert EMBED in b._ema.row_live                                        # untouched rows agree with the parameters: still skipped
    out = train(b, head, 3, 2)
    assert out["losses"] == whole["losses"][3:]
    same_floats(b.model_state_dict(), whole["snaps"][-1])
    assert b.ema_num_updates == whole["updates"] == 2
    same_floats(b.ema_state_dict(), whole["ema"])
    with pytest.raises(ValueError):
        b.load_ema_state_dict(saved["ema"], -1)
    with pytest.raises(KeyError):
        b.load_ema_state_dict({k: v for k, v in saved["ema"].items() if not k.endswith("running_var")}, 1)


def test_a_foreign_average_switches_the_row_skip_off():
    """an average that differs from the parameters in a never-live embedding row must move towards them: the dense update"""
    tr, head = make_trainer(launch="eager", ema_decay=0.9)
    train(tr, head, 0, 1)
    dead = int((tr.engine.embed_live == 0).nonzero()[0])
    sd = tr.ema_state_dict()
    sd[EMBED][dead] += 1.0
    tr.load_ema_state_dict(sd, 1)
    assert tr._ema.row_live == {} and tr.ema_num_updates == 1
    before = tr.ema_state_dict()
    train(tr, head, 1, 1)
    p = tr.model_state_dict()
    want = {k: v.clone() for k, v in before.items() if v.is_floating_point()}
    for k in want:
        want[k].add_((p[k] - want[k]) * float(ops.ema_weight(1, 0.9)))
    got = tr.ema_state_dict()
    same_floats(got, want)
    assert not torch.equal(got[EMBED][dead], before[EMBED][dead])


def test_inference_runs_on_the_average_and_switching_off_frees_it():
    r = run(5, ema_decay=0.9)
    clip, head = arch.specs_by_name("tiny")
    host, _ = host_ema(r["snaps"], 0.9)
    assembled = dict(r["snaps"][-1])                                        # num_batches_tracked of the live model
    assembled.update(host)
    img, word, _ = batch(MICRO, head, 99)
    runner = InferenceRunner(clip, head, arch.synthetic_state_dict(clip, head, 0), torch.device("cuda:0"), use_graph=False)
    runner.load_state_dict(r["tr"].ema_state_dict())
    got = runner(img, word).clone()
    want = InferenceRunner(clip, head, assembled, torch.device("cuda:0"), use_graph=False)(img, word).clone()
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    runner.load_state_dict(r["snaps"][-1])
    assert not torch.equal(runner(img, word), got)                         # the last iterate answers differently
    # switching off: a trainer of its own (the cached ones stay as they are)
    tr, head = make_trainer(launch="graph", ema_decay=0.9, ema_every=3)
    for t in range(3):
        tr.train_step(*batch(MICRO, head, t))
    assert tr._graph is not None and tr.ema_num_updates == 1
    tr.set_ema(None)
    assert tr._ema is None and tr._graph is None and tr.ema_decay is None
    with pytest.raises(RuntimeError):
        tr.ema_state_dict()
    with pytest.raises(RuntimeError):
        tr.ema_num_updates
    with pytest.raises(ValueError):
        tr.set_ema(1.0)
    tr.train_step(*batch(MICRO, head, 3))
    tr.set_ema(0.5)                                                        # on again: starts from the current weights
    assert tr.ema_num_updates == 0
    same_floats(tr.ema_state_dict(), tr.model_state_dict())
