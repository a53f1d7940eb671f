"""Per-tensor weight decay, coupled or decoupled (AdamW), in the fused Adam update: cris_adamw_step, ops.AdamTable.set_decay,
NativeTrainer(decoupled_weight_decay=..., no_decay=...).

The kernel is cris_adam_step_amp with one decay per descriptor, so nearly every comparison is bit for bit against the kernel that
existed before: coupled decay against its scalar `weight_decay`, decoupled decay against "multiply the parameters by
keep = float32(1 - float64(lr) * float64(wd)) with torch, then run it with weight_decay = 0".  One comparison is against
torch.optim.AdamW on the CPU, within the bound of the existing Adam comparisons.  Ops level: one mixed table that has every update
path (9-tap and 1-tap packed tiles, transposed and not, plain tensors, GEMM-layout gradients, an embedding with row marks).  Trainer
level: tiny spec, 64 x 64, micro-batches of two."""
import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)

pytestmark = pytest.mark.gpu

from cris.pytorch_amd import ops  # noqa: E402
from cris.pytorch_amd.trainer import EMBEDDING, no_decay_1d, no_decay_1d_and_positional  # noqa: E402
from trainer_cases import ADAM_TOL, MICRO, batch, make_trainer, recorded, relerr, same_floats  # noqa: E402

DEV = "cuda"
STEPS = 3
SENTINEL = 7.0                      # fills the padding columns of the GEMM-layout gradients: must never be read


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


def gemm_layout(g, cpad):
    """[N][C][3][3] -> [N][9 * cpad] as cris_conv_wgrad writes it, padding columns = SENTINEL"""
    N, Cc = g.shape[:2]
    out = torch.full((N, 9, cpad), SENTINEL)
    out[:, :, :Cc] = g.permute(0, 2, 3, 1).reshape(N, 9, Cc)
    return out.reshape(N, 9 * cpad)


# ---- the mixed table ----------------------------------------------------------------------------------------------------------
# name, shape, (N, Cin, taps, Cpad) of a GEMM-layout gradient or None
V, D = 3000, 48                     # embedding: 144000 elements = 18 blocks of 8192, rows straddle block edges
SHAPES = [("conv3x3 packed", (70, 66, 3, 3), (70, 66, 9, 72)),     # ragged N / Cin: partial 9-tap tiles
          ("linear packed", (100, 72), None),                      # 1-tap tiles, two along each axis
          ("linear packed transposed", (64, 136), None),           # stored [Cin][N]
          ("bias", (300,), None),
          ("three", (3,), None),
          ("two blocks", (8192 + 5,), None),
          ("conv3x3 unpacked", (24, 20, 3, 3), (24, 20, 9, 24)),
          ("embedding", (V, D), None)]
EMB = 7
LRS = [1e-2 if i % 2 == 0 else 1e-3 for i in range(len(SHAPES))]
INIT = [rnd(*shape, seed=i) for i, (_, shape, _) in enumerate(SHAPES)]
ROWS = [[3, 170, 171, 2999, 5 + 11 * s] for s in range(STEPS)]       # rows of the embedding that get a gradient in step s
UNTOUCHED = torch.ones(V, dtype=torch.bool)
UNTOUCHED[[r for rows in ROWS for r in rows]] = False


def step_grads(s):
    """gradients of step s in the parameter layout (CPU), the embedding's zero outside ROWS[s]"""
    out = [rnd(*shape, seed=100 + 10 * s + i) * (s + 1) for i, (_, shape, _) in enumerate(SHAPES)]
    e = torch.zeros(V, D)
    e[ROWS[s]] = out[EMB][ROWS[s]]
    out[EMB] = e
    return out


GRADS = [step_grads(s) for s in range(STEPS)]


def keep_of(lr, wd):
    """the kernel's factor of decoupled decay, restated in numpy"""
    return np.float32(1.0 - np.float64(np.float32(lr)) * np.float64(np.float32(wd)))


class Table:
    def __init__(self, use_live=True):
        self.p = [t.clone().to(DEV) for t in INIT]
        self.packs = ops.PackTable()
        self.packs.add(self.p[0].view(70, 66, 9), 70, 66, 9, Cpad=72)
        self.packs.add(self.p[1].view(100, 72, 1), 100, 72, 1)
        self.packs.add(self.p[2], 136, 64, 1, src_transposed=True)
        self.packs.run()                                            # real operand copies to start from
        self.g = [torch.zeros(lay[0], lay[2] * lay[3], device=DEV) if lay else torch.zeros(shape, device=DEV) for _, shape, lay in SHAPES]
        self.live = torch.zeros(V, dtype=torch.uint8, device=DEV)
        self.adam = ops.AdamTable(self.p, self.g, LRS, layouts=[lay for _, _, lay in SHAPES],
                                  packs=self.packs.info + [None] * (len(SHAPES) - 3), row_live={EMB: self.live} if use_live else None)
        assert self.adam.index == {9: [0], 1: [1, 2, 3, 4, 5, 6, 7]}
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=DEV)

    def load_grads(self, s):
        for i, (_, _, lay) in enumerate(SHAPES):
            g = GRADS[s][i]
            self.g[i].copy_(gemm_layout(g, lay[3]) if lay else g)
        self.live[ROWS[s]] = 1                                      # what cris_embed_bwd does

    def pack_tensors(self):
        return [t for f, d, *_ in self.packs.info for t in (f, d)]

    def snapshot(self):
        torch.cuda.synchronize()
        out = dict(p=[t.cpu().clone() for t in self.p], m=[t.cpu().clone() for t in self.adam.m], v=[t.cpu().clone() for t in self.adam.v],
                   packs=[t.cpu().clone() for t in self.pack_tensors()])
        return out


_RUNS = {}


def run(decays=None, decoupled=False, wd=0.0, scale_first=None, use_live=True, loss_scale=None):
    """three steps on a fresh table, computed once per configuration and read-only afterwards.
    decays: set_decay(decays, decoupled) -> cris_adamw_step; else the existing cris_adam_step_amp with the scalar wd.
    scale_first: the oracle of decoupled decay - before every step parameter i is multiplied by keep_of(LRS[i], scale_first[i]) with
    torch (tensors with decay 0 are left alone)."""
    key = (None if decays is None else tuple(decays), decoupled, wd, None if scale_first is None else tuple(scale_first), use_live, loss_scale)
    if key in _RUNS:
        return _RUNS[key]
    t = Table(use_live)
    if decays is not None:
        t.adam.set_decay(decays, decoupled)
    ls = None if loss_scale is None else torch.tensor([loss_scale], device=DEV)
    for s in range(STEPS):
        t.load_grads(s)
        t.step_dev += 1
        if scale_first is not None:
            for p, lr, w in zip(t.p, LRS, scale_first):
                if w != 0:
                    p.mul_(float(keep_of(lr, w)))
        t.adam.step_count = 100                                     # host counter deliberately wrong: the device count must win
        t.adam.step(weight_decay=wd, step_dev=t.step_dev, loss_scale_dev=ls)
    out = t.snapshot()
    t.packs.run()                                                   # the reference packing of the final parameters
    torch.cuda.synchronize()
    out["repacked"] = [x.cpu().clone() for x in t.pack_tensors()]
    _RUNS[key] = out
    return out


def same_tensor(a, b, i):
    return all(torch.equal(a[k][i], b[k][i]) for k in ("p", "m", "v"))


def assert_same(a, b):
    bad = [SHAPES[i][0] for i in range(len(SHAPES)) if not same_tensor(a, b, i)]
    assert not bad, bad
    assert all(torch.equal(x, y) for x, y in zip(a["packs"], b["packs"])), "bf16 operand copies differ"


def assert_packs_current(a):
    assert len(a["packs"]) == 6
    assert all(torch.equal(x, y) for x, y in zip(a["packs"], a["repacked"])), "operand copies are not those of the final parameters"


@pytest.mark.parametrize("w", [0.0, 0.5])
def test_coupled_uniform_equals_the_scalar_kernel(w):
    got, want = run(decays=[w] * len(SHAPES)), run(wd=w)
    assert_same(got, want)
    assert_packs_current(got)
    if w == 0.0:                                                    # the marks are honoured: untouched rows are untouched
        assert torch.equal(got["p"][EMB][UNTOUCHED], INIT[EMB][UNTOUCHED])
    else:
        assert not any(same_tensor(got, run(wd=0.0), i) for i in range(len(SHAPES)))       # the decay does something, everywhere


def test_coupled_mixed_is_tensor_by_tensor_one_of_the_scalar_runs():
    w = 0.5
    for first in (w, 0.0):                                          # both alternations: every tensor is decayed once and exempt once
        decays = [first if i % 2 == 0 else w - first for i in range(len(SHAPES))]
        got = run(decays=decays)
        for i, d in enumerate(decays):
            assert same_tensor(got, run(wd=d), i), (SHAPES[i][0], d)
            assert not same_tensor(got, run(wd=w - d), i), (SHAPES[i][0], d)
        assert_packs_current(got)
        want_packs = [run(wd=decays[i // 2])["packs"][i] for i in range(6)]                # packs 2i, 2i + 1 belong to tensor i
        assert all(torch.equal(x, y) for x, y in zip(got["packs"], want_packs))


MIXED = [0.5, 0.0, 0.25, 0.5, 0.0, 0.5, 0.1, 0.0]                   # the embedding is exempt: its marks are honoured


def test_decoupled_equals_scaling_then_the_existing_kernel():
    got, want = run(decays=MIXED, decoupled=True), run(scale_first=MIXED)
    assert_same(got, want)
    assert_packs_current(got)
    assert_same(got, run(decays=MIXED, decoupled=True, use_live=False))                    # the dense run, without marks
    assert torch.equal(got["p"][EMB][UNTOUCHED], INIT[EMB][UNTOUCHED])
    assert not torch.equal(got["p"][EMB][~UNTOUCHED], INIT[EMB][~UNTOUCHED])
    plain = run(wd=0.0)
    for i, w in enumerate(MIXED):                                   # a no-op exactly where the decay is 0
        assert same_tensor(got, plain, i) == (w == 0), SHAPES[i][0]
    # decoupled is not coupled
    assert not any(same_tensor(got, run(decays=MIXED), i) for i, w in enumerate(MIXED) if w != 0)


def test_decoupled_decay_of_the_embedding_ignores_the_row_marks():
    decays = list(MIXED)
    decays[EMB] = 0.5
    got = run(decays=decays, decoupled=True)                        # with marks
    assert_same(got, run(decays=decays, decoupled=True, use_live=False))
    assert_same(got, run(scale_first=decays, use_live=False))
    # rows without a gradient shrink: three times * keep, each product rounded
    k = torch.tensor(keep_of(LRS[EMB], 0.5))
    want = INIT[EMB][UNTOUCHED]
    for _ in range(STEPS):
        want = want * k
    assert torch.equal(got["p"][EMB][UNTOUCHED], want) and not torch.equal(want, INIT[EMB][UNTOUCHED])
    assert not got["m"][EMB][UNTOUCHED].any() and not got["v"][EMB][UNTOUCHED].any()


def test_decoupled_against_torch_adamw():
    """torch.optim.AdamW in fp32 on the CPU, one group per tensor: weight decay 0.5 / 0 and rates 1e-2 / 1e-3 in all four
    combinations.  ADAM_TOL is the bound of the existing Adam comparisons; a CPU emulation of the kernel's arithmetic is at 1.4e-7
    for lr 1e-2 / wd 0.5."""
    decays = [0.5 if (i // 2) % 2 == 0 else 0.0 for i in range(len(SHAPES))]
    assert {(lr, w) for lr, w in zip(LRS, decays)} == {(1e-2, 0.5), (1e-3, 0.5), (1e-2, 0.0), (1e-3, 0.0)}
    ref = [torch.nn.Parameter(t.clone()) for t in INIT]
    opt = torch.optim.AdamW([{"params": [p], "lr": lr, "weight_decay": w} for p, lr, w in zip(ref, LRS, decays)],
                            betas=(0.9, 0.999), eps=1e-8)
    for s in range(STEPS):
        for p, g in zip(ref, GRADS[s]):
            p.grad = g.clone()
        opt.step()
    got, plain = run(decays=decays, decoupled=True), run(wd=0.0)
    for i, (name, _, _) in enumerate(SHAPES):
        err = relerr(got["p"][i], ref[i].data)
        print("%-26s lr %g wd %g: relative L2 error %.3g" % (name, LRS[i], decays[i], err))
        assert err <= ADAM_TOL, (name, err)
        assert same_tensor(got, plain, i) == (decays[i] == 0), name                        # the decay is not a no-op


def test_skip_and_loss_scale():
    t = Table()
    t.adam.set_decay(MIXED, True)
    t.load_grads(0)
    t.step_dev += 1
    before = t.snapshot()
    t.adam.step(step_dev=t.step_dev, skip_dev=torch.tensor([1.0], device=DEV))
    after = t.snapshot()
    assert_same(after, before)
    assert any(bool(x.any()) for x in before["packs"]) and not any(bool(x.any()) for x in after["m"])
    t.adam.step(step_dev=t.step_dev, skip_dev=torch.tensor([0.0], device=DEV))             # (and a zero found_inf does not skip)
    assert not any(same_tensor(t.snapshot(), before, i) for i in range(len(SHAPES)))
    # the loss scale divides the gradient exactly as in the existing kernel
    got, want = run(decays=MIXED, decoupled=True, loss_scale=3.0), run(scale_first=MIXED, loss_scale=3.0)
    assert_same(got, want)
    assert not any(same_tensor(got, run(decays=MIXED, decoupled=True), i) for i in range(len(SHAPES)))


def test_step_refuses_a_scalar_next_to_a_list():
    t = Table()
    t.adam.set_decay(MIXED, False)
    dev = dict(t.adam._decay_dev)
    assert sorted(dev) == [1, 9] and dev[9].cpu().tolist() == [0.5]
    assert dev[1].cpu().tolist() == [float(np.float32(w)) for w in MIXED[1:]]
    with pytest.raises(ValueError):
        t.adam.step(weight_decay=0.01, step_dev=t.step_dev)
    t.adam.set_decay([0.125] * len(SHAPES), True)                   # rewritten in place: a captured graph keeps valid addresses
    assert all(t.adam._decay_dev[k] is dev[k] for k in dev) and dev[1].cpu().tolist() == [0.125] * 7
    t.adam.set_decay(None)
    assert t.adam.decays is None


# ---- the trainer ----------------------------------------------------------------------------------------------------------------
WD = 0.1
# four distinct rows (backbone, rest), none of them the constructor's (1e-4, 1e-4)
T4 = np.array([[2e-5, 3e-4], [5e-5, 2.5e-4], [8e-5, 2e-4], [6e-5, 1.5e-4]], dtype=np.float32)


def train(tr, head, steps):
    losses = []
    for t in range(steps):
        loss, _ = tr.train_step(*batch(tr.accum_steps * MICRO, head, t))
        losses.append(float(loss))
    torch.cuda.synchronize()
    out = dict(losses=losses, final=tr.model_state_dict(), m=[t.detach().cpu().clone() for t in tr.adam.m],
               v=[t.detach().cpu().clone() for t in tr.adam.v])
    if tr._ema is not None:
        out["ema"] = tr.ema_state_dict()
    return out


def scaling_oracle(steps, rule, table=T4, wd=WD, **kw):
    """a trainer WITHOUT weight decay whose Adam step is preceded by p *= keep on every tensor `rule` does not exempt, keep from the
    schedule row of the running step, the tensor's group and wd - "scale, then the existing kernel", eagerly"""
    tr, head = make_trainer(launch="eager", lr_schedule=table, **kw)
    assert tr.weight_decay == 0.0 and tr.adam.decays is None
    if tr._ema is not None:
        tr._ema.drop_row_live()                  # the scaling below moves embedding rows that never had a gradient
    original = tr.adam.step

    def step(**args):
        row = table[min(int(tr.step_dev.item()) - 1, len(table) - 1)]           # step_dev is 1-based and already advanced
        for n, p in zip(tr.names, tr.adam.params):
            if not (rule is not None and rule(n, p)):
                p.mul_(float(keep_of(row[tr.group[n]], wd)))
        return original(**args)
    tr.adam.step = step
    return train(tr, head, steps)


def same_training(a, b):
    assert a["losses"] == b["losses"], (a["losses"], b["losses"])
    same_floats(a["final"], b["final"])
    assert all(torch.equal(x, y) for x, y in zip(a["m"], b["m"])) and all(torch.equal(x, y) for x, y in zip(a["v"], b["v"]))


_ORACLES = {}


def oracle(name, *args, **kw):
    if name not in _ORACLES:
        _ORACLES[name] = scaling_oracle(*args, **kw)
    return _ORACLES[name]


@pytest.mark.parametrize("launch", ["eager", "graph", "cmdlist"])
def test_trainer_decoupled_with_schedule_equals_scaling_then_adam(launch):
    tr, head = make_trainer(launch=launch, weight_decay=WD, decoupled_weight_decay=True, no_decay=no_decay_1d_and_positional, lr_schedule=T4)
    got = train(tr, head, 4)
    assert tr.launch == launch, tr.graph_error
    want = oracle("schedule", 4, no_decay_1d_and_positional)
    same_training(got, want)
    wds = tr.weight_decays
    assert list(wds) == tr.names and set(wds.values()) == {0.0, WD}
    assert all((wds[n] == 0.0) == (tr.engine.P[n].dim() <= 1 or "positional_embedding" in n) for n in tr.names)
    if launch == "eager":                                          # the decay did something
        plain, head0 = make_trainer(launch="eager", lr_schedule=T4)
        assert train(plain, head0, 4)["losses"] != got["losses"]


@pytest.mark.parametrize("launch", ["eager", "graph"])
def test_trainer_decoupled_with_accumulation_clipping_and_ema(launch):
    kw = dict(accum_steps=2, max_norm=1e-3, ema_decay=0.9)
    tr, head = make_trainer(launch=launch, weight_decay=WD, decoupled_weight_decay=True, no_decay=no_decay_1d_and_positional, lr_schedule=T4, **kw)
    got = train(tr, head, 3)
    assert tr.launch == launch and tr.step_idx == 3 and float(tr.grad_norm) > 1e-3                         # (it does clip)
    want = oracle("accum clip ema", 3, no_decay_1d_and_positional, **kw)
    same_training(got, want)
    same_floats(got["ema"], want["ema"])


def test_trainer_coupled_with_exemptions_is_tensor_by_tensor_one_of_the_scalar_trainers():
    w = 0.5
    runs = {}
    for key, kw in (("mixed", dict(weight_decay=w, no_decay=no_decay_1d)), ("zero", {}), ("scalar", dict(weight_decay=w))):
        tr, head = make_trainer(launch="eager", **kw)
        runs[key] = train(tr, head, 1)
        runs[key]["tr"] = tr
    tr = runs["mixed"]["tr"]
    assert tr.adam.decays is not None and not tr.adam.decoupled and runs["zero"]["tr"].adam.decays is None and runs["scalar"]["tr"].adam.decays is None
    exempt = decayed = moved = 0
    for j, n in enumerate(tr.names):
        like = "zero" if tr.engine.P[n].dim() <= 1 else "scalar"
        for a, b in ((runs["mixed"]["final"][n], runs[like]["final"][n]), (runs["mixed"]["m"][j], runs[like]["m"][j]),
                     (runs["mixed"]["v"][j], runs[like]["v"][j])):
            assert torch.equal(a, b), (n, like)
        exempt += like == "zero"
        decayed += like == "scalar"
        moved += not torch.equal(runs["zero"]["m"][j], runs["scalar"]["m"][j])
    assert exempt > 10 and decayed > 10 and moved > 10              # (the two scalar trainers differ: the comparison can tell them apart)


def test_default_issues_the_launches_it_always_did():
    a, cmds_a = recorded(weight_decay=0.01)
    b, cmds_b = recorded(weight_decay=0.01, decoupled_weight_decay=False, no_decay=None)
    c, cmds_c = recorded()
    assert cmds_a == cmds_b and len(cmds_a) > 100
    for tr, cmds in ((a, cmds_a), (c, cmds_c)):
        names = [name for name, _ in cmds]
        assert "cris_adamw_step" not in names and names.count("cris_adam_step_amp") == sum(1 for t in tr.adam.tables.values() if t.n) >= 1
        assert tr.adam.decays is None and tr.adam._decay_dev is None                                       # nothing new is allocated
    assert a.engine.embed_live is None and c.engine.embed_live is not None
    d, cmds_d = recorded(weight_decay=0.01, decoupled_weight_decay=True)
    assert d.adam.decays == [0.01] * len(d.names) and d.adam.decoupled
    assert cmds_d != cmds_a
    # the same list but for the Adam calls' name (and their one more argument)
    assert [("cris_adam_step_amp", n - 1) if name == "cris_adamw_step" else (name, n) for name, n in cmds_d] == cmds_a
    assert not any(name == "cris_adam_step_amp" for name, _ in cmds_d)


def exempt_1d_positional_and_embedding(name, tensor):
    return no_decay_1d_and_positional(name, tensor) or name == EMBEDDING


def test_row_skip_stays_on_when_the_embedding_is_exempt(monkeypatch):
    kw = dict(launch="eager", weight_decay=WD, decoupled_weight_decay=True)
    tr, head = make_trainer(no_decay=exempt_1d_positional_and_embedding, **kw)
    assert tr.engine.embed_live is not None and tr.weight_decays[EMBEDDING] == 0.0 and tr.adam.row_live
    got = train(tr, head, 3)
    live = tr.engine.embed_live.cpu().bool()
    assert live.any() and not live.all()
    monkeypatch.setenv("CRIS_ADAM_ROW_SKIP", "0")
    dense, _ = make_trainer(no_decay=exempt_1d_positional_and_embedding, **kw)
    assert dense.engine.embed_live is None
    same_training(got, train(dense, head, 3))
    monkeypatch.delenv("CRIS_ADAM_ROW_SKIP")
    # with the embedding decayed there are no marks to begin with
    decayed, _ = make_trainer(no_decay=no_decay_1d_and_positional, **kw)
    assert decayed.engine.embed_live is None and decayed.weight_decays[EMBEDDING] == WD


def test_set_weight_decay_makes_a_running_ema_update_every_row():
    tr, head = make_trainer(launch="graph", ema_decay=0.9)
    assert tr.engine.embed_live is not None and tr._ema.row_live
    init = tr.engine.P[EMBEDDING].detach().cpu().clone()
    for t in range(2):
        tr.train_step(*batch(MICRO, head, t))
    torch.cuda.synchronize()
    assert tr._graph is not None
    tr.set_weight_decay(0.1, True, None)
    assert tr._graph is None and not tr._ema.row_live and tr.weight_decays[EMBEDDING] == 0.1 and tr.adam.decoupled
    dead = tr.engine.embed_live.cpu() == 0
    assert dead.any() and torch.equal(tr.ema_state_dict()[EMBEDDING][dead], init[dead])                   # so far untouched
    for t in range(2, 4):
        tr.train_step(*batch(MICRO, head, t))
    torch.cuda.synchronize()
    dead &= tr.engine.embed_live.cpu() == 0                                                                # never used, to the end
    assert dead.any()
    p, ema = tr.model_state_dict()[EMBEDDING], tr.ema_state_dict()[EMBEDDING]
    moved = init[dead] != 0
    assert moved.any()
    assert (p[dead][moved] != init[dead][moved]).all()              # the kernel ignored the marks: rows without a gradient shrank
    assert (ema[dead][moved] != init[dead][moved]).all()            # and the average followed them
    with pytest.raises(ValueError):
        tr.set_weight_decay(-1.0)
    with pytest.raises(ValueError):
        tr.set_weight_decay(0.1, False, lambda n, t: 1)


def test_optimizer_state_dict_carries_the_settings():
    base_keys = {"lr", "initial_lr", "betas", "eps", "weight_decay", "amsgrad", "params"}
    plain, head = make_trainer(launch="eager", weight_decay=0.01)
    train(plain, head, 1)
    sd0 = plain.optimizer_state_dict()
    assert set(sd0) == {"state", "param_groups"} and all(set(g) == base_keys for g in sd0["param_groups"])
    assert all(g["weight_decay"] == 0.01 for g in sd0["param_groups"])
    tr, _ = make_trainer(launch="eager", weight_decay=0.01, decoupled_weight_decay=True, no_decay=no_decay_1d_and_positional)
    train(tr, head, 1)
    sd = tr.optimizer_state_dict()
    g0, g1 = tr._param_order()
    order = g0 + g1
    for g in sd["param_groups"]:
        assert set(g) == base_keys | {"decoupled_weight_decay", "no_decay_params"}
        assert g["decoupled_weight_decay"] is True and g["weight_decay"] == 0.01
        assert set(g["no_decay_params"]) <= set(g["params"])
        want = [i for i in g["params"] if order[i] in tr.names and no_decay_1d_and_positional(order[i], tr.engine.P[order[i]])]
        assert g["no_decay_params"] == want and 0 < len(want) < len(g["params"])
    # the optimizer the reference builds over the same two groups loads it
    ps = [[torch.nn.Parameter(torch.zeros_like(tr.engine.P[n], device="cpu")) for n in names] for names in (g0, g1)]
    opt = torch.optim.Adam([{"params": ps[0]}, {"params": ps[1]}], lr=1e-4)
    opt.load_state_dict(sd)
    assert all(g["decoupled_weight_decay"] is True and g["weight_decay"] == 0.01 for g in opt.param_groups)
    assert opt.param_groups[1]["no_decay_params"] == sd["param_groups"][1]["no_decay_params"]
    # configuration is not restored
    plain.load_optimizer_state_dict(sd)
    assert plain.decoupled_weight_decay is False and plain.adam.decays is None and plain.weight_decays[tr.names[0]] == 0.01
