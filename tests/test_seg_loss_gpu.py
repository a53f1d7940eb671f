"""The configurable segmentation loss (ops.SegLoss: weighted BCE + soft Dice per sample) on the GPU, at three levels.

Ops: cris_seg_loss_fwd / cris_seg_loss_bwd against the formulas of include/cris_hip.h in float64 torch on the CPU
(F.binary_cross_entropy_with_logits with pos_weight for the BCE term, autograd of 3 * loss for the gradient with gscale = 3), every
operand inside guards, with the bounds of the BCE kernels (tests/test_hip_ops_edges.py test_bce_fwd_tails / test_bce_bwd_tails):
1e-5 * max(1, |ref|) on loss and terms, 1e-5 relative L2 per 2048-element chunk on the gradient, 1e-5 relative on coef.
Engine: the tiny spec of selfcheck.run against the CPU oracle's logits with the same loss on top, bounds selfcheck.BOUNDS["tiny"].
Trainer: the option leaves the default step alone, gives the same bits in every launch mode, reports its terms, accumulates
them over micro-batches and can be switched on and off."""
import dataclasses
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from cris.pytorch_amd import arch, ops, selfcheck, synth  # noqa: E402
from cris.pytorch_amd.ops import SegLoss  # noqa: E402
import hip_ops_edge_cases as E  # noqa: E402
from hip_ops_edge_cases import Slab, F32  # noqa: E402
from cris.pytorch_amd.trainer import NativeTrainer  # noqa: E402
from trainer_cases import MICRO, batch, make_trainer, same_floats  # noqa: E402

DEV = "cuda"
TOL = 1e-5
GSCALE = 3.0
SHAPES = [(1, 1), (2, 3), (3, 1023), (3, 1025), (5, 4099), (2, 10816), (9, 10816), (1, 131075)]
SPECS = [(1, 1, 1, 1), (0, 1, 1, 1), (0.5, 2, 3, 1e-3), (1, 0, 2.5, 1)]
# (a pure-Dice gradient of a single element is one catastrophic cancellation and tests nothing else: at (1, 1) only the first spec)
CASES = [(B, HW, s) for (B, HW) in SHAPES for s in SPECS if (B, HW) != (1, 1) or s == SPECS[0]]


# ---- reference ---------------------------------------------------------------------------------------------------------------
def formula(x, t, spec, dt):
    """(loss, bce, dice, coef [B][2]) of logits / targets [B][HW] at dtype dt"""
    w_bce, w_dice, pw, s = spec
    x, t = x.to(dt), t.to(dt)
    bce = F.binary_cross_entropy_with_logits(x, t, pos_weight=torch.tensor(pw, dtype=dt))
    p = torch.sigmoid(x).flatten(1)
    tt = t.flatten(1)
    I, D = (p * tt).sum(1), p.sum(1) + tt.sum(1) + s
    dice = (1 - (2 * I + s) / D).mean()
    return w_bce * bce + w_dice * dice, bce, dice, torch.stack([2 / D, (2 * I + s) / D ** 2], 1)


def reference(x, t, spec):
    xl = x.double().requires_grad_(True)
    loss, bce, dice, coef = formula(xl, t, spec, torch.float64)
    (GSCALE * loss).backward()
    return dict(loss=float(loss.detach()), terms=(float(bce.detach()), float(dice.detach())), coef=coef.detach(), grad=xl.grad)


@functools.lru_cache(maxsize=None)
def inputs(B, HW):
    x = E.randn_f32((B, HW), 61, 3.0)
    t = (torch.rand(B, HW, generator=E.gen(62)) > 0.7).float()
    if B > 1:
        t[0] = 0.0
    if B > 2:
        t[1] = 1.0
    t[-1, :HW // 2] = torch.rand(HW // 2, generator=E.gen(63))           # the soft borders of a bilinear warp
    return x, t


@functools.lru_cache(maxsize=None)
def case_reference(B, HW, spec):
    return reference(*inputs(B, HW), spec)


# ---- launches inside guards --------------------------------------------------------------------------------------------------
def in_slab(v):
    """[B][HW] values in NaN guards; 4 guard rows in front keep the first element on a 16-byte boundary for every HW"""
    B, HW = v.shape
    s = Slab(B, HW, F32, DEV, nan_guard=True, pre=4, post=2).set(v)
    assert s.data.is_contiguous() and s.data.data_ptr() % 16 == 0
    return s


def nan_out(M, C_, pre=2):
    return Slab(M, C_, F32, DEV, pre=pre, post=2).set(torch.full((M, C_), E.NAN))          # overwritten, not accumulated


def launch(x, t, spec, gscale=GSCALE):
    B, HW = x.shape
    sx, st = in_slab(x), in_slab(t)
    out = dict(loss=nan_out(1, 1), terms=nan_out(1, 2), coef=nan_out(B, 2), grad=nan_out(B, HW, pre=4))
    sp = SegLoss(*spec)
    ops.seg_loss_fwd(sx.data, st.data, sp, out["loss"].data, out["terms"].data, out["coef"].data)
    ops.seg_loss_bwd(sx.data, st.data, sp, out["coef"].data, torch.tensor([gscale], device=DEV), out["grad"].data)
    torch.cuda.synchronize()
    for k, s in out.items():
        s.assert_guards("seg_loss " + k)
    return {k: s.get() for k, s in out.items()}


def check(got, ref, what):
    loss, terms = float(got["loss"]), [float(v) for v in got["terms"].flatten()]
    print("%s: loss %.9g (reference %.9g), bce %.9g (%.9g), dice %.9g (%.9g)" % (what, loss, ref["loss"], terms[0], ref["terms"][0],
                                                                                 terms[1], ref["terms"][1]))
    cerr = float(((got["coef"].double() - ref["coef"]).abs() / ref["coef"].abs()).max())
    print("%s: coef worst relative error %.3e" % (what, cerr))
    assert all(bool(torch.isfinite(v).all()) for v in got.values()), what
    assert abs(loss - ref["loss"]) <= TOL * max(1.0, abs(ref["loss"])), (what, loss, ref["loss"])
    for g, r in zip(terms, ref["terms"]):
        assert abs(g - r) <= TOL * max(1.0, abs(r)), (what, terms, ref["terms"])
    assert cerr <= TOL, (what, cerr)
    E.assert_chunks(got["grad"], ref["grad"], TOL, what + " dlogits")


@pytest.mark.parametrize("B,HW,spec", CASES, ids=["%dx%d-%s" % (B, HW, "_".join("%g" % v for v in s)) for B, HW, s in CASES])
def test_ops_against_float64(B, HW, spec):
    x, t = inputs(B, HW)
    check(launch(x, t, spec), case_reference(B, HW, spec), "seg_loss %dx%d %s" % (B, HW, spec))


def test_ops_extremes():
    B, HW, spec = 2, 1025, (1, 1, 3, 1)
    i = torch.arange(B * HW)
    x = torch.tensor([-90.0, -40.0, 0.0, 40.0, 90.0])[i % 5].view(B, HW)
    t = torch.tensor([0.0, 1.0, 0.5])[i % 3].view(B, HW)
    check(launch(x, t, spec), reference(x, t, spec), "seg_loss extremes")


@pytest.mark.parametrize("B,HW", [(3, 1025), (9, 10816), (1, 131075)])
def test_ops_same_bits_every_run(B, HW):
    x, t = inputs(B, HW)
    a, b = launch(x, t, SPECS[2]), launch(x, t, SPECS[2])
    for k in a:
        assert E.bits_equal(a[k], b[k]), k


@pytest.mark.parametrize("B,HW", [(3, 1025), (2, 10816)])
def test_ops_agree_with_the_bce_kernels(B, HW):
    """spec (1, 0, 1, 1) handed to the launches directly (the host layers normalise it away): the mean BCE of cris_bce_fwd /
    cris_bce_bwd in another summation order"""
    x, t = inputs(B, HW)
    got = launch(x, t, (1, 0, 1, 1))
    pad = (-B * HW) % 4
    flat = lambda v: Slab(1, B * HW, F32, DEV, ld=B * HW + pad, nan_guard=True).set(v.reshape(1, -1))          # noqa: E731
    sx, st = flat(x), flat(t)
    loss, grad = nan_out(1, 1), nan_out(1, B * HW)
    ops.bce_fwd(sx.data, st.data, loss.data)
    ops.bce_bwd(sx.data, st.data, torch.tensor([GSCALE], device=DEV), grad.data)
    old = float(loss.get())
    print("seg_loss (1,0,1,1) %dx%d: loss %.9g, cris_bce_fwd %.9g" % (B, HW, float(got["loss"]), old))
    assert abs(float(got["loss"]) - old) <= TOL * max(1.0, abs(old))
    E.assert_chunks(got["grad"].reshape(1, -1), grad.get(), TOL, "seg_loss (1,0,1,1) against cris_bce_bwd")


# ---- engine ------------------------------------------------------------------------------------------------------------------
def test_engine_against_the_oracle():
    """selfcheck.run's configuration (tiny spec, batch 4, 64 x 64, dropout 0.1, seed 11) under SegLoss(1, 1, pos_weight 2), and
    under the default loss in the same process (the unchanged code path), against the CPU oracle with the same loss computed
    from ITS logits in float32 torch; both worst tensors are printed."""
    from oracle import cris_oracle as O
    seed, spec = 11, SegLoss(bce_weight=1, dice_weight=1, pos_weight=2)
    clip, head = arch.specs_by_name("tiny")
    head = dataclasses.replace(head, dropout=0.1)
    sd = arch.synthetic_state_dict(clip, head, 0)
    img, word, mask = synth.make_batch(4, 64, head.word_len, 0, 0)
    dev = torch.device("cuda:0")
    e = NativeTrainer(clip, head, sd, dev).engine
    hip_runs = {}
    for name, sp in (("default", None), ("seg", spec)):
        e.set_loss(sp)
        pred, msk, loss = e.forward(img.to(dev), word.to(dev), mask.to(dev), training=True, seed=seed)
        e.backward()
        torch.cuda.synchronize()
        hip_runs[name] = dict(pred=pred.detach().cpu().clone(), msk=msk.cpu().clone(), loss=float(loss),
                              terms=None if e.loss_terms is None else e.loss_terms.cpu().clone(),
                              grads={k: v.detach().cpu().clone() for k, v in e.grads_param_layout().items()})
    assert hip_runs["default"]["terms"] is None and hip_runs["seg"]["terms"] is not None

    leaf = {k: (v.clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in sd.items()}
    opred, om, oloss = O.cris_forward(leaf, clip, head, img, word, mask, training=True, drop_seed=seed)
    oseg = formula(opred.flatten(1), om.flatten(1), spec.scalars, torch.float32)[0]
    b = selfcheck.BOUNDS["tiny"]
    rep = {}
    for name, ol in (("default", oloss), ("seg", oseg)):
        for v in leaf.values():
            if v.is_floating_point():
                v.grad = None
        ol.backward(retain_graph=True)
        coss = {}
        for k, g in hip_runs[name]["grads"].items():
            og = leaf[k].grad
            if og is None or k.endswith("k_proj.bias") or float(og.norm()) == 0.0:
                continue                # (selfcheck.run's rule: d/d(key bias) == 0 analytically)
            coss[k] = selfcheck._cos(g, og)
        worst = min(coss, key=coss.get)
        rep[name] = dict(loss_hip=hip_runs[name]["loss"], loss_oracle=float(ol.detach()), cos_min=coss[worst], cos_min_name=worst,
                         cos_median=sorted(coss.values())[len(coss) // 2], n=len(coss))
        print("engine %s loss: %s" % (name, rep[name]))
    # wiring: the returned loss is the formula on the RETURNED logits and mask
    r = hip_runs["seg"]
    want, bce, dice, _ = formula(r["pred"].flatten(1), r["msk"].flatten(1), spec.scalars, torch.float64)
    print("engine seg loss: returned %.9g, formula on the returned operands %.9g; terms %s against (%.9g, %.9g)"
          % (r["loss"], float(want), r["terms"].tolist(), float(bce), float(dice)))
    assert abs(r["loss"] - float(want)) <= 1e-5
    assert abs(float(r["terms"][0]) - float(bce)) <= 1e-5 and abs(float(r["terms"][1]) - float(dice)) <= 1e-5
    assert torch.equal(r["msk"], om) and torch.equal(hip_runs["default"]["msk"], om)
    assert torch.equal(r["pred"], hip_runs["default"]["pred"])           # the loss does not reach back into the forward
    for name in ("default", "seg"):
        assert abs(rep[name]["loss_hip"] - rep[name]["loss_oracle"]) <= b["loss"], rep[name]
        assert rep[name]["cos_median"] >= b["grad_cos_median"], rep[name]
        assert rep[name]["cos_min"] >= b["grad_cos_min"], rep[name]


# ---- trainer -----------------------------------------------------------------------------------------------------------------
DICE = SegLoss(dice_weight=1.0)


def steps(tr, head, n, size=MICRO):
    losses, terms = [], []
    for t in range(n):
        loss, _ = tr.train_step(*batch(size, head, t))
        losses.append(loss.clone())
        terms.append(None if tr.loss_terms is None else tr.loss_terms.clone())
    torch.cuda.synchronize()
    return [float(v) for v in losses], [None if v is None else v.cpu() for v in terms], tr.model_state_dict()


def recorded_steps(**kw):
    """trainer_cases.recorded (three steps as a command list: eager, recording, replay) that also hands back what the steps gave"""
    tr, head = make_trainer(launch="cmdlist", **kw)
    out = steps(tr, head, 3)
    assert tr._cmds is not None and tr.launch == "cmdlist"
    return tr, out, [(name, None if args is None else len(args)) for _, args, name in tr._cmds.cmds]


def test_trainer_default_loss_is_the_step_it_was():
    _, base, base_cmds = recorded_steps()                # a trainer built without the argument
    for kw in (dict(loss=None), dict(loss=SegLoss())):
        tr, (losses, terms, final), cmds = recorded_steps(**kw)
        assert tr.loss_spec is None and tr.engine.loss_spec is None
        assert tr.loss_terms is None and tr._terms_acc is None and terms == [None] * 3
        assert losses == base[0]
        same_floats(final, base[2])
        assert cmds == base_cmds
    assert not any(name.startswith("cris_seg_loss") for name, _ in base_cmds)
    _, _, dice_cmds = recorded_steps(loss=DICE)
    swap = {"cris_bce_fwd": "cris_seg_loss_fwd", "cris_bce_bwd": "cris_seg_loss_bwd"}
    assert [swap.get(name, name) for name, _ in base_cmds] == [name for name, _ in dice_cmds]          # launch for launch


def test_trainer_same_bits_in_every_launch_mode():
    runs = {}
    for launch_mode in ("eager", "cmdlist", "graph"):
        tr, head = make_trainer(loss=DICE, launch=launch_mode)
        runs[launch_mode] = steps(tr, head, 3)
        assert tr.launch == launch_mode and (launch_mode == "eager" or tr._graph is not None or tr._cmds is not None), tr.graph_error
    losses, terms, final = runs["eager"]
    for lo, te in zip(losses, terms):
        want = 1.0 * float(te[0]) + 1.0 * float(te[1])
        assert abs(lo - want) <= 1e-6 * abs(want), (lo, te)
        assert float(te[1]) > 0.0
    for mode in ("cmdlist", "graph"):
        assert runs[mode][0] == losses, mode
        assert all(torch.equal(a, b) for a, b in zip(runs[mode][1], terms)), mode
        same_floats(runs[mode][2], final)
    plain, head = make_trainer()
    assert steps(plain, head, 3)[0] != losses            # it IS another loss


def test_trainer_terms_under_accumulation():
    spec, seed = SegLoss(bce_weight=0.5, dice_weight=2.0, pos_weight=3.0), 5
    single, head = make_trainer(loss=spec)
    assert single._terms_acc is None                     # the running mean is held only with both features on
    img, word, mask = batch(2 * MICRO, head, 0)
    micro_terms, micro_loss = [], []
    for m in range(2):                                   # what the two micro-batches of the step below see: same parameters, seed + m
        sl = slice(m * MICRO, (m + 1) * MICRO)
        _, _, loss = single.engine.forward(img[sl], word[sl], mask[sl], training=True, seed=seed + m)
        micro_terms.append(single.engine.loss_terms.cpu().double())
        micro_loss.append(float(loss))
    tr, _ = make_trainer(loss=spec, accum_steps=2)
    assert tr._terms_acc is not None
    loss, _ = tr.train_step(img, word, mask, seed=seed)
    torch.cuda.synchronize()
    got, want = tr.loss_terms.cpu().double(), (micro_terms[0] + micro_terms[1]) / 2
    print("accumulated terms %s, mean of the micro-batches %s" % (got.tolist(), want.tolist()))
    assert bool(((got - want).abs() <= 1e-6 * want.abs()).all())
    wl = (micro_loss[0] + micro_loss[1]) / 2
    assert abs(float(loss) - wl) <= 1e-6 * abs(wl)
    tr.set_accum_steps(1)
    assert tr._terms_acc is None
    plain, _ = make_trainer(accum_steps=2)
    assert plain._terms_acc is None and plain.loss_terms is None


def test_trainer_set_loss_and_back():
    a, head = make_trainer()
    b, _ = make_trainer()
    la, lb = [], []
    for t in range(2):
        if t == 1:
            b.set_loss(DICE)
            assert b.loss_spec == DICE and b._graph is None and b._cmds is None and b._eager_steps == 0          # the capture is dropped
            b.set_loss(None)
            assert b.loss_spec is None and b.loss_terms is None
        la.append(a.train_step(*batch(MICRO, head, t))[0].clone())
        lb.append(b.train_step(*batch(MICRO, head, t))[0].clone())
    torch.cuda.synchronize()
    assert [float(v) for v in la] == [float(v) for v in lb]
    same_floats(b.model_state_dict(), a.model_state_dict())
    b.set_loss(DICE)                                     # and on: the next step is the other loss
    l2 = float(b.train_step(*batch(MICRO, head, 2))[0])
    assert l2 != float(a.train_step(*batch(MICRO, head, 2))[0]) and b.loss_terms is not None
    assert "loss" not in b.optimizer_state_dict() and set(b.optimizer_state_dict()) == {"state", "param_groups"}
