"""Gradient accumulation over micro-batches on the native path: cris_grad_accumulate / cris_step_advance_micro and
NativeTrainer(accum_steps=K), against torch fp32 adds in the documented order ((g0 + g1) + g2), a plain engine that runs the
micro-batches one by one, and torch.optim.Adam on the CPU.  The suite's smallest trainer: tiny spec, 64 x 64, micro-batch 2."""
import math

import pytest
import torch

from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)

pytestmark = pytest.mark.gpu

from cris.pytorch_amd import arch, hip, ops  # noqa: E402
from trainer_cases import ADAM_TOL, MICRO, TwoEqualRanks, batch, make_trainer, relerr  # noqa: E402

DEV = "cuda"


# ---- the kernels ----------------------------------------------------------------------------------------------------
# the issue's sizes (one vector, two, around one block's 256 vectors, a few blocks, ~1 M) and one beyond 8 blocks per CU x 512
# vectors, where the grid-stride loop makes more than one trip
@pytest.mark.parametrize("n", [4, 8, 1020, 1024, 1028, 8192 + 4, (1 << 20) + 12, (5 << 20) + 4])
def test_kernel_equals_torch_bit_for_bit(n):
    g = torch.Generator(device="cpu").manual_seed(n)
    d_host, s_host = torch.randn(n + 8, generator=g), torch.randn(n + 8, generator=g)
    for scale in (1.0, 1e6):                                              # second run: operands six orders of magnitude apart
        D, S = d_host.to(DEV), (s_host * scale).to(DEV)
        D0, S0 = D.clone(), S.clone()
        dst, src = D[4:4 + n], S[4:4 + n]                                 # slices at a 4-float offset, guards on both sides
        assert dst.data_ptr() % 16 == 0 and src.data_ptr() % 16 == 0
        want = torch.add(D0[4:4 + n], S0[4:4 + n])
        ops.grad_accumulate(dst, src)
        assert torch.equal(dst, want), (n, scale, "mode 1")
        assert torch.equal(D[:4], D0[:4]) and torch.equal(D[4 + n:], D0[4 + n:]) and torch.equal(S, S0)
        ops.grad_accumulate(dst, src, add=False)
        assert torch.equal(dst, S0[4:4 + n]), (n, scale, "mode 0")
        assert torch.equal(D[:4], D0[:4]) and torch.equal(D[4 + n:], D0[4 + n:]) and torch.equal(S, S0)


def test_kernel_rejects_bad_arguments():
    lib = hip.load()
    d, s = torch.zeros(64, device=DEV), torch.ones(64, device=DEV)
    for args, msg in (((d.data_ptr(), s.data_ptr(), 6, 1), b"multiple of 4"),
                      ((d.data_ptr(), s.data_ptr(), 0, 1), b"multiple of 4"),
                      ((d.data_ptr() + 4, s.data_ptr(), 8, 1), b"16-byte aligned"),
                      ((d.data_ptr(), s.data_ptr() + 8, 8, 0), b"16-byte aligned"),
                      ((d.data_ptr(), s.data_ptr(), 8, 2), b"mode"),
                      ((d.data_ptr(), d.data_ptr() + 16, 8, 1), b"overlap"),
                      ((None, s.data_ptr(), 8, 1), b"cris_grad_accumulate")):
        assert lib.cris_grad_accumulate(*args, None) != 0, args
        assert msg in lib.cris_last_error(), (args, lib.cris_last_error())
    torch.cuda.synchronize()
    assert float(d.abs().sum()) == 0.0 and float(s.sum()) == 64.0        # nothing was launched


def test_step_advance_micro():
    """step counts optimizer steps (advanced by micro-batch 0 only), seed = (s * accum + m) * 7919 + 17 in uint32, the mailbox
    generation advances with every micro-batch; accum = 1 is cris_step_advance"""
    def state(step, gen):
        return (torch.tensor([step], dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV),
                torch.tensor([gen], dtype=torch.int32, device=DEV))
    for s0, accum in ((0, 2), (5, 3), (600000, 4)):                       # (the last one wraps the 32-bit seed)
        step, seed, gen = state(s0, 10)
        for m in range(accum):
            ops.step_advance_micro(step, seed, gen, m, accum)
            assert int(step) == s0 + 1 and int(gen) == 11 + m
            assert int(seed) & 0xFFFFFFFF == ((s0 * accum + m) * 7919 + 17) & 0xFFFFFFFF
        ops.step_advance_micro(step, seed, gen, 0, accum)
        assert int(step) == s0 + 2 and int(seed) & 0xFFFFFFFF == (((s0 + 1) * accum) * 7919 + 17) & 0xFFFFFFFF
    a, b = state(7, 3), state(7, 3)
    ops.step_advance(*a)
    ops.step_advance_micro(*b, 0, 1)
    assert [int(t) for t in a] == [int(t) for t in b]
    lib = hip.load()
    assert lib.cris_step_advance_micro(a[0].data_ptr(), a[1].data_ptr(), None, 2, 2, None) != 0
    assert b"micro" in lib.cris_last_error()


# ---- the trainer ------------------------------------------------------------------------------------------------------
def run(steps, K=2, launch="eager", changes=None, **kw):
    """`steps` optimizer steps of K micro-batches of MICRO samples (K=None: a trainer built without the argument); changes:
    {step index: K set before that step}.  Per step: loss, metric, tracked norm, float64 norm of G / K; final parameters."""
    tr, head = make_trainer(launch=launch, **({} if K is None else {"accum_steps": K}), **kw)
    out = dict(tr=tr, losses=[], metrics=[], norms=[], norms64=[], grads=[])
    for t in range(steps):
        if changes and t in changes:
            tr.set_accum_steps(changes[t])
        k = tr.accum_steps
        loss, metric = tr.train_step(*batch(k * MICRO, head, t))
        out["losses"].append(float(loss))
        out["metrics"].append(metric.cpu().tolist())
        if tr.max_norm > 0 or tr.track_grad_norm:
            out["norms"].append(float(tr.grad_norm))
        g = tr.engine.grads_param_layout()
        out["grads"].append({n: g[n].detach().cpu().clone() for n in tr.names})
        out["norms64"].append(math.sqrt(sum(float(((g[n].double() / k) ** 2).sum()) for n in tr.names)))
    torch.cuda.synchronize()
    out["params"] = {k: v.clone() for k, v in tr.engine.P.items()}
    return out


_FIRST = {}


def first_step(K):
    """computed once per K, read-only afterwards: step 0 of an accumulating trainer, and the same K micro-batches run one by
    one through the plain engine of a second trainer built from the same state dict, with the seeds of the rule
    (s * K + m) * 7919 + 17 at s = 0"""
    if K in _FIRST:
        return _FIRST[K]
    acc = run(1, K=K)
    ref, head = make_trainer(launch="eager")
    e = ref.engine
    img, word, mask = batch(K * MICRO, head, 0)
    grads, losses, metrics = [], [], []
    for m in range(K):
        sl = slice(m * MICRO, (m + 1) * MICRO)
        e.seed_dev = None
        pred, msk, loss = e.forward(img[sl], word[sl], mask[sl], training=True, seed=(0 * K + m) * 7919 + 17)
        met = torch.zeros(2, device="cuda:0")
        ops.train_metric(pred, msk, pred.shape[0], pred.shape[2] * pred.shape[3], met)
        e.backward()
        g = e.grads_param_layout()
        grads.append({n: g[n].detach().clone() for n in ref.names})
        losses.append(float(loss))
        metrics.append(met.cpu().double())
    torch.cuda.synchronize()
    _FIRST[K] = dict(acc=acc, names=ref.names, grads=grads, losses=losses, metrics=metrics,
                     ref_bn={k: v.clone() for k, v in e.Bf.items()}, acc_bn={k: v.clone() for k, v in acc["tr"].engine.Bf.items()})
    return _FIRST[K]


@pytest.fixture(scope="module")
def k2():
    """three eager K = 2 steps with the norm tracked (tracking changes no result: test_grad_clip_gpu.py)"""
    return run(3, K=2, track_grad_norm=True)


@pytest.mark.parametrize("K", [2, 3])
def test_accumulated_gradient_is_the_ordered_sum(K):
    """every micro-batch gradient is deterministic and every add is one rounding: bit for bit ((g0 + g1) + g2)"""
    f = first_step(K)
    tr = f["acc"]["tr"]
    assert tr.accum_steps == K and tr.names == f["names"] and tr._acc.numel() == tr.engine.grad_arena.numel()
    got = f["acc"]["grads"][0]
    differ = 0
    for n in tr.names:
        want = f["grads"][0][n]
        for m in range(1, K):
            want = torch.add(want, f["grads"][m][n])
        assert torch.equal(got[n], want.cpu()), n
        differ += int(not torch.equal(want, f["grads"][0][n]))
    assert differ > len(tr.names) // 2                                    # (the later micro-batches do contribute)
    loss, want = f["acc"]["losses"][0], sum(f["losses"]) / K
    print("K", K, "loss", loss, "mean of the micro-batch losses", want, f["losses"])
    assert abs(loss - want) <= 1e-6 * abs(want)
    metric, wantm = f["acc"]["metrics"][0], (sum(f["metrics"]) / K).tolist()
    print("metric", metric, "mean of the micro-batch metrics", wantm)
    assert metric == pytest.approx(wantm, rel=1e-6, abs=0)


def test_update_equals_torch_adam_on_the_averaged_gradient(k2):
    tr = k2["tr"]
    clip, head = arch.specs_by_name("tiny")
    sd = arch.synthetic_state_dict(clip, head, 0)
    ref = {n: torch.nn.Parameter(sd[n].detach().clone().float()) for n in tr.names}
    opt = torch.optim.Adam([{"params": [ref[n]], "lr": lr} for n, lr in zip(tr.names, tr.adam.lrs)], betas=(0.9, 0.999), eps=1e-8)
    assert set(tr.adam.lrs) == {tr.base_lr}                               # both groups start at base_lr
    for t in range(3):
        for n in tr.names:
            ref[n].grad = k2["grads"][t][n] / 2
        opt.step()
    worst = max((relerr(k2["params"][n], ref[n].data), n) for n in tr.names)
    print("worst relative L2 error", worst)
    assert math.isfinite(worst[0]) and worst[0] <= ADAM_TOL, worst
    assert tr.step_idx == 3
    state = tr.optimizer_state_dict()["state"]
    assert state and all(float(s["step"]) == 3.0 for s in state.values())
    tracked = [v for k, v in tr.model_state_dict().items() if k.endswith("num_batches_tracked")]
    assert tracked and all(int(v) == 6 for v in tracked)


def test_batchnorm_running_statistics_see_every_micro_batch():
    f = first_step(2)
    assert f["ref_bn"] and set(f["ref_bn"]) == set(f["acc_bn"])
    clip, head = arch.specs_by_name("tiny")
    sd = arch.synthetic_state_dict(clip, head, 0)
    moved = 0
    for k, v in f["ref_bn"].items():
        assert torch.equal(f["acc_bn"][k], v), k
        moved += int(not torch.equal(v.cpu(), sd[k].float()))
    assert moved > len(f["ref_bn"]) // 2                                  # (the forwards did update them)


def test_one_micro_batch_is_the_plain_trainer():
    a, b = run(3, K=1), run(3, K=None)
    assert a["tr"].accum_steps == b["tr"].accum_steps == 1
    assert a["tr"]._acc is None and b["tr"]._acc is None                  # no accumulation buffer
    assert a["losses"] == b["losses"], (a["losses"], b["losses"])
    assert a["metrics"] == b["metrics"]
    assert all(torch.equal(a["params"][k], b["params"][k]) for k in a["params"])


@pytest.mark.parametrize("launch", ["graph", "cmdlist"])
def test_replay_of_all_micro_batches(launch):
    e = run(5, K=2, launch="eager", track_grad_norm=True)
    r = run(5, K=2, launch=launch, track_grad_norm=True)
    tr = r["tr"]
    assert tr.launch == launch and (tr._graph is not None or tr._cmds is not None), tr.graph_error
    assert e["losses"] == r["losses"], (e["losses"], r["losses"])
    assert e["norms"] == r["norms"], (e["norms"], r["norms"])
    assert e["metrics"] == r["metrics"]
    assert all(torch.equal(e["params"][k], r["params"][k]) for k in e["params"])
    assert len(set(r["norms"][2:])) == len(r["norms"][2:]), r["norms"]   # steps 3-5 are replays
    assert tr.step_idx == 5


def test_clipping_composes(k2):
    """grad_norm is the norm of the rank- and micro-batch-averaged gradient G / K: to 1e-5 of its float64 value, the bound
    derived in test_grad_clip_gpu.py (the reduction is the same, 1/K is the update's grad_scale)"""
    for got, want in zip(k2["norms"], k2["norms64"]):
        print("tracked", got, "float64 |G / K|", want)
        assert abs(got - want) / want <= 1e-5
    max_norm = 0.5 * k2["norms"][1]
    c = run(3, K=2, max_norm=max_norm)
    for got, want in zip(c["norms"], c["norms64"]):
        print("clipping", got, "float64 |G / K|", want, "max_norm", max_norm)
        assert abs(got - want) / want <= 1e-5
    assert any(n > max_norm for n in c["norms"][:2])                      # step 2 at the latest was clipped
    assert any(not torch.equal(c["params"][k], k2["params"][k]) for k in c["params"])
    assert all(bool(torch.isfinite(p).all()) for p in c["params"].values())


def test_exchange_runs_once_per_optimizer_step(k2):
    one = run(1, K=1, comm=TwoEqualRanks())
    per_step = dict(one["tr"].comm.calls)
    assert per_step["sum"] == len(one["tr"].engine.stage_ranges) and per_step["max"] == 1
    two = run(3, K=2, comm=TwoEqualRanks())
    tr = two["tr"]
    assert tr.comm.world == 2 and tr.grad_exchange == "rccl"
    assert tr.comm.calls == {k: 3 * v for k, v in per_step.items()}, (tr.comm.calls, per_step)
    assert two["losses"] == pytest.approx(k2["losses"], rel=1e-6)
    for k in k2["params"]:
        assert relerr(two["params"][k], k2["params"][k]) <= ADAM_TOL, k


def test_arguments():
    for bad in (0, -1, 1.5, "2", True):
        with pytest.raises(ValueError):
            make_trainer(accum_steps=bad)
    tr, head = make_trainer(accum_steps=2, launch="graph")
    with pytest.raises(ValueError):
        tr.train_step(*batch(3, head, 0))
    assert tr.step_idx == 0
    e = run(6, K=2, launch="eager", changes={3: 3})
    losses = []
    for t in range(6):
        if t == 3:
            assert tr._graph is not None, tr.graph_error
            with pytest.raises(ValueError):
                tr.set_accum_steps(0)
            tr.set_accum_steps(3)
            assert tr._graph is None and tr.accum_steps == 3              # dropped: K is the shape of the schedule
        losses.append(float(tr.train_step(*batch(tr.accum_steps * MICRO, head, t))[0]))
    torch.cuda.synchronize()
    assert tr._graph is not None
    assert losses == e["losses"], (losses, e["losses"])
    assert all(torch.equal(e["params"][k], tr.engine.P[k]) for k in e["params"])
