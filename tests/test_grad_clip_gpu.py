"""Gradient clipping by global norm on the native path: cris_grad_sumsq / cris_grad_clip_finalize over the Adam tables
(ops.AdamTable.grad_norm) and NativeTrainer(max_norm=...), against float64 sums and torch.nn.utils.clip_grad_norm_ +
torch.optim.Adam on the CPU."""
import math

import pytest
import torch

from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)

pytestmark = pytest.mark.gpu

from cris.pytorch_amd import arch, hip, ops  # noqa: E402
from cris.pytorch_amd.trainer import NativeTrainer  # noqa: E402
from trainer_cases import ADAM_TOL, TwoEqualRanks, batch, make_trainer, relerr  # noqa: E402

DEV = "cuda"


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed + sum(shape))
    return torch.randn(*shape, generator=g) * scale


def gemm_layout(g, Cpad, poison):
    """[N][Cin][taps] (parameter layout) -> [N][taps][Cpad] with the padding columns set to `poison`"""
    N, Cin, taps = g.shape
    out = torch.full((N, taps, Cpad), poison, dtype=torch.float32)
    out[:, :, :Cin] = g.permute(0, 2, 1)
    return out.reshape(N, taps * Cpad)


def synthetic_table():
    """every path of the block partition: plain tensors around the block size, two 1-tap packed weights with ragged tiles (one
    stored [n][c], one stored transposed, [c][n]), two padded GEMM-layout gradients whose padding is poisoned, a row_live
    tensor with dead rows.  Returns (table, logical gradients on the CPU)."""
    E = hip.load().cris_adam_block_elems()
    logical, grads, layouts, packs, params = [], [], [], [], []

    def add(g, grad=None, layout=None, pack=None, param=None):
        logical.append(g); grads.append(g.clone() if grad is None else grad); layouts.append(layout); packs.append(pack)
        params.append(param if param is not None else torch.zeros(g.shape[0], g.numel() // g.shape[0], device=DEV))

    for k, n in enumerate((1, E - 1, E, E + 1, 3 * E + 7)):
        add(rnd(n, seed=k, scale={1: 1e-3, 4: 1e3}.get(k, 1.0)))          # two tensors six orders of magnitude apart
    pt = ops.PackTable()
    wl = torch.zeros(100, 72, device=DEV)                                 # 2 x 2 tiles of 64 x 64, both ragged
    pt.add(wl.view(100, 72, 1), 100, 72, 1)
    add(rnd(100, 72, seed=7), pack=pt.info[0], param=wl)
    wt = torch.zeros(100, 70, device=DEV)                                 # stored [c][n] (used as x @ P): N = 70, Cin = 100,
    pt.add(wt, 70, 100, 1, src_transposed=True)                           # 2 x 2 ragged tiles; the gradient is [c][n] too
    add(rnd(100, 70, seed=8), pack=pt.info[1], param=wt)
    for k, (N, Cin, taps, Cpad) in enumerate([(5, 3, 9, 8), (64, 20, 1, 32)]):
        g = rnd(N, Cin, taps, seed=10 + k)
        add(g, grad=gemm_layout(g, Cpad, 1e30), layout=(N, Cin, taps, Cpad))
    g = rnd(7, 33, seed=20)
    g[[2, 5]] = 0.0
    live = torch.ones(7, dtype=torch.uint8)
    live[[2, 5]] = 0
    add(g)
    tab = ops.AdamTable(params, [g.to(DEV) for g in grads], [1e-3] * len(params), layouts=layouts, packs=packs,
                        row_live={len(params) - 1: live.to(DEV)})
    return tab, logical


def test_sum_of_squares_over_a_synthetic_table():
    """norm to 1e-5 relative of the float64 value.  Derived, not measured: all terms are non-negative, so the relative error
    of the sum is at most (depth of additions + 1 rounding of the square) * 2^-24; the deepest path is a plain 8192-element
    block - 32 additions per thread, 6 butterfly steps, 3 additions of the wave sums = 41 - i.e. 42 * 2^-24 = 2.5e-6 on the sum,
    half of that on its square root; the partials are then added in double."""
    tab, logical = synthetic_table()
    want = math.sqrt(sum(float((g.double() ** 2).sum()) for g in logical))
    out = tab.grad_norm()
    got = out.cpu()
    print("norm", float(got[0]), "float64", want, "rel", abs(float(got[0]) - want) / want)
    assert abs(float(got[0]) - want) / want <= 1e-5
    assert float(got[1]) == 1.0
    first = got.numpy().tobytes()
    for scale, max_norm in ((0.5, 0.3 * want), (0.5, 2.0 * want), (1.0, want * (1 + 1e-3)), (1.0, 0.999 * want)):
        got = tab.grad_norm(grad_scale=scale, max_norm=max_norm).cpu()
        norm = float(got[0])
        assert abs(norm - scale * want) / (scale * want) <= 1e-5
        expect = max(1.0, (norm + 1e-6) / max_norm)
        print("grad_scale", scale, "max_norm", max_norm, "divisor", float(got[1]), "expected", expect)
        if scale * want < max_norm:
            assert float(got[1]) == 1.0                                   # not clipping: exactly 1
        else:
            assert float(got[1]) > 1.0
        assert abs(float(got[1]) - expect) / expect <= 1e-6
    again = tab.grad_norm().cpu()
    assert again.numpy().tobytes() == first, "the 8 output bytes differ from run to run"
    with pytest.raises(ValueError):
        tab.grad_norm(max_norm=0.0)
    lib = hip.load()
    assert lib.cris_grad_clip_finalize(tab._partials.data_ptr(), 1, 1.0, -1.0, out.data_ptr(), None) != 0
    assert b"max_norm" in lib.cris_last_error()


def test_each_tensor_sums_over_its_own_blocks():
    """the global norm is dominated by the tensor scaled by 1e3, so a wrong index in one of the small tensors' paths (packed
    tiles, transposed tiles, GEMM layout, row_live) would hide under its tolerance: here the partials of every tensor's own
    block range, added in double, equal that tensor's float64 sum of squares to 1e-5 (the bound derived above holds per
    block, hence per tensor).  Also the edge of the C entry point: no partials at all give norm 0 and divisor 1."""
    tab, logical = synthetic_table()
    out = tab.grad_norm()
    partials = tab._partials.cpu().double()
    off = 0
    for taps in (9, 1):                                                   # the order grad_norm() lays the two tables out in
        t, idx = tab.tables[taps], tab.index[taps]
        for j, i in enumerate(idx):
            lo = t.arr[j].block_start
            hi = t.arr[j + 1].block_start if j + 1 < len(idx) else t.total_blocks
            got, want = float(partials[off + lo:off + hi].sum()), float((logical[i].double() ** 2).sum())
            print("tensor", i, tuple(logical[i].shape), "blocks", hi - lo, "sum", got, "float64", want)
            assert hi > lo and abs(got - want) / want <= 1e-5, (i, got, want)
        off += t.total_blocks if t.n else 0
    assert off == tab._partials.numel()
    hip.call("cris_grad_clip_finalize", None, 0, 1.0, 2.0, out.data_ptr(), None)
    assert out.cpu().tolist() == [0.0, 1.0]


def test_clipped_update_equals_torch():
    """step 1 unclipped (m, v non-zero: the first Adam step is nearly invariant to the gradient's scale), step 2 with fresh
    gradients clipped to a quarter of their norm: parameters equal torch.optim.Adam after clip_grad_norm_ on fp32 CPU clones
    to the tolerance of the existing Adam tests, and differ from the unclipped update by more than it."""
    E = hip.load().cris_adam_block_elems()
    N3, C3, Cp3 = 70, 66, 72
    shapes = [(1,), (E - 1,), (E,), (E + 1,), (3 * E + 7,), (N3, C3, 3, 3)]
    init = [rnd(*s, seed=30 + k) for k, s in enumerate(shapes)]
    step_grads = [[rnd(*s, seed=40 + 10 * t + k) for k, s in enumerate(shapes)] for t in range(2)]

    def device_run(clip):
        params = [p.clone().to(DEV) for p in init]
        pt = ops.PackTable()
        pt.add(params[-1].view(N3, C3, 9), N3, C3, 9, Cpad=Cp3)
        grads = [torch.zeros(p.numel(), device=DEV) for p in params[:-1]] + [torch.zeros(N3, 9 * Cp3, device=DEV)]
        tab = ops.AdamTable(params, grads, [1e-3] * len(params), layouts=[None] * 5 + [(N3, C3, 9, Cp3)], packs=[None] * 5 + pt.info)
        for t in range(2):
            for dg, g in zip(grads[:-1], step_grads[t][:-1]):
                dg.copy_(g)
            grads[-1].copy_(gemm_layout(step_grads[t][-1].reshape(N3, C3, 9), Cp3, 1e30))
            divisor = None
            if clip and t == 1:
                divisor = tab.grad_norm(max_norm=max_norm)[1:2]
            tab.step(loss_scale_dev=divisor)
        return params

    norm2 = math.sqrt(sum(float((g.double() ** 2).sum()) for g in step_grads[1]))
    max_norm = 0.25 * norm2
    ref = [torch.nn.Parameter(p.clone()) for p in init]
    opt = torch.optim.Adam(ref, lr=1e-3)
    for t in range(2):
        for rp, g in zip(ref, step_grads[t]):
            rp.grad = g.clone()
        if t == 1:
            torch.nn.utils.clip_grad_norm_(ref, max_norm)
        opt.step()
    clipped, unclipped = device_run(True), device_run(False)
    for k, (c, u, rp) in enumerate(zip(clipped, unclipped, ref)):
        e, d = relerr(c, rp.data), relerr(c, u)
        print("tensor", k, tuple(rp.shape), "clipped vs torch", e, "clipped vs unclipped", d)
        assert math.isfinite(e) and e <= ADAM_TOL, (k, e)
        assert d > ADAM_TOL, (k, d)


# ---- the trainer: the suite's smallest NativeTrainer configuration (tiny spec, batch 2, 64 x 64) --------------------
def run_trainer(steps, launch="eager", changes=None, **kw):
    """`steps` train steps from the same state and batches; changes: {step index: max_norm set before that step}.
    Returns (trainer, losses, grad norms read from the trainer (or None), float64 norms of engine.G, parameters)."""
    tr, head = make_trainer(launch=launch, **kw)
    losses, norms, norms64 = [], [], []
    for t in range(steps):
        if changes and t in changes:
            tr.set_max_norm(changes[t])
        loss, _ = tr.train_step(*batch(2, head, t))
        losses.append(float(loss))
        if tr.max_norm > 0 or tr.track_grad_norm:
            norms.append(float(tr.grad_norm))
        g = tr.engine.grads_param_layout()
        norms64.append(math.sqrt(sum(float((g[n].double() ** 2).sum()) for n in tr.names)))
    torch.cuda.synchronize()
    return tr, losses, norms, norms64, {k: v.clone() for k, v in tr.engine.P.items()}


@pytest.fixture(scope="module")
def unclipped():
    """three unclipped steps with the norm tracked; max_norm of the clipping tests = half the norm at step 2"""
    tr, losses, norms, norms64, params = run_trainer(3, track_grad_norm=True)
    assert "backbone.logit_scale" not in tr.names
    return dict(losses=losses, norms=norms, norms64=norms64, params=params, max_norm=0.5 * norms[1])


def test_not_clipping_is_free_of_side_effects(unclipped):
    """max_norm far above the norm: the update divides by exactly 1.0 - parameters and losses bit-identical to max_norm=0;
    so are those of a run that only tracks the norm"""
    tr0, l0, _, _, p0 = run_trainer(3, max_norm=0.0)
    tr, l1, n1, _, p1 = run_trainer(3, max_norm=1e9)
    assert float(tr.adam.gnorm[1]) == 1.0 and all(n > 0 for n in n1)
    assert l0 == l1, (l0, l1)
    assert all(torch.equal(p0[k], p1[k]) for k in p0)
    assert l0 == unclipped["losses"] and all(torch.equal(p0[k], unclipped["params"][k]) for k in p0)
    with pytest.raises(RuntimeError):
        tr0.grad_norm                                                     # not computed: not readable


def test_trainer_clips_and_reports(unclipped):
    for got, want in zip(unclipped["norms"], unclipped["norms64"]):
        print("tracked", got, "float64", want)
        assert abs(got - want) / want <= 1e-5
    tr, losses, norms, norms64, params = run_trainer(3, max_norm=unclipped["max_norm"])
    for got, want in zip(norms, norms64):
        print("clipping", got, "float64", want, "max_norm", unclipped["max_norm"])
        assert abs(got - want) / want <= 1e-5
    assert any(n > unclipped["max_norm"] for n in norms[:2])              # step 2 at the latest was clipped
    assert any(not torch.equal(params[k], unclipped["params"][k]) for k in params)
    assert all(bool(torch.isfinite(p).all()) for p in params.values())


def test_norm_of_the_rank_averaged_gradient(unclipped):
    """the multi-rank placement: the norm is taken AFTER the gradient all-reduce and with the update's 1/world, so it is that
    of the averaged gradient.  Two ranks with equal batches average to the one-rank gradient (x 2, x 0.5: exact), so norms,
    losses and parameters follow the one-rank clipped run; a norm taken before the exchange, or without 1/world, would be
    half or twice it.  (Scaling by 2 is exact except where a square underflows: norms to 1e-6, not bitwise.)"""
    _, l1, n1, _, p1 = run_trainer(3, max_norm=unclipped["max_norm"])
    tr, l2, n2, _, p2 = run_trainer(3, max_norm=unclipped["max_norm"], comm=TwoEqualRanks())
    assert tr.comm.world == 2 and tr.grad_exchange == "rccl"             # the all-reduce branch of the step was taken
    for a, b in zip(n1, n2):
        print("one rank", a, "two equal ranks", b)
        assert abs(a - b) / a <= 1e-6
    assert l1 == pytest.approx(l2, rel=1e-6)
    for k in p1:
        assert relerr(p2[k], p1[k]) <= ADAM_TOL, k


@pytest.mark.parametrize("launch", ["graph", "cmdlist"])
def test_replay_recomputes_the_divisor(unclipped, launch):
    """captured graph / recorded command list against the eager schedule: bit-identical, and the norm moves from step to step
    (it is computed by the replayed launches, not baked in at capture)"""
    _, le, ne, _, pe = run_trainer(5, launch="eager", max_norm=unclipped["max_norm"])
    tr, lr, nr, _, pr = run_trainer(5, launch=launch, max_norm=unclipped["max_norm"])
    assert tr.launch == launch and (tr._graph is not None or tr._cmds is not None), tr.graph_error
    assert le == lr, (le, lr)
    assert ne == nr, (ne, nr)
    assert all(torch.equal(pe[k], pr[k]) for k in pe)
    assert len(set(nr[2:])) == len(nr[2:]), nr                            # steps 3-5 are replays


def test_arguments(unclipped):
    clip, head = arch.specs_by_name("tiny")
    with pytest.raises(ValueError):
        NativeTrainer(clip, head, arch.synthetic_state_dict(clip, head, 0), torch.device("cuda:0"), max_norm=-1)
    a, b = unclipped["max_norm"], 0.5 * unclipped["max_norm"]
    _, le, ne, _, pe = run_trainer(6, launch="eager", max_norm=a, changes={3: b})
    clip_tr, _ = make_trainer(launch="graph", max_norm=a)
    losses = []
    for t in range(6):
        if t == 3:
            assert clip_tr._graph is not None, clip_tr.graph_error
            with pytest.raises(ValueError):
                clip_tr.set_max_norm(-2.0)
            clip_tr.set_max_norm(b)
            assert clip_tr._graph is None and clip_tr.max_norm == b      # dropped: the threshold is a launch argument
        losses.append(float(clip_tr.train_step(*batch(2, head, t))[0]))
    torch.cuda.synchronize()
    assert clip_tr._graph is not None
    assert losses == le, (losses, le)
    assert all(torch.equal(pe[k], clip_tr.engine.P[k]) for k in pe)
