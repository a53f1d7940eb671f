"""The bounds and the case tables of tests/test_attn_edges.py, settled without a GPU: an fp32 emulation of the attention kernels
(tests/attn_edge_cases.py: online softmax in 32-key steps, bf16 roundings where the kernels round) stays within 0.75 of every
per-element bound in every case; the same emulation with any one of seven plausible kernel errors switched on breaks a bound in
a named case; every case meets the condition of the bound's reserve (e <= 2^-9), stays inside the launchers' argument checks
and reaches the kernel (direct or LDS: cris_attn_plan) its row of the table is there for."""
import ctypes

import pytest
import torch

import attn_edge_cases as A

_IDS = [c.name for c in A.CASES]
_WORST = A.Worst()


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


@pytest.mark.parametrize("name", _IDS)
def test_case_meets_the_conditions_of_the_bound_and_reaches_its_kernel(name):
    A.check_case(A.BY_NAME[name])


@pytest.mark.parametrize("name", _IDS)
def test_fp32_emulation_is_inside_the_bound(name):
    r = A.reference(name)
    got = A.emulate(name)
    for output in ("O", "lse", "delta", "dQ", "dK", "dV"):
        x = A.check_output(r, output, got[output], "%s %s (emulation)" % (name, output))
        launcher = next(w for w in A.LAUNCHERS if output in A.OUTPUTS[w])
        _WORST.add(output, "lds" if r.case.plan[A.LAUNCHERS.index(launcher)] else "direct", x, name)
        assert x <= A.EMU_RATIO_LIMIT, "%s %s: a correct fp32 evaluation reaches %.3f of the bound: the derivation misses a term" % (name, output, x)
        for s in r.S.values():
            assert bool(torch.isfinite(s).all())


def test_zz_worst_ratios_of_the_emulation():
    """(runs after the parametrised test above: the table of its worst ratios)"""
    print("\nworst error / bound of the fp32 emulation, per output and kernel:\n" + _WORST.table())
    assert all(v[0] <= A.EMU_RATIO_LIMIT for v in _WORST.w.values())


@pytest.mark.parametrize("bug", A.BUGS)
def test_each_kernel_error_is_caught_in_its_named_cases(bug):
    for name, outputs in A.BUG_CASES[bug]:
        r = A.reference(name)
        got = A.emulate(name, bug)
        for output in outputs:
            with pytest.raises(AssertionError):
                A.check_output(r, output, got[output], "%s %s (error %s)" % (name, output, bug))


def test_tables_cover_what_they_are_for():
    C = A.CASES
    direct = [c for c in C if 1 not in c.plan]
    # direct kernels: the Lq x Lk grid, dropout with and without the split seed, causal, the four padding masks
    grid = {(c.Lq, c.Lk) for c in direct if c.p == 0 and not c.causal and c.mask is None and c.pattern == "randn"}
    assert {(a, b) for a in (1, 16, 17, 63, 65) for b in (1, 31, 32, 33, 65)} <= grid
    for split in (False, True):
        assert {(c.Lq, c.Lk) for c in direct if c.p == 0.5 and c.split_seed == split} == {(1, 1), (17, 33), (63, 31), (65, 65)}
    assert {c.Lq for c in C if c.causal and c.p == 0} == {1, 16, 17, 33, 77} and any(c.causal and c.p == 0.1 and c.Lq == 33 for c in C)
    assert all(c.Lq == c.Lk for c in C if c.causal)
    assert {c.Lq for c in C if c.mask == "pad4"} == {17, 70}
    t = A.key_tokens(A.BY_NAME["pad-q17"])
    assert [int((row != 0).sum()) for row in t] == [9, 20, 1, 0] and int(t[1, 3]) == int(t[1, 16]) == 0 and int(t[2, 0]) != 0
    # layouts: every LDS case sliced, a third of the direct ones at least
    assert all(c.layout == "sliced" for c in C if 1 in c.plan)
    assert 3 * sum(c.layout == "sliced" for c in A.DIRECT_CASES) >= len(A.DIRECT_CASES)
    assert all(c.Hn == 3 and c.B >= 2 for c in C)
    # LDS kernels: the lengths on either side of the threshold and of the 64- and 32-row tile edges
    fd = [c for c in C if c.plan[0] == 1 and c.plan[2] == 0 and c.pattern == "randn"]
    assert {(c.Lk, c.Lq, c.p) for c in fd} == {(k, q, p) for k in (384, 385, 416, 417, 448, 449) for q in (1, 70) for p in (0.0, 0.1)}
    kv = [c for c in C if c.plan == (0, 0, 1)]
    assert {(c.Lq, c.Lk, c.p) for c in kv} == {(q, k, p) for q in (384, 385, 417, 449) for k in (1, 17, 65) for p in (0.0, 0.1)}
    assert all((c.mask == "pad2") == (c.Lk == 17) for c in kv)
    assert any(c.plan == (1, 1, 1) and c.Lq == c.Lk == 385 and c.self_attn for c in C)
    assert any(c.Lk == A.LDS_MIN - 1 and c.plan == (0, 0, 0) for c in C) and any(c.Lq == A.LDS_MIN - 1 and c.mask == "pad2" and c.plan == (0, 0, 0) for c in C)
    assert {A.pad32(c.Lk) % 64 for c in fd} == {0, 32} and {A.pad32(c.Lq) % 64 for c in kv} == {0, 32}
    # the XCD block remap: per LDS kernel a grid below 8 blocks, and totals = 1, 7 and 0 (mod 8)
    for w, launcher in enumerate(A.LAUNCHERS):
        totals = {c.grid_total(launcher) for c in C if c.plan[w] == 1}
        assert any(t < 8 for t in totals) and {1, 7, 0} <= {t % 8 for t in totals}, (launcher, sorted(totals))
    # structured scores on a direct and an LDS case; one deterministic case per kernel
    assert {(c.pattern, c.Lk, c.plan[0]) for c in C if c.pattern != "randn"} == {("rise", 65, 0), ("fall", 65, 0), ("rise", 449, 1), ("fall", 449, 1)}
    assert {(w, k) for _, w, k in A.DETERMINISM} == {(w, k) for w in A.LAUNCHERS for k in (0, 1)}
    assert all(A.BY_NAME[n].plan[A.LAUNCHERS.index(w)] == k for n, w, k in A.DETERMINISM)
    assert set(A.BUG_CASES) == set(A.BUGS) and all(n in A.BY_NAME for v in A.BUG_CASES.values() for n, _ in v)
    assert max(c.B * c.Hn * c.Lq * c.Lk for c in C) < 1 << 22          # tiny: the largest is 449 x 70 x 15 (batch, head) pairs


def test_structured_scores_move_the_maximum_as_intended():
    for name, lds in (("rise-k65", False), ("lds-rise-k449", True), ("fall-k65", False), ("lds-fall-k449", True)):
        r = A.reference(name)
        c = r.case
        s = (A.heads(r.q.double(), c.B, c.Lq, c.Hn) @ A.heads(r.k.double(), c.B, c.Lk, c.Hn).transpose(-1, -2)) * A.SCALE
        span = float((s.max(-1).values - s.min(-1).values).mean())
        assert 25 < span < 35, (name, span)
        Lkp = A.pad32(c.Lk)
        sp = torch.nn.functional.pad(s, (0, Lkp - c.Lk), value=-float("inf")).view(c.B, c.Hn, c.Lq, Lkp // 32, 32).max(-1).values
        run = torch.cummax(sp, -1).values
        moved = run[..., 1:] > run[..., :-1]
        if c.pattern == "rise":
            # the running maximum moves at every whole 32-key step (the one-key tail of Lk = 449 may tie: bf16 spacing of K)
            assert bool(moved[..., :c.Lk // 32 - 1].all()) and c.Lk // 32 >= 2, name
        else:
            assert not bool(moved.any()), name       # ... at none after the first: no rescale


def test_plan_rejects_an_unknown_launcher():
    from cris.pytorch_amd import hip
    lib = hip.load()
    o = A.build_operands(A.reference("d-q1-k1"), "cpu")
    assert lib.cris_attn_plan(ctypes.byref(o.p), 3) == -1 and b"cris_attn_plan" in lib.cris_last_error()
    assert lib.cris_attn_plan(ctypes.byref(o.p), -1) == -1


def test_plan_follows_the_launchers_predicates():
    """the threshold, the masks and the Lq_pad term of the key side, on one parameter block"""
    from cris.pytorch_amd import hip
    lib = hip.load()
    o = A.build_operands(A.reference("lds-self-385"), "cpu")
    p = o.p
    plan = lambda: tuple(lib.cris_attn_plan(ctypes.byref(p), w) for w in range(3))          # noqa: E731
    assert plan() == (1, 1, 1)
    p.causal = 1
    assert plan() == (0, 0, 0)
    p.causal = 0
    toks = torch.ones(2, 385, dtype=torch.int64)
    p.key_tokens = toks.data_ptr()
    assert plan() == (0, 0, 1)                       # a key-padding mask: the key side only
    p.key_tokens = None
    p.Lq_pad = 420                                   # a multiple of 4 (accepted), not of 8: direct key side
    assert plan() == (1, 1, 0)
    p.Lq_pad = 416
    p.Lk = 383
    assert plan() == (0, 0, 1)                       # fwd and dq loop over the keys, dkv over the queries
