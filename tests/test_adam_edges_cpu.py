"""The checks of tests/test_adam_edges.py are neither vacuous nor too tight.  For every table of tests/adam_edge_cases.py the step
evaluated with plain torch fp32 (every operation rounded on its own) passes them, against the same float64 reference; the same
evaluation made wrong in one named way - a swapped index, a stale coefficient, a forgotten tile row - is refused by them in every
table the mistake applies to.  The layout statements are consistent with themselves, the case table sits on the block and tile
edges it claims, and ops.AdamTable refuses the one combination the kernel has no code for.  No GPU.

Worst error / bound of the fp32 evaluation over all tables (printed by test_fp32_evaluation_is_inside_the_bounds):
m' 0.156, v' 0.261, p' 0.145 (the coupled tables; without coupled decay m' 0.12, v' 0.16)."""
import pytest
import torch

import adam_edge_cases as A
from hip_ops_edge_cases import BF, F64, GUARD_BITS

_STATES = {}


def states_of(case):
    if case.name not in _STATES:
        _STATES[case.name] = [A.state(case, k) for k in range(len(case.tensors))]
    return _STATES[case.name]


_WORST = {}


@pytest.mark.parametrize("case", A.CASES, ids=repr)
def test_fp32_evaluation_is_inside_the_bounds(case):
    st = states_of(case)
    report = {}
    A.check(case, st, A.emulate(case, st), report)
    for key, r in report.items():
        _WORST[key] = max(_WORST.get(key, 0.0), r)
    print("%s: worst error / bound of the fp32 evaluation: %s; over the tables so far: %s" % (
        case.name, " ".join("%s' %.3f" % kv for kv in sorted(report.items())), " ".join("%s' %.3f" % kv for kv in sorted(_WORST.items()))))
    assert case.skip or all(0 < r <= 1 for r in report.values()), report


@pytest.mark.parametrize("case", A.CASES, ids=repr)
def test_the_float64_evaluation_is_the_reference(case):
    """the emulation at float64, rounded to fp32, is within one rounding of the reference: half an fp32 ulp, far inside 2^-20 S"""
    st = states_of(case)
    report = {}
    A.check(case, st, A.emulate(case, st, dt=F64), report)
    assert all(r <= 2.0 ** -3 for r in report.values()), report


_MUTANTS = [(m, c) for m in A.MUTATIONS for c in A.CASES if A.applies(m, c)]


@pytest.mark.parametrize("mutate,case", _MUTANTS, ids=["%s-%s" % mc for mc in _MUTANTS])
def test_a_wrong_implementation_is_refused(mutate, case):
    st = states_of(case)
    with pytest.raises(AssertionError) as e:
        A.check(case, st, A.emulate(case, st, mutate=mutate))
    print("%s in %s: %s" % (mutate, case.name, str(e.value)[:300]))
    assert str(e.value).startswith(case.name + "/"), "the message names the case and the tensor"


def test_every_mutation_applies_somewhere():
    for m in A.MUTATIONS:
        assert sum(A.applies(m, c) for c in A.CASES) >= 2, m
    assert all(A.applies(m, c) for m in ("bc_prev", "no_eps", "neighbour_lr") for c in A.CASES if not c.skip)


def test_one_element_off_is_refused():
    """an m' or v' 2^-18 S off, a p' 2^-17 S off, and one element that took its neighbour's gradient: each is refused, with the
    element's coordinates"""
    case = next(c for c in A.CASES if c.name == "pack9")
    st = states_of(case)
    k = next(i for i, t in enumerate(case.tensors) if t.name == "w9-33x65")
    ref = A.reference(case, k, st[k])
    i = 9 * 65 * 32 + 9 * 64 + 4                     # n = 32, c = 64, tap = 4: the corner tile
    assert ref["Sm"][i] > 0
    for key, S, off in (("m", "Sm", 2.0 ** -18), ("v", "Sv", 2.0 ** -18), ("p", "Sp", 2.0 ** -17)):
        res = A.emulate(case, st)
        res[k][key][i] = float(ref[key][i] + off * ref[S][i])
        with pytest.raises(AssertionError, match=r"n=32, c=64, tap=4"):
            A.check(case, st, res)
    moved = [dict(s) for s in st]
    gb = st[k]["gbuf"].clone()
    gi = A.gemm_index(case.tensors[k])
    gb[gi[i]] = gb[gi[i] + 1]                        # channel 65 of the same tap: padding (NaN) - or any other value
    moved[k]["gbuf"] = gb
    with pytest.raises(AssertionError, match=r"n=32, c=64, tap=4"):
        A.check(case, st, A.emulate(case, moved))


def test_a_stray_pack_write_is_refused_by_name():
    case = next(c for c in A.CASES if c.name == "pack1")
    st = states_of(case)
    k = next(i for i, t in enumerate(case.tensors) if t.name == "w1-63x64-Fonly")
    t = case.tensors[k]
    for row in (0, A.PRE - 1, A.PRE + t.N, A.PRE + t.N + A.POST - 1):  # the rows in front of the pack and behind it
        res = A.emulate(case, st)
        res[k]["F"][row, 7] = 0
        with pytest.raises(AssertionError, match="pack1/w1-63x64-Fonly pack F: 1 guard elements"):
            A.check(case, st, res)
    # padding columns Cin..Cpad and the stride tail
    for name, which, col in (("w1-65x65-gemmgrad", "F", 65), ("w1-65x65-gemmgrad", "D", 65)):
        k = next(i for i, t in enumerate(case.tensors) if t.name == name)
        res = A.emulate(case, st)
        res[k][which][A.PRE, col] = 0
        with pytest.raises(AssertionError, match="guard elements"):
            A.check(case, st, res)
    case = next(c for c in A.CASES if c.name == "pack9")
    st = states_of(case)
    k = next(i for i, t in enumerate(case.tensors) if t.name == "w9-32x64-ld+64")
    res = A.emulate(case, st)
    res[k]["D"][A.PRE + 3, 9 * 32 + 5] = 0           # the stride tail
    with pytest.raises(AssertionError, match="pack D: 1 guard elements"):
        A.check(case, st, res)


def test_layout_statements_round_trip():
    """place, then read back: every stored element once, inside the pack's rows, padding and tails untouched"""
    for t in A.PACK9 + A.PACK1:
        vals = (torch.arange(t.numel) % 251 + 1).float()              # exact in bf16, never the guard pattern
        for which, wanted in (("F", t.want_F), ("D", t.want_D)):
            rows, ld, idx = A.pack_geometry(t, which)
            assert idx.unique().numel() == t.numel and int(idx.min()) >= 0 and int(idx.max()) < rows * ld, (t.name, which)
            img, live = A.place(t, which, vals)
            assert int(live.sum()) == t.numel and not bool(live[:A.PRE].any()) and not bool(live[A.PRE + rows:].any())
            assert torch.equal(A.read_back(t, which, img).view(BF).float(), vals)
            assert bool((img[~live] == GUARD_BITS[BF]).all())
            kpad = t.Cpad if which == "F" else t.Npad
            klive = t.Cin if which == "F" else t.N
            cols = torch.arange(ld)
            dead_col = (cols >= t.taps * kpad) | (cols % kpad >= klive)
            assert not bool(live[:, dead_col].any()) and bool(live[A.PRE:A.PRE + rows][:, ~dead_col].all()), (t.name, which)
    for t in A.GEMM + [x for x in A.PACK9 + A.PACK1 if x.grad_gemm]:
        gi = A.gemm_index(t)
        assert gi.unique().numel() == t.numel and int(gi.max()) < t.grad_numel
        buf = torch.full((t.grad_numel,), A.NAN)
        vals = torch.arange(t.numel).float()
        buf[gi] = vals
        assert torch.equal(buf[gi], vals)
        assert torch.equal(torch.isnan(buf.view(t.N, t.taps, t.Cpad)), (torch.arange(t.Cpad) >= t.Cin).expand(t.N, t.taps, t.Cpad))
    # against a loop over the issue's sentences, on one small shape
    t = A.T("w", "pack", N=3, Cin=2, taps=9, Cpad=8, Npad=8, ld_extra=8)
    Fi, Di, Gi = A.F_index(t).view(3, 2, 9), A.D_index(t).view(3, 2, 9), A.gemm_index(t).view(3, 2, 9)
    for n in range(3):
        for c in range(2):
            for tap in range(9):
                assert Fi[n, c, tap] == n * (72 + 8) + tap * 8 + c and Di[n, c, tap] == c * (72 + 8) + (8 - tap) * 8 + n
                assert Gi[n, c, tap] == (n * 9 + tap) * 8 + c
    tt = A.T("wt", "pack", N=3, Cin=2, taps=1, transposed=True)       # stored [c][n]
    n, c, tap = A.nct(tt)
    assert n.tolist() == [0, 1, 2, 0, 1, 2] and c.tolist() == [0, 0, 0, 1, 1, 1] and not tap.any()


def test_case_table_sits_on_the_edges():
    from cris.pytorch_amd import hip
    E = hip.load().cris_adam_block_elems()
    assert E == A.BLOCK_ELEMS
    assert [t.numel for t in A.PLAIN] == [1, 255, 256, 257, E - 1, E, E + 1, 2 * E + 3]
    assert [t.layout for t in A.GEMM] == [(5, 3, 9, 8), (3, 5, 1, 8), (24, 20, 9, 24), (16, 60, 9, 64)]
    assert A.GEMM[3].numel > E and E % (60 * 9) != 0                   # a block edge inside a row
    assert {(t.N, t.Cin) for t in A.PACK9} == {(1, 1), (31, 63), (32, 64), (33, 65), (70, 66)}
    assert {(t.N, t.Cin) for t in A.PACK1} == {(1, 1), (63, 64), (64, 63), (65, 65), (130, 70)}
    for tab, taps in ((A.PACK9, 9), (A.PACK1, 1)):
        TN = A.tile_rows(taps)
        assert {t.N - TN for t in tab} >= {-1, 0, 1} and {t.Cin - A.AP_T for t in tab} >= {-1, 0, 1}
        assert any(not t.want_D for t in tab) and any(not t.want_F for t in tab)
        assert all(t.numel <= 3 * E or (t.N, t.Cin, t.taps) == (70, 66, 9) for t in tab)
    assert any(t.Cpad > A.pad8(t.Cin) and t.Npad > A.pad8(t.N) for t in A.PACK9) and any(t.ld_extra == 64 for t in A.PACK9)
    assert sum(t.transposed for t in A.PACK1) >= 5 and any(t.grad_gemm and t.Cpad > t.Cin for t in A.PACK1)
    assert [(t.N, t.Cin) for t in A.ROWS] == [(400, 48), (7, 33), (300, 1)]
    for t in A.ROWS:
        assert 0 in t.dead and t.N - 1 in t.dead
    assert 170 * 48 < E < 171 * 48 and {170, 171} <= set(A.ROWS[0].dead)
    assert len(A.LOOKUP257) == 257 and [t.numel for t in A.LOOKUP257[:6]] == [1, 2, 3, 4, 5, 1] and len(A.LOOKUP3) == 3
    assert {t.kind for t in A.SUBSET} == {"plain", "gemm", "pack", "rows"} and any(t.transposed for t in A.SUBSET)
    assert {t.taps for t in A.SUBSET if t.kind == "pack"} == {1, 9}
    for c in A.CASES:
        assert all(a != b for a, b in zip(c.lrs, c.lrs[1:])), c.name
        if c.mode:
            assert all(a != b for a, b in zip(c.decays, c.decays[1:])) and 0.0 in c.decays, c.name
    by_name = {c.name: c for c in A.CASES}
    assert by_name["subset-decoupled"].marks_honoured(5) and not by_name["subset-decoupled"].marks_honoured(6)
    assert not by_name["subset-wd0.5"].marks_honoured(5) and by_name["rows"].marks_honoured(0)
    assert sorted(c.t for c in A.CASES if c.step_dev) == [1, 7, 1000]
    assert len(A.UNPACK_CASES["one"]) == 1 and len(A.UNPACK_CASES["lookup257"]) == 257


@pytest.mark.parametrize("case", A.CASES, ids=repr)
def test_states_hold_what_the_cases_promise(case):
    """exact zeros of every kind, NaN padding and dead-row gradients, and no value near the subnormal range - inputs, g~, and
    every non-zero intermediate of the reference"""
    tiny = 2.0 ** -100
    kinds = set()
    for k, t in enumerate(case.tensors):
        st = states_of(case)[k]
        assert bool((st["v"] >= 0).all())
        for key in ("p", "m", "v"):
            x = st[key]
            assert bool(torch.isfinite(x).all()) and not bool(((x != 0) & (x.abs() < 1e-13)).any())
        g = st["g"]
        assert bool(torch.isnan(g[st["dead"]]).all()) and bool(torch.isfinite(g[~st["dead"]]).all())
        assert int(torch.isnan(st["gbuf"]).sum()) == t.grad_numel - t.numel + int(st["dead"].sum())
        if case.gmag > 1:
            assert float(torch.nan_to_num(g).abs().max()) > 5e3 and float(torch.nan_to_num(g).abs().max()) <= 1e4
        ref = A.step_fn(st["p"], torch.nan_to_num(g), st["m"], st["v"], A.coefs(case, k), F64)
        assert not bool(((ref["gt"] != 0) & (ref["gt"].abs() < 1e-15)).any())
        for x in (ref["m"], ref["v"], ref["p"] - ref["pk"], (1 - A.B2) * ref["gt"] ** 2):
            assert not bool(((x != 0) & (x.abs() < tiny)).any())
        if case.coupled(k):
            assert bool((ref["gt"].abs() >= (1 - 1e-12) * (torch.nan_to_num(g).abs() * case.gscale / (case.loss_scale or 1.0))).all())
        z = lambda key: st[key] == 0                                  # noqa: E731
        kinds |= {name for name, m in (("still", z("g") & z("m") & z("v") & ~z("p")), ("all", z("g") & z("m") & z("v") & z("p")),
                                       ("p", z("p") & ~z("m")), ("v", z("v") & ~z("m"))) if bool(m.any())}
    assert kinds == {"still", "all", "p", "v"} or sum(t.numel for t in case.tensors) < 16, kinds


def test_adam_table_refuses_a_transposed_pack_with_a_gemm_layout_gradient():
    """adam_pack_tile's transposed branch reads the gradient where it reads the parameter; the engine never builds the
    combination (its only transposed weight is two-dimensional: no GEMM layout), and AdamTable says so"""
    from cris.pytorch_amd import ops
    N, Cin, Cpad = 8, 5, 8
    p, g = torch.zeros(Cin, N), torch.zeros(N, Cpad)
    dstF, dstD = torch.zeros(N, Cpad, dtype=BF), torch.zeros(Cin, 8, dtype=BF)
    ok = ops.AdamTable([p], [torch.zeros(Cin, N)], [1e-3], layouts=[None], packs=[(dstF, dstD, N, Cin, 1, Cpad, 8, True)])
    assert ok.tables[1].arr[0].transposed == 1 and ok.tables[1].arr[0].taps == 0
    with pytest.raises(AssertionError, match="transposed"):
        ops.AdamTable([p], [g], [1e-3], layouts=[(N, Cin, 1, Cpad)], packs=[(dstF, dstD, N, Cin, 1, Cpad, 8, True)])
    # a packed weight's gradient layout and its F pack share one Cpad: the descriptor has one field for both
    with pytest.raises(AssertionError, match="Cpad"):
        ops.AdamTable([torch.zeros(N, Cin)], [torch.zeros(N, 16)], [1e-3], layouts=[(N, Cin, 1, 16)],
                      packs=[(dstF, dstD, N, Cin, 1, Cpad, 8, False)])
