"""The checks of tests/test_stats_edges.py are neither vacuous nor too tight.  For every case of tests/stats_edge_cases.py two fp32
emulations pass them against the same float64 reference - one that follows the kernel's summation structure (lanes, register
entries, levels, fused multiply-adds), one plain sequential with every operation rounded on its own - and the first, made wrong
in one named way (a dropped K tail, a clamped row added, a part counted in two slices, ...), is refused at the cases named for it.
The case tables sit on the edges they claim: the dispatch constants stated in the cases file are compared with the `#define`s and
index expressions of the .hip sources, so a retune makes these tests fail, not silently miss the edges.  No GPU.

Worst error / bound of the structure-following emulation: printed by test_zz_worst_error_over_bound.  The
sequential one comes closest on the mean of the 4097-part lists (0.90): its chain is 4097 roundings long where the bound allows
for the 39 of the kernel's tree, and it stays inside only because roundings do not all point the same way."""
import os
import re

import pytest
import torch

import stats_edge_cases as E

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "cris", "pytorch_amd", "csrc")
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "cris_hip.h")
_WORST = {"struct": {}, "seq": {}}


def emulator(group, kind, mutate=None):
    return lambda c, sl: E.GROUPS[group].emulate(c, sl, kind, mutate)


@pytest.mark.parametrize("kind", ["struct", "seq"])
@pytest.mark.parametrize("group", list(E.GROUPS))
def test_fp32_emulations_are_inside_the_bounds(group, kind):
    for c in E.GROUPS[group].cases:
        rep = {}
        E.run(group, c, "cpu", emulator(group, kind), rep)
        assert all(r < 1 for r in rep.values()), (c.id, rep)
        for k, r in rep.items():
            _WORST[kind][k] = max(_WORST[kind].get(k, 0.0), r)


def _some(cases, n=12):
    """at most n of the cases, evenly spaced, first and last included"""
    if len(cases) <= n:
        return cases
    return [cases[round(i * (len(cases) - 1) / (n - 1))] for i in range(n)]


_MUTANTS = [(g.name, m) for g in E.GROUPS.values() for m in g.mutants if any(g.mutants[m](c) for c in g.cases)]


@pytest.mark.parametrize("group,mutate", _MUTANTS, ids=["%s-%s" % gm for gm in _MUTANTS])
def test_a_wrong_emulation_is_refused(group, mutate):
    g = E.GROUPS[group]
    cases = [c for c in g.cases if g.mutants[mutate](c)]
    assert cases
    for c in _some(cases):
        with pytest.raises(AssertionError) as e:
            E.run(group, c, "cpu", emulator(group, "struct", mutate))
        assert c.id in str(e.value), "the message names the case"


def test_every_listed_mutation_is_exercised():
    have = {m for _, m in _MUTANTS}
    assert have == {"ktail_dropped", "clamped_row_added", "col_N_stored", "rows_ge8_dropped", "accumulate_ignores_old", "bias_per_kgroup",
                    "last_max_wins", "relu_mask_ge", "apply_divides_by_M", "last_as_full", "drop_8PL_minus_1", "slice_boundary_double",
                    "slice_entries_beyond_64_dropped", "unbiased_omitted", "unbiased_at_count_1", "var_over_count_local",
                    "channel_C_written", "table_search_off_by_one", "parts_tail_dropped"}, have
    g = E.GROUPS["bn_finalize"]
    # named cases: the register-file edge of either finalize kernel, the merge loop, the count-1 and the global forms
    assert {c.nparts for c in g.cases if g.mutants["drop_8PL_minus_1"](c)} == {128, 512}
    assert {c.nparts for c in g.cases if g.mutants["slice_entries_beyond_64_dropped"](c)} == {4097}
    assert any(c.form == "global" for c in g.cases if g.mutants["var_over_count_local"](c))
    assert {c.K for c in E.LIN_CASES if E.LIN_MUTANTS["clamped_row_added"](c)} >= {1, 15, 17, 127, 129, 257, 2305}
    assert {c.K for c in E.LIN_CASES if E.LIN_MUTANTS["ktail_dropped"](c)} == {1, 63, 65, 129}


def test_one_part_of_4097_dropped_is_refused():
    """the reason the bound counts the depth of the tree and not the summands: an UNMARKED part (no offset) missing from the longest
    list moves the mean by 1 / 4097 of a part - inside nparts * 2^-24, far outside the derived bound"""
    c = next(x for x in E.BNF_CASES if x.nparts == 4097 and x.C == 40 and x.rpp == 32 and x.last == "one" and x.form == "plain")
    i = 2000
    assert i not in E.bnf_marked(c)

    def drop(case, sl):
        sl["psum"].data[i] = 0
        sl["pm2"].data[i] = 0
        E.bnf_emulate(case, sl)
        x = E.bnf_inputs(case)
        sl["psum"].data[i], sl["pm2"].data[i] = x["psum"][i], x["pm2"][i]

    with pytest.raises(AssertionError, match="mean"):
        E.run("bn_finalize", c, "cpu", drop)
    t_sum, t_m2 = E.bnf_depths(c)
    assert t_sum == 5 + 15 + 4 + 15 and t_sum < 4097 // 64


def test_rsqrt_margin():
    """float32 rsqrt of the emulation against float64, over the range var + eps takes: inside RSQRT_ULPS ulp"""
    v = torch.logspace(-5, 2, 20001, dtype=torch.float64).float()
    err = (torch.rsqrt(v).double() - v.double() ** -0.5).abs() / (v.double() ** -0.5)
    worst_ulp = float(err.max()) / 2.0 ** -23
    print("float32 rsqrt: worst %.3f ulp" % worst_ulp)
    assert worst_ulp <= 1.0 < E.RSQRT_ULPS


def _define(text, name):
    m = re.search(r"^#define\s+%s\s+(\d+)" % name, text, re.M)
    assert m, name
    return int(m.group(1))


def _kernel(text, name):
    """source text of one __global__ kernel: from its name to the next line that starts a definition"""
    i = text.index(name + "(")
    j = re.compile(r"^(extern \"C\"|__global__|template|static|#define)", re.M).search(text, i)
    return text[i:j.start()]


def test_dispatch_constants_match_the_sources():
    small, norm, head = (open(p).read() for p in (os.path.join(CSRC, "smallf32.hip"), os.path.join(CSRC, "norm.hip"), HEADER))
    assert _define(head, "CRIS_SMALL_MAX_ROWS") == E.SMALL_MAX_ROWS and _define(head, "CRIS_SUM_GROUP_MAX") == E.SUM_GROUP_MAX
    assert (_define(small, "LC_COLS"), _define(small, "LC_KG")) == (E.LC_COLS, E.LC_KG)
    rows = _kernel(small, "linear_rows_kernel")
    assert "threadIdx.x & %d" % (E.LR_LANES - 1) in rows and "k += %d" % E.LR_LANES in rows
    assert "blockIdx.x * %d + (threadIdx.x >> 6)" % E.LR_COLS_PER_BLOCK in rows and "cris_cdiv(N, %d)" % E.LR_COLS_PER_BLOCK in small
    cols = _kernel(small, "linear_cols_kernel")
    assert "k0 += LC_KG * %d" % E.LC_INFLIGHT in cols and "float wv[%d]" % E.LC_INFLIGHT in cols
    for k in ("outer_sum_kernel", "colstats_f32_small_kernel", "bn_relu_f32_small_kernel", "eot_gather_ln_f32_kernel"):
        assert re.search(r"hipLaunchKernelGGL\(%s, [^;]*dim3\(%d\)" % (k, E.SMALL_BLOCK), small), k
    assert (_define(norm, "BN_WIDE_MIN"), _define(norm, "BN_MERGE_MIN"), _define(norm, "BN_MERGE_SLICES")) == (
        E.BN_WIDE_MIN, E.BN_MERGE_MIN, E.BN_MERGE_SLICES)
    fin, mrg, sg = _kernel(norm, "bn_finalize_kernel"), _kernel(norm, "bn_merge_kernel"), _kernel(norm, "sum_group_kernel")
    assert "float ps[%d], pq[%d]" % (E.BN_REGS, E.BN_REGS) in fin and "blockIdx.x * %d + cl" % E.BN_CH in fin
    assert "float ps0[%d], pq0[%d]" % (E.BN_MERGE_REGS, E.BN_MERGE_REGS) in mrg and "i0 = i_begin + pl + %d" % (16 * E.BN_MERGE_REGS) in mrg
    assert "nparts <= %d * 64" % E.BN_REGS in norm and "bn_finalize_kernel<64>" in norm and "bn_finalize_kernel<16>" in norm
    assert "sh[%d][%d]" % (E.SUM_PARTLANES, E.SUM_COLS) in sg and "i += %d" % E.SUM_PARTLANES in sg and "* %d + cl" % E.SUM_COLS in sg
    from cris.pytorch_amd import hip
    lib = hip.load()
    ns = (1, 128, 129, 512, 513, 2704, 4096, 4097)
    assert [lib.cris_bn_partials_rows(n) for n in ns] == [E.partials_rows(n) for n in ns] == [1, 128, 129, 512, 577, 2768, 4160, 4161]
    assert hip.SUM_GROUP_MAX == E.SUM_GROUP_MAX


def test_case_tables_sit_on_the_edges():
    # linear, W [N][K]: rows on either side of 8 and at the unroll limit; columns around the 4 of a block; K around the 64 lanes
    assert E.LIN_NK == dict(M=[1, 8, 9, 16], N=[1, 3, 4, 5, 9], K=[1, 63, 64, 65, 129])
    assert max(E.LIN_NK["M"]) == E.SMALL_MAX_ROWS and {k - E.LR_LANES for k in E.LIN_NK["K"]} >= {-1, 0, 1}
    assert {n - E.LR_COLS_PER_BLOCK for n in E.LIN_NK["N"]} >= {-1, 0, 1}
    # W [K][N]: columns around the 16 of a block, K around one k-group round (16) and one trip (128); 2305 = 18 trips + 1
    trip = E.LC_KG * E.LC_INFLIGHT
    assert {n - E.LC_COLS for n in E.LIN_KN["N"]} >= {-1, 0, 1} and 33 in E.LIN_KN["N"]
    assert {k - E.LC_KG for k in E.LIN_KN["K"]} >= {-1, 0, 1} and {k - trip for k in E.LIN_KN["K"]} >= {-1, 0, 1}
    assert 2305 == 18 * trip + 1 and 257 == 2 * trip + 1 and 2305 in E.LIN_KN["K"]
    assert len({E.LIN_PADS[k] for k in ("A", "W", "out")}) == 3 and min(E.LIN_PADS.values()) > 0
    assert len(E.LIN_CASES) == 4 * 5 * 5 * 4 + 3 * 5 * 9 * 2
    assert {(c.M, c.R, c.Cc) for c in E.OUTER_CASES} == {(M, R, Cc) for M in (1, 9, 16) for R in (1, 3) for Cc in (1, 255, 256, 257)}
    assert {c.C - E.SMALL_BLOCK for c in E.SBN_CASES} >= {-1, 0, 1}
    for k in ("colstats", "bn_relu", "bwd_reduce", "bwd_apply"):
        assert {(c.M, c.C) for c in E.SBN_CASES if c.group == k and not getattr(c, "grid", False)} == {(M, Cn) for M in E.SBN_M for Cn in E.SBN_C}
    assert {c.countx for c in E.SBN_CASES if c.group == "bwd_apply" and not getattr(c, "grid", False)} == {1, 3}
    # grid inputs: exact zeros, +-1 ulp and negative pre-activations in every grid case wide enough to hold the five column kinds
    for c in E.SBN_CASES:
        if getattr(c, "grid", False):
            x = E.sbn_inputs(c)
            pre = x["y"].double() * x["scale"].double() + x["shift"].double()
            assert bool((pre == 0).any()) and torch.equal(pre.float().double(), pre)
            if c.C >= 5:
                assert bool((pre == 2.0 ** -24).any()) and bool((pre == -2.0 ** -23).any()) and bool((pre < -0.1).any()) and bool((pre > 0.1).any())
            assert torch.equal(x["y"].to(torch.bfloat16).float(), x["y"]) and bool((torch.log2(x["scale"]) % 1 == 0).all())
    # end of text: position 0, L - 1, the maximal token twice, all equal
    for c in E.EOT_CASES:
        toks, idx = E.eot_tokens(c)
        for b in range(c.Bn):
            row = toks[b]
            assert int(idx[b]) == int((row == row.max()).nonzero()[0])
        pats = set(E.EOT_PATTERNS) if c.pat == "mixed" else {c.pat}
        if c.L > 2 and "twice" in pats:
            assert any(int((toks[b] == toks[b].max()).sum()) == 2 for b in range(c.Bn))
        if "last" in pats:
            assert any(int(idx[b]) == c.L - 1 for b in range(c.Bn))
    assert {(c.Bn, c.L, c.D) for c in E.EOT_CASES} == {(b, l, d) for b in (1, 16) for l in (1, 2, 17, 77) for d in (1, 255, 256, 257)}
    # BatchNorm merge: the three paths, their boundaries, the register-file edges and the loop of the first-level merge
    assert E.BNF_NPARTS == (1, 2, 16, 17, 127, 128, 129, 511, 512, 513, 4096, 4097)
    assert [E.bn_path(n) for n in (128, 129, 512, 513, 4096, 4097)] == [(16, 0, 0), (64, 0, 0), (64, 0, 0), (16, 9, 57), (16, 64, 64), (16, 65, 64)]
    assert 4097 - 63 * 65 == 2 and 65 > 16 * E.BN_MERGE_REGS == 64                  # the last slice holds 2 parts; the loop runs
    assert 8 * 16 == E.BN_WIDE_MIN and 8 * 64 == E.BN_MERGE_MIN                         # both finalize kernels are used up to a full register file
    plain = [c for c in E.BNF_CASES if c.form == "plain" and not hasattr(c, "countx") and not hasattr(c, "tag")]
    assert {(c.nparts, c.C, c.rpp, c.last) for c in plain} == {(n, Cn, r, l) for n in E.BNF_NPARTS for Cn in (1, 16, 17, 40) for r in (2, 32)
                                                                for l in ("full", "one")}
    for n in E.BNF_NPARTS:
        assert {c.mom for c in plain if c.nparts == n} == {None, 0.1, 1.0}, n
    c = next(x for x in plain if x.nparts == 4097)
    assert {0, 4096, 63, 64, 65, 63 * 65 - 1, 63 * 65} <= set(E.bnf_marked(c))          # ends, register edge, first and last slice boundary
    assert {0, 127} <= set(E.bnf_marked(next(x for x in plain if x.nparts == 128)))
    assert {127, 128} <= set(E.bnf_marked(next(x for x in plain if x.nparts == 129)))
    assert {511, 512, 8, 9} <= set(E.bnf_marked(next(x for x in plain if x.nparts == 513)))
    assert any(E.bnf_counts(c)[1] == 1 and c.mom is not None for c in E.BNF_CASES)
    assert {c.form for c in E.BNF_CASES} == {"plain", "merged", "global"}
    assert any(c.form == "merged" and c.C % 16 for c in E.BNF_CASES) and any(c.form == "global" and c.countx > 1 for c in E.BNF_CASES)
    assert max(E.partials_rows(c.nparts) * c.C for c in E.BNF_CASES) == 4161 * 40
    assert {c.C for c in E.SYNC_CASES} == {1, 255, 257}
    # sum tables: groups of 1, 2 and 64; ncol around the 64 columns of a block, nparts around the 4 part lanes; ld > ncol
    assert {len(c.tables) for c in E.SUM_CASES} == {1, 2, E.SUM_GROUP_MAX}
    assert {n - E.SUM_COLS for n in E.SUM_NCOL} >= {-1, 0, 1} and {p - E.SUM_PARTLANES for p in E.SUM_NPARTS} >= {-1, 0, 1}
    big = next(c for c in E.SUM_CASES if len(c.tables) == E.SUM_GROUP_MAX)
    assert {n for n, _ in big.tables} == set(E.SUM_NCOL) and {p for _, p in big.tables} == set(E.SUM_NPARTS) and E.SUM_LDPAD > 0


def test_the_merged_form_must_leave_the_coefficients_alone():
    c = next(x for x in E.BNF_CASES if x.form == "merged" and x.nparts == 17)

    def writes_scale(case, sl):
        E.bnf_emulate(case, sl)
        sl["scale"].data[0, 3] = 1.0

    with pytest.raises(AssertionError, match="scale: written by the merged form"):
        E.run("bn_finalize", c, "cpu", writes_scale)


def test_a_stray_write_and_a_touched_input_are_refused():
    c = E.OUTER_CASES[0]

    def stray(case, sl):
        E.outer_emulate(case, sl)
        sl["G"].full[0, 0] = 0

    def touched(case, sl):
        E.outer_emulate(case, sl)
        sl["X1"].full[0, 0] = 0

    with pytest.raises(AssertionError, match="guard elements overwritten"):
        E.run("outer", c, "cpu", stray)
    with pytest.raises(AssertionError, match="an input"):
        E.run("outer", c, "cpu", touched)
    c = next(x for x in E.BNF_CASES if x.nparts == 513)

    def behind(case, sl):
        E.bnf_emulate(case, sl)
        sl["psum"].full[2 + E.partials_rows(513), 0] = 0                 # the first row behind the table's declared rows

    with pytest.raises(AssertionError, match="psum: an input"):
        E.run("bn_finalize", c, "cpu", behind)


def test_zz_worst_error_over_bound():
    for k in sorted(_WORST["struct"]):
        print("worst error / bound of the emulation: %-24s structure %.3f  sequential %.3f" % (k, _WORST["struct"][k], _WORST["seq"].get(k, float("nan"))))
