"""The fp32 sentence-vector kernels (csrc/smallf32.hip), the BatchNorm statistics kernels (cris_bn_finalize with its three merge
paths, cris_bn_sync_pack / _unpack, cris_bn_eval_coeffs) and cris_sum_tables at their own edges, element by element.

Every launcher is called alone, on inputs the test wrote, in the guarded slabs of tests/stats_edge_cases.py: outputs in guard bits
that must survive, inputs (ld padding, rows behind a table, rows that are no end-of-text row) in NaN and bit-identical afterwards.
Every output element is held against float64 of the given inputs under the bound derived there from the kernel's longest chain
of roundings; copies, masks and grid inputs bit for bit.  tests/test_stats_edges_cpu.py holds the same checks against fp32
emulations and nineteen wrong ones without a GPU.

Worst error / bound on an MI355X and of the structure-following emulation: see DESIGN.md section 6 (printed by the last test)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from cris.pytorch_amd import hip, ops  # noqa: E402
import stats_edge_cases as E  # noqa: E402
from hip_ops_edge_cases import bits_equal  # noqa: E402

DEV = "cuda"
_WORST = {}


def P(s):
    return None if s is None else s.data.data_ptr()


def launch(c, sl):
    g, S = c.group, ops._stream()
    if g in ("linear_nk", "linear_kn"):
        hip.call("cris_linear_f32_small", P(sl["A"]), sl["A"].ld, P(sl["W"]), sl["W"].ld, int(g == "linear_kn"), P(sl.get("bias")), c.M, c.N, c.K,
                 P(sl["out"]), sl["out"].ld, int(c.acc), S)
    elif g == "outer":
        hip.call("cris_outer_sum_f32_small", P(sl["X1"]), sl["X1"].ld, P(sl["X2"]), sl["X2"].ld, c.M, c.R, c.Cc, P(sl["G"]), sl["G"].ld,
                 P(sl.get("rowsum")), S)
    elif g == "colstats":
        hip.call("cris_colstats_f32_small", P(sl["y"]), sl["y"].ld, c.M, c.C, P(sl["psum"]), P(sl["pm2"]), S)
    elif g == "bn_relu":
        hip.call("cris_bn_relu_f32_small", P(sl["y"]), sl["y"].ld, P(sl["scale"]), P(sl["shift"]), c.M, c.C, P(sl["z"]), sl["z"].ld, S)
    elif g == "bwd_reduce":
        hip.call("cris_bn_relu_bwd_reduce_f32_small", P(sl["dz"]), sl["dz"].ld, P(sl["y"]), sl["y"].ld, P(sl["scale"]), P(sl["shift"]), P(sl["mean"]),
                 P(sl["invstd"]), c.M, c.C, P(sl["part"]), S)
    elif g == "bwd_apply":
        hip.call("cris_bn_relu_bwd_apply_f32_small", P(sl["dz"]), sl["dz"].ld, P(sl["y"]), sl["y"].ld, P(sl["scale"]), P(sl["shift"]), P(sl["mean"]),
                 P(sl["invstd"]), P(sl["sums"]), E.sbn_count(c), c.M, c.C, P(sl["dy"]), sl["dy"].ld, S)
    elif g == "eot_gather":
        hip.call("cris_eot_gather_ln_f32", P(sl["tokens"]), P(sl["x"]), P(sl["mean"]), P(sl["rstd"]), P(sl["gamma"]), P(sl["beta"]), c.Bn, c.L, c.D,
                 P(sl["out"]), P(sl["eot_index"]), S)
    elif g == "eot_scatter":
        hip.call("cris_eot_scatter_add_f32", P(sl["eot_index"]), P(sl["g"]), c.Bn, c.L, c.D, P(sl["dx"]), S)
    elif g == "bnf":
        bn_finalize(c, sl)
    elif g == "sync_pack":
        hip.call("cris_bn_sync_pack", P(sl["merged"]), P(sl["mean_local"]), P(sl["ref"]), E.SYNC_N, c.C, S)
    elif g == "sync_unpack":
        hip.call("cris_bn_sync_unpack", P(sl["merged"]), P(sl["ref"]), E.SYNC_COUNT, c.C, S)
    elif g == "eval_coeffs":
        hip.call("cris_bn_eval_coeffs", P(sl["gamma"]), P(sl["beta"]), P(sl["rmean"]), P(sl["rvar"]), E.EPS, c.C, P(sl["scale"]), P(sl["shift"]), S)
    elif g == "sum":
        sum_tables(c, sl, range(len(c.tables)))
    else:
        raise KeyError(g)
    torch.cuda.synchronize()


def bn_finalize(c, sl, nparts=None):
    count_local, count, _ = E.bnf_counts(c)
    glob = c.form == "global"
    hip.call("cris_bn_finalize", P(sl.get("psum")), P(sl.get("pm2")), 0 if glob else (nparts or c.nparts), 0 if glob else c.rpp, float(count_local),
             float(count), P(sl["gamma"]), P(sl["beta"]), P(sl.get("rmean")), P(sl.get("rvar")), float(c.mom or 0.0), E.EPS, c.C, P(sl["scale"]),
             P(sl["shift"]), P(sl["mean"]), P(sl["invstd"]), P(sl.get("merged")), P(sl.get("gstats")), ops._stream())


def sum_group(c, sl, which):
    off = E.sum_offsets(c)
    grp = hip.SumGroup()
    grp.n = len(which)
    for j, i in enumerate(which):
        ncol, nparts = c.tables[i]
        e = grp.e[j]
        e.part, e.out = P(sl["part%d" % i]), P(sl["out"]) + 4 * off[i]
        e.nparts, e.ncol, e.ld = nparts, ncol, sl["part%d" % i].ld
    return grp


def sum_tables(c, sl, which):
    hip.call("cris_sum_tables", C.byref(sum_group(c, sl, list(which))), ops._stream())


def run(group, case):
    rep = {}
    sl = E.run(group, case, DEV, launch, rep)
    for k, r in rep.items():
        _WORST[k] = max(_WORST.get(k, 0.0), r)
    return sl


def test_dispatch_constants_are_the_ones_the_cases_assume():
    assert ops.SMALL_MAX_ROWS == E.SMALL_MAX_ROWS and hip.SUM_GROUP_MAX == E.SUM_GROUP_MAX
    for n in E.BNF_NPARTS:
        assert ops.partials_rows(n) == E.partials_rows(n), n


_LIN_BUNDLES = sorted({(c.group, c.M, c.bias, c.acc) for c in E.LIN_CASES})


@pytest.mark.parametrize("form,M,bias,acc", _LIN_BUNDLES, ids=["%s-M%d%s%s" % (f, M, "-bias" if b else "", "-acc" if a else "") for f, M, b, a in _LIN_BUNDLES])
def test_linear(form, M, bias, acc):
    """every N x K of the table at one row count and one epilogue: per element, old contents in reference and scale"""
    for c in E.LIN_CASES:
        if (c.group, c.M, c.bias, c.acc) == (form, M, bias, acc):
            run("linear", c)


@pytest.mark.parametrize("case", E.OUTER_CASES, ids=repr)
def test_outer_sum(case):
    run("outer", case)


@pytest.mark.parametrize("case", E.SBN_CASES, ids=repr)
def test_small_bn(case):
    run("small_bn", case)


@pytest.mark.parametrize("case", E.EOT_CASES, ids=repr)
def test_eot(case):
    run("eot", case)


@pytest.mark.parametrize("case", E.BNF_CASES, ids=repr)
def test_bn_finalize(case):
    run("bn_finalize", case)


@pytest.mark.parametrize("case", E.SYNC_CASES, ids=repr)
def test_bn_sync_and_eval(case):
    run("bn_sync", case)


@pytest.mark.parametrize("case", E.SUM_CASES, ids=repr)
def test_sum_tables(case):
    """the group in one launch per element; then every table alone: the same bits"""
    sl = run("sum_tables", case)
    grouped = sl["out"].get()
    if len(case.tables) == 1:
        return
    alone = E.sum_build(case, DEV)
    for i in range(len(case.tables)):
        sum_tables(case, alone, [i])
    torch.cuda.synchronize()
    alone["out"].assert_guards(case.id + " alone")
    assert bits_equal(alone["out"].get(), grouped), case.id + ": a table summed in a group differs from the same table summed alone"


def test_sum_queue_splits_65_items_into_two_launches():
    tables = tuple((E.SUM_NCOL[i % 5], E.SUM_NPARTS[(i // 5 + 2 * i) % 5]) for i in range(E.SUM_GROUP_MAX + 1))
    case = E.Case("sum", name="queue65", tables=tables)
    sl = E.sum_build(case, DEV)
    before = E.images(sl)
    off = E.sum_offsets(case)
    q = ops.SumQueue()
    out = sl["out"].data[0]
    for i, (ncol, nparts) in enumerate(tables):
        s = sl["part%d" % i]
        q.add(s.data, out[off[i]:off[i] + ncol], nparts, ncol, s.ld)
    cl = hip.CommandList()
    with hip.recording(cl):
        q.flush()
    torch.cuda.synchronize()
    assert [name for _, _, name in cl.cmds] == ["cris_sum_tables"] * 2 and not q.items
    E.sum_check(case, sl, before)
    alone = E.sum_build(case, DEV)
    for i in range(len(tables)):
        sum_tables(case, alone, [i])
    torch.cuda.synchronize()
    assert bits_equal(alone["out"].get(), sl["out"].get())


def refused(sl, fn, match):
    before = E.images(sl)
    with pytest.raises(hip.HipLibraryError, match=match):
        fn()
    torch.cuda.synchronize()
    after = E.images(sl)
    for k in before:
        assert bits_equal(after[k], before[k]), "a refused launch wrote " + k


def test_refusals_leave_the_outputs_untouched():
    S = ops._stream()
    c = E.Case("linear_nk", M=16, N=5, K=65, bias=True, acc=False)
    sl = E.lin_build(c, DEV)
    args = lambda M, kn: ("cris_linear_f32_small", P(sl["A"]), sl["A"].ld, P(sl["W"]), sl["W"].ld, kn, P(sl["bias"]), M, c.N, c.K,  # noqa: E731
                          P(sl["out"]), sl["out"].ld, 0, S)
    refused(sl, lambda: hip.call(*args(17, 0)), "at most CRIS_SMALL_MAX_ROWS rows")
    refused(sl, lambda: hip.call(*args(16, 1)), "bias only")
    c = E.OUTER_CASES[-1]
    sl = E.outer_build(c, DEV)
    refused(sl, lambda: hip.call("cris_outer_sum_f32_small", P(sl["X1"]), sl["X1"].ld, P(sl["X2"]), sl["X2"].ld, c.M, 65536, c.Cc, P(sl["G"]),
                                 sl["G"].ld, P(sl["rowsum"]), S), "bad args")
    c = next(x for x in E.BNF_CASES if x.nparts == 17 and x.C == 17 and x.form == "plain" and x.mom is not None)
    sl = E.bnf_build(c, DEV)
    for wrong in (16, 18):                       # a list that does not cover count_local rows, and one with a part too many
        refused(sl, lambda: bn_finalize(c, sl, nparts=wrong), "must cover count_local")
    c = E.SUM_CASES[-1]
    sl = E.sum_build(c, DEV)
    for n in (0, E.SUM_GROUP_MAX + 1):
        grp = sum_group(c, sl, range(len(c.tables)))
        grp.n = n
        refused(sl, lambda: hip.call("cris_sum_tables", C.byref(grp), S), "CRIS_SUM_GROUP_MAX")


def test_zz_worst_error_over_bound():
    """the figures of DESIGN.md section 6 (run with -s); every one below 1 is what the tests above asserted"""
    for k in sorted(_WORST):
        print("worst error / bound on the GPU: %-24s %.3f" % (k, _WORST[k]))
    assert all(r <= 1.0 for r in _WORST.values())
