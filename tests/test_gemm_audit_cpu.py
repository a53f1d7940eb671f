"""The GEMM auditor (tests/gemm_audit.py) has teeth: launches are built on CPU tensors by the production parameter builders
(ops.conv_gemm / ops.conv_wgrad / ops.GemmQueue with the auditor installed as ops.KERNEL_TIMER, exactly as the GPU test
does) and "run" by a float32 emulation of the kernels (bf16 operands, fp32 accumulation, the documented epilogue).  The
audit must pass on two summation orders and fail, naming the right place, on each deliberately broken variant."""
import pytest
import torch

from cris.pytorch_amd import ops
from cris.pytorch_amd.ops import Drop, Geom

import gemm_audit as GA
from gemm_emulator import Emulator

BF = torch.bfloat16
F32 = torch.float32


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale)


def bfr(*shape, seed=0, scale=1.0):
    return rnd(*shape, seed=seed, scale=scale).to(BF)


@pytest.fixture
def audit(monkeypatch):
    def make(order="blk", mut=None):
        a = GA.Auditor(GA.CpuMemory(), Emulator(order, mut), raise_on_failure=False)
        monkeypatch.setattr(ops, "KERNEL_TIMER", a)
        return a
    return make


def _conv(seed=0, M_img=(2, 9, 11), C_=32, N=48, KH=3, stride=2, pad=1, **kw):
    Bn, H, W = M_img
    g = Geom(Bn, H, W, C_, KH, KH, stride, pad)
    ldA = C_ + 16
    A = bfr(Bn, H, W, ldA, seed=seed)
    Wt = bfr(N, g.K, seed=seed + 1, scale=0.05)
    return g, A, Wt, ldA


def case_conv_sliced(seed=0, drop=None):
    """3x3 / stride 2 / pad 1 convolution from a channel slice (a_coff 8) into a column slice (c_coff 16) of a wider buffer,
    bias + ReLU, bf16 residual, forward BatchNorm partials"""
    g, A, Wt, ldA = _conv(seed)
    N = Wt.shape[0]
    out = torch.full((g.M, N + 32), 7.0, dtype=BF)
    res = bfr(g.M, N, seed=seed + 2)
    bias = rnd(N, seed=seed + 3)
    st = ops.conv_gemm(A, Wt, g, N, lda=ldA, a_coff=8, bias=bias, act=1, resid=res, out=out, ldc=N + 32, c_coff=16, stats=True,
                       drop=drop or ops.NO_DROP)
    return out, st


def test_audit_passes_both_summation_orders(audit):
    for order in ("seq", "blk"):
        a = audit(order)
        case_conv_sliced()
        # K = 4608 linear (the long reductions), fp32 output, fp32 residual
        A, Wt = bfr(200, 4608, seed=5), bfr(64, 4608, seed=6, scale=0.05)
        out = torch.zeros(200, 64, dtype=F32)
        ops.conv_gemm(A, Wt, Geom.linear(200, 4608), 64, out=out, resid=rnd(200, 64, seed=7), act=3)
        # decoder-style projection: QuickGELU, dropout with a device seed word, head-split copy (2 heads) + pad columns
        T_L, T_Lpad, B = 10, 12, 3
        A, Wt = bfr(B * T_L, 64, seed=8), bfr(128, 64, seed=9, scale=0.2)
        outT = torch.zeros(B * 128, T_Lpad, dtype=BF)
        dev = torch.tensor([5], dtype=torch.int32)
        ops.conv_gemm(A, Wt, Geom.linear(B * T_L, 64), 128, bias=rnd(128, seed=10), act=2, out=torch.zeros(B * T_L, 128, dtype=BF),
                      outT=outT, T_L=T_L, T_Lpad=T_Lpad, T_E=128, T_sec_stride=0, drop=Drop(0.25, 123, 4, dev))
        # split-K skinny kernel with its workspace
        A, Wt = bfr(40, 2048, seed=11), bfr(96, 2048, seed=12, scale=0.05)
        ops.conv_gemm(A, Wt, Geom.linear(40, 2048), 96, out=torch.zeros(40, 96, dtype=BF))
        # BatchNorm-backward partials of an input-gradient GEMM
        _bnr_case()
        # weight gradient, pixel range split, bias gradient, padded rows; and a grouped one
        _wgrad_case()
        q = ops.WgradQueue()
        for s in range(2):
            g = Geom(2, 6, 6, 16, 3, 3, 1, 1)
            ops.conv_wgrad(bfr(g.M, 24, seed=20 + s), bfr(2, 6, 6, 16, seed=30 + s), g, 24, torch.zeros(24, 256), ldw=256,
                           dbias=torch.zeros(24), queue=q)
        q.flush()
        # a grouped forward launch: two column slices of one concatenation buffer
        _group_case()
        bad = [r.describe() for r in a.reports if not r.ok]
        assert not bad, "\n".join(bad)
        assert len(a.reports) == 8
        kinds = set().union(*[r.kinds for r in a.reports])
        for k in ("sliced output", "offset input", "BN partials", "bnr partials", "dropout", "outT", "f32 output", "f32 residual",
                  "bf16 residual", "skinny split-K with workspace", "split wgrad", "grouped wgrad", "dbias", "4-wave group"):
            assert k in kinds, k
        assert max(r.worst() for r in a.reports) < 1


def _bnr_case(N=64, seed=40):
    g = Geom(2, 12, 12, 64, 3, 3, 1, 1)
    A, Wt = bfr(2, 12, 12, 64, seed=seed), bfr(N, g.K, seed=seed + 1, scale=0.05)
    y = bfr(g.M, N + 8, seed=seed + 2)
    bnr = dict(y=y, ldy=N + 8, coff=8, mean=rnd(N, seed=seed + 3, scale=0.1), invstd=rnd(N, seed=seed + 4).abs() + 0.5,
               scale=rnd(N, seed=seed + 5), shift=rnd(N, seed=seed + 6))
    out = torch.zeros(g.M, N, dtype=BF)
    parts = ops.conv_gemm(A, Wt, g, N, out=out, bnr=bnr)
    assert parts is not None
    return out


def _wgrad_case(seed=50, splits=3):
    g = Geom(2, 20, 20, 32, 3, 3, 1, 1)
    dW = torch.full((40, 384), 3.0)
    ops.conv_wgrad(bfr(g.M, 48, seed=seed), bfr(2, 20, 20, 48, seed=seed + 1), g, 40, dW, ldy=48, x_coff=16, ldx=48, ldw=384,
                   splits=splits, dbias=torch.zeros(40))
    return dW


def _group_case(overlap=False):
    q = ops.GemmQueue()
    cat = torch.zeros(150, 3 * 64, dtype=BF)
    for i in range(3):
        A, Wt = bfr(150, 64, seed=60 + i), bfr(64, 64, seed=70 + i, scale=0.1)
        coff = 64 * i if not (overlap and i == 2) else 64 + 8
        ops.conv_gemm(A, Wt, Geom.linear(150, 64), 64, out=cat, c_coff=coff, bias=rnd(64, seed=80 + i), queue=q)
    q.flush()


def _one_failure(a, what=None):
    bad = [r for r in a.reports if not r.ok]
    assert bad, "the audit did not notice"
    msg = bad[0].describe()
    if what:
        assert what in msg, msg
    return bad[0], msg


def _first(rep):
    return next(f for r in rep.problems for f in r.findings)


def test_missing_k_step_in_one_tile(audit):
    a = audit(mut="missing_kstep")
    A, Wt = bfr(128, 4608, seed=1), bfr(128, 4608, seed=2, scale=0.05)
    ops.conv_gemm(A, Wt, Geom.linear(128, 4608), 128, out=torch.zeros(128, 128, dtype=BF))
    rep, msg = _one_failure(a, "out at")
    f = _first(rep)
    assert 32 <= f.row < 64 and 32 <= f.col < 64, msg


def test_m_tail_tile_reads_previous_rows(audit):
    a = audit(mut="mtail_prev_rows")
    A, Wt = bfr(300, 64, seed=1), bfr(80, 64, seed=2)
    ops.conv_gemm(A, Wt, Geom.linear(300, 64), 80, out=torch.zeros(300, 80, dtype=BF))
    rep, msg = _one_failure(a, "out at")
    f = _first(rep)
    BM = GA.tile_shape(rep.problems[0].family.split()[-1], 300)[0]
    t0 = 300 // BM * BM
    assert t0 < 300 and f.row >= t0 and f.tile[0] == t0 // BM, msg


def test_output_shifted_by_one_coff_step(audit):
    a = audit(mut="shift_coff")
    case_conv_sliced()
    rep, msg = _one_failure(a)
    assert rep.footprint and "out of problem 0" in rep.footprint[0], msg


def test_one_neighbour_column_written(audit):
    a = audit(mut="neighbour_col")
    out, _ = case_conv_sliced()
    rep, msg = _one_failure(a)
    assert rep.footprint and "out of problem 0" in rep.footprint[0], msg
    g = Geom(2, 9, 11, 32, 3, 3, 2, 1)
    assert ("row %d," % (g.M // 2)) in rep.footprint[0] and ("byte column %d)" % ((16 + 48) * 2)) in rep.footprint[0], msg


def test_middle_bn_partial_over_wrong_rows(audit):
    a = audit(mut="bn_wrong_block")
    case_conv_sliced()
    rep, msg = _one_failure(a, "BN partial")
    g = Geom(2, 9, 11, 32, 3, 3, 2, 1)
    nparts = -(-g.M // 32)
    assert ("part %d " % (nparts // 2)) in msg, msg


def test_flipped_dropout_decision(audit):
    a = audit(mut="flip_drop")
    case_conv_sliced(drop=Drop(0.3, 77, 2))
    rep, msg = _one_failure(a)
    g = Geom(2, 9, 11, 32, 3, 3, 2, 1)
    f = _first(rep)
    assert (f.row, f.col) == (g.M // 2, 48 // 2), msg


def test_bias_after_relu(audit):
    a = audit(mut="bias_after_relu")
    case_conv_sliced()
    _one_failure(a, "out at")


def test_residual_before_dropout(audit):
    a = audit(mut="resid_before_drop")
    case_conv_sliced(drop=Drop(0.3, 77, 2))
    _one_failure(a, "out at")


def test_split_k_slab_summed_twice(audit):
    a = audit(mut="slab_twice")
    A, Wt = bfr(40, 2048, seed=11), bfr(96, 2048, seed=12, scale=0.05)
    ops.conv_gemm(A, Wt, Geom.linear(40, 2048), 96, out=torch.zeros(40, 96, dtype=BF))
    rep, msg = _one_failure(a, "out at")
    assert "skinny9s" in msg, msg


def test_two_heads_swapped_in_outT(audit):
    a = audit(mut="swap_heads")
    A, Wt = bfr(30, 64, seed=8), bfr(128, 64, seed=9, scale=0.2)
    outT = torch.zeros(3 * 128, 12, dtype=BF)
    ops.conv_gemm(A, Wt, Geom.linear(30, 64), 128, out=torch.zeros(30, 128, dtype=BF), outT=outT, T_L=10, T_Lpad=12, T_E=128)
    _one_failure(a, "outT at")


def test_bnr_mask_on_y_instead_of_bn(audit):
    a = audit(mut="bnr_y_gt0")
    _bnr_case()
    _one_failure(a, "bnr sum g")


def test_wgrad_missing_pixel_split(audit):
    a = audit(mut="missing_split")
    _wgrad_case()
    _one_failure(a, "dW at")


def test_group_problems_with_overlapping_writes(audit):
    a = audit()
    _group_case(overlap=True)
    rep, msg = _one_failure(a, "writes out")
    assert "problem 2" in msg or "problem 1" in msg, msg


def test_region_intersection():
    R = GA.Region
    a = R("a", 1000, 10, 256, 0, 64)
    assert not GA.regions_intersect(a, R("b", 1000, 10, 256, 64, 64))           # neighbouring column slices
    assert GA.regions_intersect(a, R("b", 1000, 10, 256, 56, 64))               # one 8-byte step into a's columns
    assert not GA.regions_intersect(a, R("b", 1000 + 10 * 256, 4, 256, 0, 64))  # the rows after a
    assert GA.regions_intersect(a, R("b", 1000 + 9 * 256, 4, 256, 0, 64))
    assert GA.regions_intersect(a, R("b", 1000, 5, 512, 0, 8))                  # another stride
    assert not GA.regions_intersect(a, R("b", 1000, 5, 512, 128, 8))
