"""The GEMM auditor (tests/gemm_audit.py) has teeth: launches are built on CPU tensors by the production parameter builders
(ops.conv_gemm / ops.conv_wgrad / ops.GemmQueue with the auditor installed as ops.KERNEL_TIMER, exactly as the GPU test
does) and "run" by a float32 emulation of the kernels (bf16 operands, fp32 accumulation, the documented epilogue).  The
audit must pass on two summation orders and fail, naming the right place, on each deliberately broken variant."""
import ctypes as C

import pytest
import torch

from cris.pytorch_amd import hip, ops
from cris.pytorch_amd.ops import Drop, Geom
from oracle.dropout_hash import keep_mask_torch

import gemm_audit as GA

BF = torch.bfloat16
F32 = torch.float32


def _view(addr, rows, stride, ncols, dtype):
    """writable host view [rows][ncols] with a row stride in elements"""
    es = torch.tensor([], dtype=dtype).element_size()
    n = ((rows - 1) * stride + ncols) * es
    buf = torch.frombuffer((C.c_char * n).from_address(addr), dtype=torch.uint8).view(dtype)
    return torch.as_strided(buf, (rows, ncols), (stride, 1))


def _sum(A, W, order):
    """A [M,K] @ W[N,K]^T in fp32: sequential over k, or blocks of 32 (sequential inside) added pairwise"""
    M, K = A.shape
    N = W.shape[0]
    if order == "seq":
        acc = torch.zeros(M, N, dtype=F32)
        for k in range(K):
            acc += A[:, k:k + 1] * W[:, k].unsqueeze(0)
        return acc
    nb = -(-K // 32)
    Ap = torch.nn.functional.pad(A, (0, nb * 32 - K)).view(M, nb, 32)
    Wp = torch.nn.functional.pad(W, (0, nb * 32 - K)).view(N, nb, 32)
    acc = torch.zeros(M, N, nb, dtype=F32)
    for i in range(32):
        acc += Ap[:, :, i].unsqueeze(1) * Wp[:, :, i].unsqueeze(0)
    while acc.shape[2] > 1:
        if acc.shape[2] % 2:
            acc = torch.cat([acc, torch.zeros(M, N, 1, dtype=F32)], 2)
        acc = acc[:, :, 0::2] + acc[:, :, 1::2]
    return acc[:, :, 0]


class Emulator:
    """cris_conv_gemm_variant / _group_launch, cris_conv_wgrad / _group on host memory; `mut` names one deliberate bug"""

    def __init__(self, order="blk", mut=None):
        self.order, self.mut = order, mut

    def __call__(self, fn, args):
        a0 = GA._obj(args[0])
        if fn == "cris_conv_gemm_variant":
            p = a0
            v = hip.load().cris_conv_gemm_plan(C.byref(p), int(args[1]), None)
            self.gemm(p, v)
        elif fn == "cris_conv_gemm_group_launch":
            for i in range(a0.n):
                self.gemm(a0.prob[i], int(args[1]))
        elif fn == "cris_conv_wgrad":
            self.wgrad(a0)
        elif fn == "cris_conv_wgrad_group":
            for i in range(a0.n):
                self.wgrad(a0.prob[i])
        else:
            raise AssertionError(fn)

    def gemm(self, p, v):
        mut = self.mut
        M, N, K = p.M, p.N, p.K
        Av = _view(p.A, p.Bn * p.H * p.W, p.lda, p.a_coff + p.C, BF)[:, p.a_coff:]
        A = GA.im2col64(Av, (p.Bn, p.H, p.W, p.C, p.OH, p.OW, p.KH, p.KW), 0, M, p.stride, p.pad, "cpu").to(F32)
        W = _view(p.Wt, N, p.ldb, K, BF).to(F32)
        vn = GA.VARIANTS[v]
        BM, BN = GA.tile_shape(vn, M)
        if mut == "mtail_prev_rows":                           # the M-tail tile reads the rows of the tile before it
            t0 = (M // BM) * BM
            A = A.clone()
            A[t0:] = A[t0 - BM:M - BM]
        if vn == "skinny9s":
            slices = GA.skinny_slices(p, v)
            ks = -(-(-(-K // slices)) // 32) * 32
            acc = torch.zeros(M, N, dtype=F32)
            for s in range(slices):
                part = _sum(A[:, s * ks:(s + 1) * ks], W[:, s * ks:(s + 1) * ks], self.order)
                acc += part
                if mut == "slab_twice" and s == 1:
                    acc += part
        else:
            acc = _sum(A, W, self.order)
        if mut == "missing_kstep":                              # one 32x32 tile drops one K-step of 16
            r, c, k = slice(32, 64), slice(32, 64), slice(160, 176)
            acc[r, c] -= A[r, k] @ W[c, k].T
        x = acc
        bias = _view(p.bias, 1, N, N, F32)[0] if p.bias else torch.zeros(N)
        if mut != "bias_after_relu":
            x = x + bias
        if p.act == 1:
            x = x.clamp_min(0)
        elif p.act == 2:
            x = x / (1 + torch.exp(-1.702 * x))
        if mut == "bias_after_relu":
            x = x + bias
        res = None
        if p.resid:
            res = _view(p.resid, M, p.ldr, p.r_coff + N, F32 if p.resid_f32 else BF)[:, p.r_coff:].to(F32)
        if mut == "resid_before_drop" and res is not None:
            x = x + res
        if p.drop_thresh:
            seed = p.drop_seed + (int(_view(p.drop_seed_dev, 1, 1, 1, torch.int32)[0, 0]) if p.drop_seed_dev else 0)
            keep = keep_mask_torch(seed % 2 ** 32, p.drop_stream, M * N, p.drop_thresh / 4294967296.0, "cpu").view(M, N)
            if mut == "flip_drop":
                keep[M // 2, N // 2] = ~keep[M // 2, N // 2]
            x = torch.where(keep, x * (1.0 / (1.0 - p.drop_p)), torch.zeros_like(x))
        if res is not None and mut != "resid_before_drop":
            x = x + res
        if p.act == 3:
            x = x.clamp_min(0)
        if p.out:
            dt = F32 if p.out_f32 else BF
            coff = p.c_coff + (8 if mut == "shift_coff" else 0)
            out = _view(p.out, M, p.ldc, p.ldc, dt)
            out[:, coff:coff + N] = x.to(dt)
            if mut == "neighbour_col":
                out[M // 2, p.c_coff + N] = 1.0
        if p.outT:
            Hh = p.T_E // 64
            xs = x.to(BF)
            for n in range(N):
                sec, e = divmod(n, p.T_E)
                h, d = divmod(e, 64)
                if mut == "swap_heads" and h < 2 and Hh >= 2:
                    h = 1 - h
                tv = _view(p.outT + sec * p.T_sec_stride * 2, (M // p.T_L) * p.T_E, p.T_Lpad, p.T_L, BF)
                for b in range(M // p.T_L):
                    tv[(b * Hh + h) * 64 + d, :] = xs[b * p.T_L:(b + 1) * p.T_L, n]
        if p.colsum:
            R = hip.load().cris_conv_gemm_variant_stat_rows(C.byref(p), v)
            sld = p.stat_ld or N
            nparts = -(-M // R)
            cs, cq = _view(p.colsum, nparts, sld, N, F32), _view(p.colsq, nparts, sld, N, F32)
            if p.bnr_y:
                y = _view(p.bnr_y, M, p.bnr_ldy, p.bnr_coff + N, BF)[:, p.bnr_coff:].to(F32)
                vec = {nm: _view(getattr(p, nm), 1, N, N, F32)[0] for nm in ("bnr_mean", "bnr_invstd", "bnr_scale", "bnr_shift")}
                on = (y > 0) if mut == "bnr_y_gt0" else (y * vec["bnr_scale"] + vec["bnr_shift"] > 0)
                g = torch.where(on, x.to(BF).to(F32), torch.zeros_like(x))
                gx = g * ((y - vec["bnr_mean"]) * vec["bnr_invstd"])
                for q in range(nparts):
                    cs[q] = g[q * R:(q + 1) * R].sum(0)
                    cq[q] = gx[q * R:(q + 1) * R].sum(0)
            else:
                for q in range(nparts):
                    src = q + 1 if (mut == "bn_wrong_block" and q == nparts // 2) else q
                    blk = x[src * R:(src + 1) * R]
                    s1 = blk.sum(0)
                    mu = s1 / blk.shape[0]
                    cs[q] = s1
                    cq[q] = ((blk - mu) ** 2).sum(0)

    def wgrad(self, p):
        M, N, K = p.M, p.N, p.K
        dY = _view(p.dY, M, p.ldy, p.y_coff + N, BF)[:, p.y_coff:].to(F32)
        Xv = _view(p.X, p.Bn * p.H * p.W, p.ldx, p.x_coff + p.C, BF)[:, p.x_coff:]
        X = GA.im2col64(Xv, (p.Bn, p.H, p.W, p.C, p.OH, p.OW, p.KH, p.KW), 0, M, p.stride, p.pad, "cpu").to(F32)
        rp = GA.wgrad_rows_per_split(M, p.splits)
        dW = torch.zeros(N, K, dtype=F32)
        db = torch.zeros(N, dtype=F32)
        for s in range(GA.wgrad_effective_splits(M, p.splits)):
            if self.mut == "missing_split" and s == 1:
                continue
            sl = slice(s * rp, min(M, (s + 1) * rp))
            dW += _sum(dY[sl].T.contiguous(), X[sl].T.contiguous(), self.order)
            db += dY[sl].sum(0)
        out = _view(p.dW, N, p.ldw, p.ldw, F32)
        out[:, :K] = dW
        out[:, K:] = 0
        if p.dbias:
            _view(p.dbias, 1, N, N, F32)[0] = db


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
