"""A float32 emulation of the GEMM / weight-gradient launches on host memory (test infrastructure; importable without a GPU):
bf16 operands, fp32 accumulation in one of two summation orders, the documented epilogue.  tests/test_gemm_audit_cpu.py and
tests/test_gemm_edges_cpu.py "run" launches with it under the auditor (tests/gemm_audit.py): a correct emulation must pass, and
each `mut` - one deliberate bug of the kind a tile kernel can have - must be refused."""
import ctypes as C

import torch

from cris.pytorch_amd import hip
from oracle.dropout_hash import keep_mask_torch

import gemm_audit as GA

BF = torch.bfloat16
F32 = torch.float32
BK = 64                     # K-step of the tile kernels (gemm_common.h)


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
    if order == "seq" or K == 0:
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


def _im2col_le(Araw, p):
    """im2col whose lower-border test reads `ih <= H`: the row below an image (the next image's first row; below the last
    image, whatever follows the activation in memory) instead of the zero padding.  Araw: [Bn*H*W + W][C] view."""
    m = torch.arange(p.M)
    b = m // (p.OH * p.OW)
    r = m - b * (p.OH * p.OW)
    oh, ow = r // p.OW, r % p.OW
    cols = []
    for kh in range(p.KH):
        for kw in range(p.KW):
            ih, iw = oh * p.stride - p.pad + kh, ow * p.stride - p.pad + kw
            ok = (ih >= 0) & (ih <= p.H) & (iw >= 0) & (iw < p.W)
            idx = (b * p.H + ih.clamp(0, p.H)) * p.W + iw.clamp(0, p.W - 1)
            v = Araw.index_select(0, idx).to(F32)
            cols.append(torch.where(ok.unsqueeze(1), v, torch.zeros_like(v)))
    return torch.cat(cols, 1)


class Emulator:
    """cris_conv_gemm_variant / _group_launch, cris_conv_wgrad / _group on host memory; `mut` names one deliberate bug.
    ring: ring depth of the tile variant that runs (the "stale_ring" bug needs it)."""

    def __init__(self, order="blk", mut=None, ring=None):
        self.order, self.mut, self.ring = order, mut, ring

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
        rows_in = p.Bn * p.H * p.W
        Av = _view(p.A, rows_in, p.lda, p.a_coff + p.C, BF)[:, p.a_coff:]
        if mut == "pad_le":                                    # the padding test is off by one: `ih <= H`
            A = _im2col_le(_view(p.A, rows_in + p.W, p.lda, p.a_coff + p.C, BF)[:, p.a_coff:], p)
        else:
            A = GA.im2col64(Av, (p.Bn, p.H, p.W, p.C, p.OH, p.OW, p.KH, p.KW), 0, M, p.stride, p.pad, "cpu").to(F32)
        W = _view(p.Wt, N, p.ldb, K, BF).to(F32)
        vn = GA.VARIANTS[v]
        BM, BN = GA.tile_shape(vn, M)
        if mut == "mtail_prev_rows":                           # the M-tail tile reads the rows of the tile before it
            t0 = (M // BM) * BM
            A = A.clone()
            A[t0:] = A[t0 - BM:M - BM]
        if mut == "stale_ring":                                # the first refilled ring buffer (K-step D) still holds step 0
            D = self.ring
            assert D and K > D * BK
            A, W = A.clone(), W.clone()
            n = min(BK, K - D * BK)
            A[:, D * BK:D * BK + n] = A[:, :n]
            W[:, D * BK:D * BK + n] = W[:, :n]
        if mut == "tap_stuck":                                 # a K-step keeps the tap of its first chunk: a chunk beyond the
            A = A.clone()                                      # tap's end reads the first tap's pixel
            for k0 in range(0, K, BK):
                tap0 = k0 // p.C
                for k in range(k0, min(K, k0 + BK)):
                    if k // p.C != tap0:
                        A[:, k] = A[:, tap0 * p.C + k % p.C]
        if vn == "skinny9s":
            slices = GA.skinny_slices(p, v)
            ks = -(-(-(-K // slices)) // 32) * 32
            acc = torch.zeros(M, N, dtype=F32)
            for s in range(slices):
                if mut == "empty_slice_unwritten" and s * ks >= K:
                    # the finish pass adds the slab of a slice whose blocks never stored it: whatever the workspace held
                    nb = -(-N // 32)
                    slab = _view(p.ws + 4 * s * nb * 9 * 2 * 256, 1, nb * 9 * 2 * 256, nb * 9 * 2 * 256, F32)
                    acc += slab[0, :1]
                    continue
                part = _sum(A[:, s * ks:(s + 1) * ks], W[:, s * ks:(s + 1) * ks], self.order)
                acc += part
                if mut == "slab_twice" and s == 1:
                    acc += part
        elif vn == "64x64k2":                                  # two wave groups: the even K-steps, then + the odd ones
            nk = -(-K // BK)
            cols = [torch.cat([torch.arange(s * BK, min(K, (s + 1) * BK)) for s in range(g, nk, 2)] or [torch.arange(0)])
                    for g in (0, 1)]
            if mut == "k2_drop_last" and nk % 2 == 1 and nk > 1:   # at an odd count the second group has one step fewer:
                cols[1] = cols[1][:-BK]                            # its trip count taken from the first group's drops one
            acc = _sum(A[:, cols[0]], W[:, cols[0]], self.order) + _sum(A[:, cols[1]], W[:, cols[1]], self.order)
        else:
            acc = _sum(A, W, self.order)
        if mut == "ktail_unmasked":                             # the K tail of the last step is not masked: Wt columns [K, ldb)
            Wx = _view(p.Wt, N, p.ldb, p.ldb, BF)[:, K:].to(F32)
            acc = acc + torch.ones(M, Wx.shape[1]) @ Wx.T
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
            if mut == "mtail_row_M":                            # the M-tail tile stores one row too many
                _view(p.out, M + 1, p.ldc, p.ldc, dt)[M, coff:coff + N] = x[M - 1].to(dt)
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
                    mu = s1 / (R if mut == "bn_last_div_R" else blk.shape[0])    # the last part's mean over R rows, not its own
                    cs[q] = s1
                    cq[q] = ((blk - mu) ** 2).sum(0)

    def wgrad(self, p):
        mut = self.mut
        M, N, K = p.M, p.N, p.K
        dY = _view(p.dY, M, p.ldy, p.y_coff + N, BF)[:, p.y_coff:].to(F32)
        Xv = _view(p.X, p.Bn * p.H * p.W, p.ldx, p.x_coff + p.C, BF)[:, p.x_coff:]
        X = GA.im2col64(Xv, (p.Bn, p.H, p.W, p.C, p.OH, p.OW, p.KH, p.KW), 0, M, p.stride, p.pad, "cpu").to(F32)
        rp = GA.wgrad_rows_per_split(M, p.splits)
        dW = torch.zeros(N, K, dtype=F32)
        db = torch.zeros(N, dtype=F32)
        for s in range(GA.wgrad_effective_splits(M, p.splits)):
            if mut == "missing_split" and s == 1:
                continue
            end = min(M, (s + 1) * rp)
            if mut == "split_overrun":                          # the last 32-row pixel step of a split is not cut at its end
                end = min(M, end + 32)
            sl = slice(s * rp, end)
            dW += _sum(dY[sl].T.contiguous(), X[sl].T.contiguous(), self.order)
            db += dY[s * rp:min(M, (s + 1) * rp)].sum(0)
        if mut == "dbias_per_ktile":                            # every k-tile's block adds the column sums
            db = db * (-(-K // hip.load().cris_conv_wgrad_tile(C.byref(p))))
        out = _view(p.dW, N, p.ldw, p.ldw, F32)
        out[:, :K] = dW
        out[:, K:] = 0
        if p.dbias:
            _view(p.dbias, 1, N, N, F32)[0] = db
