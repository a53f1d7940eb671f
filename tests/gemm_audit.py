"""Element-wise audit of one GEMM / weight-gradient launch (test infrastructure; importable without a GPU).

The checker restates the C structs of include/cris_hip.h (cris_conv_gemm_params / _group, cris_wgrad_params / _group) in
float64 and compares EVERY element a launch writes with that statement - not one norm over the whole output:

    |got - ref| <= L * gamma * sum_k |a_k b_k|  +  e_epi  +  u_out * |ref|  +  tiny

  gamma   worst-case bound of the kernel's fp32 summation, gamma(n) = n u / (1 - n u), u = 2^-24, with n the depth of the
          summation tree the kernel really uses (gemm_depth / wgrad_depth below): v_mfma_f32_32x32x16_bf16 adds 16 exact
          bf16 products into the accumulator per K-step (ceil(K/16) dependent additions plus up to 16 inside the
          instruction); the skinny kernels' v_mfma_f32_16x16x32_bf16 does the same with 32; the skinny kernels then add
          their 8 (single pass) or 4 (split-K) wave partials and the split-K slices one after the other; the K-split 64x64
          tile adds its two wave groups; the weight gradient accumulates ceil(rows_per_split/16) pixel steps per split and
          then adds the splits.
  L       Lipschitz factor of the epilogue: 1/(1-p) with dropout, 1.13 for QuickGELU (max of d/dx x*sigmoid(1.702x)).
  e_epi   the fp32 roundings of the epilogue (bias add, activation, dropout scale, residual add: 4 u of the magnitudes
          involved) plus, for QuickGELU, the fast exp: 2^-18 relative plus 4 u |1.702 x| from rounding its argument.
  u_out   unit roundoff of the output: 2^-8 for bf16 (8 significant bits), u for fp32; the rounding also scales the
          accumulated error by (1 + u_out).

The BatchNorm partials (forward: per block of R = cris_conv_gemm_variant_stat_rows rows, the sum and the M2 about the block
mean of the fp32 epilogue values; backward (bnr_y): sum g and sum g*xhat with g = the STORED bf16 gradient where
scale*y + shift > 0) are checked row by row with the same element bounds propagated through the sums.  Dropout keep / drop
decisions (oracle.dropout_hash) must match exactly: a dropped element holds exactly the dropped value.

Write footprint: inside every declared row span, bytes the launch may not write must be unchanged bit for bit - the
columns of `out` outside [c_coff, c_coff + N), the padding columns [T_L, T_Lpad) of the head-split copy `outT` (the kernel
never stores there: the caller zero-fills them once, attention reads them as zeros), the columns of the statistics tables
beyond N.  A weight gradient owns whole rows of dW: the kernel WRITES ZEROS to the columns K .. ldw-1 (csrc/wgrad.hip
"columns K .. ldw are padding: zeros"; the header only says "overwritten"), so that is what is asserted there.

Groups: no problem's write range may intersect another problem's read or write range (cris_hip.h "No problem may read or
accumulate into what another one writes").

Memory is reached through a `Memory` object (read(lo, n) -> uint8 copy; extent_ok(lo, hi); sync()), so the same checker
runs on CPU tensors (tests/test_gemm_audit_cpu.py) and on device memory (tests/test_gemm_audit_gpu.py)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import torch

from cris.pytorch_amd import hip
from oracle.dropout_hash import keep_mask_torch

U32 = 2.0 ** -24
U_BF16 = 2.0 ** -8
TINY = 2.0 ** -120
BF = torch.bfloat16
F64 = torch.float64

VARIANTS = ["skinny1", "skinny9", "skinny9s", "128x64", "64x64", "64x128", "128x128", "8w256x256", "8w256x128", "8w128x256",
            "8w128x128", "64x64k2"]


class AuditError(AssertionError):
    pass


def gamma(n):
    return n * U32 / (1.0 - n * U32)


def tile_shape(vname, M):
    """output tile (rows, columns) of one block of a variant"""
    if vname.startswith("skinny"):
        return (16 if vname == "skinny1" else 144), 32
    rows, cols = vname.replace("8w", "").replace("k2", "").split("x")
    return int(rows), int(cols)


def skinny_slices(p, v):
    """K slices of the split-K skinny launch (cris_conv_gemm_ws_floats = slices * ceil(N/32) * 9*2*256 floats)"""
    if VARIANTS[v] != "skinny9s":
        return 1
    return int(hip.load().cris_conv_gemm_ws_floats(C.byref(p), v)) // (((p.N + 31) // 32) * 9 * 2 * 256)


def gemm_depth(p, v):
    """depth of the fp32 summation tree of one output element under variant v (see the module docstring)"""
    name = VARIANTS[v]
    if name.startswith("skinny"):
        d = -(-p.K // 32) + 32
        d += 8 if name != "skinny9s" else 4 + skinny_slices(p, v)
    else:
        d = -(-p.K // 16) + 16
        if name == "64x64k2":
            d += 1
    return d


def wgrad_rows_per_split(M, splits):
    r = -(-M // max(splits, 1))
    return -(-r // 128) * 128


def wgrad_effective_splits(M, splits):
    rp = wgrad_rows_per_split(M, splits)
    return -(-M // rp)


def wgrad_depth(p):
    s = wgrad_effective_splits(p.M, p.splits)
    return -(-wgrad_rows_per_split(p.M, p.splits) // 16) + 16 + s


def wgrad_bias_depth(p):
    s = wgrad_effective_splits(p.M, p.splits)
    return wgrad_rows_per_split(p.M, p.splits) + s


# ---- regions ------------------------------------------------------------------------------------------------------------
@dataclass
class Region:
    """rows x [col0, col0 + width) bytes at base + r * stride"""
    name: str
    base: int
    rows: int
    stride: int
    col0: int
    width: int
    write: bool = False
    scratch: bool = False          # a workspace: any byte may change, nothing to compare

    @property
    def lo(self):
        return self.base + self.col0

    @property
    def hi(self):
        return self.base + (self.rows - 1) * self.stride + self.col0 + self.width


def _intersect_same_stride(a: Region, b: Region):
    """do two regions of the same row stride share a byte?"""
    s = a.stride
    d = b.lo - a.lo
    q, rem = divmod(d, s)
    # b's row r2 starts at a's row (r2 + q) plus rem bytes; it can touch a's rows r2+q (if rem < a.width) and r2+q+1
    # (if rem + b.width > s)
    for shift, ok in ((q, rem < a.width), (q + 1, rem + b.width > s)):
        if not ok:
            continue
        lo, hi = max(0, -shift), min(b.rows, a.rows - shift)      # r2 range with r1 = r2 + shift inside a
        if lo < hi:
            return True
    return False


def regions_intersect(a: Region, b: Region):
    if a.hi <= b.lo or b.hi <= a.lo:
        return False
    if a.rows == 1 or b.rows == 1 or a.stride == b.stride:
        if a.rows == 1 and b.rows == 1:
            return True
        if a.rows == 1 or b.rows == 1:
            one, many = (a, b) if a.rows == 1 else (b, a)
            one = Region(one.name, one.base, 1, many.stride, one.col0, one.width)
            if one.width > many.stride:
                return True
            return _intersect_same_stride(many, one)
        return _intersect_same_stride(a, b)
    lo, hi = max(a.lo, b.lo), min(a.hi, b.hi)                     # different strides: byte masks of the common window
    return bool((_mask(a, lo, hi) & _mask(b, lo, hi)).any())


def _mask(r: Region, lo, hi):
    m = torch.zeros(hi - lo, dtype=torch.bool)
    first = max(0, (lo - r.lo) // r.stride)
    for row in range(first, r.rows):
        a = r.base + row * r.stride + r.col0
        if a >= hi:
            break
        m[max(a, lo) - lo:max(min(a + r.width, hi) - lo, 0)] = True
    return m


def gemm_regions(p, v):
    """read and write regions of one cris_conv_gemm_params under resolved variant v"""
    R = []
    rows_in = p.Bn * p.H * p.W
    R.append(Region("A", p.A, rows_in, p.lda * 2, p.a_coff * 2, p.C * 2))
    R.append(Region("Wt", p.Wt, p.N, p.ldb * 2, 0, p.K * 2))
    if p.bias:
        R.append(Region("bias", p.bias, 1, p.N * 4, 0, p.N * 4))
    if p.resid:
        es = 4 if p.resid_f32 else 2
        R.append(Region("resid", p.resid, p.M, p.ldr * es, p.r_coff * es, p.N * es))
    if p.drop_seed_dev:
        R.append(Region("seed_dev", p.drop_seed_dev, 1, 4, 0, 4))
    if p.bnr_y:
        R.append(Region("bnr_y", p.bnr_y, p.M, p.bnr_ldy * 2, p.bnr_coff * 2, p.N * 2))
        for nm in ("bnr_mean", "bnr_invstd", "bnr_scale", "bnr_shift"):
            R.append(Region(nm, getattr(p, nm), 1, p.N * 4, 0, p.N * 4))
    if p.out:
        es = 4 if p.out_f32 else 2
        R.append(Region("out", p.out, p.M, p.ldc * es, p.c_coff * es, p.N * es, write=True))
    if p.outT:
        rows = (p.M // p.T_L) * p.T_E
        for sec in range(-(-p.N // p.T_E)):
            R.append(Region("outT%d" % sec, p.outT + sec * p.T_sec_stride * 2, rows, p.T_Lpad * 2, 0, p.T_L * 2, write=True))
    if p.colsum:
        rows = hip.load().cris_conv_gemm_variant_stat_rows(C.byref(p), v)
        nparts = -(-p.M // rows)
        sld = p.stat_ld or p.N
        R.append(Region("colsum", p.colsum, nparts, sld * 4, 0, p.N * 4, write=True))
        R.append(Region("colsq", p.colsq, nparts, sld * 4, 0, p.N * 4, write=True))
    if p.ws and VARIANTS[v] == "skinny9s":
        nws = int(hip.load().cris_conv_gemm_ws_floats(C.byref(p), v))
        R.append(Region("ws", p.ws, 1, nws * 4, 0, nws * 4, write=True, scratch=True))
    return R


def wgrad_regions(p):
    R = [Region("dY", p.dY, p.M, p.ldy * 2, p.y_coff * 2, p.N_ld * 2),
         Region("X", p.X, p.Bn * p.H * p.W, p.ldx * 2, p.x_coff * 2, p.C * 2),
         Region("dW", p.dW, p.N, p.ldw * 4, 0, p.ldw * 4, write=True)]
    if p.dbias:
        R.append(Region("dbias", p.dbias, 1, p.N * 4, 0, p.N * 4, write=True))
    s = wgrad_effective_splits(p.M, p.splits)
    if s > 1:
        nws = int(hip.load().cris_wgrad_ws_floats(p.M, p.N, p.ldw, p.splits))
        R.append(Region("ws", p.ws, 1, nws * 4, 0, nws * 4, write=True, scratch=True))
    return R


# ---- memory -------------------------------------------------------------------------------------------------------------
class CpuMemory:
    """host memory (CPU tensors' data_ptr()): the CPU tests"""
    device = torch.device("cpu")

    def read(self, lo, n):
        return torch.frombuffer(bytearray(C.string_at(lo, n)), dtype=torch.uint8)

    def extent_ok(self, lo, hi):
        return True

    def sync(self):
        pass


class _CAI:
    def __init__(self, addr, n):
        self.__cuda_array_interface__ = {"data": (addr, False), "shape": (n,), "typestr": "|u1", "version": 2, "strides": None}


class DeviceMemory:
    """device memory of torch's caching allocator: raw-pointer views through __cuda_array_interface__; every extent must lie
    inside ONE live (allocated) block of torch.cuda.memory_snapshot() before anything is read or launched"""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self.blocks = None

    def refresh(self):
        blocks = []
        for seg in torch.cuda.memory_snapshot():
            addr = seg["address"]
            for b in seg["blocks"]:
                if b["state"] == "active_allocated":
                    blocks.append((b.get("address", addr), b.get("address", addr) + b["size"]))
                addr += b["size"]
        blocks.sort()
        self.blocks = blocks

    def extent_ok(self, lo, hi):
        import bisect
        i = bisect.bisect_right(self.blocks, (lo, float("inf"))) - 1
        return i >= 0 and self.blocks[i][0] <= lo and hi <= self.blocks[i][1]

    def read(self, lo, n):
        return torch.as_tensor(_CAI(lo, n), device=self.device).clone()

    def sync(self):
        torch.cuda.synchronize(self.device)


# ---- snapshots ----------------------------------------------------------------------------------------------------------
class Snapshot:
    """copies of byte spans; typed strided views of regions"""

    def __init__(self, mem, spans):
        self.spans = {k: (lo, mem.read(lo, hi - lo)) for k, (lo, hi) in spans.items()}

    def raw(self, key):
        return self.spans[key][1]

    def view(self, key, r: Region, dtype, es, ncols=None):
        lo, buf = self.spans[key]
        off = r.base + r.col0 - lo
        assert off % es == 0 and r.stride % es == 0 and len(buf) % es == 0
        t = buf.view(dtype)
        return torch.as_strided(t, (r.rows, (ncols if ncols is not None else r.width) // es), (r.stride // es, 1), off // es)


def _span(r: Region, full_rows: bool):
    """bytes to copy for a region: a written one from the start of its first row (the declared row span; it ends with the
    last byte the region may write), a read one from its first byte"""
    lo = r.base if full_rows else r.lo
    return lo - lo % 4, r.hi + (-r.hi) % 4


# ---- the reference ------------------------------------------------------------------------------------------------------
def im2col64(Av, g, m0, m1, stride_, pad, dev):
    """float64 im2col rows [m0, m1) of an NHWC input viewed as Av [Bn*H*W, C] -> [rows, KH*KW*C], k = tap*C + c,
    tap = kh*KW + kw"""
    Bn, H, W, Cc, OH, OW, KH, KW = g
    m = torch.arange(m0, m1, device=dev)
    b = m // (OH * OW)
    r = m - b * (OH * OW)
    oh, ow = r // OW, r % OW
    cols = []
    for kh in range(KH):
        for kw in range(KW):
            ih, iw = oh * stride_ - pad + kh, ow * stride_ - pad + kw
            ok = (ih >= 0) & (ih < H) & (iw >= 0) & (iw < W)
            idx = (b * H + ih.clamp(0, H - 1)) * W + iw.clamp(0, W - 1)
            cols.append(Av.index_select(0, idx).to(F64) * ok.unsqueeze(1).to(F64))
    return torch.cat(cols, 1) if len(cols) > 1 else cols[0]


def _chunk_rows(M, K, N, align, budget=1.5e9):
    per = K * 8 * 3 + N * 8 * 10
    r = max(align, int(budget // per) // align * align)
    return min(r, -(-M // align) * align)


@dataclass
class Finding:
    what: str
    row: int
    col: int
    got: float
    ref: float
    bound: float
    tile: tuple

    def __str__(self):
        return "%s at (row %d, col %d) tile %s: got %.6g ref %.6g |err| %.3g > bound %.3g" % (
            self.what, self.row, self.col, self.tile, self.got, self.ref, abs(self.got - self.ref), self.bound)


@dataclass
class ProblemReport:
    label: str
    family: str
    worst: float = 0.0                     # worst err/bound ratio over everything checked
    findings: list = field(default_factory=list)
    elements: int = 0

    def ratio(self, err, bound):
        r = float((err / bound).max()) if err.numel() else 0.0
        self.worst = max(self.worst, r)

    @property
    def ok(self):
        return not self.findings


def _first_bad(bad, m0):
    idx = bad.nonzero()
    i, j = int(idx[0, 0]), int(idx[0, 1])
    return i, j, m0 + i


def _fail(rep, what, bad, got, ref, bound, m0, col_off, tile):
    i, j, row = _first_bad(bad, m0)
    col = j + col_off
    rep.findings.append(Finding(what, row, col, float(got[i, j]), float(ref[i, j]), float(bound[i, j]),
                                (row // tile[0], col // tile[1])))


def check_gemm(p, v, before: Snapshot, after: Snapshot, key, label, dev):
    """key(region) -> snapshot key of the span holding it"""
    regs = {r.name: r for r in gemm_regions(p, v)}
    vname = VARIANTS[v]
    tile = tile_shape(vname, p.M)
    fam = "gemm " + vname
    rep = ProblemReport(label, fam)
    lib = hip.load()
    gam = gamma(gemm_depth(p, v))
    M, N, K = p.M, p.N, p.K
    Av = before.view(key("A"), regs["A"], BF, 2)                           # [Bn*H*W, C]
    W64 = before.view(key("Wt"), regs["Wt"], BF, 2).to(F64)               # [N, K]
    Wabs = W64.abs()
    bias = before.view(key("bias"), regs["bias"], torch.float32, 4).to(F64)[0] if p.bias else None
    res = None
    if p.resid:
        res = before.view(key("resid"), regs["resid"], torch.float32 if p.resid_f32 else BF, 4 if p.resid_f32 else 2)
    drop = p.drop_thresh > 0
    keep = None
    if drop:
        seed = p.drop_seed
        if p.drop_seed_dev:
            seed = (seed + int(before.view(key("seed_dev"), regs["seed_dev"], torch.int32, 4)[0, 0]) % 2 ** 32) % 2 ** 32
        keep = keep_mask_torch(seed, p.drop_stream, M * N, p.drop_thresh / 4294967296.0, dev).view(M, N)
        dscale = 1.0 / (1.0 - float(C.c_float(p.drop_p).value))
    L = (dscale if drop else 1.0) * (1.13 if p.act == 2 else 1.0)
    out_es = 4 if p.out_f32 else 2
    out_dt = torch.float32 if p.out_f32 else BF
    u_out = U32 if p.out_f32 else U_BF16
    got = after.view(key("out"), regs["out"], out_dt, out_es).to(F64) if p.out else None
    stats = bool(p.colsum) and not p.bnr_y
    R = lib.cris_conv_gemm_variant_stat_rows(C.byref(p), v) if p.colsum else 16
    if p.colsum:
        cs_got = after.view(key("colsum"), regs["colsum"], torch.float32, 4).to(F64)
        cq_got = after.view(key("colsq"), regs["colsq"], torch.float32, 4).to(F64)
    if p.bnr_y:
        y_all = before.view(key("bnr_y"), regs["bnr_y"], BF, 2)
        vec = {nm: before.view(key(nm), regs[nm], torch.float32, 4)[0] for nm in ("bnr_mean", "bnr_invstd", "bnr_scale", "bnr_shift")}
    if p.outT:
        Hh = p.T_E // 64
        tv = [after.view(key("outT%d" % s), regs["outT%d" % s], BF, 2) for s in range(-(-N // p.T_E))]
    geo = (p.Bn, p.H, p.W, p.C, p.OH, p.OW, p.KH, p.KW)
    step = _chunk_rows(M, K, N, 128)
    for m0 in range(0, M, step):
        m1 = min(M, m0 + step)
        Acol = im2col64(Av, geo, m0, m1, p.stride, p.pad, dev)
        acc = Acol @ W64.T
        S = Acol.abs() @ Wabs.T
        del Acol
        x = acc + bias if bias is not None else acc.clone()
        mag = acc.abs() + (bias.abs() if bias is not None else 0.0)
        extra = torch.zeros_like(x)
        if p.act == 1:
            x = x.clamp_min(0)
        elif p.act == 2:
            pre = x
            x = pre * torch.sigmoid(1.702 * pre)
            extra = x.abs() * (2.0 ** -18 + 4 * U32 * 1.702 * pre.abs())
        kp = None
        if drop:
            kp = keep[m0:m1]
            x = torch.where(kp, x * dscale, torch.zeros_like(x))
            extra = torch.where(kp, extra * dscale, torch.zeros_like(extra))
        rr = res[m0:m1].to(F64) if res is not None else None
        if rr is not None:
            x = x + rr
        if p.act == 3:
            x = x.clamp_min(0)
        e_x = L * gam * S + extra + 4 * U32 * (L * mag + (rr.abs() if rr is not None else 0.0)) + TINY
        if kp is not None:
            e_x = torch.where(kp, e_x, 4 * U32 * (rr.abs() if rr is not None else 0.0) + TINY)
        ref = x
        rep.elements += ref.numel()
        if got is not None:
            g = got[m0:m1]
            bound = (1 + u_out) * e_x + u_out * ref.abs()         # |fl(x) - ref| <= u |ref| + (1 + u) |x - ref|
            err = (g - ref).abs()
            rep.ratio(err, bound)
            bad = ~(err <= bound)
            if bool(bad.any()):
                _fail(rep, "out", bad, g, ref, bound, m0, 0, tile)
            if kp is not None:
                dropped = (rr if rr is not None else torch.zeros_like(ref))
                if p.act == 3:
                    dropped = dropped.clamp_min(0)
                dropped = dropped.to(out_dt).to(F64)
                wrong = (~kp) & (g != dropped)              # a dropped element must hold exactly the dropped value
                wrong |= kp & (g == dropped) & ((ref - dropped).abs() > bound)
                if bool(wrong.any()):
                    _fail(rep, "dropout decision", wrong, g, ref, bound, m0, 0, tile)
        if p.outT:
            m = torch.arange(m0, m1, device=dev)
            b, l = m // p.T_L, m % p.T_L
            for n0 in range(0, N, p.T_E):
                sec = n0 // p.T_E
                ncol = min(p.T_E, N - n0)
                e = torch.arange(ncol, device=dev)
                h, d = e // 64, e % 64
                rowsT = (b.unsqueeze(1) * Hh + h.unsqueeze(0)) * 64 + d.unsqueeze(0)       # [rows, ncol]
                gT = tv[sec][rowsT, l.unsqueeze(1).expand_as(rowsT)].to(F64)
                refT = ref[:, n0:n0 + ncol]
                bT = (1 + U_BF16) * e_x[:, n0:n0 + ncol] + U_BF16 * refT.abs()
                errT = (gT - refT).abs()
                rep.ratio(errT, bT)
                bad = ~(errT <= bT)
                if bool(bad.any()):
                    _fail(rep, "outT", bad, gT, refT, bT, m0, n0, tile)
        if stats:
            _check_stats(rep, ref, e_x, cs_got, cq_got, m0, m1, R, tile)
        if p.bnr_y:
            _check_bnr(rep, got[m0:m1], y_all[m0:m1].to(F64), vec, cs_got, cq_got, m0, m1, R, tile)
    return rep


def _blocks(t, R, pad_value=0.0):
    """[rows, N] -> [parts, R, N] (rows padded to a multiple of R)"""
    rows = t.shape[0]
    np_ = -(-rows // R)
    if np_ * R != rows:
        t = torch.cat([t, torch.full((np_ * R - rows,) + tuple(t.shape[1:]), pad_value, dtype=t.dtype, device=t.device)])
    return t.view(np_, R, *t.shape[1:])


def _check_stats(rep, x, e, cs_got, cq_got, m0, m1, R, tile):
    """forward partials: row `part` = (sum, M2 about the part mean) of the fp32 epilogue values of rows part*R .. +R"""
    assert m0 % R == 0
    xb, eb = _blocks(x, R), _blocks(e, R)
    cnt = torch.clamp(m1 - m0 - torch.arange(xb.shape[0], device=x.device) * R, max=R).to(F64).view(-1, 1)
    gR = gamma(R + 2)
    s_ref = xb.sum(1)
    s_bound = eb.sum(1) + gR * xb.abs().sum(1) + TINY
    mu = s_ref / cnt
    e_mu = s_bound / cnt + 2 * U32 * mu.abs()
    valid = (torch.arange(R, device=x.device).view(1, R, 1) < cnt.view(-1, 1, 1))
    dlt = torch.where(valid, xb - mu.unsqueeze(1), torch.zeros_like(xb))
    delta = torch.where(valid, eb + e_mu.unsqueeze(1) + U32 * dlt.abs(), torch.zeros_like(eb))
    q_ref = (dlt * dlt).sum(1)
    q_bound = (2 * dlt.abs() * delta + delta * delta).sum(1) + gamma(R + 3) * ((dlt.abs() + delta) ** 2).sum(1) + TINY
    p0, p1 = m0 // R, m0 // R + xb.shape[0]
    N = x.shape[1]
    for nm, gt, rf, bd in (("BN partial sum", cs_got[p0:p1, :N], s_ref, s_bound), ("BN partial M2", cq_got[p0:p1, :N], q_ref, q_bound)):
        err = (gt - rf).abs()
        rep.ratio(err, bd)
        bad = ~(err <= bd)
        if bool(bad.any()):
            i, j = [int(v) for v in bad.nonzero()[0]]
            part = p0 + i
            rep.findings.append(Finding(nm + " (part %d = rows %d..%d)" % (part, part * R, part * R + R - 1), part * R, j,
                                        float(gt[i, j]), float(rf[i, j]), float(bd[i, j]), (part * R // tile[0], j // tile[1])))


def _check_bnr(rep, dz, y, vec, cs_got, cq_got, m0, m1, R, tile):
    """backward partials from the STORED gradient dz: (sum g, sum g * xhat), g = dz where scale*y + shift > 0"""
    assert m0 % R == 0
    sc, sh = vec["bnr_scale"].to(F64), vec["bnr_shift"].to(F64)
    mean, inv = vec["bnr_mean"].to(F64), vec["bnr_invstd"].to(F64)
    z = y * sc + sh
    amb = z.abs() <= 2 * U32 * ((y * sc).abs() + sh.abs())            # fp32 may decide either way
    g = torch.where(z > 0, dz, torch.zeros_like(dz))
    xhat = (y - mean) * inv
    gx = g * xhat
    gb, gxb = _blocks(g, R), _blocks(gx, R)
    ab = _blocks(amb.to(F64) * dz.abs(), R)
    abx = _blocks(amb.to(F64) * (dz * xhat).abs(), R)
    gR = gamma(R + 2)
    s0, s1 = gb.sum(1), gxb.sum(1)
    b0 = gR * gb.abs().sum(1) + ab.sum(1) + TINY
    b1 = (gR + 3 * U32) * gxb.abs().sum(1) + 4 * U32 * (gb.abs() * _blocks((y - mean).abs() * inv + mean.abs() * inv, R)).sum(1) \
        + abx.sum(1) + TINY
    p0, p1 = m0 // R, m0 // R + gb.shape[0]
    N = dz.shape[1]
    for nm, gt, rf, bd in (("bnr sum g", cs_got[p0:p1, :N], s0, b0), ("bnr sum g*xhat", cq_got[p0:p1, :N], s1, b1)):
        err = (gt - rf).abs()
        rep.ratio(err, bd)
        bad = ~(err <= bd)
        if bool(bad.any()):
            i, j = [int(v) for v in bad.nonzero()[0]]
            part = p0 + i
            rep.findings.append(Finding(nm + " (part %d)" % part, part * R, j, float(gt[i, j]), float(rf[i, j]), float(bd[i, j]),
                                        (part * R // tile[0], j // tile[1])))


def check_wgrad(p, before: Snapshot, after: Snapshot, key, label, dev):
    regs = {r.name: r for r in wgrad_regions(p)}
    tsz = hip.load().cris_conv_wgrad_tile(C.byref(p))
    rep = ProblemReport(label, "wgrad %d" % tsz)
    tile = (tsz, tsz)
    dY = before.view(key("dY"), regs["dY"], BF, 2, ncols=p.N * 2)
    Xv = before.view(key("X"), regs["X"], BF, 2)
    geo = (p.Bn, p.H, p.W, p.C, p.OH, p.OW, p.KH, p.KW)
    ref = torch.zeros(p.N, p.K, dtype=F64, device=dev)
    S = torch.zeros_like(ref)
    db = torch.zeros(p.N, dtype=F64, device=dev)
    dbS = torch.zeros_like(db)
    step = _chunk_rows(p.M, p.K, 0, 128)
    for m0 in range(0, p.M, step):
        m1 = min(p.M, m0 + step)
        Xc = im2col64(Xv, geo, m0, m1, p.stride, p.pad, dev)
        Yc = dY[m0:m1].to(F64)
        ref += Yc.T @ Xc
        S += Yc.abs().T @ Xc.abs()
        db += Yc.sum(0)
        dbS += Yc.abs().sum(0)
        del Xc
    got_all = after.view(key("dW"), regs["dW"], torch.float32, 4).to(F64)
    got = got_all[:, :p.K]
    bound = gamma(wgrad_depth(p)) * S + U32 * ref.abs() + TINY
    err = (got - ref).abs()
    rep.ratio(err, bound)
    rep.elements = ref.numel()
    bad = ~(err <= bound)
    if bool(bad.any()):
        _fail(rep, "dW", bad, got, ref, bound, 0, 0, tile)
    if p.ldw > p.K:
        padv = got_all[:, p.K:]
        bad = padv != 0
        if bool(bad.any()):
            _fail(rep, "dW padding column (must be 0)", bad, padv, torch.zeros_like(padv), torch.zeros_like(padv), 0, p.K, tile)
    if p.dbias:
        g = after.view(key("dbias"), regs["dbias"], torch.float32, 4)[0].to(F64)
        bd = gamma(wgrad_bias_depth(p)) * dbS + U32 * db.abs() + TINY
        e = (g - db).abs()
        rep.ratio(e, bd)
        bad = ~(e <= bd)
        if bool(bad.any()):
            j = int(bad.nonzero()[0, 0])
            rep.findings.append(Finding("dbias", 0, j, float(g[j]), float(db[j]), float(bd[j]), (j // tsz, 0)))
    return rep


# ---- one launch ---------------------------------------------------------------------------------------------------------
def _obj(a):
    return getattr(a, "_obj", a)


def _copy(st):
    return type(st).from_buffer_copy(bytes(memoryview(st)))


@dataclass
class LaunchReport:
    fn: str
    tag: str
    problems: list
    kinds: set
    footprint: list

    @property
    def ok(self):
        return not self.footprint and all(r.ok for r in self.problems)

    def worst(self):
        return max([r.worst for r in self.problems] + [0.0])

    def describe(self):
        lines = ["%s [%s]: worst err/bound %.3g" % (self.fn, self.tag, self.worst())]
        for r in self.problems:
            for f in r.findings[:3]:
                lines.append("  %s (%s): %s" % (r.label, r.family, f))
        lines += ["  footprint: " + s for s in self.footprint[:3]]
        return "\n".join(lines)


class Auditor:
    """Has the signature of ops.KernelTimer.launch: install as ops.KERNEL_TIMER.  execute(fn, args) performs the launch
    (the GPU: hip.call on the current stream; the CPU tests: an emulation)."""

    def __init__(self, mem, execute, raise_on_failure=True):
        self.mem, self.execute = mem, execute
        self.raise_on_failure = raise_on_failure
        self.reports = []

    def launch(self, name, flops, nbytes, fn, *args, tag="", tile=False):
        lib = hip.load()
        a0 = _obj(args[0])
        probs = []                                   # ("gemm", params, resolved variant) / ("wgrad", params)
        kinds = set()
        if fn == "cris_conv_gemm_variant":
            p = _copy(a0)
            v = lib.cris_conv_gemm_plan(C.byref(p), int(args[1]), None)
            if int(args[1]) < 0 and VARIANTS[v] == "skinny9s" and not p.ws:
                v = VARIANTS.index("skinny9")
            probs.append(("gemm", p, v))
            kinds.add("solo tile" if not VARIANTS[v].startswith("skinny") else "solo skinny")
        elif fn == "cris_conv_gemm_group_launch":
            g = _copy(a0)
            v = int(args[1])
            for i in range(g.n):
                probs.append(("gemm", _copy(g.prob[i]), v))
            kinds.add(("8-wave group" if VARIANTS[v].startswith("8w") else "4-wave group") if g.n > 1 else "solo tile")
        elif fn == "cris_conv_wgrad":
            p = _copy(a0)
            probs.append(("wgrad", p, None))
        elif fn == "cris_conv_wgrad_group":
            g = _copy(a0)
            for i in range(g.n):
                probs.append(("wgrad", _copy(g.prob[i]), None))
            kinds.add("grouped wgrad")
        else:
            raise AuditError("unaudited launch %s" % fn)
        regions = []
        for i, (kind, p, v) in enumerate(probs):
            if kind == "gemm":
                if v < 0:
                    raise AuditError("%s: no tile variant can run problem %d (%s)" % (fn, i, tag))
                regions.append(gemm_regions(p, v))
                vn = VARIANTS[v]
                kinds.add("variant " + vn)
                if vn == "skinny9s" and p.ws:
                    kinds.add("skinny split-K with workspace")
                if p.out and p.out_f32:
                    kinds.add("f32 output")
                if p.resid:
                    kinds.add("f32 residual" if p.resid_f32 else "bf16 residual")
                if p.drop_thresh:
                    kinds.add("dropout")
                if p.outT:
                    kinds.add("outT")
                if p.colsum and not p.bnr_y:
                    kinds.add("BN partials")
                if p.bnr_y:
                    kinds.add("bnr partials")
                if p.out and p.ldc > p.N:
                    kinds.add("sliced output")
                if p.a_coff > 0:
                    kinds.add("offset input")
            else:
                regions.append(wgrad_regions(p))
                if wgrad_effective_splits(p.M, p.splits) > 1:
                    kinds.add("split wgrad")
                if p.dbias:
                    kinds.add("dbias")
        # 1. every declared extent inside one live allocation - before anything is read or launched
        if hasattr(self.mem, "refresh"):
            self.mem.refresh()
        for i, regs in enumerate(regions):
            for r in regs:
                if not self.mem.extent_ok(r.lo, r.hi):
                    raise AuditError("%s [%s] problem %d: %s extent [%#x, %#x) is not inside one live allocation - not launched"
                                     % (fn, tag, i, r.name, r.lo, r.hi))
        # 2. group independence
        foot = []
        for i in range(len(regions)):
            for j in range(len(regions)):
                if i == j:
                    continue
                for w in regions[i]:
                    if not w.write:
                        continue
                    for o in regions[j]:
                        if regions_intersect(w, o):
                            foot.append("problem %d writes %s, which intersects %s of problem %d" % (i, w.name, o.name, j))
        if foot:
            rep = LaunchReport(fn, tag, [], kinds, foot)
            self._record(rep)
            return
        # 3. snapshots, launch, snapshots
        spans, keys = {}, []
        for i, regs in enumerate(regions):
            km = {}
            for r in regs:
                if r.scratch:
                    continue
                full = r.write and self.mem.extent_ok(r.base, r.hi)
                k = (i, r.name)
                spans[k] = _span(r, full)
                km[r.name] = k
            keys.append(km)
        self.mem.sync()
        before = Snapshot(self.mem, spans)
        self.execute(fn, args)
        self.mem.sync()
        after = Snapshot(self.mem, {k: s for k, s in spans.items() if any(r.name == k[1] and r.write for r in regions[k[0]])})
        # 4. footprint: bytes of the write spans outside every region a problem may write are unchanged
        for k, (lo, buf) in after.spans.items():
            allowed = torch.zeros(len(buf), dtype=torch.bool, device=buf.device)
            for regs in regions:
                for r in regs:
                    if r.write and not (r.hi <= lo or lo + len(buf) <= r.lo):
                        _mark(allowed, r, lo)
            changed = (buf != before.spans[k][1]) & ~allowed
            if bool(changed.any()):
                off = int(changed.nonzero()[0, 0])
                r = next(r for r in regions[k[0]] if r.name == k[1])
                row, col = divmod(lo + off - r.base, r.stride)
                foot.append("%s of problem %d: byte (row %d, byte column %d) outside the declared write range changed"
                            % (r.name, k[0], row, col))
        reps = []
        for i, (kind, p, v) in enumerate(probs):
            lab = "%s#%d" % (tag, i)
            key = (lambda name, km=keys[i]: km[name])
            if kind == "gemm":
                reps.append(check_gemm(p, v, before, after, key, lab, self.mem.device))
            else:
                reps.append(check_wgrad(p, before, after, key, lab, self.mem.device))
        self._record(LaunchReport(fn, tag, reps, kinds, foot))

    def _record(self, rep):
        self.reports.append(rep)
        if self.raise_on_failure and not rep.ok:
            raise AuditError(rep.describe())


def _mark(allowed, r: Region, lo):
    """allowed[byte - lo] = True for every byte of region r inside the buffer"""
    n = len(allowed)
    start = r.base + r.col0 - lo
    if r.rows == 1 or r.width <= r.stride:
        if start >= 0 and start + (r.rows - 1) * r.stride + r.width <= n:
            torch.as_strided(allowed, (r.rows, r.width), (r.stride, 1), start).fill_(True)
            return
    for row in range(r.rows):
        a = start + row * r.stride
        allowed[max(a, 0):max(min(a + r.width, n), 0)] = True
