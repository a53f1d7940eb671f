"""Case tables, float64 references and per-element bounds shared by tests/test_hip_ops_edges.py (the HIP kernels on the GPU)
and tests/test_hip_ops_edges_cpu.py (the same bounds against a plain torch fp32 evaluation, no GPU).

Every linear op is stated once, as a function of a dtype: evaluated in float64 it is the reference, evaluated in float32 (and
rounded once to bf16 where the kernel rounds) it is the "correct fp32 implementation" the CPU file holds against the bound, and
evaluated in float64 on the absolute values of inputs and weights it is the scale S of the bound

    |got - ref| <= REL * |ref| + ABS * S        REL = 2^-8 for a bf16 result (half a bf16 ulp of rounding + a float64
                                                reference next to a rounding tie), 0 for an fp32 result;
                                                ABS = 2^-20 (16 fp32 roundings), 2^-24 * terms above 16 accumulated terms.
"""
import numpy as np
import torch
import torch.nn.functional as F

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64

# guard fills: finite bit patterns far outside anything a case computes (1.1e36 in either format); compared as integers
GUARD_BITS = {BF: 0x7B5A, F32: 0x7B5A5A5A, torch.int32: 0x5A5A5A5A, torch.uint8: 0x5A}
_INT_OF = {BF: torch.int16, F32: torch.int32, torch.int32: torch.int32, torch.uint8: torch.uint8}
NAN = float("nan")

REL_BF16 = 2.0 ** -8
ABS_F32 = 2.0 ** -20

GRID_ITEMS = 8192 * 256           # work items of one trip of a capped grid-stride launch
FAST_DIV_LIMIT = 1 << 24          # cris_split4: reciprocal division below, 64-bit division from here


def abs_coef(terms):
    return ABS_F32 if terms <= 16 else terms * 2.0 ** -24


def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def randn_bf(shape, seed, scale=1.0):
    """N(0, scale) rounded to bf16, returned as float32 (exactly representable in bf16)"""
    return (torch.randn(*shape, generator=gen(seed)) * scale).to(BF).float()


def randn_f32(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=gen(seed)) * scale


# ----------------------------------------------------------------------------------------------------
# guarded buffers
# ----------------------------------------------------------------------------------------------------
class Slab:
    """M rows of C live columns at [coff, coff + C) of a [pre + M + post][ld] buffer.  As an OUTPUT the rest holds GUARD_BITS and
    must still hold them after the launch; as an INPUT (nan_guard) the rest holds NaN, so that a read outside the slice poisons
    what it feeds.  `rows` is what the kernel gets (its first element is row 0, column 0)."""

    def __init__(self, M, C, dtype, device, ld=None, coff=0, nan_guard=False, pre=2, post=2):
        ld = C if ld is None else ld
        assert 0 <= coff and coff + C <= ld
        self.M, self.C, self.ld, self.coff, self.dtype = M, C, ld, coff, dtype
        if nan_guard:
            self.full = torch.full((pre + M + post, ld), NAN, dtype=dtype, device=device)
        else:
            bits = GUARD_BITS[dtype]
            it = _INT_OF[dtype]
            if it == torch.int16 and bits >= 1 << 15:
                bits -= 1 << 16
            self.full = torch.full((pre + M + post, ld), bits, dtype=it, device=device).view(dtype)
        self.nan_guard = nan_guard
        self.rows = self.full[pre:pre + M]
        self.data = self.rows[:, coff:coff + C]
        live = torch.zeros(pre + M + post, ld, dtype=torch.bool, device=device)
        live[pre:pre + M, coff:coff + C] = True
        self._guard = ~live

    def set(self, values):
        self.data.copy_(values.reshape(self.M, self.C).to(self.data.device))
        return self

    def get(self):
        """the live slice as a CPU tensor [M][C]"""
        return self.data.detach().cpu().clone()

    def assert_guards(self, what=""):
        assert not self.nan_guard
        it = _INT_OF[self.dtype]
        raw = self.full.view(it)[self._guard]
        want = GUARD_BITS[self.dtype]
        if it == torch.int16 and want >= 1 << 15:
            want -= 1 << 16
        bad = (raw != want).nonzero().flatten()
        assert bad.numel() == 0, "%s: %d guard elements overwritten (first: guard element %d of %d)" % (
            what, bad.numel(), int(bad[0]), raw.numel())


def bits_equal(a, b):
    """bit identity of two tensors of one dtype (NaN == NaN, -0 != +0)"""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    it = _INT_OF.get(a.dtype)
    if it is None or it == a.dtype:
        return bool(torch.equal(a, b))
    return bool(torch.equal(a.contiguous().view(it), b.contiguous().view(it)))


def first_bad(bad, dims=None, names=None):
    """description of the first True of a boolean tensor: flat index and its coordinates over `dims`"""
    idx = int(bad.flatten().nonzero()[0])
    dims = tuple(bad.shape) if dims is None else tuple(dims)
    coord = np.unravel_index(idx, dims)
    names = names or ["i%d" % k for k in range(len(dims))]
    return "flat index %d = (%s)" % (idx, ", ".join("%s=%d" % (n, int(c)) for n, c in zip(names, coord)))


def assert_exact(got, ref, what="", dims=None, names=None):
    assert got.shape == ref.shape and got.dtype == ref.dtype, "%s: shape/dtype %s %s vs %s %s" % (what, got.shape, got.dtype, ref.shape, ref.dtype)
    if bits_equal(got, ref):
        return
    it = _INT_OF.get(got.dtype, got.dtype)
    bad = got.contiguous().view(it) != ref.contiguous().view(it)
    i = int(bad.flatten().nonzero()[0])
    assert False, "%s: %d elements differ; first at %s: got %r, expected %r" % (
        what, int(bad.sum()), first_bad(bad, dims, names), got.flatten()[i].item(), ref.flatten()[i].item())


def assert_bound(got, ref, S, rel, ab, what="", dims=None, names=None):
    """|got - ref| <= rel * |ref| + ab * S for every element (got: any float dtype; ref, S: float64 or, on the device, float32)"""
    g = got.to(ref.dtype)
    assert g.shape == ref.shape == S.shape, "%s: shapes %s %s %s" % (what, g.shape, ref.shape, S.shape)
    err = (g - ref).abs()
    lim = rel * ref.abs() + ab * S
    bad = ~(err <= lim)                              # NaN fails
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        assert False, "%s: %d of %d elements out of bound; first at %s: got %.9g, reference %.9g, |error| %.3e > %.3e" % (
            what, int(bad.sum()), bad.numel(), first_bad(bad, dims, names), float(g.flatten()[i]), float(ref.flatten()[i]),
            float(err.flatten()[i]), float(lim.flatten()[i]))


def chunk_relerr(got, ref, chunk=2048):
    """relative L2 error of every contiguous chunk of `chunk` elements (the ragged last chunk is its own chunk)"""
    g, r = got.double().flatten().cpu(), ref.double().flatten().cpu()
    out = []
    for i in range(0, r.numel(), chunk):
        d, n = (g[i:i + chunk] - r[i:i + chunk]).norm(), r[i:i + chunk].norm()
        out.append(float(d / (n + 1e-30)))
    return out


def assert_chunks(got, ref, tol, what="", chunk=2048):
    errs = chunk_relerr(got, ref, chunk)
    worst = max(range(len(errs)), key=lambda i: errs[i] if np.isfinite(errs[i]) else np.inf)
    print("%s: worst chunk %d of %d rel L2 %.3e (tol %.1e)" % (what, worst, len(errs), errs[worst], tol))
    assert all(np.isfinite(e) and e <= tol for e in errs), "%s: chunk %d (elements %d..) rel L2 err %.3e > %.1e" % (
        what, worst, worst * chunk, errs[worst], tol)


def assert_rows(got, ref, tol, what=""):
    """relative L2 error of every row of [rows][C]"""
    g, r = got.double().cpu(), ref.double().cpu()
    e = (g - r).norm(dim=1) / (r.norm(dim=1) + 1e-30)
    bad = ~(e <= tol)
    worst = int(torch.nan_to_num(e, nan=float("inf")).argmax())
    print("%s: worst row %d of %d rel L2 %.3e (tol %.1e)" % (what, worst, e.numel(), float(e[worst]), tol))
    assert not bool(bad.any()), "%s: %d rows out of tolerance; row %d rel L2 err %.3e > %.1e" % (what, int(bad.sum()), worst, float(e[worst]), tol)


# ----------------------------------------------------------------------------------------------------
# linear ops: one statement each, evaluated at a dtype.  Activations are NHWC: [B][H][W][C].
# ----------------------------------------------------------------------------------------------------
def avgpool2_fwd(x, dt):
    B, H, W, C = x.shape
    return x.to(dt).view(B, H // 2, 2, W // 2, 2, C).sum((2, 4)) * 0.25


def avgpool2_bwd(dy, old, dt):
    """dx = (old +) 0.25 * dy of the pooled pixel; old: None without accumulation"""
    B, OH, OW, C = dy.shape
    g = (dy.to(dt) * 0.25).view(B, OH, 1, OW, 1, C).expand(B, OH, 2, OW, 2, C).reshape(B, 2 * OH, 2 * OW, C)
    return g if old is None else old.to(dt) + g


def upsample2_fwd(x, dt):
    """x2 bilinear, align_corners=False (torch's own statement of it)"""
    return F.interpolate(x.to(dt).permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1).contiguous()


def upsample2_bwd(dy, old, dt):
    """gradient of upsample2_fwd (through autograd: the transpose of the same linear map); old: None without accumulation"""
    B, OH, OW, C = dy.shape
    x = torch.zeros(B, OH // 2, OW // 2, C, dtype=dt, requires_grad=True)
    (upsample2_fwd(x, dt) * dy.to(dt)).sum().backward()
    return x.grad if old is None else old.to(dt) + x.grad


def add2(a, b, dt):
    return a.to(dt) if b is None else a.to(dt) + b.to(dt)


def add_rowtable(a, table, dt):
    M, trows = a.shape[0], table.shape[0]
    return a.to(dt) + table.to(dt).repeat((M + trows - 1) // trows, 1)[:M]


def batch_rowsum(x, dt):
    """x [B][T][C] -> [T][C]"""
    return x.to(dt).sum(0)


def colstats(x, rows_per_part, dt):
    """x [M][C] -> (sum [parts][C], centred second moment about the part mean [parts][C])"""
    x = x.to(dt)
    s, q = [], []
    for r0 in range(0, x.shape[0], rows_per_part):
        p = x[r0:r0 + rows_per_part]
        s.append(p.sum(0))
        q.append(((p - p.mean(0)) ** 2).sum(0))
    return torch.stack(s), torch.stack(q)


def colstats_scale(x, rows_per_part):
    """S of colstats: sums of |x|; for the second moment every term (x - mean)^2 carries the roundings of x - mean, relative to
    |x| + |mean|, twice (squared), so its scale is sum (|x| + mean|x|)^2 - the statement on absolute values with the
    subtraction, whose operands both round, taken as an addition."""
    a = x.double().abs()
    s, q = [], []
    for r0 in range(0, a.shape[0], rows_per_part):
        p = a[r0:r0 + rows_per_part]
        s.append(p.sum(0))
        q.append(((p + p.mean(0)) ** 2).sum(0))
    return torch.stack(s), torch.stack(q)


def axpy(dst, src, alpha, dt):
    return dst.to(dt) + torch.tensor(alpha, dtype=F32).to(dt) * src.to(dt)


def embed_bwd(tokens, dx, V, P, dt):
    """tokens [B][L], dx [B*L][D] -> (dtable [V][D] rows of the batch's tokens, dpos [P][D] rows < L), and the touched-row masks"""
    B, L = tokens.shape
    D = dx.shape[1]
    dtab = torch.zeros(V, D, dtype=dt).index_add_(0, tokens.flatten(), dx.to(dt))
    dpos = torch.zeros(P, D, dtype=dt)
    dpos[:L] = dx.to(dt).view(B, L, D).sum(0)
    return dtab, dpos


def posresize_fwd(R, pos, dt):
    """R [T][GG], pos [1 + GG][C] (row 0: the class token, not resized)"""
    return R.to(dt) @ pos[1:].to(dt)


def posresize_bwd(R, dposr, old, dt):
    """dpos[1:] += R^T dposr; row 0 untouched"""
    out = old.to(dt).clone()
    out[1:] += R.to(dt).t() @ dposr.to(dt)
    return out


def to_result(v, bf16_result):
    """what a correct fp32 implementation hands back: one rounding to bf16 where the kernel stores bf16"""
    return v.to(BF).double() if bf16_result else v.double()


# ----------------------------------------------------------------------------------------------------
# case tables
# ----------------------------------------------------------------------------------------------------
HW_A = [(2, 2), (4, 6), (6, 10)]
C_A = [8, 24, 40]                                  # CV = 1, 3 (the plain-division divisor), 5
HW_UP_EXTRA = [(1, 1), (1, 5), (3, 3)]             # clamped taps; divisors 1 and 3
B_A, LD_PAD, COFF = 2, 16, 8                        # ld = C + 16, coff = 8 on every operand that has the parameters

POOL_CASES = [(H, W, C) for (H, W) in HW_A for C in C_A]
UP_CASES = POOL_CASES + [(H, W, C) for (H, W) in HW_UP_EXTRA for C in (8, 24)]
ADD_FORMS = ["copy", "sliced", "alias", "mixed_ld"]
ADD_SHAPES = [(7, 8), (30, 24), (33, 40)]
ROWTABLE_CASES = [(30, 24, 7), (5, 8, 6), (33, 40, 4)]          # (M, C, trows): M not a multiple of trows; trows > M
ROWSUM_CASES = [(3, 7, 24), (1, 5, 8), (5, 9, 40)]              # (B, T, C)
COLSTATS_CASES = [(37, 24, 8), (5, 8, 16), (33, 40, 4)]         # (M, C, rows_per_part): ragged last part; one short part
TAIL_N = [1, 255, 257]
POSRESIZE_CASES = [(3, 5, 4, 24), (2, 3, 3, 8)]                 # (G, H, W, C): T = H*W rows


def linear_cases():
    """(id, bf16_result, terms, build) for every linear-op case of groups A and B; build() -> (eval(dt), eval_abs()) where
    eval(dt) is the op at dtype dt and eval_abs() its float64 value on absolute inputs.  Tuple results are compared leaf by leaf."""
    out = []

    def add(name, bf16_result, terms, ev, ev_abs):
        out.append((name, bf16_result, terms, ev, ev_abs))

    for (H, W, C) in POOL_CASES:
        x = randn_bf((B_A, H, W, C), 11)
        add("avgpool2_fwd-%dx%dx%d" % (H, W, C), True, 4, lambda dt, x=x: avgpool2_fwd(x, dt), lambda x=x: avgpool2_fwd(x.abs(), F64))
        dy = randn_bf((B_A, H // 2, W // 2, C), 12)
        old = randn_bf((B_A, H, W, C), 13)
        add("avgpool2_bwd-accum-%dx%dx%d" % (H, W, C), True, 2, lambda dt, dy=dy, old=old: avgpool2_bwd(dy, old, dt),
            lambda dy=dy, old=old: avgpool2_bwd(dy.abs(), old.abs(), F64))
    for (H, W, C) in UP_CASES:
        x = randn_bf((B_A, H, W, C), 14)
        add("upsample2_fwd-%dx%dx%d" % (H, W, C), True, 4, lambda dt, x=x: upsample2_fwd(x, dt), lambda x=x: upsample2_fwd(x.abs(), F64))
        dy = randn_bf((B_A, 2 * H, 2 * W, C), 15)
        old = randn_bf((B_A, H, W, C), 16)
        for accum in (False, True):
            o = old if accum else None
            add("upsample2_bwd-%s-%dx%dx%d" % ("accum" if accum else "store", H, W, C), True, 10,
                lambda dt, dy=dy, o=o: upsample2_bwd(dy, o, dt),
                lambda dy=dy, o=o: upsample2_bwd(dy.abs(), None if o is None else o.abs(), F64))
    for (M, C) in ADD_SHAPES:
        a, b = randn_bf((M, C), 17), randn_bf((M, C), 18)
        add("add_bf16-%dx%d" % (M, C), True, 2, lambda dt, a=a, b=b: add2(a, b, dt), lambda a=a, b=b: add2(a.abs(), b.abs(), F64))
    for (M, C, trows) in ROWTABLE_CASES:
        a, t = randn_bf((M, C), 19), randn_f32((trows, C), 20)
        add("add_rowtable-%dx%d-t%d" % (M, C, trows), True, 2, lambda dt, a=a, t=t: add_rowtable(a, t, dt),
            lambda a=a, t=t: add_rowtable(a.abs(), t.abs(), F64))
    for (B, T, C) in ROWSUM_CASES:
        x = randn_bf((B, T, C), 21)
        add("batch_rowsum-%dx%dx%d" % (B, T, C), False, B, lambda dt, x=x: batch_rowsum(x, dt), lambda x=x: batch_rowsum(x.abs(), F64))
    for (M, C, rpp) in COLSTATS_CASES:
        x = randn_bf((M, C), 22) + 0.5
        x = x.to(BF).float()
        add("colstats-%dx%d-r%d" % (M, C, rpp), False, rpp, lambda dt, x=x, rpp=rpp: colstats(x, rpp, dt),
            lambda x=x, rpp=rpp: colstats_scale(x, rpp))
    for n in TAIL_N:
        x, old = randn_bf((n,), 23), randn_f32((n,), 24)
        add("cast_bf16_f32-accum-%d" % n, False, 2, lambda dt, x=x, old=old: add2(old, x, dt), lambda x=x, old=old: add2(old.abs(), x.abs(), F64))
        d, s = randn_f32((n,), 25), randn_f32((n,), 26)
        add("axpy_f32-%d" % n, False, 2, lambda dt, d=d, s=s: axpy(d, s, 0.37, dt), lambda d=d, s=s: axpy(d.abs(), s.abs(), 0.37, F64))
    for (G, H, W, C) in POSRESIZE_CASES:
        from cris.pytorch_amd.tables import bicubic_resize_matrix
        R = torch.from_numpy(bicubic_resize_matrix(G, H, W)).float()
        pos, d, old = randn_f32((G * G + 1, C), 27), randn_f32((H * W, C), 28), randn_f32((G * G + 1, C), 29)
        add("posresize_fwd-g%d-%dx%dx%d" % (G, H, W, C), False, G * G, lambda dt, R=R, pos=pos: posresize_fwd(R, pos, dt),
            lambda R=R, pos=pos: posresize_fwd(R.abs(), pos.abs(), F64))
        add("posresize_bwd-g%d-%dx%dx%d" % (G, H, W, C), False, H * W + 1, lambda dt, R=R, d=d, old=old: posresize_bwd(R, d, old, dt),
            lambda R=R, d=d, old=old: posresize_bwd(R.abs(), d.abs(), old.abs(), F64))
    toks, dx = EMBED_TOKENS, randn_f32((EMBED_TOKENS.numel(), EMBED_D), 30)
    add("embed_bwd", False, EMBED_TOKENS.numel(), lambda dt: embed_bwd(toks, dx, EMBED_V, EMBED_P, dt),
        lambda: embed_bwd(toks, dx.abs(), EMBED_V, EMBED_P, F64))
    return out


# a token repeated across rows (40 at position 0 of every row; 7) and within a row (5 twice in row 0, 0 as padding)
EMBED_TOKENS = torch.tensor([[40, 5, 7, 5, 49, 0, 0], [40, 3, 49, 0, 0, 0, 0], [40, 7, 2, 3, 4, 5, 49]])
EMBED_V, EMBED_P, EMBED_D = 50, 9, 24

# group C: (kernel, shape, work items) - the smallest shapes that reach each index path
STRIDE2_CASES = {                                   # second grid-stride trip, ragged: GRID_ITEMS < items < 2 * GRID_ITEMS
    "avgpool2_fwd": (dict(B=3, H=1190, W=1186, C=16), 3 * 595 * 593 * 2),
    "add_bf16": (dict(M=262500, C=64), 262500 * 8),
    "cast_f32_bf16_drop": (dict(n=GRID_ITEMS + 1000), GRID_ITEMS + 1000),
}
RCP_TOP_CASES = {                                   # top of the reciprocal-division range: [2^24 - 4096, 2^24)
    "avgpool2_bwd": (dict(B=1, H=1446, W=1450, C=64), 1446 * 1450 * 8),
    "upsample2_fwd": (dict(B=1, H=724, W=724, C=64), 1448 * 1448 * 8),
    "stem_im2col": (dict(B=1, H=4094, W=4098), 2047 * 2049 * 4),          # 4 below 2^24
}
# the square stem shape next to it: 16,760,836 items, 16,380 below 2^24 - under the window above, still in the reciprocal range
STEM_SQUARE_CASE = (dict(B=1, H=4094, W=4094), 2047 * 2047 * 4)
DIV64_CASES = {                                     # 64-bit division branch: >= 2^24
    "avgpool2_bwd": (dict(B=1, H=1450, W=1450, C=64), 1450 * 1450 * 8),
    "upsample2_fwd": (dict(B=1, H=725, W=725, C=64), 1450 * 1450 * 8),
}

# LayerNorm: (C, rows).  C: 1, 3, 64+1, 128+1, 192+1 live lanes and one lane short of full; rows: one wave, a few, the backward
# grid cap (512 blocks x 4 waves) + 1, the forward cap (2048 x 4) + 1
LN_CASES = [(C, 5) for C in (8, 24, 520, 1032, 1544, 2040)] + [(C, r) for C in (24, 520) for r in (1, 2049, 8193)]
LN_POS_ROWS = 4                                     # divides none of the row counts 1, 5, 2049, 8193
