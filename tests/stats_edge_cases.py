"""Case tables, float64 references, derived bounds and fp32 emulations for the per-element audit of three kernel groups that run in
every training step: the fp32 sentence-vector kernels of csrc/smallf32.hip, the BatchNorm statistics kernels of csrc/norm.hip
(cris_bn_finalize with its three merge paths, cris_bn_sync_pack / _unpack, cris_bn_eval_coeffs) and cris_sum_tables.
tests/test_stats_edges.py runs the HIP launchers through these checks on the GPU, tests/test_stats_edges_cpu.py the emulations
below (one that follows each kernel's summation structure, one plain sequential, and the same made wrong in one named way).
No GPU and no `hip` import in here.

Every buffer is a guarded slab (tests/hip_ops_edge_cases.py): outputs lie in guard bits that must survive the launch, inputs lie
in NaN and must be bit-identical afterwards.  A launcher - or an emulation - gets a dict of slabs from `build(case, device)` and
writes its outputs into them; `check(case, slabs, before)` then holds every element against float64 of the given inputs:

    |got - ref| <= rel * |ref| + t * 2^-24 * S

S is the same expression on absolute values, t the length of the LONGEST CHAIN OF ROUNDINGS that reaches one output, read off the
kernel's structure (for a reduction the depth of its tree: entries per lane + lanes + levels - never the number of summands), plus
one for the second-order terms of (1 + 2^-24)^t.  Where a value is copied, masked or computed on grid inputs: bit equality.
"""
import numpy as np
import torch

from hip_ops_edge_cases import BF, F32, F64, NAN, REL_BF16, Slab, assert_bound, assert_exact, bits_equal, gen

U = 2.0 ** -24
I32 = torch.int32
f32, f64 = np.float32, np.float64

# ---- the kernels' dispatch constants, stated independently (tests/test_stats_edges_cpu.py compares them with the sources) --------
SMALL_MAX_ROWS = 16               # CRIS_SMALL_MAX_ROWS: rows of every smallf32 kernel
LR_LANES, LR_COLS_PER_BLOCK = 64, 4   # linear_rows_kernel: one wave per output column, lanes stride K; four columns per block
LC_COLS, LC_KG, LC_INFLIGHT = 16, 16, 8   # linear_cols_kernel: 16 columns x 16 k-groups, eight rows of W in flight (128 k per trip)
SMALL_BLOCK = 256                 # outer_sum / colstats / bn_relu / eot kernels: 256 threads over the columns
BN_WIDE_MIN, BN_MERGE_MIN, BN_MERGE_SLICES = 128, 512, 64
BN_CH, BN_REGS, BN_MERGE_REGS = 16, 8, 4   # channels per block; register entries per lane of bn_finalize_kernel / bn_merge_kernel
SUM_COLS, SUM_PARTLANES, SUM_GROUP_MAX = 64, 4, 64
RSQRT_ULPS = 2                    # margin for rsqrtf itself: 2 ulp (= 4 * 2^-24 relative).  HIP documents 1 ulp for rsqrtf; the
                                  # emulation's float32 rsqrt measures <= 1 ulp against float64 (test_rsqrt_margin)
EPS = 1e-5


def partials_rows(nparts):
    """rows of a partials table (cris_bn_partials_rows): the first-level merge writes its slices behind the parts"""
    return nparts + BN_MERGE_SLICES if nparts > BN_MERGE_MIN else nparts


def bn_path(nparts):
    """(PL of the finalize launch, parts per slice or 0, slices or 0) for a list of nparts"""
    if nparts > BN_MERGE_MIN:
        pps = -(-nparts // BN_MERGE_SLICES)
        slices = -(-nparts // pps)
        return (64 if slices > BN_WIDE_MIN else 16), pps, slices
    return (64 if nparts > BN_WIDE_MIN else 16), 0, 0


class Case:
    def __init__(self, group, **kw):
        self.group = group
        self.__dict__.update(kw)
        self.id = group + "-" + (kw["name"] if "name" in kw else "-".join(
            "%s%s" % (k, _short(v)) for k, v in kw.items() if v is not None and v is not False))

    def __repr__(self):
        return self.id


def _short(v):
    return "" if v is True else str(v)


class Raw:
    """an integer input in guard rows of `fill` (no NaN for integers): [pre + M + post][C], dense"""
    nan_guard = True

    def __init__(self, values, fill, device, pre=1, post=1):
        M, Cn = values.shape
        self.full = torch.full((pre + M + post, Cn), fill, dtype=values.dtype, device=device)
        self.data = self.full[pre:pre + M]
        self.data.copy_(values)
        self.ld = Cn

    def get(self):
        return self.data.detach().cpu().clone()


def mat(M, Cn, dev, values=None, nan_guard=False, pad=0, dtype=F32, pre=2, post=2):
    """[M][Cn] at column pad // 2 of rows of ld = Cn + pad"""
    s = Slab(M, Cn, dtype, dev, ld=Cn + pad, coff=pad // 2, nan_guard=nan_guard, pre=pre, post=post)
    if values is not None:
        s.set(torch.as_tensor(values))
    return s


def vec(n, dev, values=None, nan_guard=False, dtype=F32):
    """n elements with 8 guard elements on either side and a guard row in front and behind"""
    return mat(1, n, dev, values, nan_guard, pad=16, dtype=dtype, pre=1, post=1)


def np32(s):
    """the live slice of a CPU slab as a numpy float32 array"""
    return s.data.detach().cpu().numpy().astype(f32)


def put(s, values):
    s.data.copy_(torch.as_tensor(np.asarray(values)).reshape(s.data.shape).to(s.data.dtype))


def fma(a, b, c):
    """one rounding of a * b + c (the product of two float32 is exact in float64; the double rounding of the sum is far below
    anything the bounds resolve)"""
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def rnd(shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=gen(seed)) * scale).float()


def images(sl):
    return {k: s.full.detach().cpu().clone() for k, s in sl.items()}


def check_buffers(case, sl, before):
    """outputs: guard bits intact; inputs: bit-identical, guards included (a partials table: all but its merge rows)"""
    for k, s in sl.items():
        what = "%s slab %s" % (case.id, k)
        if s.nan_guard:
            now, was = s.full.detach().cpu(), before[k]
            scratch = getattr(s, "scratch_rows", None)
            if scratch:
                keep = torch.ones(now.shape[0], dtype=torch.bool)
                keep[scratch[0]:scratch[1]] = False
                now, was = now[keep], was[keep]
            assert bits_equal(now, was), what + ": an input (or its guard) was written"
        else:
            s.assert_guards(what)


def bounded(report, key, got, ref, lim, what, names=None):
    """|got - ref| <= lim per element (assert_bound with the limit as its scale); the worst error / bound goes to report[key]"""
    got, ref, lim = got.double(), ref.double(), lim.double()
    err = (got - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / lim)
    worst = float(torch.nan_to_num(r, nan=float("inf")).max()) if r.numel() else 0.0
    if report is not None:
        report[key] = max(report.get(key, 0.0), worst)
    assert_bound(got, ref, lim, 0.0, 1.0, what, names=names)


def exact(report, key, got, ref, what, names=None):
    assert_exact(got, ref.to(got.dtype), what, names=names)
    if report is not None:
        report.setdefault(key, 0.0)


# ====================================================================================================
# 1. cris_linear_f32_small
# ====================================================================================================
LIN_NK = dict(M=[1, 8, 9, 16], N=[1, 3, 4, 5, 9], K=[1, 63, 64, 65, 129])
LIN_KN = dict(M=[1, 9, 16], N=[1, 15, 16, 17, 33], K=[1, 15, 16, 17, 127, 128, 129, 257, 2305])
LIN_CASES = [Case("linear_nk", M=M, N=N, K=K, bias=b, acc=a) for M in LIN_NK["M"] for b in (False, True) for a in (False, True)
             for N in LIN_NK["N"] for K in LIN_NK["K"]]
LIN_CASES += [Case("linear_kn", M=M, N=N, K=K, bias=False, acc=a) for M in LIN_KN["M"] for a in (False, True)
              for N in LIN_KN["N"] for K in LIN_KN["K"]]
LIN_PADS = dict(A=6, W=10, out=14)           # lda, ldw, ldo: all different, all padded


def lin_build(c, dev):
    kn = c.group == "linear_kn"
    seed = 1000 + 97 * c.M + 13 * c.N + c.K
    sl = dict(A=mat(c.M, c.K, dev, rnd((c.M, c.K), seed), True, LIN_PADS["A"]),
              W=mat(c.K if kn else c.N, c.N if kn else c.K, dev, rnd((c.K, c.N) if kn else (c.N, c.K), seed + 1), True, LIN_PADS["W"]),
              out=mat(c.M, c.N, dev, rnd((c.M, c.N), seed + 2, 3.0), False, LIN_PADS["out"]))
    if c.bias:
        sl["bias"] = vec(c.N, dev, rnd((c.N,), seed + 3), True)
    return sl


def lin_depth(c):
    """rows form: ceil(K / 64) fused multiply-adds per lane, six butterfly levels, bias, accumulate; columns form: ceil(K / 16) per
    k-group, the 16 group sums in order (the first onto 0: exact), accumulate"""
    if c.group == "linear_kn":
        return -(-c.K // LC_KG) + (LC_KG - 1) + int(c.acc) + 1
    return -(-c.K // LR_LANES) + 6 + int(c.bias) + int(c.acc) + 1


def lin_emulate(c, sl, kind="struct", mutate=None):
    kn = c.group == "linear_kn"
    A, W, old = np32(sl["A"]), np32(sl["W"]), np32(sl["out"])
    Wk = W if kn else W.T.copy()                                   # [K][N]
    M, N, K = c.M, c.N, c.K
    bias = np32(sl["bias"])[0] if c.bias else None
    if kind == "seq":
        s = np.zeros((M, N), f32)
        for k in range(K):
            s = (s + (A[:, k:k + 1] * Wk[k:k + 1, :]).astype(f32)).astype(f32)
    else:
        lanes = LC_KG if kn else LR_LANES
        Kuse = K
        if mutate == "ktail_dropped" and not kn:
            Kuse = K // LR_LANES * LR_LANES
        acc = np.zeros((lanes, M, N), f32)
        trips = -(-K // lanes)
        for j in range(trips):
            for l in range(lanes):
                k = j * lanes + l
                if k < Kuse:
                    acc[l] = fma(A[:, k:k + 1], Wk[k:k + 1, :], acc[l])
        if mutate == "clamped_row_added" and kn:                   # slots k >= K of a k-group's last trip of 8 x 16
            for kg in range(min(LC_KG, K)):
                k0 = kg + (K - 1 - kg) // (LC_KG * LC_INFLIGHT) * (LC_KG * LC_INFLIGHT)
                for u in range(LC_INFLIGHT):
                    if k0 + u * LC_KG >= K:
                        acc[kg] = fma(A[:, K - 1:K], Wk[K - 1:K, :], acc[kg])
        if mutate == "bias_per_kgroup" and c.bias:
            acc = (acc + bias[None, None, :]).astype(f32)
        if kn:
            s = np.zeros((M, N), f32)
            for g in range(LC_KG):
                s = (s + acc[g]).astype(f32)
        else:
            v = acc
            o = 32
            while o:
                v = (v + v[np.arange(64) ^ o]).astype(f32)
                o >>= 1
            s = v[0]
    if c.bias and mutate != "bias_per_kgroup":
        s = (s + bias[None, :]).astype(f32)
    if c.acc and mutate != "accumulate_ignores_old":
        s = (old + s).astype(f32)
    if mutate == "rows_ge8_dropped":
        s[8:] = old[8:]
    put(sl["out"], s)
    if mutate == "col_N_stored":
        o = sl["out"]
        o.rows[:, o.coff + N] = o.rows[:, o.coff + N - 1]


def lin_check(c, sl, before, report=None):
    check_buffers(c, sl, before)
    kn = c.group == "linear_kn"
    o = sl["out"]
    A, W = sl["A"].get().double(), sl["W"].get().double()
    old = before["out"][2:2 + c.M, o.coff:o.coff + c.N].double()
    Wk = W if kn else W.t()
    ref, S = A @ Wk, A.abs() @ Wk.abs()
    if c.bias:
        b = sl["bias"].get().double()
        ref, S = ref + b, S + b.abs()
    if c.acc:
        ref, S = ref + old, S + old.abs()
    bounded(report, c.group, o.get(), ref, lin_depth(c) * U * S, c.id + " out", names=["m", "n"])


LIN_MUTANTS = {
    "ktail_dropped": lambda c: c.group == "linear_nk" and c.K % LR_LANES != 0,
    "clamped_row_added": lambda c: c.group == "linear_kn" and c.K % (LC_KG * LC_INFLIGHT) != 0,
    "col_N_stored": lambda c: True,
    "rows_ge8_dropped": lambda c: c.M > 8,
    "accumulate_ignores_old": lambda c: c.acc,
    "bias_per_kgroup": lambda c: c.bias,
}

# ====================================================================================================
# 2. cris_outer_sum_f32_small
# ====================================================================================================
OUTER_CASES = [Case("outer", M=M, R=R, Cc=Cc, rowsum=rs) for M in (1, 9, 16) for R in (1, 3) for Cc in (1, 255, 256, 257)
               for rs in (False, True)]


def outer_build(c, dev):
    seed = 2000 + 31 * c.M + 7 * c.R + c.Cc
    sl = dict(X1=mat(c.M, c.R, dev, rnd((c.M, c.R), seed), True, 6), X2=mat(c.M, c.Cc, dev, rnd((c.M, c.Cc), seed + 1), True, 10),
              G=mat(c.R, c.Cc, dev, None, False, 14))
    if c.rowsum:
        sl["rowsum"] = vec(c.R, dev)
    return sl


def outer_emulate(c, sl, kind="struct", mutate=None):
    X1, X2 = np32(sl["X1"]), np32(sl["X2"])
    Muse = min(c.M, 8) if mutate == "rows_ge8_dropped" else c.M
    G, rs = np.zeros((c.R, c.Cc), f32), np.zeros(c.R, f32)
    for m in range(Muse):
        if kind == "seq":
            G = (G + (X1[m][:, None] * X2[m][None, :]).astype(f32)).astype(f32)
        else:
            G = fma(X1[m][:, None], X2[m][None, :], G)
        rs = (rs + X1[m]).astype(f32)
    put(sl["G"], G)
    if c.rowsum:
        put(sl["rowsum"], rs)


def outer_check(c, sl, before, report=None):
    check_buffers(c, sl, before)
    X1, X2 = sl["X1"].get().double(), sl["X2"].get().double()
    t = c.M + 1                                                     # M multiply-adds in sequence
    bounded(report, "outer G", sl["G"].get(), X1.t() @ X2, t * U * (X1.abs().t() @ X2.abs()), c.id + " G", names=["r", "c"])
    if c.rowsum:
        bounded(report, "outer rowsum", sl["rowsum"].get(), X1.sum(0, keepdim=True), t * U * X1.abs().sum(0, keepdim=True), c.id + " rowsum")


OUTER_MUTANTS = {"rows_ge8_dropped": lambda c: c.M > 8}

# ====================================================================================================
# 3. BatchNorm1d + ReLU over at most 16 rows: colstats, bn_relu, bwd_reduce, bwd_apply - each launcher alone
# ====================================================================================================
SBN_M, SBN_C = (1, 2, 9, 16), (1, 255, 256, 257)
SBN_CASES = [Case(k, M=M, C=Cn) for k in ("colstats", "bn_relu", "bwd_reduce") for M in SBN_M for Cn in SBN_C]
SBN_CASES += [Case("bwd_apply", M=M, C=Cn, countx=cx) for M in SBN_M for Cn in SBN_C for cx in (1, 3)]
SBN_CASES += [Case(k, M=M, C=Cn, grid=True) for k in ("bn_relu", "bwd_reduce", "bwd_apply") for M in (1, 9, 16) for Cn in (1, 257)]
MASK_MARGIN = 2.0 ** -18          # random cases keep |scale y + shift| this far (relative) from 0: the fp32 mask is the float64 one


def sbn_inputs(c):
    """y, dz [M][C]; scale, shift, mean, invstd [C]; sums [2C].  grid: y in bf16, scale a power of two, shift so that the
    pre-activation is exact in fp32 and cycles through 0, +2^-24, -2^-23, a negative and a positive value down every column"""
    M, Cn = c.M, c.C
    seed = 3000 + 17 * M + Cn
    if getattr(c, "grid", False):
        ri = lambda lo, hi, shape, k: torch.randint(lo, hi + 1, shape, generator=gen(seed + k)).float()      # noqa: E731
        y, scale, shift = ri(-64, 64, (M, Cn), 0) / 16, 2.0 ** ri(-2, 2, (Cn,), 1), ri(-32, 32, (Cn,), 2) / 16
        # column c with c % 5 < 3 is special: scale <= 1, y is 1 on even rows and 0 on odd rows, shift = want - scale, so that the
        # pre-activation is exactly want (0, +2^-24, -2^-23) on even rows and want - scale < 0 on odd ones
        kind = torch.arange(Cn) % 5
        want = torch.tensor([0.0, 2.0 ** -24, -2.0 ** -23, 0.0, 0.0], dtype=F64)[kind]
        special = kind < 3
        scale = torch.where(special, scale.clamp(max=1.0), scale)
        shift = torch.where(special, (want - scale.double()).float(), shift)
        y01 = (torch.arange(M) % 2 == 0).float()[:, None].expand(M, Cn)
        y = torch.where(special[None, :] & (kind[None, :] > 0), y01, y)
        y = torch.where((kind == 0)[None, :] & (y01 > 0), y01, y)              # kind 0: any y is exact, y = 1 gives the exact zero
        mean, invstd = ri(-16, 16, (Cn,), 5) / 8, 2.0 ** ri(-1, 1, (Cn,), 6)
        dz = ri(1, 8, (M, Cn), 7) * (1 - 2 * ri(0, 1, (M, Cn), 8))
        sums = torch.zeros(2 * Cn)
    else:
        y = rnd((M, Cn), seed)
        scale, shift = rnd((Cn,), seed + 1) + 1.5, rnd((Cn,), seed + 2, 0.5)
        pre = y.double() * scale.double() + shift.double()
        near = pre.abs() <= MASK_MARGIN * (y.abs() * scale.abs() + shift.abs()).double()
        y = torch.where(near, y + 0.25, y)
        mean, invstd = rnd((Cn,), seed + 5, 0.5), rnd((Cn,), seed + 6).abs() + 0.5
        dz = rnd((M, Cn), seed + 7)
        sums = rnd((2 * Cn,), seed + 9, 2.0)
    return dict(y=y, scale=scale, shift=shift, mean=mean, invstd=invstd, dz=dz, sums=sums)


def sbn_build(c, dev):
    x = sbn_inputs(c)
    M, Cn = c.M, c.C
    sl = dict(y=mat(M, Cn, dev, x["y"], True, 6))
    if c.group == "colstats":
        sl.update(psum=vec(Cn, dev), pm2=vec(Cn, dev))
        return sl
    sl.update(scale=vec(Cn, dev, x["scale"], True), shift=vec(Cn, dev, x["shift"], True))
    if c.group == "bn_relu":
        sl["z"] = mat(M, Cn, dev, None, False, 10)
        return sl
    sl.update(dz=mat(M, Cn, dev, x["dz"], True, 10), mean=vec(Cn, dev, x["mean"], True), invstd=vec(Cn, dev, x["invstd"], True))
    if c.group == "bwd_reduce":
        sl["part"] = vec(2 * Cn, dev)
    else:
        sl.update(sums=vec(2 * Cn, dev, x["sums"], True), dy=mat(M, Cn, dev, None, False, 14))
    return sl


def sbn_count(c):
    return float(c.M * getattr(c, "countx", 1))


def sbn_emulate(c, sl, kind="struct", mutate=None):
    """the kernels are sequential over the rows; `struct` contracts a * b + c into one rounding where the compiler may, `seq` rounds
    every operation"""
    M = c.M
    y = np32(sl["y"])
    mad = fma if kind == "struct" else (lambda a, b, cc: ((np.asarray(a, f32) * np.asarray(b, f32)).astype(f32) + cc).astype(f32))
    if c.group == "colstats":
        s = np.zeros(c.C, f32)
        for m in range(M):
            s = (s + y[m]).astype(f32)
        mu = (s / f32(M)).astype(f32)
        q = np.zeros(c.C, f32)
        for m in range(M):
            d = (y[m] - mu).astype(f32)
            q = mad(d, d, q)
        put(sl["psum"], s)
        put(sl["pm2"], q)
        return
    sc, sh = np32(sl["scale"])[0], np32(sl["shift"])[0]
    pre = mad(y, sc[None, :], sh[None, :])
    if c.group == "bn_relu":
        put(sl["z"], np.maximum(pre, f32(0)))
        return
    passes = pre >= 0 if mutate == "relu_mask_ge" else pre > 0
    dz, mu, iv = np32(sl["dz"]), np32(sl["mean"])[0], np32(sl["invstd"])[0]
    g = np.where(passes, dz, f32(0)).astype(f32)
    xh = ((y - mu[None, :]).astype(f32) * iv[None, :]).astype(f32)
    if c.group == "bwd_reduce":
        s0, s1 = np.zeros(c.C, f32), np.zeros(c.C, f32)
        for m in range(M):
            s0 = (s0 + g[m]).astype(f32)
            s1 = mad(g[m], xh[m], s1)
        put(sl["part"], np.concatenate([s0, s1]))
        return
    sums = np32(sl["sums"])[0]
    count = f32(M) if mutate == "apply_divides_by_M" else f32(sbn_count(c))
    invc = (f32(1) / count).astype(f32)
    a0, a1 = (sums[:c.C] * invc).astype(f32), sums[c.C:]
    t3 = ((xh * a1[None, :]).astype(f32) * invc).astype(f32)
    put(sl["dy"], (sc[None, :] * ((g - a0[None, :]).astype(f32) - t3).astype(f32)).astype(f32))


def sbn_check(c, sl, before, report=None):
    check_buffers(c, sl, before)
    M, Cn, k = c.M, c.C, c.group
    grid = getattr(c, "grid", False)
    y = sl["y"].get().double()
    if k == "colstats":
        s, S = y.sum(0, keepdim=True), y.abs().sum(0, keepdim=True)
        d = y - s / M
        Sq = ((y.abs() + S / M) ** 2).sum(0, keepdim=True)
        if M == 1:
            exact(report, "colstats sum", sl["psum"].get(), y.float(), c.id + " sum (M = 1: y itself)")
            exact(report, "colstats M2", sl["pm2"].get(), torch.zeros(1, Cn), c.id + " M2 (M = 1: 0)")
            return
        # sum: M - 1 roundings.  M2: the mean carries M (sum and division), y - mean one more, twice through the square
        # (2 a b <= (a + b)^2 turns that into a multiple of S), then M accumulations: 2 M + 3
        bounded(report, "colstats sum", sl["psum"].get(), s, M * U * S, c.id + " sum")
        bounded(report, "colstats M2", sl["pm2"].get(), (d * d).sum(0, keepdim=True), (2 * M + 3) * U * Sq, c.id + " M2")
        return
    sc, sh = sl["scale"].get().double(), sl["shift"].get().double()
    pre = y * sc + sh
    if grid:
        assert bits_equal(pre.float().double(), pre), "grid pre-activations are exact in fp32"
    else:
        assert bool((pre.abs() > MASK_MARGIN * (y.abs() * sc.abs() + sh.abs())).all()), c.id + ": a pre-activation too close to 0"
    if k == "bn_relu":
        ref = pre.clamp(min=0)
        if grid:
            exact(report, "bn_relu z grid", sl["z"].get(), ref.float(), c.id + " z", names=["m", "c"])
        else:
            bounded(report, "bn_relu z", sl["z"].get(), ref, 3 * U * (y.abs() * sc.abs() + sh.abs()), c.id + " z", names=["m", "c"])
        return
    dz, mu, iv = sl["dz"].get().double(), sl["mean"].get().double(), sl["invstd"].get().double()
    g = torch.where(pre > 0, dz, torch.zeros_like(dz))
    xh, Sxh = (y - mu) * iv, (y.abs() + mu.abs()) * iv.abs()
    if k == "bwd_reduce":
        ref = torch.cat([g.sum(0), (g * xh).sum(0)])[None, :]
        S = torch.cat([g.abs().sum(0), (g.abs() * Sxh).sum(0)])[None, :]
        if grid:
            exact(report, "bwd_reduce grid", sl["part"].get(), ref.float(), c.id + " part")
        else:
            # sum g: M; sum g xhat: xhat two roundings, then M multiply-adds
            t = torch.cat([torch.full((Cn,), M + 1.0), torch.full((Cn,), M + 3.0)])[None, :].double()
            bounded(report, "bwd_reduce", sl["part"].get(), ref, t * U * S, c.id + " part")
        return
    sums, count = sl["sums"].get().double()[0], sbn_count(c)
    a0, a1 = sums[:Cn] / count, sums[Cn:]
    ref = sc * (g - a0 - xh * a1 / count)
    S = sc.abs() * (g.abs() + a0.abs() + Sxh * a1.abs() / count)
    if grid:
        got = sl["dy"].get()
        exact(report, "bwd_apply grid", got, (sc * g).float(), c.id + " dy (sums 0: scale * masked dz)", names=["m", "c"])
        assert bool(((got != 0) == (pre > 0)).all()), c.id + ": backward passes gradient exactly where forward z > 0"
        assert bool((pre == 0).any()) and bool((got[pre == 0] == 0).all()), c.id + ": a zero pre-activation passes no gradient"
    else:
        # 1 / count, xhat (2), xhat a1, ... invc: 5; the two subtractions and the scale: 8
        bounded(report, "bwd_apply", sl["dy"].get(), ref, 9 * U * S, c.id + " dy", names=["m", "c"])


SBN_MUTANTS = {
    "relu_mask_ge": lambda c: getattr(c, "grid", False) and c.group in ("bwd_reduce", "bwd_apply"),
    "apply_divides_by_M": lambda c: c.group == "bwd_apply" and getattr(c, "countx", 1) == 3,
}

# ====================================================================================================
# 4. cris_eot_gather_ln_f32 / cris_eot_scatter_add_f32
# ====================================================================================================
EOT_PATTERNS = ("first", "last", "twice", "equal")
EOT_CASES = [Case(k, Bn=Bn, L=L, D=D, pat=p) for k in ("eot_gather", "eot_scatter") for Bn in (1, 16) for L in (1, 2, 17, 77)
             for D in (1, 255, 256, 257) for p in (EOT_PATTERNS if Bn == 1 else ("mixed",))]
EOT_TOKEN = 49407


def eot_tokens(c):
    """[Bn][L] int64 and the index of the end-of-text row of every sample: the FIRST position of the maximal token"""
    toks = torch.randint(1, 1000, (c.Bn, c.L), generator=gen(4000 + c.L + c.Bn))
    idx = []
    for b in range(c.Bn):
        p = c.pat if c.pat != "mixed" else EOT_PATTERNS[b % 4]
        if p == "first":
            toks[b, 0] = EOT_TOKEN
            i = 0
        elif p == "last":
            toks[b, c.L - 1] = EOT_TOKEN
            i = c.L - 1
        elif p == "twice":
            i = (c.L // 3 + b) % c.L
            j = min(c.L - 1, i + 1 + (b % 3))
            toks[b, i] = toks[b, j] = EOT_TOKEN
        else:
            toks[b, :] = 7
            i = 0
        idx.append(i)
    return toks, torch.tensor(idx, dtype=I32)


def eot_build(c, dev):
    toks, idx = eot_tokens(c)
    Bn, L, D = c.Bn, c.L, c.D
    rows = torch.arange(Bn) * L + idx.long()
    seed = 4100 + L + D
    if c.group == "eot_gather":
        x, mean, rstd = torch.full((Bn * L, D), NAN), torch.full((Bn * L,), NAN), torch.full((Bn * L,), NAN)
        x[rows], mean[rows], rstd[rows] = rnd((Bn, D), seed), rnd((Bn,), seed + 1, 0.3), rnd((Bn,), seed + 2).abs() + 0.5
        return dict(tokens=Raw(toks, 1 << 40, dev), x=mat(Bn * L, D, dev, x, True), mean=vec(Bn * L, dev, mean, True),
                    rstd=vec(Bn * L, dev, rstd, True), gamma=vec(D, dev, rnd((D,), seed + 3) + 1.0, True),
                    beta=vec(D, dev, rnd((D,), seed + 4), True), out=mat(Bn, D, dev), eot_index=vec(Bn, dev, dtype=I32))
    return dict(eot_index=Raw(idx[None, :], 0, dev), g=mat(Bn, D, dev, rnd((Bn, D), seed + 5), True),
                dx=mat(Bn * L, D, dev, rnd((Bn * L, D), seed + 6).to(BF), False, dtype=BF))


def eot_emulate(c, sl, kind="struct", mutate=None):
    Bn, L = c.Bn, c.L
    if c.group == "eot_gather":
        toks = sl["tokens"].get()
        idx = []
        for b in range(Bn):
            best = 0
            for l in range(1, L):
                if (toks[b, l] >= toks[b, best]) if mutate == "last_max_wins" else (toks[b, l] > toks[b, best]):
                    best = l
            idx.append(best)
        idx = np.array(idx)
        rows = np.arange(Bn) * L + idx
        x, mu, rs = np32(sl["x"])[rows], np32(sl["mean"])[0][rows], np32(sl["rstd"])[0][rows]
        ga, be = np32(sl["gamma"])[0], np32(sl["beta"])[0]
        xn = ((x - mu[:, None]).astype(f32) * rs[:, None]).astype(f32)
        out = fma(xn, ga[None, :], be[None, :]) if kind == "struct" else ((xn * ga[None, :]).astype(f32) + be[None, :]).astype(f32)
        put(sl["out"], out)
        sl["eot_index"].data.copy_(torch.from_numpy(idx.astype(np.int32))[None, :])
        return
    idx = sl["eot_index"].get()[0].long()
    rows = torch.arange(Bn) * L + idx
    dx = sl["dx"].data
    dx[rows] = (dx[rows].float() + sl["g"].get()).to(BF)


def eot_check(c, sl, before, report=None):
    check_buffers(c, sl, before)
    Bn, L, D = c.Bn, c.L, c.D
    toks, idx = eot_tokens(c)
    rows = torch.arange(Bn) * L + idx.long()
    if c.group == "eot_gather":
        exact(report, "eot index", sl["eot_index"].get(), idx[None, :], c.id + " eot_index")
        x, mu, rs = sl["x"].get().double()[rows], sl["mean"].get().double()[0][rows, None], sl["rstd"].get().double()[0][rows, None]
        ga, be = sl["gamma"].get().double(), sl["beta"].get().double()
        ref, S = (x - mu) * rs * ga + be, (x.abs() + mu.abs()) * rs.abs() * ga.abs() + be.abs()
        bounded(report, "eot gather", sl["out"].get(), ref, 5 * U * S, c.id + " out", names=["b", "d"])      # sub, mul, mul, add
        return
    s = sl["dx"]
    old = before["dx"][2:2 + Bn * L, s.coff:s.coff + D]
    got = s.get()
    hit = torch.zeros(Bn * L, dtype=torch.bool)
    hit[rows] = True
    exact(report, "eot scatter rest", got[~hit], old[~hit], c.id + " rows that are no end-of-text row")
    g = sl["g"].get().double()
    ref, S = old[rows].double() + g, old[rows].double().abs() + g.abs()
    bounded(report, "eot scatter", got[rows], ref, REL_BF16 * ref.abs() + 2 * U * S, c.id + " dx", names=["b", "d"])


EOT_MUTANTS = {"last_max_wins": lambda c: c.group == "eot_gather" and c.L > 1 and c.pat in ("twice", "equal", "mixed")}

# ====================================================================================================
# 5. cris_bn_finalize
# ====================================================================================================
BNF_NPARTS = (1, 2, 16, 17, 127, 128, 129, 511, 512, 513, 4096, 4097)
BNF_RUN = (None, 0.1, 1.0)        # running statistics absent, momentum 0.1, momentum 1.0


def _bnf_cases():
    out, i = [], 0
    for nparts in BNF_NPARTS:
        for Cn in (1, 16, 17, 40):
            for rpp in (2, 32):
                for last in ("full", "one"):
                    out.append(Case("bnf", nparts=nparts, C=Cn, rpp=rpp, last=last, mom=BNF_RUN[i % 3], form="plain"))
                    i += 1
    for nparts in (1, 17, 129, 513, 4097):                                   # the first launch of SyncBatchNorm: merged[2C] + local mean
        out.append(Case("bnf", nparts=nparts, C=17, rpp=2, last="one", mom=None, form="merged"))
        out.append(Case("bnf", nparts=nparts, C=40, rpp=32, last="full", mom=None, form="merged"))
    for Cn in (1, 17, 40):                                                   # the second: coefficients from global (sum, M2)
        for mom in BNF_RUN:
            out.append(Case("bnf", nparts=3, C=Cn, rpp=32, last="one", mom=mom, form="global", countx=3))
    for nparts in (2, 129, 513):                                             # count != count_local without global statistics
        out.append(Case("bnf", nparts=nparts, C=17, rpp=32, last="one", mom=0.1, form="plain", countx=2))
    for mom in BNF_RUN:                                                      # one row in all: no unbiased factor
        out.append(Case("bnf", nparts=1, C=17, rpp=2, last="one", mom=mom, form="plain", tag="count1"))
        out.append(Case("bnf", nparts=1, C=1, rpp=1, last="full", mom=mom, form="plain", tag="count1"))
    return out


BNF_CASES = _bnf_cases()


def bnf_counts(c):
    n_last = c.rpp if c.last == "full" else 1
    count_local = (c.nparts - 1) * c.rpp + n_last
    return count_local, count_local * getattr(c, "countx", 1), n_last


def bnf_marked(c):
    """parts that get an offset of their own: first, last, 8 PL - 1 and 8 PL, both sides of every slice boundary"""
    n = c.nparts
    PL, pps, slices = bn_path(n)
    m = {0, n - 1, 8 * 16 - 1, 8 * 16, 8 * 64 - 1, 8 * 64}
    if pps:
        for s in range(1, slices):
            m |= {s * pps - 1, s * pps}
        m |= {BN_MERGE_REGS * 16 - 1, BN_MERGE_REGS * 16}                       # the last register entry of a merge lane and the loop's first
    return sorted(i for i in m if 0 <= i < n)


def bnf_inputs(c):
    """partials of a population N(mu_c, sigma_c): part means scatter by sigma / sqrt(n), marked parts sit 5 .. 12 sigma off"""
    n, Cn = c.nparts, c.C
    count_local, count, n_last = bnf_counts(c)
    seed = 5000 + 7 * n + 3 * Cn + c.rpp + (1 if c.last == "one" else 0)
    mu, sigma = rnd((Cn,), seed, 0.5), rnd((Cn,), seed + 1).abs() * 0.5 + 0.5
    ni = torch.full((n, 1), float(c.rpp))
    ni[n - 1] = n_last
    pmean = mu[None, :] + sigma[None, :] * rnd((n, Cn), seed + 2) / ni.sqrt()
    for j, i in enumerate(bnf_marked(c)):
        pmean[i] += sigma * (5.0 + (j % 8)) * (1 if j % 2 == 0 else -1)
    psum = (pmean * ni).float()
    pm2 = (sigma[None, :] ** 2 * (ni - 1) * (0.5 + torch.rand(n, Cn, generator=gen(seed + 3)))).float()
    x = dict(psum=psum, pm2=pm2, gamma=rnd((Cn,), seed + 4) + 1.0, beta=rnd((Cn,), seed + 5), rmean=rnd((Cn,), seed + 6, 0.5),
             rvar=rnd((Cn,), seed + 7).abs() + 0.5)
    if c.form == "global":
        x["gstats"] = torch.cat([rnd((Cn,), seed + 8, 0.5) * count, (rnd((Cn,), seed + 9).abs() + 0.5) * count])
    return x


def bnf_build(c, dev):
    x = bnf_inputs(c)
    n, Cn = c.nparts, c.C
    rows = partials_rows(n)
    sl = {}
    if c.form != "global":
        for k in ("psum", "pm2"):
            v = torch.full((rows, Cn), NAN)
            v[:n] = x[k]
            sl[k] = mat(rows, Cn, dev, v, True)
            sl[k].scratch_rows = (2 + n, 2 + rows)
    else:
        sl["gstats"] = vec(2 * Cn, dev, x["gstats"], True)
    sl.update(gamma=vec(Cn, dev, x["gamma"], True), beta=vec(Cn, dev, x["beta"], True))
    for k in ("scale", "shift", "mean", "invstd"):
        sl[k] = vec(Cn, dev)
    if c.form == "merged":
        sl["merged"] = vec(2 * Cn, dev)
    if c.mom is not None:
        sl.update(rmean=vec(Cn, dev, x["rmean"]), rvar=vec(Cn, dev, x["rvar"]))
    return sl


def _lane_sum(v, PL):
    """bn_lane_sum<PL> of v [PL][C]: PL = 64 eight groups of eight (each onto 0), then the eight group sums; PL = 16 in order"""
    if PL == 64:
        g = np.zeros((8,) + v.shape[1:], f32)
        for j in range(8):
            g = (g + v.reshape(8, 8, *v.shape[1:])[:, j]).astype(f32)
        v = g
    t = v[0]
    for j in range(1, v.shape[0]):
        t = (t + v[j]).astype(f32)
    return t


def _merge_list(ps, pq, n_i, n_total, lanes, entries=None):
    """the two-pass, division-free merge of one list by `lanes` part lanes: lane l walks parts l, l + lanes, ... in order.
    ps, pq [n][C]; n_i [n] rows of every part; -> (total, mean, m2)"""
    n, Cn = ps.shape
    J = -(-n // lanes)
    if entries is not None:
        J = min(J, entries)
    s = np.zeros((lanes, Cn), f32)
    for j in range(J):
        blk = ps[j * lanes:(j + 1) * lanes]
        s[:blk.shape[0]] = (s[:blk.shape[0]] + blk).astype(f32)
    total = _lane_sum(s, lanes)
    mean = (total / f32(n_total)).astype(f32)
    inv = (f32(1) / n_i.astype(f32)).astype(f32)
    q = np.zeros((lanes, Cn), f32)
    for j in range(J):
        sl_ = slice(j * lanes, min(n, (j + 1) * lanes))
        d = fma(ps[sl_], inv[sl_, None], -mean[None, :])
        term = fma((n_i[sl_, None].astype(f32) * d).astype(f32), d, pq[sl_])
        k = term.shape[0]
        q[:k] = (q[:k] + term).astype(f32)
    return total, mean, _lane_sum(q, lanes)


def bnf_emulate(c, sl, kind="struct", mutate=None):
    n, Cn = c.nparts, c.C
    count_local, count, n_last = bnf_counts(c)
    if mutate == "var_over_count_local":
        count = count_local
    if c.form == "global":
        gs = np32(sl["gstats"])[0]
        mean, m2 = (gs[:Cn] / f32(count)).astype(f32), gs[Cn:]
    else:
        ps, pq = np32(sl["psum"])[:n].copy(), np32(sl["pm2"])[:n].copy()
        n_i = np.full(n, c.rpp, f64)
        n_i[-1] = c.rpp if mutate == "last_as_full" else n_last
        PL, pps, slices = bn_path(n)
        if mutate == "drop_8PL_minus_1" and 8 * PL - 1 < n and not pps:
            ps[8 * PL - 1] = 0
            pq[8 * PL - 1] = 0
            n_i = n_i.copy()
        if kind == "seq":
            total = np.zeros(Cn, f32)
            for i in range(n):
                total = (total + ps[i]).astype(f32)
            mean = (total / f32(count_local)).astype(f32)
            m2 = np.zeros(Cn, f32)
            for i in range(n):
                d = ((ps[i] / f32(n_i[i])).astype(f32) - mean).astype(f32)
                m2 = (m2 + (pq[i] + (f32(n_i[i]) * d * d).astype(f32)).astype(f32)).astype(f32)
        else:
            if pps:
                osum, om2, on = np.zeros((slices, Cn), f32), np.zeros((slices, Cn), f32), np.zeros(slices, f64)
                for s in range(slices):
                    a, b = s * pps, min(n, (s + 1) * pps)
                    b2 = min(n, b + 1) if mutate == "slice_boundary_double" else b
                    rows_s = min(count_local, b * c.rpp) - a * c.rpp
                    t, _, q = _merge_list(ps[a:b2], pq[a:b2], n_i[a:b2], rows_s, 16,
                                          entries=BN_MERGE_REGS if mutate == "slice_entries_beyond_64_dropped" else None)
                    osum[s], om2[s], on[s] = t, q, c.rpp * pps
                on[-1] = count_local - (slices - 1) * c.rpp * pps
                if mutate == "last_as_full":
                    on[-1] = c.rpp * pps
                sl["psum"].data[n:n + slices] = torch.from_numpy(osum)
                sl["pm2"].data[n:n + slices] = torch.from_numpy(om2)
                ps, pq, n_i = osum, om2, on
            total, mean, m2 = _merge_list(ps, pq, n_i, count_local, PL)
        if c.form == "merged":
            put(sl["merged"], np.concatenate([total, m2]))
            put(sl["mean"], mean)
            if mutate == "channel_C_written":
                o = sl["merged"]
                o.rows[0, o.coff + Cn] = o.rows[0, o.coff + Cn - 1]
            return
    var = np.maximum((m2 / f32(count)).astype(f32), f32(0))
    inv = torch.rsqrt(torch.from_numpy((var + f32(EPS)).astype(f32))).numpy()
    ga, be = np32(sl["gamma"])[0], np32(sl["beta"])[0]
    sc = (ga * inv).astype(f32)
    put(sl["scale"], sc)
    put(sl["shift"], fma(-mean, sc, be) if kind == "struct" else (be - (mean * sc).astype(f32)).astype(f32))
    put(sl["mean"], mean)
    put(sl["invstd"], inv)
    if c.mom is not None:
        mom = f32(c.mom)
        with np.errstate(all="ignore"):
            factor = (f32(count) / (f32(count) - f32(1))) if (count > 1 or mutate == "unbiased_at_count_1") else None
            unb = var if (factor is None or mutate == "unbiased_omitted") else (var * f32(factor)).astype(f32)
        rm0, rv0 = np32(sl["rmean"])[0], np32(sl["rvar"])[0]
        keep = f32(f32(1) - mom)
        put(sl["rmean"], ((keep * rm0).astype(f32) + (mom * mean).astype(f32)).astype(f32))
        put(sl["rvar"], ((keep * rv0).astype(f32) + (mom * unb).astype(f32)).astype(f32))
    if mutate == "channel_C_written":
        for k in ("scale", "shift", "mean", "invstd"):
            o = sl[k]
            o.rows[0, o.coff + Cn] = o.rows[0, o.coff + Cn - 1]


def bnf_depths(c):
    """(t_sum, t_m2): roundings on the longest path into the merged sum and into the merged M2.
    One level: entries per lane e = ceil(n / PL), then PL = 16: 15 lane additions, PL = 64: 7 + 7.  Two levels: the same for a slice of
    pps parts over 16 lanes, then for the slices.  M2: the mean (t_sum + division) enters every term through d = S_i / n_i - mean
    (1 / n_i, the multiply-subtract: 2 more) and d enters squared (2 a b <= (a + b)^2: twice), n d d + M2_i: 3 - then t_sum additions"""
    n = c.nparts
    PL, pps, slices = bn_path(n)
    lanes = lambda P: 15 if P == 16 else 14                         # noqa: E731
    if pps:
        t_sum = -(-pps // 16) + 15 + -(-slices // PL) + lanes(PL)
    else:
        t_sum = -(-n // PL) + lanes(PL)
    t_mean = t_sum + 1
    return t_sum, 2 * (t_mean + 3) + 3 + t_sum


def bnf_check(c, sl, before, report=None):
    check_buffers(c, sl, before)
    n, Cn = c.nparts, c.C
    count_local, count, n_last = bnf_counts(c)
    row = lambda k: sl[k].get().double()                              # noqa: E731
    if c.form == "global":
        gs = row("gstats")[0]
        mean, m2 = gs[None, :Cn] / count, gs[None, Cn:]
        lim_mean, lim_m2 = 2 * U * mean.abs(), torch.zeros_like(m2)
        t_sum = 0
    else:
        ps, pq = sl["psum"].get().double()[:n], sl["pm2"].get().double()[:n]
        ni = torch.full((n, 1), float(c.rpp), dtype=F64)
        ni[n - 1] = n_last
        total, Stot = ps.sum(0, keepdim=True), ps.abs().sum(0, keepdim=True)
        mean, Smean = total / count_local, Stot / count_local
        m2 = (pq + ni * (ps / ni - mean) ** 2).sum(0, keepdim=True)
        PL, pps, slices = bn_path(n)
        if pps:                                                     # the slice level, on absolute values
            Sm2 = torch.zeros(1, Cn, dtype=F64)
            for s in range(slices):
                a, b = s * pps, min(n, (s + 1) * pps)
                ns = float(ni[a:b].sum())
                As = ps[a:b].abs().sum(0, keepdim=True)
                Sm2 += (pq[a:b] + ni[a:b] * (ps[a:b].abs() / ni[a:b] + As / ns) ** 2).sum(0, keepdim=True) + ns * (As / ns + Smean) ** 2
        else:
            Sm2 = (pq + ni * (ps.abs() / ni + Smean) ** 2).sum(0, keepdim=True)
        t_sum, t_m2 = bnf_depths(c)
        lim_mean, lim_m2 = (t_sum + 2) * U * Smean, (t_m2 + 1) * U * Sm2
        if c.form == "merged":
            got = row("merged")
            bounded(report, "bnf sum", got[:, :Cn], total, (t_sum + 1) * U * Stot, c.id + " merged sum")
            bounded(report, "bnf M2", got[:, Cn:], m2, lim_m2, c.id + " merged M2")
            bounded(report, "bnf mean", row("mean"), mean, lim_mean, c.id + " local mean")
            for k in ("scale", "shift", "invstd"):                  # the merged form writes merged[2C] and the local mean only
                assert bits_equal(sl[k].full.detach().cpu(), before[k]), "%s slab %s: written by the merged form" % (c.id, k)
            return
    ga, be = row("gamma"), row("beta")
    var = (m2 / count).clamp(min=0)
    v = var + float(f32(EPS))
    inv = v ** -0.5
    # var: the division; var + eps: one more; x^-1/2 halves a relative error; rsqrtf itself RSQRT_ULPS ulp; + 1 % for second order
    lim_v = lim_m2 / count + U * var + U * v
    lim_inv = inv * (0.5 * lim_v / v * 1.01 + (2 * RSQRT_ULPS + 1) * U)
    sc = ga * inv
    lim_sc = ga.abs() * lim_inv + U * sc.abs()
    sh = be - mean * sc
    lim_sh = mean.abs() * lim_sc + sc.abs() * lim_mean + 2 * U * (be.abs() + (mean * sc).abs())
    bounded(report, "bnf mean", row("mean"), mean, lim_mean, c.id + " mean")
    bounded(report, "bnf invstd", row("invstd"), inv, lim_inv, c.id + " invstd")
    bounded(report, "bnf scale", row("scale"), sc, lim_sc, c.id + " scale")
    bounded(report, "bnf shift", row("shift"), sh, lim_sh, c.id + " shift")
    if c.mom is not None:
        mom = float(f32(c.mom))
        o = sl["rmean"]
        rm0 = before["rmean"][1:2, o.coff:o.coff + Cn].double()
        rv0 = before["rvar"][1:2, o.coff:o.coff + Cn].double()
        f = count / (count - 1.0) if count > 1 else 1.0
        unb = var * f
        lim_var = lim_m2 / count + U * var
        rm = (1 - mom) * rm0 + mom * mean
        rv = (1 - mom) * rv0 + mom * unb
        # 1 - momentum, the two products, the sum: 3 roundings on either term; the unbiased factor: division and product
        bounded(report, "bnf running mean", row("rmean"), rm, 4 * U * ((1 - mom) * rm0.abs() + mom * mean.abs()) + mom * lim_mean, c.id + " running mean")
        bounded(report, "bnf running var", row("rvar"), rv, 4 * U * ((1 - mom) * rv0.abs() + mom * unb) + mom * f * (lim_var + 3 * U * var),
                c.id + " running var")
        if c.mom == 1.0:
            exact(report, "bnf running mean", sl["rmean"].get(), sl["mean"].get(), c.id + " running mean at momentum 1: the mean itself")


BNF_MUTANTS = {
    "last_as_full": lambda c: c.form != "global" and c.last == "one" and c.rpp > 1,
    "drop_8PL_minus_1": lambda c: c.form != "global" and c.nparts in (128, 512),
    "slice_boundary_double": lambda c: c.form != "global" and c.nparts > BN_MERGE_MIN,
    "slice_entries_beyond_64_dropped": lambda c: c.form != "global" and c.nparts == 4097,
    "unbiased_omitted": lambda c: c.form != "merged" and c.mom is not None and 1 < bnf_counts(c)[1] <= 64,
    "unbiased_at_count_1": lambda c: c.mom is not None and bnf_counts(c)[1] == 1,
    "var_over_count_local": lambda c: c.form != "merged" and getattr(c, "countx", 1) > 1,
    "channel_C_written": lambda c: True,
}

# ====================================================================================================
# 6. cris_bn_sync_pack / cris_bn_sync_unpack / cris_bn_eval_coeffs
# ====================================================================================================
SYNC_CASES = [Case(k, C=Cn, grid=g) for k in ("sync_pack", "sync_unpack") for Cn in (1, 255, 257) for g in (False, True)]
SYNC_CASES += [Case("eval_coeffs", C=Cn) for Cn in (1, 255, 257)]
SYNC_N, SYNC_COUNT = 8.0, 32.0


def sync_build(c, dev):
    Cn, seed = c.C, 6000 + c.C
    if c.group == "eval_coeffs":
        return dict(gamma=vec(Cn, dev, rnd((Cn,), seed) + 1.0, True), beta=vec(Cn, dev, rnd((Cn,), seed + 1), True),
                    rmean=vec(Cn, dev, rnd((Cn,), seed + 2), True), rvar=vec(Cn, dev, rnd((Cn,), seed + 3).abs() + 0.01, True),
                    scale=vec(Cn, dev), shift=vec(Cn, dev))
    if c.grid:                                                      # multiples of 2^-3 below 8: every fused step is exact in float64 AND fp32
        q = lambda s: torch.randint(-32, 33, (Cn,), generator=gen(s)).float() / 8       # noqa: E731
        ref, mean_l, a, b = q(seed), q(seed + 1), q(seed + 2) * 8, q(seed + 3).abs() * 64        # (b = 0 somewhere: the clamp at 0)
    else:
        ref, mean_l, a, b = rnd((Cn,), seed), rnd((Cn,), seed + 1), rnd((Cn,), seed + 2) * 8, rnd((Cn,), seed + 3).abs() * 8 + 1
    sl = dict(merged=vec(2 * Cn, dev, torch.cat([a, b])), ref=vec(Cn, dev, ref, True))
    if c.group == "sync_pack":
        sl["mean_local"] = vec(Cn, dev, mean_l, True)
    return sl


def sync_formulas(c, x, dt):
    """the header's formulas; x: dict of [C] tensors at dtype dt.  -> (first half, second half) of merged"""
    if c.group == "sync_pack":           # S1 = sum - n c,  S2 = M2 + n (mean_l - c)^2
        d = x["mean_local"] - x["ref"]
        return x["a"] - SYNC_N * x["ref"], x["b"] + (SYNC_N * d) * d
    return x["a"] + SYNC_COUNT * x["ref"], (x["b"] - (x["a"] * x["a"]) / SYNC_COUNT).clamp(min=0)


def sync_emulate(c, sl, kind="struct", mutate=None):
    Cn = c.C
    if c.group == "eval_coeffs":
        ga, be, rm, rv = (np32(sl[k])[0] for k in ("gamma", "beta", "rmean", "rvar"))
        sc = (ga * torch.rsqrt(torch.from_numpy((rv + f32(EPS)).astype(f32))).numpy()).astype(f32)
        put(sl["scale"], sc)
        put(sl["shift"], fma(-rm, sc, be) if kind == "struct" else (be - (rm * sc).astype(f32)).astype(f32))
        return
    m, ref = np32(sl["merged"])[0], np32(sl["ref"])[0]
    a, b = m[:Cn], m[Cn:]
    if c.group == "sync_pack":           # the explicit single roundings of bn_sync_pack_vals
        d = (np32(sl["mean_local"])[0] - ref).astype(f32)
        n = f32(SYNC_N)
        if kind == "struct":
            s1, s2 = fma(-n, ref, a), fma((n * d).astype(f32), d, b)
        else:
            s1, s2 = (a - (n * ref).astype(f32)).astype(f32), (b + ((n * d).astype(f32) * d).astype(f32)).astype(f32)
    else:
        cnt = f32(SYNC_COUNT)
        s1 = fma(cnt, ref, a) if kind == "struct" else (a + (cnt * ref).astype(f32)).astype(f32)
        s2 = np.maximum((b - ((a * a).astype(f32) / cnt).astype(f32)).astype(f32), f32(0))
    put(sl["merged"], np.concatenate([s1, s2]))
    if mutate == "channel_C_written":
        o = sl["merged"]
        o.rows[0, o.coff + 2 * Cn] = o.rows[0, o.coff + 2 * Cn - 1]


def sync_check(c, sl, before, report=None):
    check_buffers(c, sl, before)
    Cn = c.C
    if c.group == "eval_coeffs":
        ga, be, rm, rv = (sl[k].get().double() for k in ("gamma", "beta", "rmean", "rvar"))
        sc = ga * (rv + float(f32(EPS))) ** -0.5
        lim_sc = sc.abs() * (0.5 + 2 * RSQRT_ULPS + 1 + 1) * U                   # rv + eps (halved), rsqrtf, the product, second order
        bounded(report, "eval scale", sl["scale"].get(), sc, lim_sc, c.id + " scale")
        bounded(report, "eval shift", sl["shift"].get(), be - rm * sc, rm.abs() * lim_sc + 2 * U * (be.abs() + (rm * sc).abs()), c.id + " shift")
        return
    o = sl["merged"]
    m0 = before["merged"][1, o.coff:o.coff + 2 * Cn].double()
    x = dict(a=m0[:Cn], b=m0[Cn:], ref=sl["ref"].get().double()[0])
    if c.group == "sync_pack":
        x["mean_local"] = sl["mean_local"].get().double()[0]
    r1, r2 = sync_formulas(c, x, F64)
    got = o.get()[0]
    if c.grid:
        exact(report, c.group + " grid", got, torch.cat([r1, r2]).float(), c.id + " merged")
        return
    ab = {k: v.abs() for k, v in x.items()}
    if c.group == "sync_pack":
        S1, S2 = ab["a"] + SYNC_N * ab["ref"], ab["b"] + SYNC_N * (ab["mean_local"] + ab["ref"]) ** 2
        t1, t2 = 2, 5                   # one fused multiply-add; the difference (twice through the square), n d, the fused step
    else:
        S1, S2 = ab["a"] + SYNC_COUNT * ab["ref"], ab["b"] + ab["a"] ** 2 / SYNC_COUNT
        t1, t2 = 2, 4                   # one fused multiply-add; square, division, difference
    bounded(report, c.group + " first", got[:Cn], r1, t1 * U * S1, c.id + " merged[:C]")
    bounded(report, c.group + " second", got[Cn:], r2, t2 * U * S2, c.id + " merged[C:]")


SYNC_MUTANTS = {"channel_C_written": lambda c: c.group != "eval_coeffs"}

# ====================================================================================================
# 7. cris_sum_tables
# ====================================================================================================
SUM_NCOL, SUM_NPARTS = (1, 63, 64, 65, 130), (1, 3, 4, 5, 9)


def _sum_cases():
    out = [Case("sum", name="one-%dx%d" % (p, n), tables=((n, p),)) for n in SUM_NCOL for p in SUM_NPARTS]
    pairs = [(63, 65), (64, 64), (65, 1), (1, 130), (130, 63), (64, 65)]
    out += [Case("sum", name="two-%d-%d" % (a, b), tables=((a, SUM_NPARTS[i % 5]), (b, SUM_NPARTS[(i + 2) % 5]))) for i, (a, b) in enumerate(pairs)]
    out.append(Case("sum", name="max64", tables=tuple((SUM_NCOL[i % 5], SUM_NPARTS[(i // 5 + i) % 5]) for i in range(SUM_GROUP_MAX))))
    return out


SUM_CASES = _sum_cases()
SUM_LDPAD = 6


def sum_build(c, dev):
    sl = {}
    total = sum(n for n, _ in c.tables)
    sl["out"] = vec(total, dev)                                     # every table's out vector next to its neighbours in one arena
    for i, (ncol, nparts) in enumerate(c.tables):
        sl["part%d" % i] = mat(nparts, ncol, dev, rnd((nparts, ncol), 7000 + 131 * i + ncol + nparts), True, SUM_LDPAD)
    return sl


def sum_offsets(c):
    off, o = [], 0
    for n, _ in c.tables:
        off.append(o)
        o += n
    return off


def sum_emulate(c, sl, kind="struct", mutate=None):
    off = sum_offsets(c)
    out = sl["out"].data[0]
    for i, (ncol, nparts) in enumerate(c.tables):
        p = np32(sl["part%d" % i])
        use = nparts // SUM_PARTLANES * SUM_PARTLANES if mutate == "parts_tail_dropped" else nparts
        if kind == "seq":
            s = np.zeros(ncol, f32)
            for r in range(use):
                s = (s + p[r]).astype(f32)
        else:
            lane = np.zeros((SUM_PARTLANES, ncol), f32)
            for r in range(use):
                lane[r % SUM_PARTLANES] = (lane[r % SUM_PARTLANES] + p[r]).astype(f32)
            s = ((lane[0] + lane[1]).astype(f32) + (lane[2] + lane[3]).astype(f32)).astype(f32)
        lo = SUM_COLS if (mutate == "table_search_off_by_one" and i > 0) else 0       # the first block of a table goes to its predecessor
        out[off[i] + lo:off[i] + ncol] = torch.from_numpy(s[lo:])


def sum_check(c, sl, before, report=None):
    check_buffers(c, sl, before)
    off = sum_offsets(c)
    got = sl["out"].get()[0]
    for i, (ncol, nparts) in enumerate(c.tables):
        p = sl["part%d" % i].get().double()
        t = -(-nparts // SUM_PARTLANES) + 2 + 1                       # entries per part lane, two levels
        bounded(report, "sum_tables", got[off[i]:off[i] + ncol], p.sum(0), t * U * p.abs().sum(0), "%s table %d (%d x %d)" % (c.id, i, nparts, ncol))


SUM_MUTANTS = {
    "table_search_off_by_one": lambda c: len(c.tables) > 1,
    "parts_tail_dropped": lambda c: any(p % SUM_PARTLANES for _, p in c.tables),
}


# ====================================================================================================
class Group:
    def __init__(self, name, cases, build, emulate, check, mutants):
        self.name, self.cases, self.build, self.emulate, self.check, self.mutants = name, cases, build, emulate, check, mutants


GROUPS = {g.name: g for g in (
    Group("linear", LIN_CASES, lin_build, lin_emulate, lin_check, LIN_MUTANTS),
    Group("outer", OUTER_CASES, outer_build, outer_emulate, outer_check, OUTER_MUTANTS),
    Group("small_bn", SBN_CASES, sbn_build, sbn_emulate, sbn_check, SBN_MUTANTS),
    Group("eot", EOT_CASES, eot_build, eot_emulate, eot_check, EOT_MUTANTS),
    Group("bn_finalize", BNF_CASES, bnf_build, bnf_emulate, bnf_check, BNF_MUTANTS),
    Group("bn_sync", SYNC_CASES, sync_build, sync_emulate, sync_check, SYNC_MUTANTS),
    Group("sum_tables", SUM_CASES, sum_build, sum_emulate, sum_check, SUM_MUTANTS),
)}


def run(group, case, device, launch, report=None):
    """build the case's slabs on `device`, let `launch(case, slabs)` write the outputs, check every element and every guard"""
    g = GROUPS[group]
    sl = g.build(case, device)
    before = images(sl)
    launch(case, sl)
    g.check(case, sl, before, report)
    return sl
