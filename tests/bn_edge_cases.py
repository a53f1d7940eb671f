"""BatchNorm apply / backward (csrc/norm.hip): statements, bounds, launch-geometry mirrors and case tables shared by
tests/test_bn_edges.py (the HIP kernels on the GPU) and tests/test_bn_edges_cpu.py (the same checks against a plain torch fp32
evaluation, and the path every case is named for; no GPU).

Conventions of tests/hip_ops_edge_cases.py: one function of a dtype per op - float64 is the reference, float32 the "correct
implementation", float64 with `absolute=True` the scale S of  |got - ref| <= REL |ref| + ABS S.

A case is a dict of tensors on one device (float32 tensors holding the exact values the kernel gets, bf16-representable where
the kernel reads bf16) and flags.  Activations are NHWC [B][H][W][C].

Grid inputs.  y, y2, ident: multiples of 2^-4 in [-8, 8]; scale, scale2: multiples of 2^-3 in [-2, 2]; shift, shift2: odd
multiples of 2^-8 in (-2, 2); mul: multiples of 2^-2 in [0, 4].  Then scale * y is a multiple of 2^-7 below 16, every sum of
the forward is a multiple of 2^-8 below 64, pooled and multiplied a multiple of 2^-10 below 256: at most 18 significant bits,
exact in fp32 whatever the order or FMA contraction, so the bf16 result is the unique rounding of the exact value.  A single
branch's pre-activation is an odd multiple of 2^-8: never zero, so the recomputed ReLU mask is exact as well.
"""
import torch

import hip_ops_edge_cases as E
from hip_ops_edge_cases import BF, F32, F64

DIV24_LIMIT = 1 << 24             # the generic kernels: reciprocal division below, 64-bit division from here
BF16_MIN_NORMAL = 2.0 ** -126


# ----------------------------------------------------------------------------------------------------
# mirrors of the launch geometry (test code only)
# ----------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return (a + b - 1) // b


def grid_1d(items, per_block, cap=8192):
    return max(1, min(cap, cdiv(items, per_block)))


def cv_shift(C):
    """log2(C/8) when C/8 is a power of two <= 256 (the fast kernels' thread mapping), else -1"""
    CV = C >> 3
    if CV < 1 or CV > 256 or CV & (CV - 1):
        return -1
    return CV.bit_length() - 1


def fast_grid(total, U):
    few, many = grid_1d(total, 256 * U, 2048), grid_1d(total, 256, 1024)
    return few if few > many else many


def fast_rows(M, C, U):
    """(rows_per_pass, grid, step) of a fast apply launch over M rows"""
    s = cv_shift(C)
    rpp = 256 >> s
    grid = fast_grid(M << s, U)
    return rpp, grid, grid * rpp


def last_pass_partial(M, C, U):
    """the last trip's last (U-th) pass holds some rows below M and some past it"""
    _, _, step = fast_rows(M, C, U)
    return (U - 1) * step < M % (step * U) < U * step


def bwd_geometry(M, C):
    """chunk width in 8-channel vectors, chunks, rows per row block, row blocks"""
    CV = C >> 3
    chv = 1
    while chv < 8 and chv * 2 <= CV // 4:
        chv *= 2
    chunks = cdiv(CV, chv)
    rbs = max(1, min(64, 512 // chunks))
    rpb = max(32, cdiv(M, rbs))
    return dict(chv=chv, chunks=chunks, rpb=rpb, rbs=cdiv(M, rpb), last_cvn=CV - (chunks - 1) * chv)


def row_blocks(M, C):
    g = bwd_geometry(M, C)
    return [(rb * g["rpb"], min(M, (rb + 1) * g["rpb"])) for rb in range(g["rbs"])]


def fwd_path(c):
    return "fast" if cv_shift(c["y"].shape[3]) >= 0 and not c["pool"] and c.get("mul") is None else "generic"


def bwd_mask(c):
    """0: no ReLU, 1: from the stored z, 2: recomputed"""
    if not c["relu"]:
        return 0
    return 1 if not c["pool"] and (c.get("y2") is not None or c.get("z") is not None) else 2


def reduce_instance(c):
    """(MASK, Y2, POOL, MUL) of the one reduce kernel the case launches"""
    return bwd_mask(c), c.get("y2") is not None, bool(c["pool"]), c.get("mul") is not None


# the instantiations the reduce launcher admits: pooling goes with a plain BatchNorm (no y2, no mul) and never takes its mask
# from z; over two branches the mask is never recomputed
REDUCE_INSTANCES = ({(m, False, True, False) for m in (0, 2)} | {(m, True, False, mul) for m in (0, 1) for mul in (False, True)} |
                    {(m, False, False, mul) for m in (0, 1, 2) for mul in (False, True)})


def wants_dmul(c):
    """the reduce launcher computes the multiplier's gradient for a plain BatchNorm + ReLU only"""
    return c.get("mul") is not None and c["relu"] and not c["pool"] and c.get("y2") is None


def bwd_apply_path(c):
    two, z = c.get("y2") is not None, c.get("z") is not None
    if cv_shift(c["y"].shape[3]) < 0 or c["pool"] or c.get("mul") is not None or (two and not z):
        return "generic"
    return "fast"


# ----------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------
def _gen(seed, device):
    return torch.Generator(device=device).manual_seed(seed)


def grid_vals(shape, seed, step, lo, hi, device="cpu", odd=False):
    """multiples of `step` in [lo, hi]; odd: odd multiples of `step` inside (lo, hi)"""
    if odd:
        k = torch.randint(round(lo / step / 2), round(hi / step / 2), shape, generator=_gen(seed, device), device=device) * 2 + 1
    else:
        k = torch.randint(round(lo / step), round(hi / step) + 1, shape, generator=_gen(seed, device), device=device)
    return k.float() * step


def rand_f32(shape, seed, device="cpu", scale=1.0):
    return torch.randn(*shape, generator=_gen(seed, device), device=device) * scale


def rand_bf(shape, seed, device="cpu", scale=1.0):
    return rand_f32(shape, seed, device, scale).to(BF).float()


def rand_invstd(shape, seed, device="cpu"):
    return torch.rand(*shape, generator=_gen(seed, device), device=device) * 1.5 + 0.5


FWD_VARIANTS = ["plain", "pool", "ident", "two", "two_ident", "mul"]


def make_fwd(variant, relu, B, H, W, C, device="cpu"):
    act = lambda seed: grid_vals((B, H, W, C), seed, 2.0 ** -4, -8, 8, device)
    c = dict(y=act(101), scale=grid_vals((C,), 102, 2.0 ** -3, -2, 2, device), shift=grid_vals((C,), 103, 2.0 ** -8, -2, 2, device, odd=True),
             relu=bool(relu), pool=variant == "pool")
    if variant in ("two", "two_ident"):
        c.update(y2=act(104), scale2=grid_vals((C,), 105, 2.0 ** -3, -2, 2, device),
                 shift2=grid_vals((C,), 106, 2.0 ** -8, -2, 2, device, odd=True))
    if variant in ("ident", "two_ident"):
        c["ident"] = act(107)
    if variant == "mul":
        c["mul"] = grid_vals((B, C), 108, 2.0 ** -2, 0, 4, device)
    return c


def plant_z(z):
    """z [B][H][W][C] with the decision boundary of `z > 0` planted in the first and the last row: +0 and -0 (masked), the
    smallest positive normal bf16 (passes), its negative (masked)"""
    C = z.shape[-1]
    flat = z.view(-1, C)
    vals = torch.tensor([0.0, -0.0, BF16_MIN_NORMAL, -BF16_MIN_NORMAL], device=z.device)
    flat[0, :4] = vals
    flat[-1, C - 4:] = vals
    return z


def make_bwd(variant, B, H, W, C, device="cpu", dident=None, dy2=True, count_factor=1):
    """variant: m0 / m2 (plain, ReLU off / recomputed mask), m1 (mask from z), pool_m0 / pool_m2, two_m0 (y2, no ReLU, no z),
    two_m0z (the same with z passed), two_m1, mul_m0 / mul_m1 / mul_m2 (per-sample multiplier on m0 / m1 / m2; dmul where
    wants_dmul), two_mul_m0 / two_mul_m1 (the multiplier over two branches).  dz, mean, invstd and the old / supplied sums are random."""
    M = B * H * W
    act = lambda seed: grid_vals((B, H, W, C), seed, 2.0 ** -4, -8, 8, device)
    pool, two = variant.startswith("pool"), variant.startswith("two")
    OH, OW = (H // 2, W // 2) if pool else (H, W)
    c = dict(y=act(201), scale=grid_vals((C,), 202, 2.0 ** -3, -2, 2, device), shift=grid_vals((C,), 203, 2.0 ** -8, -2, 2, device, odd=True),
             mean=rand_f32((C,), 204, device), invstd=rand_invstd((C,), 205, device), dz=rand_bf((B, OH, OW, C), 206, device),
             relu=variant not in ("m0", "pool_m0", "two_m0", "two_m0z", "mul_m0", "two_mul_m0"), pool=pool, count=float(M * count_factor))
    ncol = (4 if two else 2) * C
    c["sums_old"] = rand_f32((ncol,), 207, device, scale=4.0)                        # reduce: += into these
    c["sums"] = rand_f32((ncol,), 208, device, scale=(M * count_factor) ** 0.5)     # apply: the supplied batch totals
    if variant in ("m1", "two_m1", "two_m0z", "mul_m1", "two_mul_m1"):
        c["z"] = plant_z(rand_bf((B, H, W, C), 209, device))
        c["dz"].view(-1, C)[0, :4] = 4.0                                             # a wrong decision there is no rounding error
        c["dz"].view(-1, C)[-1, C - 4:] = 4.0
    if two:
        c.update(y2=act(210), mean2=rand_f32((C,), 211, device), invstd2=rand_invstd((C,), 212, device),
                 scale2=grid_vals((C,), 213, 2.0 ** -3, -2, 2, device), want_dy2=bool(dy2))
    if "mul" in variant:
        c["mul"] = grid_vals((B, C), 214, 2.0 ** -2, 0, 4, device)
    if dident is not None:
        c["dident"] = dident                                                         # "store" or "accum"
        if dident == "accum":
            c["dident_old"] = rand_bf((B, H, W, C), 215, device)
    return c


def to_device(c, device):
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in c.items()}


# ----------------------------------------------------------------------------------------------------
# statements
# ----------------------------------------------------------------------------------------------------
def _pool4(x):
    B, H, W, C = x.shape
    return x.view(B, H // 2, 2, W // 2, 2, C).sum((2, 4)) * 0.25


def _unpool4(dz, H, W):
    B, OH, OW, C = dz.shape
    return (dz * 0.25).view(B, OH, 1, OW, 1, C).expand(B, OH, 2, OW, 2, C).reshape(B, H, W, C)


def bn_fwd(c, dt):
    """z [rows][C] of cris_bn_apply"""
    o = c["y"].to(dt) * c["scale"].to(dt) + c["shift"].to(dt)
    if c.get("y2") is not None:
        o = o + (c["y2"].to(dt) * c["scale2"].to(dt) + c["shift2"].to(dt))
    if c.get("ident") is not None:
        o = o + c["ident"].to(dt)
    if c["relu"]:
        o = torch.relu(o)
    if c.get("mul") is not None:
        o = o * c["mul"].to(dt)[:, None, None, :]
    if c["pool"]:
        o = _pool4(o)
    return o.reshape(-1, o.shape[-1])


def relu_mask(c, dt):
    m = bwd_mask(c)
    if m == 0:
        return None
    if m == 1:
        return c["z"] > 0
    return (c["y"].to(dt) * c["scale"].to(dt) + c["shift"].to(dt)) > 0


def bn_bwd_g(c, dt, absolute=False):
    """the gradient entering the BatchNorm output, per full-resolution row: [M][C]"""
    B, H, W, C = c["y"].shape
    dz = c["dz"].to(dt)
    if absolute:
        dz = dz.abs()
    if c["pool"]:
        dz = _unpool4(dz, H, W)
    if c.get("mul") is not None:
        dz = dz * c["mul"].to(dt).abs()[:, None, None, :]            # (mul >= 0)
    mask = relu_mask(c, dt)
    if mask is not None:
        dz = torch.where(mask, dz, torch.zeros((), dtype=dt, device=dz.device))
    return dz.reshape(-1, C)


def xhat(c, dt, absolute=False, second=False):
    y, mean, inv = (c["y2"], c["mean2"], c["invstd2"]) if second else (c["y"], c["mean"], c["invstd"])
    C = y.shape[-1]
    if absolute:
        return ((y.to(dt).abs() + mean.to(dt).abs()) * inv.to(dt).abs()).reshape(-1, C)
    return ((y.to(dt) - mean.to(dt)) * inv.to(dt)).reshape(-1, C)


def bn_bwd_sums(c, dt, absolute=False, old=True):
    """[2C] = [sum g | sum g xhat], with y2 [4C] = [sum g | sum g xhat | sum g | sum g xhat2]; added to `sums_old`"""
    g = bn_bwd_g(c, dt, absolute)
    s = [g.sum(0), (g * xhat(c, dt, absolute)).sum(0)]
    if c.get("y2") is not None:
        s += [g.sum(0), (g * xhat(c, dt, absolute, second=True)).sum(0)]
    s = torch.cat(s)
    if old:
        o = c["sums_old"].to(dt)
        s = s + (o.abs() if absolute else o)
    return s


def bn_bwd_dmul(c, dt, absolute=False):
    """dmul [B][C] = sum over the sample's pixels of dz * relu(scale y + shift)"""
    B, H, W, C = c["y"].shape
    if absolute:
        t = c["dz"].to(dt).abs() * (c["y"].to(dt).abs() * c["scale"].to(dt).abs() + c["shift"].to(dt).abs())
    else:
        t = c["dz"].to(dt) * torch.relu(c["y"].to(dt) * c["scale"].to(dt) + c["shift"].to(dt))
    return t.view(B, H * W, C).sum(1)


def bn_bwd_apply(c, dt, absolute=False, sums=None):
    """dy (dy2, dident) [M][C] from the supplied sums and count"""
    C = c["y"].shape[-1]
    sums = (c["sums"] if sums is None else sums).to(dt)
    cnt = c["count"]
    g = bn_bwd_g(c, dt, absolute)
    out = {}

    def one(scale, xh, s0, s1):
        if absolute:
            return scale.to(dt).abs() * (g + s0.abs() / cnt + xh * s1.abs() / cnt)
        return scale.to(dt) * (g - s0 / cnt - xh * s1 / cnt)

    out["dy"] = one(c["scale"], xhat(c, dt, absolute), sums[:C], sums[C:2 * C])
    if c.get("y2") is not None and c.get("want_dy2"):
        out["dy2"] = one(c["scale2"], xhat(c, dt, absolute, second=True), sums[:C], sums[3 * C:])
    if c.get("dident") == "store":
        out["dident"] = g
    elif c.get("dident") == "accum":
        o = c["dident_old"].to(dt).reshape(-1, C)
        out["dident"] = g + (o.abs() if absolute else o)
    return out


def sum_parts(table, old, dt, absolute=False):
    t, o = table.to(dt), old.to(dt)
    return (t.abs().sum(0) + o.abs()) if absolute else (t.sum(0) + o)


# ----------------------------------------------------------------------------------------------------
# checks: `got` is what the kernel (GPU file) or the float32 statement (CPU file) returned
# ----------------------------------------------------------------------------------------------------
def ref_dtype(c):
    """float64, except for the 2^24 cases: their references are computed in float32 (the arithmetic of the grid is exact in it;
    the bounded results carry 2^-20 S of slack for its roundings)"""
    return c.get("ref_dtype", F64)


def check_fwd(got_bf, c, what):
    E.assert_exact(got_bf, bn_fwd(c, ref_dtype(c)).to(BF), what, names=("row", "c"))


def check_sums(got, c, what):
    M = c["y"].shape[0] * c["y"].shape[1] * c["y"].shape[2]
    C = c["y"].shape[-1]
    ref, S = bn_bwd_sums(c, F64), bn_bwd_sums(c, F64, absolute=True)
    n = ref.numel() // C
    E.assert_bound(got.to(F64).view(n, C), ref.view(n, C), S.view(n, C), 0.0, E.abs_coef(M + 16), what + " sums", names=("slot", "c"))


def check_dmul(got, c, what):
    HW = c["y"].shape[1] * c["y"].shape[2]
    E.assert_bound(got.to(F64), bn_bwd_dmul(c, F64), bn_bwd_dmul(c, F64, absolute=True), 0.0, E.abs_coef(HW + 16), what + " dmul",
                   names=("b", "c"))


def check_apply(got, c, what, sums=None, extra_S=None):
    """got: {"dy", "dy2", "dident"} as bf16 tensors [M][C]"""
    dt = ref_dtype(c)
    ref, S = bn_bwd_apply(c, dt, sums=sums), bn_bwd_apply(c, dt, absolute=True, sums=sums)
    assert sorted(got) == sorted(ref), "%s: outputs %s, expected %s" % (what, sorted(got), sorted(ref))
    for k in sorted(ref):
        if k == "dident" and c["dident"] == "store":
            E.assert_exact(got[k], ref[k].to(BF), what + " dident (g itself)", names=("row", "c"))
            continue
        s = S[k] if extra_S is None or k not in extra_S else S[k] + extra_S[k]
        E.assert_bound(got[k], ref[k], s, E.REL_BF16, E.ABS_F32, what + " " + k, names=("row", "c"))


# ----------------------------------------------------------------------------------------------------
# end to end: the float64 torch statement of the forward, differentiated by autograd
# ----------------------------------------------------------------------------------------------------
E2E_MARGIN = 2.0 ** -12


def make_e2e(variant, dident, B, H, W, C):
    """_make_e2e with the first beta offset k * 2^-6 (k = 0, 1, ...) at which, where the kernels recompute the ReLU mask from fp32
    scale and shift, no pre-activation is nearer to zero than E2E_MARGIN: the roundings of the coefficients (some 2^-22 of
    |scale y| + |shift| < 64) then decide no ReLU differently from float64"""
    for k in range(16):
        c, ref = _make_e2e(variant, dident, B, H, W, C, k * 2.0 ** -6)
        if bwd_mask(c) != 2 or c["margin"] >= E2E_MARGIN:
            return c, ref
    raise AssertionError("no beta offset keeps the pre-activations away from zero")


def _make_e2e(variant, dident, B, H, W, C, beta_offset):
    """-> (case, ref).  gamma (the grid `scale` of make_bwd), beta (its `shift`), y, y2, ident and dz define the float64 forward
    relu(bn(y) [+ bn(y2)] [+ ident]) [* mul] [pooled]; `ref` holds its autograd gradients.  The case gets what the engine would
    pass: the float64 batch statistics and coefficients rounded to fp32, z (where the mask comes from it) as the forward's
    bf16 output, zeroed sums and count = M."""
    import torch.nn.functional as F
    c = make_bwd(variant, B, H, W, C, dident=dident)
    two, pool, relu = c.get("y2") is not None, c["pool"], c["relu"]
    leaf = lambda t: t.double().clone().requires_grad_(True)
    y, gamma, beta, dz = leaf(c["y"]), leaf(c["scale"]), leaf(c["shift"] + beta_offset), c["dz"].double()

    def bn(t, g_, b_):
        return F.batch_norm(t.permute(0, 3, 1, 2), None, None, g_, b_, True, 0.0, 1e-5).permute(0, 2, 3, 1)

    def stats(t):
        t2 = t.detach().reshape(-1, C)
        return t2.mean(0), (t2.var(0, unbiased=False) + 1e-5).rsqrt()

    pre = bn(y, gamma, beta)
    if two:
        y2, gamma2 = leaf(c["y2"]), leaf(c["scale2"])
        pre = pre + bn(y2, gamma2, None)
    if dident is not None:
        ident = leaf(grid_vals((B, H, W, C), 216, 2.0 ** -4, -8, 8))
        pre = pre + ident
    out = torch.relu(pre) if relu else pre
    if c.get("mul") is not None:
        mul = leaf(c["mul"])
        out = out * mul[:, None, None, :]
    if pool:
        out = _pool4(out)
    (out * dz).sum().backward()

    mean, inv = stats(y)
    c.update(mean=mean.float(), invstd=inv.float(), scale=(gamma.detach() * inv).float(),
             shift=(beta.detach() - mean * gamma.detach() * inv).float(), sums_old=torch.zeros_like(c["sums_old"]), count=float(B * H * W))
    sums = [beta.grad, gamma.grad]
    ref = dict(dy=y.grad.reshape(-1, C))
    if two:
        mean2, inv2 = stats(y2)
        c.update(mean2=mean2.float(), invstd2=inv2.float(), scale2=(gamma2.detach() * inv2).float())
        sums += [beta.grad, gamma2.grad]
        ref["dy2"] = y2.grad.reshape(-1, C)
    if bwd_mask(c) == 1:
        c["z"] = torch.relu(pre.detach()).to(BF).float()
    if dident is not None:
        old = c["dident_old"].double() if dident == "accum" else 0.0
        ref["dident"] = (ident.grad + old).reshape(-1, C)
    if c.get("mul") is not None:
        ref["dmul"] = mul.grad
    ref["sums"] = torch.cat(sums)
    c["margin"] = float(pre.detach().abs().min())          # distance of the nearest pre-activation from the ReLU decision
    return c, ref


def check_e2e(got, c, ref, what):
    """got: {"sums", "dy", ["dy2", "dident", "dmul"]}.  Bounds of the stages; the reduce stage's own tolerance on the sums enters
    the scale of dy: |scale| (E0 + xhat E1) / count, with E = abs_coef(M + 16) S of the sums."""
    B, H, W, C = c["y"].shape
    M = B * H * W
    n = ref["sums"].numel() // C
    Ssum = bn_bwd_sums(c, F64, absolute=True)
    E.assert_bound(got["sums"].to(F64).view(n, C), ref["sums"].view(n, C), Ssum.view(n, C), 0.0, E.abs_coef(M + 16), what + " sums",
                   names=("slot", "c"))
    Esum = E.abs_coef(M + 16) * Ssum
    S = bn_bwd_apply(c, F64, absolute=True, sums=ref["sums"])
    feed = lambda scale, xh, e1: scale.double().abs() * (Esum[:C] + xh * e1) / c["count"] / E.ABS_F32
    E.assert_bound(got["dy"], ref["dy"], S["dy"] + feed(c["scale"], xhat(c, F64, True), Esum[C:2 * C]), E.REL_BF16, E.ABS_F32,
                   what + " dy", names=("row", "c"))
    if "dy2" in ref:
        E.assert_bound(got["dy2"], ref["dy2"], S["dy2"] + feed(c["scale2"], xhat(c, F64, True, second=True), Esum[3 * C:]), E.REL_BF16,
                       E.ABS_F32, what + " dy2", names=("row", "c"))
    if "dident" in ref:
        if c["dident"] == "store":
            E.assert_exact(got["dident"], ref["dident"].to(BF), what + " dident (g itself)", names=("row", "c"))
        else:
            E.assert_bound(got["dident"], ref["dident"], S["dident"], E.REL_BF16, E.ABS_F32, what + " dident", names=("row", "c"))
    if "dmul" in ref:
        HW = H * W
        E.assert_bound(got["dmul"].to(F64), ref["dmul"], bn_bwd_dmul(c, F64, absolute=True), 0.0, E.abs_coef(HW + 16), what + " dmul",
                       names=("b", "c"))


# ----------------------------------------------------------------------------------------------------
# case tables
# ----------------------------------------------------------------------------------------------------
FAST_C = [8, 16, 64, 256, 2048]                  # cv_shift 0, 1, 3, 5, 8
GENERIC_C = [24, 40, 72, 280]                    # CV = 3 (the plain-division divisor), 5, 9, 35
ON_DEVICE = 1 << 20                              # cases above this many elements: inputs and reference made on the device


def partial_M(C):
    """rows that fill three passes of a 1024-block grid and part of a fourth: the last of U = 4 passes is partial, and so is the
    second of U = 2 (tests/test_bn_edges_cpu.py asserts both)"""
    rpp = 256 >> cv_shift(C)
    return 3072 * rpp + 2 * rpp + 1


def fast_ladder(C):
    rpp = 256 >> cv_shift(C)
    return sorted({m for m in (1, rpp - 1, rpp + 1) if m >= 1}), partial_M(C)


def fwd_cases():
    """(id, variant, relu, (B, H, W, C))"""
    out = []

    def add(variant, relu, B, H, W, C):
        out.append(("%s-%s-%dx%dx%dx%d" % (variant, "relu" if relu else "lin", B, H, W, C), variant, relu, (B, H, W, C)))

    for C in FAST_C:
        small, big = fast_ladder(C)
        for M in small:
            for variant in ("plain", "ident", "two", "two_ident"):
                for relu in (True, False):
                    add(variant, relu, 1, M, 1, C)
        for variant, relu in (("plain", True), ("ident", False), ("two", True), ("two_ident", False)):
            add(variant, relu, 1, big, 1, C)
    for C in GENERIC_C:
        for relu in (True, False):
            for variant in ("plain", "ident", "two", "two_ident"):
                add(variant, relu, 2, 3, 5, C)
            for (B, H, W) in ((2, 2, 2), (1, 4, 6), (3, 2, 6), (2, 4, 10)):          # OH*OW = 1; OW = 3; OH*OW = OW = 3; OW = 5
                add("pool", relu, B, H, W, C)
            for (H, W) in ((1, 1), (3, 11)):
                add("mul", relu, 3, H, W, C)
    for relu in (True, False):                                                       # pool / mul keep a power-of-two C off the fast kernel
        add("pool", relu, 2, 4, 6, 64)
        add("mul", relu, 3, 3, 11, 64)
    return out


# 8 M just above 2^20 vectors: `few` (1025 blocks) decides the grid;  64 M just above 2^21: the 2048-block cap and a second trip
GRID_BOUNDARY_CASES = [("few-gt-many", (1, 131077, 1, 64)), ("cap-second-trip", (1, 32773, 1, 512))]

REDUCE_C = [8, 40, 72, 136, 280, 2048, 8192]
REDUCE_M = [1, 31, 33, 65, 2049]
REDUCE_M_RAGGED = {8: 65927}                     # rpb = 1031: a second, ragged trip of RS * U = 1024 rows
POOL_SHAPES = [(1, 2, 2), (2, 4, 6), (3, 26, 26)]
# M = 65933, rpb = 1031 as REDUCE_M_RAGGED; HW = 9419 is no multiple of 256, so sample boundaries fall inside a group of in-flight
# rows and inside row blocks
REDUCE_MUL_RAGGED = (7, 9419, 1, 8)


def reduce_cases():
    """(id, variant, (B, H, W, C))"""
    out = []

    def add(variant, B, H, W, C):
        out.append(("%s-%dx%dx%dx%d" % (variant, B, H, W, C), variant, (B, H, W, C)))

    for C in REDUCE_C:
        for M in REDUCE_M + ([REDUCE_M_RAGGED[C]] if C in REDUCE_M_RAGGED else []):
            add("m2", 1, M, 1, C)
    for variant in ("m0", "m1", "two_m0", "two_m0z", "two_m1"):
        for C in (8, 72, 280, 2048):
            for M in (33, 2049):
                add(variant, 1, M, 1, C)
    add("two_m1", 1, REDUCE_M_RAGGED[8], 1, 8)                                     # U = 2: rpb = 1031 against RS * U = 512
    for variant in ("pool_m0", "pool_m2"):
        for C in (8, 64, 280):
            for (B, H, W) in POOL_SHAPES:
                add(variant, B, H, W, C)
    for C in (40, 72):                                                               # CV = 5, 9
        for (H, W) in ((1, 1), (3, 11), (10, 10)):
            add("mul_m2", 3, H, W, C)
    # the multiplier through the U-unrolled row loop.  M = 99 in row blocks of 32, no more than the RS row lanes (256 at C = 8, 128 at
    # C = 64, 32 and - in its 3-vector last chunk - 85 at C = 280): every in-flight row after the first is a clamped re-read of the
    # block's last row, which can lie in another sample (HW = 33) than the row it stands in for
    for C in (8, 64, 280):
        add("mul_m2", 3, 11, 3, C)
    add("mul_m2", *REDUCE_MUL_RAGGED)
    for variant in ("mul_m0", "mul_m1", "two_mul_m0", "two_mul_m1"):
        for C in (8, 280):
            add(variant, 3, 11, 3, C)
    return out


# sentinel rows: (id, variant, (B, H, W, C)) - few row blocks, so that every block's first and last row gets a launch
SENTINEL_CASES = [("m2-c64", "m2", (1, 100, 1, 64)), ("m1-c64", "m1", (1, 100, 1, 64)), ("m2-c280", "m2", (1, 130, 1, 280)),
                  ("m0-c2048", "m0", (1, 300, 1, 2048)), ("pool_m2-c64", "pool_m2", (2, 6, 10, 64)), ("pool_m2-c280", "pool_m2", (2, 6, 10, 280)),
                  ("two_m1-c64", "two_m1", (1, 100, 1, 64)), ("mul_m2-c64", "mul_m2", (2, 50, 1, 64))]


def sentinel_rows(M, C):
    rows = {0, M - 1}
    for r0, r1 in row_blocks(M, C):
        rows.update((r0, r1 - 1))
    return sorted(rows)


SUM_NPARTS = [1, 15, 16, 17, 63, 64, 65, 130]
SUM_C = [8, 40]

# backward apply: (variant, dident, dy2, count_factor)
APPLY_FAST_CONFIGS = [("m2", None, True, 1), ("m1", "store", True, 1), ("m0", "accum", True, 2), ("two_m1", "accum", True, 1),
                      ("two_m0z", "store", False, 1), ("two_m1", None, True, 2)]
APPLY_FAST_BIG = [("m2", "accum", True, 1), ("two_m1", "store", True, 1)]           # U = 4 and U = 2 at partial_M
APPLY_GENERIC_CONFIGS = [("m2", None, True, 1), ("m1", "store", True, 2), ("m0", "accum", True, 1), ("two_m0", "store", True, 1),
                         ("two_m1", "accum", True, 1), ("two_m0", None, False, 1)]


def apply_cases():
    """(id, variant, dident, dy2, count_factor, (B, H, W, C))"""
    out = []

    def add(cfg, B, H, W, C):
        variant, dident, dy2, cf = cfg
        name = "%s-%s%s%s-%dx%dx%dx%d" % (variant, dident or "nodi", "" if dy2 else "-nody2", "-count2" if cf == 2 else "", B, H, W, C)
        out.append((name, variant, dident, dy2, cf, (B, H, W, C)))

    for C in FAST_C:
        small, big = fast_ladder(C)
        for M in small:
            for cfg in APPLY_FAST_CONFIGS:
                add(cfg, 1, M, 1, C)
        for cfg in APPLY_FAST_BIG:
            add(cfg, 1, big, 1, C)
    for C in (24, 40, 280):
        for cfg in APPLY_GENERIC_CONFIGS:
            add(cfg, 1, 33, 1, C)
        add(("pool_m2", None, True, 1), 1, 4, 6, C)
        add(("pool_m0", None, True, 2), 3, 2, 6, C)
        add(("mul_m2", None, True, 1), 3, 3, 11, C)
    add(("pool_m2", None, True, 1), 2, 4, 6, 64)
    add(("mul_m2", "store", True, 1), 3, 3, 11, 64)
    return out


# end to end through ops.bn_bwd: (id, variant, dident, (B, H, W, C))
E2E_CASES = [("plain", "m2", None, (2, 5, 7, 64)), ("plain-lin", "m0", None, (2, 5, 7, 40)), ("ident", "m1", "store", (2, 5, 7, 64)),
             ("pool", "pool_m2", None, (2, 6, 10, 72)), ("two", "two_m1", "accum", (2, 5, 7, 256)), ("two-lin", "two_m0", None, (2, 5, 7, 64)),
             ("mul", "mul_m2", None, (3, 3, 11, 40))]

# the two sides of 2^24 work items of the generic kernels, C = 40 (CV = 5): 16,777,215 and 16,777,220 vectors
DIV24_M = [3355443, 3355444]
