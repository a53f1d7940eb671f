"""Case tables, the float64 reference, the per-element bounds and the layout statements shared by tests/test_adam_edges.py (the
fused multi-tensor update of csrc/elementwise.hip on the GPU: adam_kernel<PT, MODE>, adam_pack_tile, unpack_grads_kernel,
grad_sumsq_kernel) and tests/test_adam_edges_cpu.py (the same checks against a plain torch fp32 evaluation and against wrong
ones, no GPU).  Nothing here imports the GPU library.

ONE STEP FROM AN ARBITRARY STATE.  Every check is a single update of fp32 p, m and v >= 0 that the test wrote (not zeros), so no
error hides in a later step or compounds from an earlier one.  The step is stated once (step_fn), as a function of a dtype:

    g~ = g * gscale / loss_scale      (+ wd * p when coupled)
    p_k = p * keep                    (decoupled only; keep = float32(1 - f64(lr) * f64(wd)); else p)
    m' = b1 * m + (1 - b1) * g~
    v' = b2 * v + (1 - b2) * g~^2
    p' = p_k - (lr / bc1) * m' / (sqrt(v') * rsb2 + eps)

Evaluated in float64 on the exact fp32 inputs it is the reference; evaluated in float32 it is the "correct fp32 implementation"
of the CPU file.  The fp32 coefficients the kernel receives are inputs, restated in numpy (coefs): bc1 / bc2 from the host formula
float32(1 - beta ** t) or, with the step count on the device, float32(1 - float64(float32(beta)) ** t); keep as above;
rsb2 = 1 / sqrt(float64(bc2)).

BOUNDS.  |got - ref| <= coef * S, S the same expression on absolute values:

    S_m = b1 |m| + (1 - b1) |g~|abs          |g~|abs = |g| gscale / loss_scale + wd |p|
    S_v = v'_ref                             all its terms are non-negative
    S_p = |p_k| + (lr / bc1) S_m / den_ref   the numerator may cancel, the denominator may not

coef is the number of separately rounded fp32 operations on the output's path (a fused multiply-add counts as the two roundings
it replaces, rsqrtf as two), rounded up to a power of two, times 2^-24:

    m'   gscale / loss_scale 1, g * gscale 1, wd * p 1, the sum 1, 1 - b1 1, its product with g~ 1, b1 * m 1, the sum 1 = 8
    v'   g~ as above 4, entering squared = 8; 1 - b2 1, two products 2, b2 * v 1, the sum 1                               = 13
         both <= 16: COEF_MV = 2^-20 (ABS_F32 of hip_ops_edge_cases)
    p'   on the update term: m' 8, lr / bc1 1, its product with m' 1, the division 1, and the denominator - sqrt of v' carries
         half of v's 13 = 6.5, sqrtf 1, rsqrtf(bc2) 2, the product 1, + eps 1 = 11.5 - together 22.5; the subtraction 1 more
         on the whole of S_p; p * keep 1 on |p_k|                                                                       = 23.5
         rounded up to 32: COEF_P = 2^-19

S_v = v'_ref and the "denominator does not cancel" of S_p hold because g~ does not cancel: without coupled decay it is one
product, and the coupled cases draw g with the sign of p (state), so that |g~| = |g~|abs there too.  Coefficients are not measured
and not widened; the worst observed ratios error / bound are printed by both test files.

LAYOUTS, stated in plain indexing, independent of the kernels and of cris_pack_weights (nct / gemm_index / F_index / D_index):
a logical weight is W[n][c][tap]; the parameter is stored [n][c][tap] or, transposed (one tap), [c][n], and so is its gradient
unless that is in the GEMM layout [n][tap][cpad] with NaN in the padding columns; F[n * ldF + tap * Cpad + c];
D[c * ldD + (taps - 1 - tap) * Npad + n].  After a step the live elements of each pack equal p_new.to(bfloat16) placed by these
statements, everything else of the pack's slab still holds GUARD_BITS.

No subnormal inputs or intermediates: every non-zero |g~| is >= 1e-15 (state: non-zero |g|, |m|, |p| >= 1e-6, v >= 1e-12)."""
import numpy as np
import torch

from hip_ops_edge_cases import ABS_F32, BF, F32, F64, GUARD_BITS, NAN, assert_bound, assert_exact, first_bad, gen

BLOCK_ELEMS = 8192                  # cris_adam_block_elems(), restated; both test files assert that the library agrees
AP_T = 64                           # channels of a packed tile
COEF_MV = ABS_F32                   # 2^-20
COEF_P = 2.0 ** -19
GUARD_BF = GUARD_BITS[BF]           # 0x7B5A fits int16
PRE = POST = 2                      # guard rows in front of and behind a pack
B1, B2, EPS = 0.9, 0.999, 1e-8
LRS3 = [4e-3, 1e-2, 2.5e-2]         # rate of tensor k: LRS3[k % 3] - neighbours in a table never share one
DECAYS4 = [0.5, 0.0, 0.25, 0.1]     # decay of tensor k under MODE 1 / 2: DECAYS4[k % 4] - neighbours differ, zeros among them


def pad8(n):
    return (n + 7) // 8 * 8


def tile_rows(taps):
    """output rows of a packed tile (AP_TN)"""
    return 32 if taps == 9 else 64


# ----------------------------------------------------------------------------------------------------
# tensors of a table
# ----------------------------------------------------------------------------------------------------
class T:
    """One tensor of a table.  kind: "plain" (n elements), "gemm" (not packed, gradient in the GEMM layout), "pack" (bf16 operand
    copies refreshed by the update), "rows" (V rows of D, `dead` rows without a gradient: row_live)."""

    def __init__(self, name, kind, n=0, N=0, Cin=0, taps=0, Cpad=None, Npad=None, transposed=False, grad_gemm=False, want_F=True,
                 want_D=True, ld_extra=0, dead=()):
        self.name, self.kind = name, kind
        self.N, self.Cin, self.taps = N, Cin, taps
        self.Cpad = Cpad if Cpad is not None else pad8(Cin)
        self.Npad = Npad if Npad is not None else pad8(N)
        self.transposed, self.want_F, self.want_D, self.ld_extra = transposed, want_F, want_D, ld_extra
        self.grad_gemm = grad_gemm or kind == "gemm" or (kind == "pack" and taps == 9)
        self.dead = tuple(dead)
        if kind == "plain":
            self.dims, self.names = (n,), ("i",)
        elif kind == "rows":
            self.dims, self.names = (N, Cin), ("row", "col")
        elif transposed:
            assert taps == 1 and not self.grad_gemm
            self.dims, self.names = (Cin, N), ("c", "n")
        else:
            self.dims, self.names = (N, Cin, taps), ("n", "c", "tap")
        self.numel = int(np.prod(self.dims))
        self.ldF = taps * self.Cpad + ld_extra
        self.ldD = taps * self.Npad + ld_extra

    @property
    def layout(self):
        """AdamTable(layouts=...) / UnpackTable entry"""
        return (self.N, self.Cin, self.taps, self.Cpad) if self.grad_gemm else None

    @property
    def grad_numel(self):
        return self.N * self.taps * self.Cpad if self.grad_gemm else self.numel

    @property
    def ragged_rows(self):
        return self.kind == "pack" and self.N % tile_rows(self.taps) != 0

    def dead_elems(self):
        m = torch.zeros(self.dims, dtype=torch.bool)
        if self.dead:
            m[list(self.dead)] = True
        return m.flatten()


def nct(t):
    """(n, c, tap) of every element of the stored parameter, in storage order"""
    if t.transposed:
        c, n = torch.meshgrid(torch.arange(t.Cin), torch.arange(t.N), indexing="ij")
        return n.flatten(), c.flatten(), torch.zeros(t.numel, dtype=torch.long)
    n, c, tap = torch.meshgrid(torch.arange(t.N), torch.arange(t.Cin), torch.arange(t.taps), indexing="ij")
    return n.flatten(), c.flatten(), tap.flatten()


def gemm_index(t):
    """GEMM-layout gradient [n][tap][cpad]: where the gradient of each stored parameter element lies"""
    n, c, tap = nct(t)
    return (n * t.taps + tap) * t.Cpad + c


def F_index(t):
    n, c, tap = nct(t)
    return n * t.ldF + tap * t.Cpad + c


def D_index(t, reverse=True):
    n, c, tap = nct(t)
    return c * t.ldD + ((t.taps - 1 - tap) if reverse else tap) * t.Npad + n


def grad_index(t):
    return gemm_index(t) if t.grad_gemm else torch.arange(t.numel)


def pack_geometry(t, which):
    """(rows, ld, index of every stored parameter element) of pack "F" / "D" """
    return (t.N, t.ldF, F_index(t)) if which == "F" else (t.Cin, t.ldD, D_index(t))


def place(t, which, values, index=None, keep=None):
    """image of a pack's whole slab [PRE + rows + POST][ld] as int16 bits: GUARD everywhere, `values` (bf16, storage order of the
    parameter) at the layout statement's places.  keep: elements that are placed (None: all).  Returns (image, live mask)."""
    rows, ld, idx = pack_geometry(t, which)
    idx = (idx if index is None else index) + PRE * ld
    img = torch.full(((PRE + rows + POST) * ld,), GUARD_BF, dtype=torch.int16)
    live = torch.zeros(img.numel(), dtype=torch.bool)
    live[idx] = True
    bits = values.to(BF).view(torch.int16).flatten()
    if keep is not None:
        idx, bits = idx[keep], bits[keep]
    img[idx] = bits
    return img.view(-1, ld), live.view(-1, ld)


def read_back(t, which, img):
    """the stored-order bf16 bits a pack image holds at the layout statement's places"""
    rows, ld, idx = pack_geometry(t, which)
    return img.flatten()[idx + PRE * ld]


# ----------------------------------------------------------------------------------------------------
# tables
# ----------------------------------------------------------------------------------------------------
class Case:
    """One table and one way to step it.  mode 0: cris_adam_step_amp with the scalar `wd`; 1 / 2: cris_adamw_step with
    DECAYS4, coupled / decoupled.  t: the step count - the host counter, or with step_dev the device's (the host's is then
    deliberately wrong).  gmag: scale of the gradients."""

    def __init__(self, name, tensors, mode=0, wd=0.0, gscale=1.0, loss_scale=None, gmag=1.0, t=3, step_dev=False, skip=False, seed=1):
        self.name, self.tensors, self.mode, self.wd = name, tensors, mode, wd
        self.gscale, self.loss_scale, self.gmag, self.t, self.step_dev, self.skip, self.seed = gscale, loss_scale, gmag, t, step_dev, skip, seed
        self.lrs = [LRS3[k % 3] for k in range(len(tensors))]
        self.decays = [DECAYS4[k % 4] for k in range(len(tensors))] if mode else None

    def decay(self, k):
        return self.decays[k] if self.mode else self.wd

    def coupled(self, k):
        return self.mode != 2 and self.decay(k) != 0

    def marks_honoured(self, k):
        """dead rows are skipped only while the tensor's decay is 0 (cris_adam_desc.row_live)"""
        return bool(self.tensors[k].dead) and self.decay(k) == 0

    def __repr__(self):
        return self.name


E = BLOCK_ELEMS
PLAIN = [T("n%d" % n, "plain", n=n) for n in (1, 255, 256, 257, E - 1, E, E + 1, 2 * E + 3)]
GEMM = [T("g%dx%dx%d/%d" % s, "gemm", N=s[0], Cin=s[1], taps=s[2], Cpad=s[3]) for s in ((5, 3, 9, 8), (3, 5, 1, 8), (24, 20, 9, 24), (16, 60, 9, 64))]
PACK9 = [T("w9-%dx%d" % s, "pack", N=s[0], Cin=s[1], taps=9) for s in ((1, 1), (31, 63), (32, 64), (33, 65), (70, 66))] + [
    T("w9-33x65-wide", "pack", N=33, Cin=65, taps=9, Cpad=pad8(65) + 8, Npad=pad8(33) + 8),
    T("w9-31x63-Fonly", "pack", N=31, Cin=63, taps=9, want_D=False),
    T("w9-33x65-Donly", "pack", N=33, Cin=65, taps=9, want_F=False),
    T("w9-32x64-ld+64", "pack", N=32, Cin=64, taps=9, ld_extra=64)]
_P1 = ((1, 1), (63, 64), (64, 63), (65, 65), (130, 70))
PACK1 = [T("w1-%dx%d" % s, "pack", N=s[0], Cin=s[1], taps=1) for s in _P1] + [
    T("w1T-%dx%d" % s, "pack", N=s[0], Cin=s[1], taps=1, transposed=True) for s in _P1] + [
    T("w1-65x65-gemmgrad", "pack", N=65, Cin=65, taps=1, Cpad=80, grad_gemm=True),
    T("w1-63x64-Fonly", "pack", N=63, Cin=64, taps=1, want_D=False),
    T("w1T-64x63-Donly", "pack", N=64, Cin=63, taps=1, transposed=True, want_F=False)]
# dead rows: the first, the last, and (400 x 48: element 8192 lies in row 170) the rows on either side of a block edge
ROWS = [T("r400x48", "rows", N=400, Cin=48, dead=(0, 170, 171, 399)), T("r7x33", "rows", N=7, Cin=33, dead=(0, 2, 6)),
        T("r300x1", "rows", N=300, Cin=1, dead=(0, 5, 299))]
LOOKUP257 = [T("t%d" % k, "plain", n=1 + k % 5) for k in range(257)]
LOOKUP3 = [T("t%d" % k, "plain", n=1 + k % 5) for k in range(3)]
# one shape of each family; under DECAYS4 the first row-marked tensor (k = 5) is exempt - its marks count - and the second (k = 6)
# is decayed - its marks are ignored
SUBSET = [T("n%d" % (E + 1), "plain", n=E + 1), T("g16x60x9/64", "gemm", N=16, Cin=60, taps=9, Cpad=64), T("w9-33x65", "pack", N=33, Cin=65, taps=9),
          T("w1-65x65", "pack", N=65, Cin=65, taps=1), T("w1T-64x63", "pack", N=64, Cin=63, taps=1, transposed=True),
          T("r7x33", "rows", N=7, Cin=33, dead=(0, 2, 6)), T("r300x1", "rows", N=300, Cin=1, dead=(0, 5, 299))]
assert DECAYS4[5 % 4] == 0 and DECAYS4[6 % 4] != 0

CASES = [Case("plain", PLAIN), Case("gemm", GEMM), Case("pack9", PACK9), Case("pack1", PACK1), Case("rows", ROWS),
         Case("lookup257", LOOKUP257), Case("lookup3", LOOKUP3),
         Case("lookup257-coupled", LOOKUP257, mode=1), Case("lookup257-decoupled", LOOKUP257, mode=2),
         Case("lookup3-coupled", LOOKUP3, mode=1), Case("lookup3-decoupled", LOOKUP3, mode=2),
         Case("subset-wd0.5", SUBSET, wd=0.5), Case("subset-coupled", SUBSET, mode=1), Case("subset-decoupled", SUBSET, mode=2),
         Case("subset-scaled", SUBSET, gscale=0.5, loss_scale=65536.0, gmag=3e3),
         Case("subset-t1", SUBSET, t=1, step_dev=True), Case("subset-t7", SUBSET, t=7, step_dev=True),
         Case("subset-t1000", SUBSET, t=1000, step_dev=True),
         Case("subset-skip", SUBSET, mode=2, skip=True)]

# cris_unpack_grads: the unpacked GEMM-layout tensors, a table of one, a table of 257 small ones
_U5 = [(1, 1, 9, 8), (2, 3, 1, 8), (1, 2, 9, 8), (3, 1, 1, 8), (2, 2, 9, 16)]
UNPACK_CASES = {"gemm": GEMM, "one": GEMM[:1],
                "lookup257": [T("u%d" % k, "gemm", N=_U5[k % 5][0], Cin=_U5[k % 5][1], taps=_U5[k % 5][2], Cpad=_U5[k % 5][3]) for k in range(257)]}


# ----------------------------------------------------------------------------------------------------
# state, coefficients, the step
# ----------------------------------------------------------------------------------------------------
def _floor(x, lo):
    """non-zero magnitudes below `lo` raised to it (no subnormal inputs or intermediates)"""
    small = (x != 0) & (x.abs() < lo)
    return torch.where(small, torch.where(x < 0, -lo, lo).to(x.dtype), x)


def state(case, k):
    """p, g, m, v of tensor k in storage order (fp32, CPU) and `gbuf`, the gradient buffer as the kernel gets it.  m ~ N(0, 0.1),
    v a squared normal; by element index i, r = (7 i + 3 k) % 16: r = 0: g = m = v = 0; 1: p = 0; 2: v = 0; 3: g = m = v = p = 0.
    Coupled decay: g takes the sign of p (the module docstring says why).  Dead rows: random p, m, v; g NaN where the marks
    count, 0 where the decay makes the kernel ignore them."""
    t = case.tensors[k]
    n, s = t.numel, 100000 * case.seed + 16 * k
    p = _floor(torch.randn(n, generator=gen(s)), 1e-6)
    g = _floor(torch.randn(n, generator=gen(s + 1)) * case.gmag, 1e-6).clamp(-1e4, 1e4)
    m = _floor(torch.randn(n, generator=gen(s + 2)) * 0.1, 1e-6)
    v = (torch.randn(n, generator=gen(s + 3)) * 0.1) ** 2
    v = torch.where(v < 1e-12, torch.full_like(v, 1e-12), v)
    r = (7 * torch.arange(n) + 3 * k) % 16
    zero = torch.zeros(n)
    g = torch.where((r == 0) | (r == 3), zero, g)
    m = torch.where((r == 0) | (r == 3), zero, m)
    v = torch.where((r == 0) | (r == 2) | (r == 3), zero, v)
    p = torch.where((r == 1) | (r == 3), zero, p)
    if case.coupled(k):
        g = torch.where(p != 0, g.abs() * torch.sign(p), g)
    dead = t.dead_elems()
    if t.dead:
        g = torch.where(dead, torch.full_like(g, NAN if case.marks_honoured(k) else 0.0), g)
    gbuf = torch.full((t.grad_numel,), NAN)
    gbuf[grad_index(t)] = g
    return dict(p=p, g=g, m=m, v=v, gbuf=gbuf, dead=dead if case.marks_honoured(k) else torch.zeros(n, dtype=torch.bool))


def keep_of(lr, wd):
    """the kernel's factor of decoupled decay, restated in numpy (as in test_adamw_gpu.py)"""
    return np.float32(1.0 - np.float64(np.float32(lr)) * np.float64(np.float32(wd)))


def bias_corrections(case, t):
    if case.step_dev:               # on the device: float32(1 - pow((double)beta_f32, t))
        return tuple(np.float32(1.0 - np.float64(np.float32(b)) ** t) for b in (B1, B2))
    return tuple(np.float32(1.0 - b ** t) for b in (B1, B2))         # ops.AdamTable.step: python doubles, rounded at the call


def coefs(case, k, mutate=None):
    """the fp32 coefficients of tensor k's update, as the kernel receives or derives them"""
    n = len(case.tensors)
    lr = np.float32(case.lrs[(k + 1) % n] if mutate == "neighbour_lr" else case.lrs[k])
    bc1, bc2 = bias_corrections(case, case.t - 1 if mutate == "bc_prev" else case.t)
    wd = np.float32(case.decay(k))
    decoupled = case.mode == 2 and mutate != "coupled_for_decoupled"
    with np.errstate(divide="ignore"):
        rsb2 = np.float64(1.0) / np.sqrt(np.float64(bc2))
    return dict(lr=lr, b1=np.float32(B1), b2=np.float32(B2), eps=np.float32(0.0 if mutate == "no_eps" else EPS), bc1=bc1, rsb2=rsb2,
                gs=np.float32(case.gscale), ls=None if case.loss_scale is None else np.float32(case.loss_scale),
                wd=np.float32(0.0) if decoupled else wd, keep=keep_of(lr, wd) if decoupled else None,
                keep_after=mutate == "keep_after")


def step_fn(p, g, m, v, co, dt):
    """the update at dtype dt; the scales S are meaningful at float64"""
    def c(x):
        return torch.tensor(float(x), dtype=F64).to(dt)
    p, g, m, v = p.to(dt), g.to(dt), m.to(dt), v.to(dt)
    one = torch.ones((), dtype=dt)
    gs = c(co["gs"]) if co["ls"] is None else c(co["gs"]) / c(co["ls"])
    gt, ga = g * gs, g.abs() * gs
    if co["wd"] != 0:
        gt, ga = gt + c(co["wd"]) * p, ga + c(co["wd"]) * p.abs()
    pk = p if co["keep"] is None or co["keep_after"] else p * c(co["keep"])
    m2 = c(co["b1"]) * m + (one - c(co["b1"])) * gt
    v2 = c(co["b2"]) * v + (one - c(co["b2"])) * gt * gt
    step = c(co["lr"]) / c(co["bc1"])
    den = v2.sqrt() * c(co["rsb2"]) + c(co["eps"])
    p2 = pk - step * m2 / den
    if co["keep"] is not None and co["keep_after"]:
        p2 = p2 * c(co["keep"])
    Sm = c(co["b1"]) * m.abs() + (one - c(co["b1"])) * ga
    return dict(p=p2, m=m2, v=v2, pk=pk, gt=gt, Sm=Sm, Sv=v2, Sp=pk.abs() + step * Sm / den)


def reference(case, k, st):
    """float64 p', m', v' and their scales; on dead rows whose marks count, and everywhere in a skipped step, the state itself
    with scale 0 (bit for bit is asserted separately)"""
    ref = step_fn(st["p"], torch.nan_to_num(st["g"]), st["m"], st["v"], coefs(case, k), F64)
    same = torch.ones_like(st["dead"]) if case.skip else st["dead"]
    out = {}
    for key, S in (("p", "Sp"), ("m", "Sm"), ("v", "Sv")):
        out[key] = torch.where(same, st[key].double(), ref[key])
        out[S] = torch.where(same, torch.zeros((), dtype=F64), ref[S])
    # elements whose g~, m and v are zero: p' is p_k exactly (the product of two fp32 values is exact in float64: one rounding)
    out["still"] = (ref["gt"] == 0) & (st["m"] == 0) & (st["v"] == 0) & ~same
    out["pk32"] = ref["pk"].float()
    out["update"] = ref["p"] - ref["pk"]
    return out


# ----------------------------------------------------------------------------------------------------
# a plain torch evaluation of a whole table (the CPU file: correct, or wrong in one named way)
# ----------------------------------------------------------------------------------------------------
MUTATIONS = ["swap_tap_channel", "d_not_reversed", "bc_prev", "no_eps", "neighbour_lr", "coupled_for_decoupled", "keep_after",
             "stale_last_row"]


def applies(mutate, case):
    if case.skip:
        return False
    ts = case.tensors
    if mutate == "swap_tap_channel":
        return any(t.grad_gemm and t.taps > 1 for t in ts)
    if mutate == "d_not_reversed":
        return any(t.kind == "pack" and t.want_D and t.taps > 1 for t in ts)
    if mutate in ("coupled_for_decoupled", "keep_after"):
        return case.mode == 2 and any(d != 0 for d in case.decays)
    if mutate == "stale_last_row":
        return any(t.ragged_rows for t in ts)
    return True


def emulate(case, states, dt=F32, mutate=None):
    """result of the table's step as {p, m, v [, F, D]} per tensor: fp32 state in storage order, pack images as int16 bits"""
    out = []
    for k, t in enumerate(case.tensors):
        st = states[k]
        gi = grad_index(t)
        if mutate == "swap_tap_channel" and t.grad_gemm:         # the gradient read as [n][cpad][tap]
            n, c, tap = nct(t)
            gi = (n * t.Cpad + c) * t.taps + tap
        g = st["gbuf"][gi]
        new = {key: st[key].clone() for key in ("p", "m", "v")}
        done = torch.zeros(t.numel, dtype=torch.bool)
        if not case.skip:
            done = ~st["dead"]
            if mutate == "stale_last_row" and t.ragged_rows:
                done = done & (nct(t)[0] != t.N - 1)
            r = step_fn(st["p"], g, st["m"], st["v"], coefs(case, k, mutate), dt)
            for key in new:
                new[key] = torch.where(done, r[key].float(), st[key])
        if t.kind == "pack":
            if t.want_F:
                new["F"] = place(t, "F", new["p"], keep=done)[0]
            if t.want_D:
                new["D"] = place(t, "D", new["p"], index=D_index(t, reverse=mutate != "d_not_reversed"), keep=done)[0]
        out.append(new)
    return out


# ----------------------------------------------------------------------------------------------------
# the checks, shared by the GPU run and the CPU evaluations
# ----------------------------------------------------------------------------------------------------
def _ratio(got, ref, S, coef):
    err, lim = (got.double() - ref).abs(), coef * S
    ok = lim > 0
    return float((err[ok] / lim[ok]).max()) if bool(ok.any()) else 0.0


def check_pack(t, which, img, p_new, what, written=True):
    """live elements = p_new.to(bfloat16) at the layout statement's places, bit for bit; the rest of the slab = GUARD_BITS.
    written=False (a skipped step): the whole slab still holds GUARD_BITS."""
    want, live = place(t, which, p_new)
    slab = "%s pack %s" % (what, which)
    assert img.shape == want.shape and img.dtype == torch.int16, "%s: image %s %s" % (slab, tuple(img.shape), img.dtype)
    if not written:
        live = torch.zeros_like(live)
    bad = (img != GUARD_BF) & ~live
    assert not bool(bad.any()), "%s: %d guard elements of the slab overwritten; first at %s (%d rows in front, ld %d)" % (
        slab, int(bad.sum()), first_bad(bad, names=("slab row", "col")), PRE, img.shape[1])
    if written:
        assert_exact(read_back(t, which, img).view(BF).view(t.dims), read_back(t, which, want).view(BF).view(t.dims), slab, names=t.names)


def check(case, states, result, report=None):
    """every tensor of the table against the reference.  report: {"p" / "m" / "v": worst error / bound so far}, updated."""
    for k, t in enumerate(case.tensors):
        st, got = states[k], result[k]
        what = "%s/%s" % (case.name, t.name)
        ref = reference(case, k, st)
        same = torch.ones_like(st["dead"]) if case.skip else st["dead"]
        for key, S, coef in (("m", "Sm", COEF_MV), ("v", "Sv", COEF_MV), ("p", "Sp", COEF_P)):
            x = got[key]
            assert x.dtype == F32 and x.numel() == t.numel, "%s %s: %s %s" % (what, key, x.dtype, tuple(x.shape))
            x = x.flatten()
            zero = torch.zeros_like(x)
            assert_exact(torch.where(same, x, zero).view(t.dims), torch.where(same, st[key], zero).view(t.dims),
                         "%s %s of rows without a gradient / of a skipped step" % (what, key), names=t.names)
            assert_bound(x.view(t.dims), ref[key].view(t.dims), ref[S].view(t.dims), 0.0, coef, "%s %s'" % (what, key), names=t.names)
            if report is not None:
                report[key] = max(report.get(key, 0.0), _ratio(x, ref[key], ref[S], coef))
        x, zero = got["p"].flatten(), torch.zeros(t.numel)
        assert_exact(torch.where(ref["still"], x, zero).view(t.dims), torch.where(ref["still"], ref["pk32"], zero).view(t.dims),
                     "%s p' where g~ = m = v = 0 (p_k exactly)" % what, names=t.names)
        if t.kind == "pack":
            for which, wanted in (("F", t.want_F), ("D", t.want_D)):
                assert (which in got) == wanted, "%s pack %s" % (what, which)
                if wanted:
                    check_pack(t, which, got[which], got["p"], what, written=not case.skip)


def grad_sumsq_reference(states):
    """float64 sum of squares of every tensor's logical gradient (dead rows whose marks count are not part of it: NaN there)"""
    return [float((torch.nan_to_num(st["g"]).double() ** 2).sum()) for st in states]
