"""Case tables, float64 references, per-element bounds and an fp32 emulation of the six attention kernels (csrc/attention.hip),
shared by tests/test_attn_edges.py (the HIP kernels on the GPU) and tests/test_attn_edges_cpu.py (the emulation and the tables
against the same bounds, no GPU).  Buffers, comparisons and the form of the bound are those of tests/hip_ops_edge_cases.py.

The operations (every input rounded to bf16 first; s = scale * Q K^T; a key is valid unless it is padded - token 0 - or, under
the causal mask, later than the query; keep = oracle.dropout_hash.keep_mask over [B][Hn][Lq][Lk]; r = 1 / (1 - p)):

    forward     m = max over valid keys, lse = m + log sum exp(s - m), P = exp(s - lse) on valid keys and 0 elsewhere,
                O = (P * keep * r) V.  A row without a valid key has O = +0 and lse = +inf.
    bwd_dq      of GIVEN O (the float64 O rounded to bf16), lse (rounded to fp32) and dO - not of the forward kernel's output:
                delta = rowsum(dO * O), P = exp(s - lse), dS = P * (keep * r * (dO V^T) - delta), dQ = scale * dS K.
    bwd_dkv     of the same and of GIVEN delta (the float64 delta rounded to fp32):
                dV = (P * keep * r)^T dO, dK = scale * dS^T Q.
                A row without a valid key has lse = +inf, hence P = 0: dQ = 0 and no contribution to dK, dV.

The bound is |got - ref| <= REL * |ref| + C * S per element, S the same product evaluated in float64 on absolute values:

    S_O = Pd |V|                       Pd = P * keep * r
    S_dV = Pd^T |dO|
    dSabs = P * (keep * r * (|dO| |V|^T) + sum_d |dO| |O|)
    S_dQ = scale * dSabs |K|,  S_dK = scale * dSabs^T |Q|

bf16 results (O, dQ, dK, dV): REL = 2^-8 (REL_BF16: the rounding of the result), C = 2^-7 = 2^-8 + 2^-8:
  * 2^-8 S for the ONE rounding to bf16 inside the kernel - of P (forward, dV) or of dS (dQ, dK) in pack_frag, before the second
    MFMA product.  Half a bf16 ulp is at most 2^-8 of the value, every term of the second product is off by at most that fraction
    of itself, and the terms in absolute value sum to S.  (In the forward the rounded value is exp(s - running max), rescaled
    later in fp32: the error stays relative.)
  * 2^-8 S in reserve for everything that is fp32: the relative error e of P itself (below), the fp32 accumulation of the second
    product and of the running sum (at most Lk 2^-24 <= 2^-15 for the 449 rows of the largest case, in fact a few tens of
    roundings: 8 terms per lane, two cross-lane adds, one update per 32-key step), the fp32 value of 1 / (1 - p) (2^-23), the
    final scaling by 1 / l or by `scale`, and for dS the fp32 products dO V^T and delta (64 terms each, 2^-18 of their absolute
    sums, which dSabs contains).  These add up to e + 2^-14 at the very most, so the reserve holds while e <= 2^-9 - a CONDITION
    that check_case() asserts for every case, with

        e = abs_coef(64) * scale * max_{q,k} sum_d |Q_qd| |K_kd|  +  2^-22 * max_{valid q,k} |s - lse|

    the first term being the fp32 accumulation of a 64-term score (an absolute error of the exponent = a relative error of P), the
    second the argument scaling of __expf (exp2(x * log2 e): the product rounds to 2^-24 |x| log2 e, times ln 2 in the result) plus
    the unit in the last place of the hardware exp2 and of the subtraction s - m or s - lse.
  With |ref| <= S a correct kernel reaches at most (2^-8 + 2^-8 (1 + small)) / (2^-8 + 2^-7) = 2/3 of the bound; the CPU test holds
  the emulation below to 0.75.

delta (fp32): REL = 0, C = abs_coef(64) = 2^-18 on S_delta = sum_d |dO| |O| (64 exact products accumulated in fp32).

lse (fp32), an absolute bound:  2 e + 2^-17 + 2^-22 (|m| + |lse|), counted as
  * e: log-sum-exp is 1-Lipschitz in the maximum norm of the scores, so the score errors (first term of e) move it by at most that;
    the kernel's m is one of its own computed scores, so its error is inside this term and needs no other;
  * e: the running sum l = sum exp(s - m) carries the relative error of its terms (the second term of e; the whole of e is
    taken, which is more than needed) and log l moves by dl / l;
  * 2^-17: the fp32 accumulation of l and its rescaling (at most 10 + 2 * steps <= 40 roundings of 2^-24 relative, 2^-18.7), and
    __logf = log2(l) * ln 2 with l in [1, Lk]: one unit in the last place of log2 l <= 9 and the rounding of the product, 2^-19.8;
  * 2^-22 (|m| + |lse|): the final addition m + log l rounds to 2^-24 |lse|, the comparison reads an fp32 result against a
    float64 reference (another 2^-24 |lse|), and m enters as an fp32 number next to s (2^-24 |m|); the factor 4 is slack.
A row without a valid key must give exactly +inf.

What settles that these bounds admit a correct kernel is emulate(): plain torch fp32, online softmax in 32-key steps, rounding to
bf16 exactly where the kernels round (P, dS, the results).  Its switches restate seven plausible kernel errors, each of which the
bounds must refuse in a named case (tests/test_attn_edges_cpu.py).
"""
import functools
import math
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional, Tuple

import torch

from hip_ops_edge_cases import BF, F32, F64, REL_BF16, Slab, abs_coef, gen, randn_bf
from oracle import dropout_hash

SCALE = 0.125                      # 64 ** -0.5, exact in fp32
SEED, STREAM = 4321, 2
SEED_HOST, SEED_DEV = 4000, 321    # the split seed: drop.seed + the device word = SEED
C_BF16 = 2.0 ** -7
E_LIMIT = 2.0 ** -9
EMU_RATIO_LIMIT = 0.75
LDS_MIN = 384                      # fewest loop rows that take the LDS kernels (csrc/attention.hip: ATTN_LDS_MIN)
PAD_HUGE = 2.0 ** 100              # exact in bf16
LAUNCHERS = ("fwd", "dq", "dkv")   # cris_attn_plan's `which`, in order
OUTPUTS = {"fwd": ("O", "lse"), "dq": ("delta", "dQ"), "dkv": ("dK", "dV")}
BUGS = "abcdefg"


def pad32(n):
    return (n + 31) // 32 * 32


def cdiv(a, b):
    return (a + b - 1) // b


@dataclass(frozen=True)
class Case:
    name: str
    B: int
    Hn: int
    Lq: int
    Lk: int
    p: float = 0.0
    causal: bool = False
    mask: Optional[str] = None          # None | "pad4" (the four masks of the Lk = 22 table) | "pad2" (suffix + holes, Lk = 17)
    layout: str = "plain"               # "plain" | "sliced"
    self_attn: bool = False             # sliced: Q, K, V in one buffer
    pattern: str = "randn"              # "randn" | "rise" | "fall"
    split_seed: bool = False
    plan: Tuple[int, int, int] = (0, 0, 0)      # expected cris_attn_plan of fwd, dq, dkv

    @property
    def E(self):
        return self.Hn * 64

    def grid_total(self, launcher):
        return cdiv(self.Lk if launcher == "dkv" else self.Lq, 64) * self.B * self.Hn


# ----------------------------------------------------------------------------------------------------
# case tables
# ----------------------------------------------------------------------------------------------------
def _direct_cases():
    out = []
    n = 0
    for Lq in (1, 16, 17, 63, 65):
        for Lk in (1, 31, 32, 33, 65):
            out.append(Case("d-q%d-k%d" % (Lq, Lk), 2, 3, Lq, Lk, layout="sliced" if n % 3 == 0 else "plain", self_attn=Lq == Lk))
            n += 1
    for (Lq, Lk) in ((1, 1), (17, 33), (63, 31), (65, 65)):
        lay = "sliced" if Lq in (17, 65) else "plain"
        out.append(Case("drop-q%d-k%d" % (Lq, Lk), 2, 3, Lq, Lk, p=0.5, layout=lay, self_attn=Lq == Lk))
        out.append(Case("dropsplit-q%d-k%d" % (Lq, Lk), 2, 3, Lq, Lk, p=0.5, layout=lay, self_attn=Lq == Lk, split_seed=True))
    for L in (1, 16, 17, 33, 77):
        out.append(Case("causal-%d" % L, 2, 3, L, L, causal=True, layout="sliced" if L in (17, 77) else "plain", self_attn=True))
    out.append(Case("causal-drop-33", 2, 3, 33, 33, p=0.1, causal=True, layout="sliced", self_attn=True))
    for Lq in (17, 70):
        out.append(Case("pad-q%d" % Lq, 4, 3, Lq, 22, mask="pad4", layout="sliced" if Lq == 70 else "plain"))
    out.append(Case("rise-k65", 2, 3, 17, 65, pattern="rise", layout="sliced"))
    out.append(Case("fall-k65", 2, 3, 17, 65, pattern="fall"))
    return out


# (B, Hn) per LDS case: with one and with two 64-row tiles per (batch, head) the grid totals are 6, 9, 15, 12 and 12, 18, 30, 24 -
# one below 8, one = 1, one = 7 and one = 0 (mod 8): the remainder branches of al_block
_LDS_BH = [(2, 3), (3, 3), (5, 3), (4, 3)]


def _lds_cases():
    out = []
    for i, Lk in enumerate((384, 385, 416, 417, 448, 449)):
        B, Hn = _LDS_BH[i % 4]
        for Lq in (1, 70):
            for p in (0.0, 0.1):
                out.append(Case("lds-q%d-k%d-p%g" % (Lq, Lk, p), B, Hn, Lq, Lk, p=p, layout="sliced", plan=(1, 1, 0)))
    out.append(Case("lds-edge-q70-k383", 2, 3, 70, 383, p=0.1, layout="sliced", plan=(0, 0, 0)))
    for i, Lq in enumerate((384, 385, 417, 449)):
        B, Hn = _LDS_BH[i % 4]
        for (Lk, mask) in ((1, None), (17, "pad2"), (65, None)):
            for p in (0.0, 0.1):
                out.append(Case("ldskv-q%d-k%d-p%g" % (Lq, Lk, p), B, Hn, Lq, Lk, p=p, mask=mask, layout="sliced", plan=(0, 0, 1)))
    out.append(Case("ldskv-edge-q383-k17", 2, 3, 383, 17, p=0.1, mask="pad2", layout="sliced", plan=(0, 0, 0)))
    out.append(Case("lds-self-385", 2, 3, 385, 385, p=0.1, layout="sliced", self_attn=True, plan=(1, 1, 1)))
    out.append(Case("lds-rise-k449", 2, 3, 70, 449, pattern="rise", layout="sliced", plan=(1, 1, 0)))
    out.append(Case("lds-fall-k449", 2, 3, 70, 449, pattern="fall", layout="sliced", plan=(1, 1, 0)))
    return out


DIRECT_CASES = _direct_cases()
LDS_CASES = _lds_cases()
CASES = DIRECT_CASES + LDS_CASES
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# one case per kernel whose second launch must be bit-identical: (case, launcher, expected plan)
DETERMINISM = [("drop-q65-k65", "fwd", 0), ("drop-q65-k65", "dq", 0), ("drop-q65-k65", "dkv", 0),
               ("lds-self-385", "fwd", 1), ("lds-self-385", "dq", 1), ("lds-self-385", "dkv", 1)]
# the named cases in which each emulation switch must break a bound, and the outputs that must see it
BUG_CASES = {
    "a": [("d-q17-k33", ("O", "lse")), ("lds-q70-k385-p0", ("O", "lse"))],
    "b": [("causal-17", ("O", "lse", "dQ", "dK", "dV"))],
    "c": [("pad-q17", ("O", "lse", "dQ", "dK", "dV")), ("ldskv-q385-k17-p0", ("dK", "dV"))],
    "d": [("drop-q17-k33", ("O", "dQ", "dK", "dV")), ("lds-q70-k449-p0.1", ("O", "dQ"))],
    "e": [("d-q17-k33", ("lse", "delta", "dQ", "dK", "dV")), ("ldskv-q385-k65-p0", ("dK", "dV"))],
    "f": [("d-q17-k33", ("O", "lse", "dQ")), ("lds-q70-k417-p0", ("O", "lse", "dQ")), ("ldskv-q417-k65-p0", ("dK", "dV"))],
    "g": [("rise-k65", ("O",)), ("lds-rise-k449", ("O",))],
}


def key_tokens(c):
    """int64 [B][Lk] or None; 0 = padded"""
    if c.mask is None:
        return None
    t = torch.arange(1, c.Lk + 1, dtype=torch.int64).repeat(c.B, 1) + 10
    if c.mask == "pad4":
        assert c.B == 4 and c.Lk == 22
        t[0, 9:] = 0                # suffix padding
        t[1, 3] = t[1, 16] = 0      # holes; key 16 is the first key of the second 16-key MFMA block
        t[2, 1:] = 0                # only key 0 valid
        t[3, :] = 0                 # nothing valid: the fully masked contract
    else:
        assert c.mask == "pad2" and c.Lk == 17 and c.B >= 2
        t[0, 9:] = 0
        t[1, 3] = t[1, 16] = 0
    return t


def heads(x, B, L, Hn):
    """[B*L][Hn*64] -> [B][Hn][L][64]"""
    return x.reshape(B, L, Hn, 64).permute(0, 2, 1, 3)


def tokens_major(xh):
    """[B][Hn][L][64] -> [B*L][Hn*64]"""
    B, Hn, L, _ = xh.shape
    return xh.permute(0, 2, 1, 3).reshape(B * L, Hn * 64)


def _inputs(c):
    B, Hn, Lq, Lk, E = c.B, c.Hn, c.Lq, c.Lk, c.E
    if c.pattern == "randn":
        q, k = randn_bf((B * Lq, E), 101), randn_bf((B * Lk, E), 102)
    else:
        # scores 4 * g_k + noise with g running over 7.5 in all: they rise (fall) by about 30 along the keys
        u = torch.zeros(64)
        u[:16] = 1.0
        g = 7.5 * torch.arange(Lk, dtype=F32) / max(Lk - 1, 1)
        if c.pattern == "fall":
            g = g.flip(0)
        q = (2.0 * u.repeat(Hn)[None, :] + 0.05 * torch.randn(B * Lq, E, generator=gen(101))).to(BF).float()
        k = (g.repeat(B)[:, None] * u.repeat(Hn)[None, :] + 0.05 * torch.randn(B * Lk, E, generator=gen(102))).to(BF).float()
    return q, k, randn_bf((B * Lk, E), 103), randn_bf((B * Lq, E), 104)


def _keep_full(c, stride, cols):
    """keep decisions at index (bh * Lq + q) * stride + kk for kk < cols, bool [B][Hn][Lq][cols]"""
    rows = c.B * c.Hn * c.Lq
    flat = torch.from_numpy(dropout_hash.keep_mask(SEED, STREAM, rows * stride + cols, c.p))
    idx = torch.arange(rows)[:, None] * stride + torch.arange(cols)[None, :]
    return flat[idx].view(c.B, c.Hn, c.Lq, cols)


def _valid(c, toks, Lcols=None, causal_ge=False, batch0=False):
    """bool [B][1][Lq][Lcols]: key kk may be attended (columns beyond Lk read the clamped last token)"""
    Lcols = c.Lk if Lcols is None else Lcols
    kk = torch.arange(Lcols)
    ok = torch.ones(c.B, 1, c.Lq, Lcols, dtype=torch.bool)
    if c.causal:
        qq = torch.arange(c.Lq)[:, None]
        ok &= ~((kk[None, :] >= qq) if causal_ge else (kk[None, :] > qq))
    if toks is not None:
        t = toks[:, kk.clamp(max=c.Lk - 1)] != 0
        if batch0:
            t = t[:1].expand(c.B, -1)
        ok &= t[:, None, None, :]
    return ok


@functools.lru_cache(maxsize=None)
def reference(name):
    """inputs, float64 results, scales and bounds of a case; computed once, never modified"""
    c = BY_NAME[name]
    B, Hn, Lq, Lk = c.B, c.Hn, c.Lq, c.Lk
    q, k, v, do = _inputs(c)
    toks = key_tokens(c)
    qh, kh, vh, doh = (heads(t.double(), B, L, Hn) for t, L in ((q, Lq), (k, Lk), (v, Lk), (do, Lq)))
    r = 1.0 / (1.0 - c.p)
    keep = _keep_full(c, Lk, Lk).double() if c.p > 0 else torch.ones(1, 1, 1, 1, dtype=F64)
    valid = _valid(c, toks).expand(B, Hn, Lq, Lk)
    s = (qh @ kh.transpose(-1, -2)) * SCALE
    sm = s.masked_fill(~valid, -math.inf)
    m = sm.max(-1).values
    dead = m == -math.inf
    m0 = m.masked_fill(dead, 0.0)
    lsum = torch.exp(sm - m0[..., None]).sum(-1)
    lse = torch.where(dead, torch.full_like(m, math.inf), m0 + torch.log(lsum.masked_fill(dead, 1.0)))
    P = torch.exp(sm - lse.masked_fill(dead, 0.0)[..., None]).masked_fill(~valid, 0.0)
    Pd = P * keep * r
    O = Pd @ vh
    S_O = Pd @ vh.abs()
    assert bool((O[dead] == 0).all())
    # the backward of GIVEN O (bf16), lse (fp32) and, for the key side, delta (fp32)
    O_bf = O.to(BF)
    lse32 = lse.float()
    Ob = O_bf.double()
    delta = (doh * Ob).sum(-1)
    S_delta = (doh.abs() * Ob.abs()).sum(-1)
    delta32 = delta.float()
    Pg = torch.exp(sm - lse32.double()[..., None]).masked_fill(~valid, 0.0)          # lse = inf -> 0
    Pgd = Pg * keep * r
    dP = (doh @ vh.transpose(-1, -2)) * keep * r
    dS = Pg * (dP - delta[..., None])
    dS_kv = Pg * (dP - delta32.double()[..., None])
    dSabs = Pg * ((doh.abs() @ vh.abs().transpose(-1, -2)) * keep * r + S_delta[..., None])
    dQ = SCALE * (dS @ kh)
    dK = SCALE * (dS_kv.transpose(-1, -2) @ qh)
    dV = Pgd.transpose(-1, -2) @ doh
    # the condition of the reserve, and the lse bound
    e = abs_coef(64) * SCALE * float((qh.abs() @ kh.abs().transpose(-1, -2)).max())
    live = valid & ~dead[..., None]
    if bool(live.any()):
        e += 2.0 ** -22 * float((sm - lse[..., None])[live].abs().max())
    lse_fin = lse.masked_fill(dead, 0.0)
    lse_bound = (2 * e + 2.0 ** -17 + 2.0 ** -22 * (m0.abs() + lse_fin.abs())).masked_fill(dead, 0.0)
    return SimpleNamespace(
        case=c, q=q, k=k, v=v, do=do, toks=toks, e=e, dead=dead.reshape(B * Hn, Lq),
        O_bf=tokens_major(O_bf.float()), lse32=lse32.reshape(B * Hn, Lq), delta32=delta32.reshape(B * Hn, Lq),
        ref=dict(O=tokens_major(O), lse=lse.reshape(B * Hn, Lq), delta=delta.reshape(B * Hn, Lq), dQ=tokens_major(dQ),
                 dK=tokens_major(dK), dV=tokens_major(dV)),
        S=dict(O=tokens_major(S_O), lse=lse_bound.reshape(B * Hn, Lq), delta=S_delta.reshape(B * Hn, Lq),
               dQ=tokens_major(SCALE * (dSabs @ kh.abs())), dK=tokens_major(SCALE * (dSabs.transpose(-1, -2) @ qh.abs())),
               dV=tokens_major(Pgd.transpose(-1, -2) @ doh.abs())))


# ----------------------------------------------------------------------------------------------------
# bounds
# ----------------------------------------------------------------------------------------------------
def coefs(output):
    """(REL, C) of |got - ref| <= REL |ref| + C S"""
    if output == "lse":
        return 0.0, 1.0              # S is the absolute bound itself
    if output == "delta":
        return 0.0, abs_coef(64)
    return REL_BF16, C_BF16


def names_of(c, output):
    """(dims, names) that turn a flat index of `output` into (b, row, h, d) or (b, h, row)"""
    if output in ("lse", "delta"):
        return (c.B, c.Hn, c.Lq), ("b", "h", "q")
    L = c.Lk if output in ("dK", "dV") else c.Lq
    return (c.B, L, c.Hn, 64), ("b", "row", "h", "d")


def ratio(r, output, got):
    """worst |error| / bound over the elements of an output (0 / 0 = 0: an exact result where the bound is 0; NaN or any error
    where the bound is 0 = inf).  Rows of lse without a valid key are held to +inf separately (check_output)."""
    ref, S = r.ref[output], r.S[output]
    rel, ab = coefs(output)
    g = got.double().reshape(ref.shape)
    if output == "lse":
        live = ~r.dead
        g, ref, S = g[live], ref[live], S[live]
    err = (g - ref).abs()
    lim = rel * ref.abs() + ab * S
    x = torch.where(err == 0, torch.zeros_like(err), err / lim)
    x = torch.nan_to_num(x, nan=math.inf, posinf=math.inf)
    return float(x.max()) if x.numel() else 0.0


def check_output(r, output, got, what):
    """the per-element assertion (assert_bound) plus the exact parts of the contract; returns the worst error / bound ratio"""
    from hip_ops_edge_cases import assert_bound, assert_exact
    c = r.case
    ref, S = r.ref[output], r.S[output]
    rel, ab = coefs(output)
    dims, names = names_of(c, output)
    g = got.reshape(ref.shape)
    if output == "lse":
        inf = torch.full_like(g, math.inf)
        assert_exact(torch.where(r.dead, g, inf), inf, what + " (rows without a valid key: +inf)", dims, names)
        fin = lambda t: torch.where(r.dead, torch.zeros_like(t), t)          # noqa: E731
        assert_bound(fin(g.double()), fin(ref), S, rel, ab, what, dims, names)
    else:
        assert_bound(g.double(), ref, S, rel, ab, what, dims, names)
    if output == "O" and bool(r.dead.any()):
        rows = heads(g.float(), c.B, c.Lq, c.Hn)[r.dead.view(c.B, c.Hn, c.Lq)].to(BF)
        assert_exact(rows, torch.zeros_like(rows), what + " (rows without a valid key: +0 bit for bit)")
    return ratio(r, output, got)


# ----------------------------------------------------------------------------------------------------
# operands as the kernels get them
# ----------------------------------------------------------------------------------------------------
def head_T(x, B, L, Hn, fill, device, guard=2):
    """[B*L][Hn*64] -> ([guard + B*Hn*64 + guard][pad32(L)] bf16, the view of its B*Hn*64 live rows): the head-split transposed
    copy [(b*Hn+h)*64+d][Lpad].  Padding columns and guard rows hold +-fill (finite: the kernels multiply them by an exact 0)."""
    Lpad = pad32(L)
    rows = B * Hn * 64
    full = torch.full((guard + rows + guard, Lpad), float(fill))
    full[:, 1::2] *= -1.0
    full[guard:guard + rows, :L] = x.view(B, L, Hn, 64).permute(0, 2, 3, 1).reshape(rows, L)
    full = full.to(BF).to(device)
    return full, full[guard:guard + rows]


def in_slab(values, device, ld=None, coff=0, dtype=BF):
    M, C_ = values.shape
    return Slab(M, C_, dtype, device, ld=ld, coff=coff, nan_guard=True).set(values)


def build_operands(r, device, fill=0.0):
    """every operand of the three launchers in the layout of the case: NaN-guarded input slabs, transposed copies padded with
    +-fill, guarded output slabs.  `p` is the parameter block (the tensors it points into are held by the result)."""
    from cris.pytorch_amd import ops
    from cris.pytorch_amd.ops import Drop
    c = r.case
    B, Hn, Lq, Lk, E = c.B, c.Hn, c.Lq, c.Lk, c.E
    o = SimpleNamespace(case=c)
    sl = c.layout == "sliced"
    if not sl:
        o.Q, o.K, o.V = in_slab(r.q, device), in_slab(r.k, device), in_slab(r.v, device)
        Qv, Kv, Vv = o.Q.rows, o.K.rows, o.V.rows
        ldq = ldk = ldv = E
    elif c.self_attn:
        assert Lq == Lk
        o.QKV = in_slab(torch.cat([r.q, r.k, r.v], 1), device, ld=3 * E + 24, coff=8)
        Qv, Kv, Vv = o.QKV.rows[:, 8:], o.QKV.rows[:, 8 + E:], o.QKV.rows[:, 8 + 2 * E:]
        ldq = ldk = ldv = 3 * E + 24
    else:
        o.Q = in_slab(r.q, device, ld=E + 16, coff=8)
        o.KV = in_slab(torch.cat([r.k, r.v], 1), device, ld=2 * E + 24, coff=8)
        Qv, Kv, Vv = o.Q.rows[:, 8:], o.KV.rows[:, 8:], o.KV.rows[:, 8 + E:]
        ldq, ldk, ldv = E + 16, 2 * E + 24, 2 * E + 24
    o.Vt_full, Vt = head_T(r.v, B, Lk, Hn, fill, device)
    o.Kt_full, Kt = head_T(r.k, B, Lk, Hn, fill, device)
    o.Qt_full, Qt = head_T(r.q, B, Lq, Hn, fill, device)
    o.dOt_full, o.dOt = head_T(r.do, B, Lq, Hn, fill, device)
    o.toks = None if r.toks is None else r.toks.to(device)
    if c.split_seed:
        o.seed_dev = torch.tensor([SEED_DEV], dtype=torch.int32, device=device)
        drop = Drop(c.p, SEED_HOST, STREAM, o.seed_dev)
    else:
        drop = Drop(c.p, SEED, STREAM)
    o.views = (Qv, Kv, Vv, Vt, Kt, Qt)
    o.p = ops.attn_params(Qv, Kv, Vv, Vt, B, Hn, Lq, Lk, pad32(Lk), SCALE, ldq=ldq, ldk=ldk, ldv=ldv, Kt=Kt, Qt=Qt, Lq_pad=pad32(Lq),
                          key_tokens=o.toks, causal=c.causal, drop=drop)
    # given inputs of the backward
    o.dO = in_slab(r.do, device, ld=E + 32, coff=16) if sl else in_slab(r.do, device)
    o.O_in = in_slab(r.O_bf, device, ld=E + 24, coff=8) if sl else in_slab(r.O_bf, device)
    o.lse_in = in_slab(r.lse32, device, dtype=F32)
    o.delta_in = in_slab(r.delta32, device, dtype=F32)
    # outputs
    out = lambda M, ld, coff: Slab(M, E, BF, device, ld=ld if sl else E, coff=coff if sl else 0)          # noqa: E731
    o.O = out(B * Lq, E + 24, 8)
    o.dQ = out(B * Lq, E + 16, 8)
    o.dK = out(B * Lk, E + 24, 16)
    o.dV = out(B * Lk, E + 32, 8)
    o.lse = Slab(B * Hn, Lq, F32, device)
    o.delta = Slab(B * Hn, Lq, F32, device)
    return o


def set_launch(o, launcher):
    """point the parameter block at the operands of one launcher (every pointer it does not use stays what the other launchers
    need: the three share the block, as in the engine)"""
    from cris.pytorch_amd.hip import ptr
    p = o.p
    first = lambda s: s.rows[:, s.coff:]          # noqa: E731
    if launcher == "fwd":
        p.O, p.ldo, p.lse = ptr(first(o.O)), o.O.ld, ptr(o.lse.rows)
        return
    p.O, p.ldo, p.lse = ptr(first(o.O_in)), o.O_in.ld, ptr(o.lse_in.rows)
    p.dO, p.lddo, p.dOt = ptr(first(o.dO)), o.dO.ld, ptr(o.dOt)
    p.delta = ptr(o.delta.rows) if launcher == "dq" else ptr(o.delta_in.rows)
    p.dQ, p.lddq = ptr(first(o.dQ)), o.dQ.ld
    p.dK, p.lddk = ptr(first(o.dK)), o.dK.ld
    p.dV, p.lddv = ptr(first(o.dV)), o.dV.ld


def plan(o):
    """cris_attn_plan of the three launchers for a built parameter block (host arithmetic: no GPU needed)"""
    import ctypes
    from cris.pytorch_amd import hip
    return tuple(hip.load().cris_attn_plan(ctypes.byref(o.p), w) for w in range(3))


def check_case(c):
    """what must hold of a row of the tables before any kernel runs: the condition of the bound's reserve, the kernel it is meant
    to reach, the argument contract"""
    r = reference(c.name)
    assert r.e <= E_LIMIT, "%s: e = %.3e > 2^-9: the reserve of the bound does not hold at these amplitudes" % (c.name, r.e)
    o = build_operands(r, "cpu")
    for w in LAUNCHERS:
        set_launch(o, w)
    p = o.p
    assert all(v % 8 == 0 for v in (p.ldq, p.ldk, p.ldv, p.ldo, p.lddo, p.lddq, p.lddk, p.lddv)), c.name
    assert all(v.data_ptr() % 16 == 0 for v in o.views), c.name
    assert plan(o) == c.plan, "%s: cris_attn_plan %r, the table expects %r" % (c.name, plan(o), c.plan)
    assert c.B >= 2 and (c.layout == "sliced" or 1 not in c.plan)
    return r


# ----------------------------------------------------------------------------------------------------
# fp32 emulation of the kernels, with switches for seven plausible errors
# ----------------------------------------------------------------------------------------------------
def _bf(x):
    return x.to(BF).float()


def _perm_bh(x, B, Hn):
    """[B][Hn][L] as a kernel that indexes [h*B + b] where [b*Hn + h] is meant would read (or write) it"""
    return x.reshape(B * Hn, -1)[(torch.arange(Hn)[None, :] * B + torch.arange(B)[:, None]).flatten()].view(B, Hn, -1)


def emulate(name, bugs=""):
    """{output: tensor} of a correct fp32 implementation (bugs = ""), or of one with the errors named in `bugs`:
    a  keys >= Lk of the last tile not masked (the clamped last key counts again)        e  lse / delta indexed [h*B + b]
    b  causal mask off by one (kk >= q masked)                                            f  the second 32-row half of the last
    c  the key-padding row of batch 0 used for every batch                                   64-row tile dropped
    d  dropout index computed with Lk_pad in place of Lk                                  g  the O rescale skipped"""
    r = reference(name)
    c = r.case
    B, Hn, Lq, Lk = c.B, c.Hn, c.Lq, c.Lk
    Lkp, Lqp = pad32(Lk), pad32(Lq)
    scale = torch.tensor(SCALE, dtype=F32)
    qh, kh, vh, doh = (heads(t, B, L, Hn).contiguous() for t, L in ((r.q, Lq), (r.k, Lk), (r.v, Lk), (r.do, Lq)))
    kcl = torch.arange(Lkp).clamp(max=Lk - 1)
    kc, vc = kh[:, :, kcl], vh[:, :, kcl]                     # clamped loads of rows beyond Lk
    kz, vz = torch.zeros_like(kc), torch.zeros_like(vc)       # the zero-padded transposed copies
    kz[:, :, :Lk], vz[:, :, :Lk] = kh, vh
    valid = _valid(c, r.toks, Lkp, causal_ge="b" in bugs, batch0="c" in bugs).expand(B, Hn, Lq, Lkp).clone()
    if "a" not in bugs:
        valid[..., Lk:] = False
    has_drop = c.p > 0
    inv_keep = (torch.tensor(1.0, dtype=F32) / (torch.tensor(1.0, dtype=F32) - torch.tensor(c.p, dtype=F32))) if has_drop else None
    keep = _keep_full(c, Lkp if "d" in bugs else Lk, Lkp) if has_drop else None
    ksteps = Lkp // 32 - (1 if "f" in bugs and (Lkp // 32) % 2 == 0 else 0)
    qsteps = Lqp // 32 - (1 if "f" in bugs and (Lqp // 32) % 2 == 0 else 0)
    out = {}

    # forward: online softmax in 32-key steps
    s_all = (qh @ kc.transpose(-1, -2)) * scale
    s_all = s_all.masked_fill(~valid, -math.inf)
    m = torch.full((B, Hn, Lq), -math.inf)
    l = torch.zeros(B, Hn, Lq)
    acc = torch.zeros(B, Hn, Lq, 64)
    for t in range(ksteps):
        sl = slice(32 * t, 32 * t + 32)
        s = s_all[..., sl]
        m_new = torch.maximum(m, s.max(-1).values)
        dead = m_new == -math.inf
        m_safe = m_new.masked_fill(dead, 0.0)
        alpha = torch.where(dead, torch.ones_like(m), torch.exp(m - m_safe))
        pv = torch.exp(s - m_safe[..., None]).masked_fill(dead[..., None], 0.0)
        l = l * alpha + pv.sum(-1)
        if "g" not in bugs:
            acc = acc * alpha[..., None]
        m = m_new
        if has_drop:
            pv = torch.where(keep[..., sl], pv * inv_keep, torch.zeros_like(pv))
        acc = acc + _bf(pv) @ vz[:, :, sl]
    inv_l = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
    lse = torch.where(l > 0, m + torch.log(l), torch.full_like(l, math.inf))
    out["O"] = tokens_major((acc * inv_l[..., None]).to(BF))
    out["lse"] = (_perm_bh_inv(lse, B, Hn) if "e" in bugs else lse).reshape(B * Hn, Lq)

    # backward of the given O, lse, delta
    Oin = heads(r.O_bf, B, Lq, Hn)
    delta = (doh * Oin).sum(-1)
    out["delta"] = (_perm_bh_inv(delta, B, Hn) if "e" in bugs else delta).reshape(B * Hn, Lq)
    lse_in, delta_in = r.lse32.view(B, Hn, Lq), r.delta32.view(B, Hn, Lq)
    if "e" in bugs:
        lse_in, delta_in = _perm_bh(lse_in, B, Hn), _perm_bh(delta_in, B, Hn)
    st = (qh @ kc.transpose(-1, -2)) * scale
    pr = torch.exp(st - lse_in[..., None]).masked_fill(~valid, 0.0)
    dpv = doh @ vc.transpose(-1, -2)
    if has_drop:
        dpv = torch.where(keep, dpv * inv_keep, torch.zeros_like(dpv))
    ds = _bf(pr * (dpv - delta[..., None]))
    ds[..., 32 * ksteps:] = 0.0
    out["dQ"] = tokens_major(((ds @ kz) * scale).to(BF))
    prd = torch.where(keep, pr * inv_keep, torch.zeros_like(pr)) if has_drop else pr
    prd, ds2 = _bf(prd), _bf(pr * (dpv - delta_in[..., None]))
    live_q = min(Lq, 32 * qsteps)
    prd, ds2 = prd[:, :, :live_q, :Lk], ds2[:, :, :live_q, :Lk]
    out["dV"] = tokens_major((prd.transpose(-1, -2) @ doh[:, :, :live_q]).to(BF))
    out["dK"] = tokens_major(((ds2.transpose(-1, -2) @ qh[:, :, :live_q]) * scale).to(BF))
    return out


def _perm_bh_inv(x, B, Hn):
    """[B][Hn][L] as it lands in a [B*Hn][L] result when the kernel writes row h*B + b"""
    out = torch.empty(B * Hn, x.shape[-1], dtype=x.dtype)
    out[(torch.arange(Hn)[None, :] * B + torch.arange(B)[:, None]).flatten()] = x.reshape(B * Hn, -1)
    return out.view(B, Hn, -1)


# ----------------------------------------------------------------------------------------------------
# worst ratios, per output and per kernel
# ----------------------------------------------------------------------------------------------------
class Worst:
    """worst error / bound ratio per (output, kernel) with the case that gave it"""

    def __init__(self):
        self.w = {}

    def add(self, output, kernel, ratio_, case):
        key = "%s/%s" % (output, kernel)
        if key not in self.w or ratio_ > self.w[key][0]:
            self.w[key] = (ratio_, case)

    def table(self):
        return "\n".join("%-14s %.3f  (%s)" % (k, v[0], v[1]) for k, v in sorted(self.w.items()))

    def as_json(self):
        return {k: {"ratio": v[0], "case": v[1]} for k, v in sorted(self.w.items())}
