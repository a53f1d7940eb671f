"""Case tables and operand builders of the GEMM / weight-gradient edge suite: tests/test_gemm_edges.py (the HIP kernels on the
GPU) and tests/test_gemm_edges_cpu.py (the float32 emulation of tests/gemm_emulator.py, no GPU).  Importable without a GPU.

Every row forces one tile variant by name at the smallest shape that still reaches one edge of that kernel - the pipeline
prologue longer than the loop, one K-step more than the ring, M / N one off a tile, a channel chunk that straddles a tap, a
pixel step that spans two images, an empty split-K slice - and is audited element by element by gemm_audit.Auditor (its own
derived bound, `worst < 1`; no tolerance is introduced here).

Operands: inputs (A, Wt, bias, resid, bnr_y, dY, X) are slices of NaN-filled slabs (column offset 8, a row stride wider than the
slice, NaN rows before and after), so a read outside the declared slice poisons what it feeds; the columns [N, N_ld) of dY,
which the contract allows the kernel to read, hold +-2^100.  Outputs (out, outT, dW, dbias) are slices of guard-bit slabs with
two guard rows before and after and guard columns where the layout has any: the auditor's footprint check ends with the last
declared row, the guards see a store to row M or to the row before row 0.  Workspaces are filled with NaN before the launch."""
import ctypes as C
import zlib
from dataclasses import dataclass
from typing import Optional

import torch

from cris.pytorch_amd import hip, ops
from cris.pytorch_amd.ops import Drop, Geom, pad8

import gemm_audit as GA
from gemm_audit import Auditor
from hip_ops_edge_cases import Slab, assert_exact, randn_bf, randn_f32      # (Slab fills with GUARD_BITS; assert_exact: for the test files)

BF, F32 = torch.bfloat16, torch.float32
BK = 64                                        # K-step of the tile kernels (gemm_common.h BK)

TILE4 = ["128x64", "64x64", "64x128", "128x128"]
TILE8 = ["8w256x256", "8w256x128", "8w128x256", "8w128x128"]
K2 = "64x64k2"
# K-steps a variant keeps in LDS.  4-wave tiles: ST_128x64, ST_64x64, ST_64x128, ST_128x128 of csrc/gemm.hip; 64x64k2: the
# STAGES argument (2) of its conv_gemm_kernel instantiations in the variant table, one ring per wave group; 8-wave tiles:
# gemm8_nbuf(PA, PB) of csrc/gemm8.hip (2 for 256x256, 5 for 128x128, 3 otherwise).
RING = {"128x64": 3, "64x64": 3, "64x128": 3, "128x128": 2, K2: 2,
        "8w256x256": 2, "8w256x128": 3, "8w128x256": 3, "8w128x128": 5}
BNR_VARIANTS = TILE4 + ["8w128x128"]           # the variants with a BatchNorm-backward epilogue (variant table: kern[3])
GROUP_VARIANTS = TILE4 + ["8w128x128"]         # ... and with group kernels (group_kern)
SKINNY_M = {"skinny1": (1, 15, 16), "skinny9": (17, 143, 144), "skinny9s": (17, 143, 144)}
SKINNY_N = (1, 31, 32, 33, 65)
SKINNY_K = (8, 32, 40, 128, 264)
WGRAD_TILES = (128, 256)
A_COFF = R_COFF = Y_COFF = X_COFF = C_COFF = 8


def lin(M, K):
    return (M, 1, 1, K, 1, 1, 0)


@dataclass(frozen=True)
class GemmCase:
    id: str
    variant: str                  # forced by name; cris_conv_gemm_plan must resolve the launch to it
    geom: tuple                   # (Bn, H, W, C, KH = KW, stride, pad)
    N: int
    epi: str = "lean"             # lean | bias_relu | bias_res_relu3 | general | dropout | stats | bnr | outT
    outT: Optional[tuple] = None  # (T_L, T_Lpad, T_E)
    slices: int = 0               # skinny9s: the K slices cris_conv_gemm_ws_floats must report

    @property
    def family(self):
        return "gemm " + self.variant

    @property
    def g(self):
        Bn, H, W, Cc, KH, stride, pad = self.geom
        return Geom(Bn, H, W, Cc, KH, KH, stride, pad)


@dataclass(frozen=True)
class GemmGroupCase:
    id: str
    variant: str
    probs: tuple                  # GemmCase: column slices of one buffer

    @property
    def family(self):
        return "gemm " + self.variant


@dataclass(frozen=True)
class WgradCase:
    id: str
    tile: int                     # forced; cris_conv_wgrad_tile must resolve to it
    geom: tuple
    N: int
    splits: int = 1
    ldw: int = 0                  # 0: K
    eff: int = 1                  # splits the launch really makes (wgrad_effective_splits)

    @property
    def family(self):
        return "wgrad %d" % self.tile

    @property
    def g(self):
        Bn, H, W, Cc, KH, stride, pad = self.geom
        return Geom(Bn, H, W, Cc, KH, KH, stride, pad)


@dataclass(frozen=True)
class WgradGroupCase:
    id: str
    tile: int
    probs: tuple

    @property
    def family(self):
        return "wgrad %d" % self.tile


def eff_splits(M, splits):
    """every split takes a multiple of 128 pixel rows (wg_rows_per_split of csrc/wgrad.hip); splits left empty are not made"""
    rows = -(-(-(-M // splits)) // 128) * 128
    return -(-M // rows)


def tail_case(v, epi="lean"):
    """the tail shape of a tile variant: one row and one column beyond a tile, three K-steps"""
    BM, BN = GA.tile_shape(v, 0)
    return GemmCase("%s-tail-%s" % (v, epi), v, lin(BM + 1, 192), BN + 1, epi)


def tile_cases():
    out = []
    for v in TILE4 + [K2] + TILE8:
        BM, BN = GA.tile_shape(v, 0)
        D = RING[v]
        for (M, N) in [(1, 1), (BM - 1, BN - 1), (BM, BN), (BM + 1, BN + 1), (2 * BM + 17, BN + 33)]:
            out.append(GemmCase("%s-mn-%dx%d" % (v, M, N), v, lin(M, BK), N))
        # K-steps: the prologue covers the whole loop (nk < D), exactly the ring, the first refill, every buffer refilled twice;
        # 64x64k2: 1 .. 5 and 9 - an odd count leaves the second wave group a step short
        for nk in ([1, 2, 3, 4, 5, 9] if v == K2 else sorted({1, D - 1, D, D + 1, 2 * D + 1} - {0})):
            out.append(GemmCase("%s-nk%d" % (v, nk), v, lin(BM + 1, BK * nk), BN + 1))
        # taps and borders, C % 64 == 0 (the fast K-step issue): the tap changes at every step / every second step
        for name, geom in [("3x3-c64", (3, 5, 7, 64, 3, 1, 1)), ("3x3-c128", (3, 5, 7, 128, 3, 1, 1)),
                           ("3x3s2-c64", (3, 7, 5, 64, 3, 2, 1)), ("1x1s2-c64", (3, 5, 7, 64, 1, 2, 0))]:
            out.append(GemmCase("%s-%s" % (v, name), v, geom, BN + 1))
        if not v.startswith("8w"):                                  # (the 8-wave tiles need C % 64 == 0)
            # the general K-step issue: 8-channel chunks straddle taps, the last step is partial (K = 72, 216, 360, 648, 1224)
            for Cc in (8, 24, 40, 72, 136):
                out.append(GemmCase("%s-3x3-c%d" % (v, Cc), v, (2, 5, 7, Cc, 3, 1, 1), BN + 1))
            for K in (8, 56, 72):
                out.append(GemmCase("%s-lin-k%d" % (v, K), v, lin(BM + 1, K), BN + 1))
        for epi in ("lean", "bias_relu", "bias_res_relu3", "general", "dropout", "stats") + (("bnr",) if v in BNR_VARIANTS else ()):
            out.append(tail_case(v, epi))
        out.append(GemmCase("%s-outT" % v, v, lin(2 * 17, BK), 192, "outT", outT=(17, 32, 64)))
    return out


def gemm_group_cases():
    out = []
    for v in GROUP_VARIANTS:
        BM, BN = GA.tile_shape(v, 0)
        probs = tuple(GemmCase("%s-group-p%d" % (v, i), v, lin(M, BK), N) for i, (M, N) in enumerate([(1, BN), (BM + 1, BN + 1), (BM, 8)]))
        out.append(GemmGroupCase("%s-group" % v, v, probs))
    return out


def skinny_cases():
    out = []
    for v, Ms in SKINNY_M.items():
        for M in Ms:
            for N in SKINNY_N:
                for K in SKINNY_K:
                    out.append(GemmCase("%s-%dx%dx%d" % (v, M, N, K), v, lin(M, K), N))
        out.append(GemmCase("%s-general" % v, v, lin(Ms[1], 264), 33, "general"))
        if v == "skinny1":
            # the head-split copy needs M % T_L == 0 and skinny1 takes M <= 16 rows (variant_applicable: `lin && p.M <= r.bm`,
            # behind CRIS_CHECK_ARG(v >= 0, "tile variant not applicable to this problem")): T_L = 17 cannot run, T_L = 5 does
            out.append(GemmCase("%s-outT" % v, v, lin(3 * 5, BK), 192, "outT", outT=(5, 8, 64)))
        else:
            out.append(GemmCase("%s-outT" % v, v, lin(2 * 17, BK), 192, "outT", outT=(17, 32, 64)))
    # skinny_split_slices: min(192 blocks / 1 column block, K / 128) = 8 slices of skinny_kslice = ceil(ceil(1032 / 8) / 32) * 32
    # = 160: slice 7 starts at 1120 >= K and is empty - its slab must still be written
    out.append(GemmCase("skinny9s-empty-slice", "skinny9s", lin(143, 1032), 32, slices=8))
    return out


def _wg(tile, name, geom, N, splits=1, ldw=0):
    g = Geom(geom[0], geom[1], geom[2], geom[3], geom[4], geom[4], geom[5], geom[6])
    return WgradCase("wgrad%d-%s" % (tile, name), tile, geom, N, splits, ldw, eff_splits(g.M, splits))


def wgrad_cases():
    out = []
    for t in WGRAD_TILES:
        for M in (1, 31, 32, 33, 127, 129, 257):                    # pixel rows against the 32-row step and the 128-row split unit
            for s in (1, 2, 3):
                out.append(_wg(t, "m%d-s%d" % (M, s), lin(M, 72), 33, s))
        for N in (1, 127, 129, 257):
            out.append(_wg(t, "n%d" % N, lin(33, 72), N))
        for K in (8, 72, 128, 136, 264):
            for ldw in sorted({K, -(-K // 128) * 128}):             # padding columns K .. ldw: zeros (the auditor asserts it)
                out.append(_wg(t, "k%d-ldw%d" % (K, ldw), lin(33, K), 33, 1, ldw))
        # OH*OW = 1, 25, 32, 35: a 32-pixel step spans several images, ends on an image edge or carries across one
        for (H, W) in ((1, 1), (5, 5), (4, 8), (5, 7)):
            out.append(_wg(t, "3x3-%dx%d" % (H, W), (5, H, W, 8, 3, 1, 1), 33))
        out.append(_wg(t, "3x3s2-7x5", (5, 7, 5, 8, 3, 2, 1), 33))
    return out


def wgrad_group_cases():
    out = []
    for t in WGRAD_TILES:
        probs = (_wg(t, "group-p0", lin(33, 72), 33), _wg(t, "group-p1", (5, 5, 7, 8, 3, 1, 1), 129), _wg(t, "group-p2", lin(129, 136), 1))
        out.append(WgradGroupCase("wgrad%d-group" % t, t, probs))
    return out


def all_cases():
    return tile_cases() + gemm_group_cases() + skinny_cases() + wgrad_cases() + wgrad_group_cases()


# ---- the launchers' argument checks, restated (conv_gemm_check of csrc/gemm.hip, wgrad_check of csrc/wgrad.hip) -------------
def gemm_arg_violations(p):
    bad = []

    def need(cond, msg):
        if not cond:
            bad.append(msg)
    need(p.A and p.Wt, "null operand")
    need(p.M > 0 and p.N > 0 and p.K > 0, "empty problem")
    need(p.C % 8 == 0 and p.lda % 8 == 0 and p.a_coff % 8 == 0, "A channels/ld/offset must be multiples of 8")
    need(p.ldb % 8 == 0 and p.K % 8 == 0 and p.ldb >= p.K, "W ld / K must be multiples of 8")
    need(p.K == p.KH * p.KW * p.C, "K != KH*KW*C")
    need(p.M == p.Bn * p.OH * p.OW, "M != Bn*OH*OW")
    need(p.out or p.outT or p.colsum, "no output")
    need(not p.bnr_y or (p.colsum and p.colsq and p.bnr_ldy % 8 == 0), "BatchNorm-backward partials need both tables")
    need(p.stat_ld == 0 or p.stat_ld >= p.N, "stat_ld < N")
    need(not p.outT or (p.T_E % 64 == 0 and p.T_L > 0 and p.T_Lpad % 4 == 0 and p.T_Lpad >= p.T_L and p.M % p.T_L == 0),
         "bad transposed-store geometry")
    need(p.A % 16 == 0 and p.Wt % 16 == 0, "operands must be 16-byte aligned")
    return bad


def wgrad_arg_violations(p):
    bad = []

    def need(cond, msg):
        if not cond:
            bad.append(msg)
    eff = GA.wgrad_effective_splits(p.M, p.splits)
    need(p.dY and p.X and p.dW, "null operand")
    need(p.M > 0 and p.N > 0 and p.K > 0 and p.splits > 0, "empty problem")
    need(p.C % 8 == 0 and p.ldx % 8 == 0 and p.x_coff % 8 == 0, "X channels/ld/offset must be multiples of 8")
    need(p.ldy % 8 == 0 and p.y_coff % 8 == 0 and p.N_ld % 8 == 0 and p.N_ld >= p.N, "dY ld/offset/N_ld")
    need(p.K == p.KH * p.KW * p.C and p.M == p.Bn * p.OH * p.OW, "geometry")
    need(p.K <= p.ldw <= -(-p.K // 128) * 128, "ldw must lie in [K, K rounded up to 128]")
    need(p.dY % 16 == 0 and p.X % 16 == 0, "operands must be 16-byte aligned")
    need(eff == 1 or (p.ws and (p.N * p.ldw) % 4 == 0 and p.ws % 16 == 0 and p.dW % 16 == 0), "a split reduction needs the workspace")
    return bad


def raw_f32(addr, n, device):
    """n floats at a raw address as a writable tensor"""
    if torch.device(device).type == "cpu":
        buf = torch.frombuffer((C.c_char * (n * 4)).from_address(addr), dtype=torch.uint8)
    else:
        buf = torch.as_tensor(GA._CAI(addr, n * 4), device=device)
    return buf.view(F32)


def guarded_execute(inner, device):
    """execute hook of the Auditor: the launchers' preconditions hold, every workspace is NaN before the launch"""
    lib = hip.load()

    def one_wgrad(p):
        assert not wgrad_arg_violations(p), wgrad_arg_violations(p)
        nws = int(lib.cris_wgrad_ws_floats(p.M, p.N, p.ldw, p.splits))
        if nws:
            raw_f32(p.ws, nws, device).fill_(float("nan"))

    def run(fn, args):
        a0 = GA._obj(args[0])
        if fn == "cris_conv_gemm_variant":
            assert not gemm_arg_violations(a0), gemm_arg_violations(a0)
            nws = int(lib.cris_conv_gemm_ws_floats(C.byref(a0), int(args[1])))
            if nws and a0.ws:
                raw_f32(a0.ws, nws, device).fill_(float("nan"))
        elif fn == "cris_conv_gemm_group_launch":
            for i in range(a0.n):
                assert not gemm_arg_violations(a0.prob[i]), gemm_arg_violations(a0.prob[i])
        elif fn == "cris_conv_wgrad":
            one_wgrad(a0)
        elif fn == "cris_conv_wgrad_group":
            for i in range(a0.n):
                one_wgrad(a0.prob[i])
        inner(fn, args)
    return run


def make_auditor(mem, inner, device):
    return Auditor(mem, guarded_execute(inner, device), raise_on_failure=False)


# ---- operands -------------------------------------------------------------------------------------------------------------------
def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x3FFFFFFF


def _in(vals, dtype, device, ld=None, coff=0, post=2):
    M, Cc = vals.shape
    return Slab(M, Cc, dtype, device, ld=ld, coff=coff, nan_guard=True, post=post).set(vals)


class Run:
    """the slabs of one launched problem: outputs by name (`out`, `outT`, `dW`, `dbias`), inputs kept alive"""

    def __init__(self):
        self.outputs, self.inputs, self.ret = {}, [], None

    def assert_guards(self, what):
        for name, s in self.outputs.items():
            s.assert_guards("%s: %s" % (what, name))

    def get(self, name):
        return self.outputs[name].get()


def run_gemm(case: GemmCase, device, queue=None, variant=None, into=None):
    """build the operands of a case (values depend on the shape and the epilogue only, not on the variant) and launch it through
    ops.conv_gemm with the variant forced.  into = (slab, c_coff): write a column slice of that slab instead of an own one."""
    g, N = case.g, case.N
    M, K, Cc = g.M, g.K, g.C
    sd = _seed(case.geom, N, case.epi)
    r = Run()
    rows_in = g.Bn * g.H * g.W
    A = _in(randn_bf((rows_in, Cc), sd), BF, device, ld=Cc + 16, coff=A_COFF, post=g.W + 2)
    Wt = _in(randn_bf((N, K), sd + 1, K ** -0.5), BF, device, ld=K + 8)             # ldb = K + 8: NaN in [K, ldb)
    r.inputs += [A, Wt]
    kw = dict(lda=Cc + 16, a_coff=A_COFF, ldb=K + 8)
    epi = case.epi
    ldn = pad8(N) + 16
    if epi in ("bias_relu", "bias_res_relu3", "general", "dropout", "outT"):
        b = _in(randn_f32((1, N), sd + 2), F32, device)
        r.inputs.append(b)
        kw["bias"] = b.rows[0]
    kw["act"] = {"bias_relu": 1, "bias_res_relu3": 3, "general": 2}.get(epi, 0)
    if epi in ("bias_res_relu3", "general"):
        rdt = F32 if epi == "general" else BF
        res = _in(randn_bf((M, N), sd + 3), rdt, device, ld=ldn, coff=R_COFF)
        r.inputs.append(res)
        kw.update(resid=res.rows, ldr=ldn, r_coff=R_COFF)
    if into is None:
        out = Slab(M, N, F32 if epi == "general" else BF, device, ld=N + 24, coff=C_COFF)
        r.outputs["out"] = out
        kw.update(out=out.rows, ldc=N + 24, c_coff=C_COFF)
    else:
        kw.update(out=into[0].rows, ldc=into[0].ld, c_coff=into[1])
    if epi == "dropout":
        word = torch.tensor([5], dtype=torch.int32, device=device)
        r.inputs.append(word)
        kw["drop"] = Drop(0.25, 1234, 3, word)
    if epi == "stats":
        kw["stats"] = True
    if epi == "bnr":
        y = _in(randn_bf((M, N), sd + 4), BF, device, ld=ldn, coff=Y_COFF)
        vec = dict(mean=randn_f32((N,), sd + 5, 0.1), invstd=randn_f32((N,), sd + 6).abs() + 0.5, scale=randn_f32((N,), sd + 7),
                   shift=randn_f32((N,), sd + 8))
        vec = {k: v.to(device) for k, v in vec.items()}
        r.inputs += [y, vec]
        kw["bnr"] = dict(y=y.rows, ldy=ldn, coff=Y_COFF, **vec)
    if case.outT:
        T_L, T_Lpad, T_E = case.outT
        rows = (M // T_L) * T_E
        nsec = -(-N // T_E)
        oT = Slab(nsec * rows, T_L, BF, device, ld=T_Lpad, coff=0)            # guard bits in the padding columns [T_L, T_Lpad)
        r.outputs["outT"] = oT
        kw.update(outT=oT.rows, T_L=T_L, T_Lpad=T_Lpad, T_E=T_E, T_sec_stride=rows * T_Lpad)
    r.ret = ops.conv_gemm(A.rows, Wt.rows, g, N, variant=variant or case.variant, queue=queue, **kw)
    if epi in ("stats", "bnr"):
        assert r.ret is not None, "%s: the variant has no such epilogue" % case.id
    return r


def run_gemm_group(gc: GemmGroupCase, device):
    """three problems writing column slices of one buffer, in one grouped launch; returns (shared slab, [(M, c_coff, N)], runs)"""
    offs, c = [], C_COFF
    for p in gc.probs:
        offs.append(c)
        c += pad8(p.N) + 8
    rows = max(p.g.M for p in gc.probs)
    shared = Slab(rows, c + 8, BF, device)
    live = torch.zeros_like(shared._guard)
    for p, o in zip(gc.probs, offs):
        live[2:2 + p.g.M, o:o + p.N] = True
    shared._guard = ~live                                          # everything outside the three written slices is guard
    q = ops.GemmQueue()
    runs = [run_gemm(p, device, queue=q, into=(shared, o)) for p, o in zip(gc.probs, offs)]
    q.flush()
    return shared, [(p.g.M, o, p.N) for p, o in zip(gc.probs, offs)], runs


def run_wgrad(case: WgradCase, device, queue=None):
    g, N = case.g, case.N
    M, K, Cc = g.M, g.K, g.C
    sd = _seed(case.geom, N)
    r = Run()
    N_ld = pad8(N) + 8                                             # columns [N, N_ld) may be read: +-2^100, finite and exact in bf16
    fill = torch.full((M, N_ld - N), 2.0 ** 100)
    fill[:, 1::2] = -2.0 ** 100
    dY = _in(torch.cat([randn_bf((M, N), sd), fill], 1), BF, device, ld=N_ld + 16, coff=Y_COFF)
    rows_in = g.Bn * g.H * g.W
    X = _in(randn_bf((rows_in, Cc), sd + 1), BF, device, ld=Cc + 16, coff=X_COFF, post=g.W + 2)
    ldw = case.ldw or K
    dW = Slab(N, ldw, F32, device)                                 # the kernel owns whole rows of dW: guard rows only
    db = Slab(1, N, F32, device, ld=N + 16, coff=8)
    r.inputs += [dY, X]
    r.outputs.update(dW=dW, dbias=db)
    ops.conv_wgrad(dY.rows, X.rows, g, N, dW.rows, ldy=N_ld + 16, y_coff=Y_COFF, N_ld=N_ld, ldx=Cc + 16, x_coff=X_COFF, ldw=ldw,
                   splits=None if queue is not None else case.splits, dbias=db.data[0], queue=queue, tile=case.tile)
    return r


def run_wgrad_group(gc: WgradGroupCase, device):
    q = ops.WgradQueue()
    runs = [run_wgrad(p, device, queue=q) for p in gc.probs]
    q.flush()
    return runs


def run_case(case, device):
    """launch any table row; returns the Run objects whose guards must hold (and, for a group, what to compare with solo runs)"""
    if isinstance(case, GemmCase):
        return [run_gemm(case, device)]
    if isinstance(case, WgradCase):
        return [run_wgrad(case, device)]
    if isinstance(case, WgradGroupCase):
        return run_wgrad_group(case, device)
    shared, _, runs = run_gemm_group(case, device)
    runs[0].outputs["shared out"] = shared
    return runs


def check_reports(aud, case, n_launches=1):
    """report.ok, worst < 1, the family the row names; returns the worst err/bound ratio"""
    assert len(aud.reports) == n_launches, "%s: %d launches went through the hook" % (case.id, len(aud.reports))
    worst = 0.0
    for rep in aud.reports:
        assert rep.ok, rep.describe()
        for pr in rep.problems:
            assert pr.family == case.family, "%s resolved to %r, the row names %r" % (case.id, pr.family, case.family)
            assert pr.elements > 0
        worst = max(worst, rep.worst())
    assert worst < 1.0, "%s: worst err/bound %.3g" % (case.id, worst)
    return worst


def check_plan(case):
    """what the row states about the launch plan, from the library (no launch)"""
    lib = hip.load()
    if isinstance(case, GemmCase) and case.slices:
        p = hip.ConvGemmParams()
        g = case.g
        p.Bn, p.H, p.W, p.C, p.OH, p.OW, p.KH, p.KW, p.stride, p.pad = g.Bn, g.H, g.W, g.C, g.OH, g.OW, 1, 1, 1, 0
        p.M, p.N, p.K = g.M, case.N, g.K
        v = GA.VARIANTS.index(case.variant)
        assert lib.cris_conv_gemm_plan(C.byref(p), v, None) == v
        assert GA.skinny_slices(p, v) == case.slices
        ks = -(-(-(-g.K // case.slices)) // 32) * 32
        assert (case.slices - 1) * ks >= g.K, "the last slice is not empty"
    if isinstance(case, WgradCase):
        assert GA.wgrad_effective_splits(case.g.M, case.splits) == case.eff
        ldw = case.ldw or case.g.K
        assert (int(lib.cris_wgrad_ws_floats(case.g.M, case.N, ldw, case.splits)) > 0) == (case.eff > 1)
