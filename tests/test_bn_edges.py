"""BatchNorm apply / backward kernels (csrc/norm.hip) at strided operands and edges, element by element.

The launchers are called directly (cris_bn_apply, cris_bn_bwd_reduce, cris_bn_bwd_sum, cris_bn_bwd_apply), one stage at a time,
with scale / shift / mean / invstd / sums / z supplied by the test, so that a stage's inputs are exact and not another kernel's
output.  Every output lives in a Slab of guard bits that must survive, every input in a Slab of NaN guards, and every operand of
a call has its own leading dimension and column offset.  Statements, bounds and case tables: tests/bn_edge_cases.py; that a
plain fp32 evaluation meets the same checks, and that every case reaches the kernel it is named for: tests/test_bn_edges_cpu.py.

Group A: the forward on grid inputs, bit for bit.  Group B: the backward stage by stage (reduce, sentinel rows, the summation
of hand-made partial tables, apply with supplied sums, end to end through ops.bn_bwd).  Group C (last): the two sides of 2^24
work items of the generic apply kernels."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from cris.pytorch_amd import hip, ops  # noqa: E402
import hip_ops_edge_cases as E  # noqa: E402
import bn_edge_cases as N  # noqa: E402
from hip_ops_edge_cases import Slab, BF, F32, F64  # noqa: E402

DEV = "cuda"

# (ld - C, coff) of every activation operand: all different within a call, all multiples of 8
FWD_LAYOUT = {"y": (8, 8), "y2": (24, 16), "z": (32, 24), "ident": (64, 56)}
BWD_LAYOUT = {"y": (8, 8), "y2": (24, 16), "z": (32, 24), "dz": (40, 32), "dy": (48, 40), "dy2": (56, 48), "dident": (64, 56)}
FWD_FIELDS = {"y": ("y", "ldy", "y_coff"), "y2": ("y2", "ldy2", "y2_coff"), "ident": ("ident", "ldi", "i_coff"), "z": ("z", "ldz", "z_coff")}
BWD_FIELDS = {"y": ("y", "ldy", "y_coff"), "y2": ("y2", "ldy2", "y2_coff"), "z": ("z", "ldz", "z_coff"), "dz": ("dz", "lddz", "dz_coff"),
              "dy": ("dy", "lddy", "dy_coff"), "dy2": ("dy2", "lddy2", "dy2_coff"), "dident": ("dident", "lddi", "di_coff")}


def stream():
    return torch.cuda.current_stream().cuda_stream


def case_device(shape):
    B, H, W, C_ = shape
    return DEV if B * H * W * C_ > N.ON_DEVICE else "cpu"


def act_in(name, t, layout):
    C_ = t.shape[-1]
    pad, coff = layout[name]
    return Slab(t.numel() // C_, C_, BF, DEV, ld=C_ + pad, coff=coff, nan_guard=True).set(t)


def act_out(name, rows, C_, layout, init=None):
    pad, coff = layout[name]
    s = Slab(rows, C_, BF, DEV, ld=C_ + pad, coff=coff)
    return s.set(init) if init is not None else s


def vec(t, nan_guard=True):
    """a [n] fp32 vector (or [rows][n] table) between guard rows"""
    t2 = t.reshape(1, -1) if t.dim() == 1 else t
    return Slab(t2.shape[0], t2.shape[1], F32, DEV, nan_guard=nan_guard).set(t2)


def bind(p, fields, name, slab):
    f_ptr, f_ld, f_coff = fields[name]
    setattr(p, f_ptr, hip.ptr(slab.rows))
    setattr(p, f_ld, slab.ld)
    setattr(p, f_coff, slab.coff)


def result(slab, c):
    """the live slice of an output, guards checked, on the device the case (and its reference) lives on"""
    slab.assert_guards()
    return slab.data.to(c["y"].device).contiguous()


# ====================================================================================================
# A. forward, bit for bit
# ====================================================================================================
def run_fwd(c):
    B, H, W, C_ = c["y"].shape
    rows = B * (H // 2) * (W // 2) if c["pool"] else B * H * W
    p, keep = hip.BnApplyParams(), {}
    for name in ("y", "y2", "ident"):
        if c.get(name) is not None:
            keep[name] = act_in(name, c[name], FWD_LAYOUT)
            bind(p, FWD_FIELDS, name, keep[name])
    for name in ("scale", "shift", "scale2", "shift2", "mul"):
        if c.get(name) is not None:
            keep[name] = vec(c[name])
            setattr(p, name, hip.ptr(keep[name].rows))
    z = act_out("z", rows, C_, FWD_LAYOUT)
    bind(p, FWD_FIELDS, "z", z)
    p.Bn, p.H, p.W, p.C, p.relu, p.pool = B, H, W, C_, int(c["relu"]), int(c["pool"])
    hip.call("cris_bn_apply", C.byref(p), stream())
    return result(z, c)


_FWD = N.fwd_cases()


@pytest.mark.parametrize("variant,relu,shape", [x[1:] for x in _FWD], ids=[x[0] for x in _FWD])
def test_bn_apply_exact(variant, relu, shape):
    c = N.make_fwd(variant, relu, *shape, device=case_device(shape))
    N.check_fwd(run_fwd(c), c, "bn_apply %s %s" % (variant, shape))


@pytest.mark.parametrize("shape", [x[1] for x in N.GRID_BOUNDARY_CASES], ids=[x[0] for x in N.GRID_BOUNDARY_CASES])
def test_bn_apply_grid_boundaries(shape):
    c = N.make_fwd("plain", True, *shape, device=DEV)
    N.check_fwd(run_fwd(c), c, "bn_apply grid boundary %s" % (shape,))


# ====================================================================================================
# B. backward, stage by stage
# ====================================================================================================
def bwd_setup(c):
    """params with every input of the case bound (outputs, sums and part are the caller's), and the slabs that back them"""
    B, H, W, C_ = c["y"].shape
    p, keep = hip.BnBwdParams(), {}
    for name in ("y", "dz", "z", "y2"):
        if c.get(name) is not None:
            keep[name] = act_in(name, c[name], BWD_LAYOUT)
            bind(p, BWD_FIELDS, name, keep[name])
    for name in ("scale", "shift", "mean", "invstd", "mean2", "invstd2", "scale2", "mul"):
        if c.get(name) is not None:
            keep[name] = vec(c[name])
            setattr(p, name, hip.ptr(keep[name].rows))
    p.Bn, p.H, p.W, p.C, p.relu, p.pool, p.count = B, H, W, C_, int(c["relu"]), int(c["pool"]), c["count"]
    return p, keep


def reduce_outputs(p, keep, c, sums_init):
    """sums (pre-filled), the partials table and dmul as guarded outputs; the table has exactly the rows the library asks for"""
    B, H, W, C_ = c["y"].shape
    ncol = (4 if c.get("y2") is not None else 2) * C_
    rbs = N.bwd_geometry(B * H * W, C_)["rbs"]
    assert hip.load().cris_bn_bwd_ws_floats(C.byref(p)) == rbs * ncol, "the Python mirror of bn_bwd_geometry disagrees with the library"
    keep["sums"] = vec(sums_init, nan_guard=False)
    keep["part"] = Slab(rbs, ncol, F32, DEV)
    p.sums, p.part = hip.ptr(keep["sums"].rows), hip.ptr(keep["part"].rows)
    if N.wants_dmul(c):
        keep["dmul"] = Slab(B, C_, F32, DEV)
        p.dmul = hip.ptr(keep["dmul"].rows)


_REDUCE = N.reduce_cases()


@pytest.mark.parametrize("variant,shape", [x[1:] for x in _REDUCE], ids=[x[0] for x in _REDUCE])
def test_bn_bwd_reduce(variant, shape):
    c = N.make_bwd(variant, *shape, device=case_device(shape))
    p, keep = bwd_setup(c)
    reduce_outputs(p, keep, c, c["sums_old"])
    hip.call("cris_bn_bwd_reduce", C.byref(p), stream())
    what = "bn_bwd_reduce %s %s" % (variant, shape)
    keep["part"].assert_guards(what + " partials")
    N.check_sums(result(keep["sums"], c).flatten(), c, what)
    if "dmul" in keep:
        N.check_dmul(result(keep["dmul"], c), c, what)


@pytest.mark.parametrize("variant,shape", [x[1:] for x in N.SENTINEL_CASES], ids=[x[0] for x in N.SENTINEL_CASES])
def test_bn_bwd_reduce_sentinel_rows(variant, shape):
    """dz is zero except for one (pooled) row of ones: sum g must be that row's mask exactly - a dropped row gives 0, a row
    counted twice (the clamped re-read with a weight) gives 2 - and sum g xhat that row's xhat to two roundings (2^-22 relative).
    A pooled row feeds four rows: 0.25 x their masks, exact, and 0.25 x the sum of their xhat, four terms of two roundings each
    and three additions, bounded by 2^-21 of the sum of magnitudes.  With a multiplier the row's g is mask x mul[b] of its sample
    b: a quarter of a small integer times one, exact; its product with xhat is a third rounding, still within 2^-22."""
    B, H, W, C_ = shape
    M = B * H * W
    c = N.make_bwd(variant, *shape)
    two, pool = c.get("y2") is not None, c["pool"]
    p, keep = bwd_setup(c)
    reduce_outputs(p, keep, c, torch.zeros_like(c["sums_old"]))
    mask = N.relu_mask(c, F64)
    mask = torch.ones(M, C_, dtype=F64) if mask is None else mask.reshape(M, C_).double()
    if c.get("mul") is not None:
        mask = mask * c["mul"].double().repeat_interleave(H * W, 0)
    xh = [N.xhat(c, F64)] + ([N.xhat(c, F64, second=True)] if two else [])
    rows = N.sentinel_rows(M, C_)
    assert 2 <= len(rows) <= 48
    feeds = {}                                           # dz row -> the full-resolution rows it feeds
    for r in rows:
        if not pool:
            feeds[r] = [r]
            continue
        b, h, w = r // (H * W), (r % (H * W)) // W, r % W
        mo = (b * (H // 2) + h // 2) * (W // 2) + w // 2
        h0, w0 = h // 2 * 2, w // 2 * 2
        feeds[mo] = [(b * H + h0 + i) * W + w0 + j for i in (0, 1) for j in (0, 1)]
    gs = 0.25 if pool else 1.0
    keep["dz"].data.zero_()
    for mo, full in feeds.items():
        keep["dz"].data[mo] = 1.0
        keep["sums"].data.zero_()
        hip.call("cris_bn_bwd_reduce", C.byref(p), stream())
        got = keep["sums"].get().flatten()
        keep["dz"].data[mo] = 0.0
        what = "sentinel dz row %d (rows %s) of %s %s" % (mo, full, variant, shape)
        want0 = gs * mask[full].sum(0)
        for k, x in enumerate(xh):
            E.assert_exact(got[2 * k * C_:(2 * k + 1) * C_], want0.float(), what + " sum g, slot %d" % (2 * k))
            want1 = gs * (mask[full] * x[full]).sum(0)
            lim = gs * (mask[full] * x[full].abs()).sum(0)
            E.assert_bound(got[(2 * k + 1) * C_:(2 * k + 2) * C_].double(), want1, lim, 0.0, 2.0 ** (-21 if pool else -22),
                           what + " sum g xhat, slot %d" % (2 * k + 1))
    keep["sums"].assert_guards("sentinel sums")
    keep["part"].assert_guards("sentinel partials")


@pytest.mark.parametrize("C_", N.SUM_C)
@pytest.mark.parametrize("nparts", N.SUM_NPARTS)
def test_bn_bwd_sum_partial_tables(nparts, C_):
    table, old = N.rand_f32((nparts, 2 * C_), 301), N.rand_f32((2 * C_,), 302)
    st = Slab(nparts, 2 * C_, F32, DEV, nan_guard=True, post=64).set(table)          # rows after the table: NaN, never to be read
    so = vec(old, nan_guard=False)
    p = hip.BnBwdParams()
    p.part, p.sums, p.C = hip.ptr(st.rows), hip.ptr(so.rows), C_
    hip.call("cris_bn_bwd_sum", C.byref(p), nparts, stream())
    so.assert_guards("bn_bwd_sum")
    E.assert_bound(so.get().double().flatten(), N.sum_parts(table, old, F64), N.sum_parts(table, old, F64, absolute=True), 0.0,
                   E.abs_coef(nparts + 1), "bn_bwd_sum %d parts" % nparts)


def run_bwd_apply(c, p=None, keep=None, sums=None):
    B, H, W, C_ = c["y"].shape
    M = B * H * W
    if p is None:
        p, keep = bwd_setup(c)
        keep["sums"] = vec(c["sums"] if sums is None else sums)                        # NaN-guarded: [2C] without y2, [4C] with
        p.sums = hip.ptr(keep["sums"].rows)
    outs = {"dy": act_out("dy", M, C_, BWD_LAYOUT)}
    if c.get("y2") is not None and c.get("want_dy2"):
        outs["dy2"] = act_out("dy2", M, C_, BWD_LAYOUT)
    if c.get("dident") is not None:
        outs["dident"] = act_out("dident", M, C_, BWD_LAYOUT, init=c.get("dident_old"))
        p.dident_accum = int(c["dident"] == "accum")
    for name, s in outs.items():
        bind(p, BWD_FIELDS, name, s)
    hip.call("cris_bn_bwd_apply", C.byref(p), stream())
    return {name: result(s, c) for name, s in outs.items()}


_APPLY = N.apply_cases()


@pytest.mark.parametrize("variant,dident,dy2,count_factor,shape", [x[1:] for x in _APPLY], ids=[x[0] for x in _APPLY])
def test_bn_bwd_apply(variant, dident, dy2, count_factor, shape):
    c = N.make_bwd(variant, *shape, device=case_device(shape), dident=dident, dy2=dy2, count_factor=count_factor)
    N.check_apply(run_bwd_apply(c), c, "bn_bwd_apply %s %s" % (variant, shape))


@pytest.mark.parametrize("variant,dident,shape", [x[1:] for x in N.E2E_CASES], ids=[x[0] for x in N.E2E_CASES])
def test_bn_bwd_end_to_end(variant, dident, shape):
    """ops.bn_bwd (reduce -> summation -> apply on one params block) with sliced operands against autograd of the float64
    statement: the stages agree on the layout of `sums`"""
    B, H, W, C_ = shape
    M = B * H * W
    c, ref = N.make_e2e(variant, dident, *shape)
    s = {name: act_in(name, c[name], BWD_LAYOUT) for name in ("y", "dz", "z", "y2") if c.get(name) is not None}
    v = {name: vec(c[name]) for name in ("scale", "shift", "mean", "invstd", "mean2", "invstd2", "scale2", "mul") if c.get(name) is not None}
    outs = {"dy": act_out("dy", M, C_, BWD_LAYOUT)}
    sums = vec(c["sums_old"], nan_guard=False)
    kw = dict(lddz=s["dz"].ld, dz_coff=s["dz"].coff, ldy=s["y"].ld, y_coff=s["y"].coff, lddy=outs["dy"].ld, dy_coff=outs["dy"].coff,
              relu=c["relu"], pool=c["pool"])
    if "z" in s:
        kw.update(z=s["z"].rows, ldz=s["z"].ld, z_coff=s["z"].coff)
    if "y2" in s:
        outs["dy2"] = act_out("dy2", M, C_, BWD_LAYOUT)
        kw.update(y2=s["y2"].rows, ldy2=s["y2"].ld, y2_coff=s["y2"].coff, mean2=v["mean2"].rows, invstd2=v["invstd2"].rows,
                  scale2=v["scale2"].rows, dy2=outs["dy2"].rows, lddy2=outs["dy2"].ld, dy2_coff=outs["dy2"].coff)
    if dident is not None:
        outs["dident"] = act_out("dident", M, C_, BWD_LAYOUT, init=c.get("dident_old"))
        kw.update(dident=outs["dident"].rows, lddi=outs["dident"].ld, di_coff=outs["dident"].coff, dident_accum=dident == "accum")
    if "mul" in v:
        outs["dmul"] = Slab(B, C_, F32, DEV)
        kw.update(mul=v["mul"].rows, dmul=outs["dmul"].rows)
    ops.bn_bwd(s["dz"].rows, s["y"].rows, v["scale"].rows, v["shift"].rows, v["mean"].rows, v["invstd"].rows, sums.rows, outs["dy"].rows,
               B, H, W, C_, M, **kw)
    got = {name: result(o, c) for name, o in outs.items()}
    got["sums"] = result(sums, c).flatten()
    N.check_e2e(got, c, ref, "ops.bn_bwd %s %s" % (variant, shape))


def test_relu_over_two_branches_needs_z():
    """relu + y2 without z has no mask source (it cannot be recomputed from one branch): both launchers refuse it before any
    launch; without ReLU the same operands are accepted (MASK 0 reads no z: the reduce and apply cases `two_m0`)"""
    shape = (1, 33, 1, 64)
    c = N.make_bwd("two_m0", *shape)
    p, keep = bwd_setup(c)
    reduce_outputs(p, keep, c, c["sums_old"])
    dy = act_out("dy", 33, 64, BWD_LAYOUT)
    bind(p, BWD_FIELDS, "dy", dy)
    p.relu = 1
    for fn in ("cris_bn_bwd_reduce", "cris_bn_bwd_apply"):
        with pytest.raises(hip.HipLibraryError, match="stored output z"):
            hip.call(fn, C.byref(p), stream())
    torch.cuda.synchronize()
    E.assert_exact(keep["sums"].get().flatten(), c["sums_old"], "sums untouched by the refused calls")
    dy.assert_guards("dy untouched by the refused calls")
    p.relu = 0
    hip.call("cris_bn_bwd_reduce", C.byref(p), stream())
    N.check_sums(result(keep["sums"], c).flatten(), c, "two_m0 accepted")


# ====================================================================================================
# C. the 2^24 boundary of the generic kernels (large: inputs and fp32 references on the device; keep these last)
# ====================================================================================================
@pytest.mark.parametrize("M", N.DIV24_M)
def test_bn_apply_generic_div24(M):
    c = N.make_fwd("plain", True, 1, M, 1, 40, device=DEV)
    c["ref_dtype"] = F32
    N.check_fwd(run_fwd(c), c, "bn_apply generic, %d vectors" % (M * 5))


@pytest.mark.parametrize("M", N.DIV24_M)
def test_bn_bwd_apply_generic_div24(M):
    c = N.make_bwd("m2", 1, M, 1, 40, device=DEV)
    c["ref_dtype"] = F32
    N.check_apply(run_bwd_apply(c), c, "bn_bwd_apply generic, %d vectors" % (M * 5))
