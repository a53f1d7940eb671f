"""Elementwise, resampling, zero-fill and LayerNorm kernels at their edges, element by element.

Every output lives inside a larger buffer of guard bits that must survive the launch, every input inside NaN guards that
poison a read outside its slice, and every comparison is per element (bounds: tests/hip_ops_edge_cases.py; the CPU file
tests/test_hip_ops_edges_cpu.py shows that a plain fp32 evaluation meets them) or, for the kernels with fast-math
transcendentals, the tolerances of tests/test_hip_ops.py applied per row / per 2048-element chunk instead of per tensor.
Group A: column slices, accumulation, aliasing.  Group B: tails and partial shapes.  Group C: the second grid-stride trip,
the top of the reciprocal-division range and the 64-bit division branch (large, references on the device)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from cris.pytorch_amd import hip, ops  # noqa: E402
from cris.pytorch_amd.ops import Drop  # noqa: E402
from oracle import dropout_hash  # noqa: E402
import hip_ops_edge_cases as E  # noqa: E402
from hip_ops_edge_cases import Slab, BF, F32, F64, randn_bf, randn_f32  # noqa: E402

DEV = "cuda"
B_A = E.B_A
NHWC = ("b", "y", "x", "c")


def sliced(values, dtype=BF, nan_guard=False, pad=E.LD_PAD, coff=E.COFF):
    """[M][C] values inside a column slice [coff, coff + C) of rows ld = C + pad wide"""
    M, C_ = values.shape
    return Slab(M, C_, dtype, DEV, ld=C_ + pad, coff=coff, nan_guard=nan_guard).set(values)


def dense(values, dtype, nan_guard=False):
    M, C_ = values.shape
    return Slab(M, C_, dtype, DEV, nan_guard=nan_guard).set(values)


def out_slab(M, C_, dtype, pad=E.LD_PAD, coff=E.COFF, init=None):
    s = Slab(M, C_, dtype, DEV, ld=C_ + pad, coff=coff if pad else 0)
    return s.set(init) if init is not None else s


def check_linear(slab, ref, S, bf16_result, terms, what, names=None):
    slab.assert_guards(what)
    got = slab.get().double().reshape(ref.shape)
    E.assert_bound(got, ref, S, E.REL_BF16 if bf16_result else 0.0, E.abs_coef(terms), what, names=names)


def check_exact(slab, ref, what, names=None):
    slab.assert_guards(what)
    E.assert_exact(slab.get().reshape(ref.shape), ref, what, names=names)


def keep_mask(seed, stream, n, p):
    return torch.from_numpy(dropout_hash.keep_mask(seed, stream, n, p))


# ====================================================================================================
# A. slices, accumulation, aliasing
# ====================================================================================================
@pytest.mark.parametrize("H,W,C_", E.POOL_CASES)
def test_avgpool2_fwd_sliced(H, W, C_):
    x = randn_bf((B_A, H, W, C_), 11)
    xs = sliced(x.view(-1, C_), nan_guard=True)
    ys = out_slab(B_A * (H // 2) * (W // 2), C_, BF)
    ops.avgpool2_fwd(xs.rows, B_A, H, W, C_, ys.rows, ldx=xs.ld, xcoff=xs.coff, ldy=ys.ld, ycoff=ys.coff)
    check_linear(ys, E.avgpool2_fwd(x, F64), E.avgpool2_fwd(x.abs(), F64), True, 4, "avgpool2_fwd", NHWC)


@pytest.mark.parametrize("accum", [False, True])
@pytest.mark.parametrize("H,W,C_", E.POOL_CASES)
def test_avgpool2_bwd_sliced(H, W, C_, accum):
    dy = randn_bf((B_A, H // 2, W // 2, C_), 12)
    old = randn_bf((B_A, H, W, C_), 13)
    ds = sliced(dy.view(-1, C_), nan_guard=True)
    xs = out_slab(B_A * H * W, C_, BF, init=old.view(-1, C_) if accum else None)
    ops.avgpool2_bwd(ds.rows, B_A, H, W, C_, xs.rows, lddy=ds.ld, dycoff=ds.coff, lddx=xs.ld, dxcoff=xs.coff, accum=accum)
    if accum:
        check_linear(xs, E.avgpool2_bwd(dy, old, F64), E.avgpool2_bwd(dy.abs(), old.abs(), F64), True, 2, "avgpool2_bwd accum", NHWC)
    else:                                            # 0.25 x is exact in bf16
        check_exact(xs, E.avgpool2_bwd(dy, None, F32).to(BF), "avgpool2_bwd", NHWC)


@pytest.mark.parametrize("H,W,C_", E.UP_CASES)
def test_upsample2_fwd_sliced(H, W, C_):
    x = randn_bf((B_A, H, W, C_), 14)
    xs = sliced(x.view(-1, C_), nan_guard=True)
    ys = out_slab(B_A * 4 * H * W, C_, BF)
    ops.upsample2_fwd(xs.rows, B_A, H, W, C_, ys.rows, ldx=xs.ld, xcoff=xs.coff, ldy=ys.ld, ycoff=ys.coff)
    check_linear(ys, E.upsample2_fwd(x, F64), E.upsample2_fwd(x.abs(), F64), True, 4, "upsample2_fwd", NHWC)


@pytest.mark.parametrize("accum", [False, True])
@pytest.mark.parametrize("H,W,C_", E.UP_CASES)
def test_upsample2_bwd_sliced(H, W, C_, accum):
    dy = randn_bf((B_A, 2 * H, 2 * W, C_), 15)
    old = randn_bf((B_A, H, W, C_), 16) if accum else None
    ds = sliced(dy.view(-1, C_), nan_guard=True)
    xs = out_slab(B_A * H * W, C_, BF, init=old.view(-1, C_) if accum else None)
    ops.upsample2_bwd(ds.rows, B_A, H, W, C_, xs.rows, lddy=ds.ld, dycoff=ds.coff, lddx=xs.ld, dxcoff=xs.coff, accum=accum)
    check_linear(xs, E.upsample2_bwd(dy, old, F64), E.upsample2_bwd(dy.abs(), None if old is None else old.abs(), F64), True, 10,
                 "upsample2_bwd", NHWC)


@pytest.mark.parametrize("M,C_", E.ADD_SHAPES)
@pytest.mark.parametrize("form", E.ADD_FORMS)
def test_add_bf16_forms(form, M, C_):
    a, b = randn_bf((M, C_), 17), randn_bf((M, C_), 18)
    if form == "copy":                               # b = None: a strided copy, bit exact
        sa, sy = sliced(a, nan_guard=True), out_slab(M, C_, BF)
        ops.add_bf16(sa.rows, sy.rows, M, C_, lda=sa.ld, acoff=sa.coff, ldy=sy.ld, ycoff=sy.coff)
        return check_exact(sy, a.to(BF), "add_bf16 copy")
    if form == "sliced":
        sa, sb, sy = sliced(a, nan_guard=True), sliced(b, nan_guard=True, pad=24, coff=16), out_slab(M, C_, BF)
        ops.add_bf16(sa.rows, sy.rows, M, C_, b=sb.rows, lda=sa.ld, acoff=sa.coff, ldb=sb.ld, bcoff=sb.coff, ldy=sy.ld, ycoff=sy.coff)
    elif form == "alias":                            # the engine's gradient accumulation: y += a, b is y itself
        sa, sy = dense(a, BF, nan_guard=True), out_slab(M, C_, BF, init=b)
        ops.add_bf16(sa.rows, sy.rows, M, C_, b=sy.rows, lda=C_, ldb=sy.ld, bcoff=sy.coff, ldy=sy.ld, ycoff=sy.coff)
    else:                                            # a and y with different leading dimensions, b dense
        sa, sb, sy = sliced(a, nan_guard=True), dense(b, BF, nan_guard=True), out_slab(M, C_, BF, pad=24, coff=16)
        ops.add_bf16(sa.rows, sy.rows, M, C_, b=sb.rows, lda=sa.ld, acoff=sa.coff, ldb=C_, ldy=sy.ld, ycoff=sy.coff)
    check_linear(sy, E.add2(a, b, F64), E.add2(a.abs(), b.abs(), F64), True, 2, "add_bf16 " + form)


@pytest.mark.parametrize("M,C_,trows", E.ROWTABLE_CASES)
def test_add_rowtable_wide_rows(M, C_, trows):
    a, t = randn_bf((M, C_), 19), randn_f32((trows, C_), 20)
    sa = sliced(a, nan_guard=True, coff=0)
    st = dense(t, F32, nan_guard=True)
    sy = out_slab(M, C_, BF, pad=8, coff=0)
    ops.add_rowtable(sa.rows, st.rows, trows, sy.rows, M, C_, lda=sa.ld, ldy=sy.ld)
    check_linear(sy, E.add_rowtable(a, t, F64), E.add_rowtable(a.abs(), t.abs(), F64), True, 2, "add_rowtable")


@pytest.mark.parametrize("Bn,T,C_", E.ROWSUM_CASES)
def test_batch_rowsum_wide_rows(Bn, T, C_):
    x = randn_bf((Bn, T, C_), 21)
    sx = sliced(x.view(-1, C_), nan_guard=True, coff=0)
    so = out_slab(T, C_, F32, pad=0)
    ops.batch_rowsum(sx.rows, Bn, T, C_, so.rows, ldx=sx.ld)
    check_linear(so, E.batch_rowsum(x, F64), E.batch_rowsum(x.abs(), F64), False, Bn, "batch_rowsum")


@pytest.mark.parametrize("M,C_,rpp", E.COLSTATS_CASES)
def test_colstats_sliced(M, C_, rpp):
    x = (randn_bf((M, C_), 22) + 0.5).to(BF).float()
    sx = sliced(x, nan_guard=True)
    nparts = (M + rpp - 1) // rpp
    ssum, sm2 = out_slab(nparts, C_, F32, pad=0), out_slab(nparts, C_, F32, pad=0)
    hip.call("cris_colstats_bf16", hip.ptr(sx.rows), sx.ld, sx.coff, M, C_, rpp, hip.ptr(ssum.rows), hip.ptr(sm2.rows),
             torch.cuda.current_stream().cuda_stream)
    (rs, rq), (Ss, Sq) = E.colstats(x, rpp, F64), E.colstats_scale(x, rpp)
    check_linear(ssum, rs, Ss, False, rpp, "colstats sum")
    check_linear(sm2, rq, Sq, False, rpp, "colstats centred second moment")
    st = ops.colstats(sx.rows, M, C_, rpp, DEV, ldx=sx.ld, coff=sx.coff)          # the wrapper: same launch, its own buffers
    assert st.nparts == nparts
    E.assert_exact(st[0][:nparts].cpu(), ssum.get(), "ops.colstats sum")
    E.assert_exact(st[1][:nparts].cpu(), sm2.get(), "ops.colstats m2")


def test_gather_samples_sliced():
    K, R, C_, n_samples = 5, 7, 24, 3
    index = [2, 0, 2, 1, 0]                          # a repeated and an out-of-order index
    x = randn_bf((n_samples * R, C_), 31)
    sx, sy = sliced(x, nan_guard=True), out_slab(K * R, C_, BF, pad=24, coff=16)
    ops.gather_samples(sx.rows, torch.tensor(index, dtype=torch.int32, device=DEV), K, R, C_, sy.rows, ldx=sx.ld, xcoff=sx.coff,
                       ldy=sy.ld, ycoff=sy.coff)
    check_exact(sy, x.view(n_samples, R, C_)[index].reshape(K * R, C_).to(BF), "gather_samples", ("row", "c"))


@pytest.mark.parametrize("nfill,H,W", [(2, 5, 7), (8, 4, 6), (2, 1, 5), (8, 5, 1), (2, 1, 1), (8, 2, 3)])
def test_fill_coords_edges(nfill, H, W):
    s = out_slab(B_A * H * W, nfill, BF)
    ops.fill_coords(s.rows, s.ld, s.coff, nfill, B_A, H, W)
    ref = torch.zeros(B_A, H, W, nfill)
    ref[..., 0] = torch.linspace(-1, 1, W).view(1, 1, W)          # n == 1: -1; odd n: the midpoint 0 from the upper half's formula
    ref[..., 1] = torch.linspace(-1, 1, H).view(1, H, 1)
    check_exact(s, ref.view(-1, nfill).to(BF), "fill_coords", ("pixel", "c"))


def _byte_range(n):
    """n bytes at a 16-byte-aligned address between 64 guard bytes on either side; everything pre-filled with 0x5A"""
    buf = torch.full((64 + n + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[64:64 + n]


def _assert_zeroed(buf, n, what):
    b = buf.cpu()
    nz = b[64:64 + n].nonzero().flatten()
    assert nz.numel() == 0, "%s: %d of %d bytes not zeroed, first at byte %d" % (what, nz.numel(), n, int(nz[0]))
    assert bool((b[:64] == 0x5A).all()) and bool((b[64 + n:] == 0x5A).all()), "%s: guard bytes overwritten" % what


ZERO_SIZES = [1, 15, 16, 17, 4096 + 3, 3 << 20, 2, 31, 33, 48, 255, 256, 257, 1000, 4095, 4097, 64, 65, 7]


def test_zero_ranges_chunks_and_tails():
    assert len(ZERO_SIZES) > hip.ZERO_RANGES_MAX        # two launches; the grid of the first is sized by the 3 MB range
    pairs = [_byte_range(n) for n in ZERO_SIZES]
    ops.zero_ranges([v for _, v in pairs])
    for (buf, _), n in zip(pairs, ZERO_SIZES):
        _assert_zeroed(buf, n, "zero_ranges %d bytes" % n)


@pytest.mark.parametrize("n", [1, 15, 17, 16 * 256 * 4096 + 5])
def test_zero_bytes_tails(n):
    buf, v = _byte_range(n)
    ops.zero_(v)
    _assert_zeroed(buf, n, "zero_ %d bytes" % n)


# ====================================================================================================
# B. tails and partial shapes
# ====================================================================================================
@pytest.mark.parametrize("n", E.TAIL_N)
def test_cast_tails(n):
    x = randn_f32((1, n), 40)
    so = out_slab(1, n, BF, pad=0)
    ops.cast_f32_bf16(dense(x, F32, nan_guard=True).rows, so.data)
    check_exact(so, x.to(BF), "cast_f32_bf16")
    xb, old = randn_bf((1, n), 23), randn_f32((1, n), 24)
    sf = out_slab(1, n, F32, pad=0)
    ops.cast_bf16_f32(dense(xb, BF, nan_guard=True).data, sf.data, accum=False)
    check_exact(sf, xb, "cast_bf16_f32")
    sf = out_slab(1, n, F32, pad=0, init=old)
    ops.cast_bf16_f32(dense(xb, BF, nan_guard=True).data, sf.data, accum=True)
    check_linear(sf, E.add2(old, xb, F64), E.add2(old.abs(), xb.abs(), F64), False, 2, "cast_bf16_f32 accum")


@pytest.mark.parametrize("n", E.TAIL_N)
def test_cast_drop_tails(n):
    p, seed, stream = 0.25, 99, 5
    x = randn_f32((1, n), 41)
    x[x == 0] = 1.0
    so = out_slab(1, n, BF, pad=0)
    ops.cast_f32_bf16_drop(dense(x, F32, nan_guard=True).data, so.data, Drop(p, seed, stream))
    so.assert_guards("cast_f32_bf16_drop")
    got = so.get()
    keep = keep_mask(seed, stream, n, p).view(1, n)
    assert torch.equal(got != 0, keep), "keep decisions: %s" % E.first_bad((got != 0) != keep)
    ref = x.double() * keep / (1 - p)
    E.assert_bound(got.double(), ref, ref.abs(), E.REL_BF16, E.ABS_F32, "cast_f32_bf16_drop")


@pytest.mark.parametrize("n", E.TAIL_N)
def test_axpy_tails(n):
    d, s = randn_f32((1, n), 25), randn_f32((1, n), 26)
    sd = out_slab(1, n, F32, pad=0, init=d)
    ops.axpy_f32(sd.data, dense(s, F32, nan_guard=True).data, 0.37)
    check_linear(sd, E.axpy(d, s, 0.37, F64), E.axpy(d.abs(), s.abs(), 0.37, F64), False, 2, "axpy_f32")


@pytest.mark.parametrize("n", [8, 2056])
def test_quickgelu_tails(n):
    x, g = randn_bf((1, n), 42, 2.0), randn_bf((1, n), 43)
    sx, sg = dense(x, BF, nan_guard=True), dense(g, BF, nan_guard=True)
    sy, sd = out_slab(1, n, BF, pad=0), out_slab(1, n, BF, pad=0)
    ops.quickgelu_fwd(sx.data, sy.data)
    ops.quickgelu_bwd(sx.data, sg.data, sd.data)
    xl = x.double().requires_grad_(True)
    ref = xl * torch.sigmoid(1.702 * xl)
    (ref * g.double()).sum().backward()
    sy.assert_guards("quickgelu_fwd")
    sd.assert_guards("quickgelu_bwd")
    E.assert_chunks(sy.get(), ref.detach(), 4e-3, "quickgelu_fwd")
    E.assert_chunks(sd.get(), xl.grad, 5e-3, "quickgelu_bwd")


def _bce_inputs(n, seed):
    """logits and 0/1 targets in rows padded to a multiple of 4 floats (the kernel wants 16-byte-aligned operands), NaN around"""
    x = randn_f32((1, n), seed, 3.0)
    t = (torch.rand(1, n, generator=E.gen(seed + 1)) > 0.5).float()
    pad = (-n) % 4
    sx = Slab(1, n, F32, DEV, ld=n + pad, nan_guard=True).set(x)
    st = Slab(1, n, F32, DEV, ld=n + pad, nan_guard=True).set(t)
    return x, t, sx, st


@pytest.mark.parametrize("n", [1, 3, 5, 1023, 128 * 256 * 4 + 3])
def test_bce_fwd_tails(n):
    x, t, sx, st = _bce_inputs(n, 44)
    loss = out_slab(1, 1, F32, pad=0, init=torch.full((1, 1), E.NAN))          # overwritten, not accumulated
    ops.bce_fwd(sx.data, st.data, loss.data)
    loss.assert_guards("bce_fwd")
    ref = F.binary_cross_entropy_with_logits(x.double(), t.double())
    got = float(loss.get())
    print("bce_fwd n=%d: got %.9g, reference %.9g" % (n, got, float(ref)))
    assert abs(got - float(ref)) < 1e-5


@pytest.mark.parametrize("n", E.TAIL_N)
def test_bce_bwd_tails(n):
    x, t, sx, st = _bce_inputs(n, 45)
    sd = out_slab(1, n, F32, pad=0)
    ops.bce_bwd(sx.data, st.data, torch.tensor([3.0], device=DEV), sd.data)
    sd.assert_guards("bce_bwd")
    ref = (torch.sigmoid(x.double()) - t.double()) * 3.0 / n
    E.assert_chunks(sd.get(), ref, 1e-5, "bce_bwd")


@pytest.mark.parametrize("Bn", [1, 3])
@pytest.mark.parametrize("HW", [1, 1023, 1025, 10816])
def test_train_metric_strides(HW, Bn):
    thr, pr_iou = 0.35, 0.5
    x = randn_f32((Bn, HW), 46, 3.0)
    edge = float(np.log(thr / (1 - thr)))
    x[(x - edge).abs() < 1e-3] = edge + 0.01         # no decision within fast-math reach of the threshold
    t = (torch.rand(Bn, HW, generator=E.gen(47)) > 0.5).float()
    if Bn > 1:                                       # one sample with an empty union: iou = 0 / 1e-6
        x[1], t[1] = -10.0, 0.0
    out = out_slab(1, 2, F32, pad=0, init=torch.full((1, 2), E.NAN))
    ops.train_metric(dense(x, F32, nan_guard=True).data, dense(t, F32, nan_guard=True).data, Bn, HW, out.data, thr=thr, pr_iou=pr_iou)
    out.assert_guards("train_metric")
    o, g = torch.sigmoid(x.double()) >= thr, t.bool()
    ious = (o & g).sum(1).double() / ((o | g).sum(1).double() + 1e-6)
    if Bn > 1:
        assert float(ious[1]) == 0.0
    got = out.get().flatten()
    print("train_metric: got %r, reference %.9g %.9g" % (got.tolist(), float(100 * ious.mean()), float(100 * (ious > pr_iou).double().mean())))
    assert abs(float(got[0]) - float(100 * ious.mean())) < 1e-3
    assert abs(float(got[1]) - float(100 * (ious > pr_iou).double().mean())) < 1e-3


@pytest.mark.parametrize("IH,IW,OH,OW", [(416, 416, 104, 104), (50, 70, 13, 23), (7, 7, 13, 13), (480, 480, 120, 120)])
def test_mask_resize_nearest_ratios(IH, IW, OH, OW):
    Bn = 2
    mask = (torch.rand(Bn, 1, IH, IW, generator=E.gen(48)) > 0.5).float()
    sm = dense(mask.view(Bn * IH, IW), F32, nan_guard=True)
    so = out_slab(Bn * OH, OW, F32, pad=0)
    ops.mask_resize_nearest(sm.data.view(Bn, 1, IH, IW), OH, OW, so.data)
    check_exact(so, F.interpolate(mask, (OH, OW), mode="nearest").view(Bn * OH, OW), "mask_resize_nearest", ("b*OH+y", "x"))


@pytest.mark.parametrize("H,W", [(21, 27), (1, 1), (2, 3)])
def test_stem_im2col_odd_sizes(H, W):
    Bn, OH, OW = 2, (H - 1) // 2 + 1, (W - 1) // 2 + 1
    img = randn_f32((Bn, 3, H, W), 49)
    si = dense(img.view(Bn * 3 * H, W), F32, nan_guard=True)
    so = out_slab(Bn * OH * OW, 32, BF, pad=0)
    ops.stem_im2col(si.data.view(Bn, 3, H, W), so.data)
    ref = torch.zeros(Bn, OH * OW, 32)
    ref[..., :27] = F.unfold(img.to(BF).float(), 3, padding=1, stride=2).transpose(1, 2)
    check_exact(so, ref.view(-1, 32).to(BF), "stem_im2col", ("pixel", "k"))


def test_embedding_sentinels():
    toks, V, P, D = E.EMBED_TOKENS, E.EMBED_V, E.EMBED_P, E.EMBED_D
    Bn, L = toks.shape
    table, pos = randn_f32((V, D), 50), randn_f32((P, D), 51)
    so = out_slab(Bn * L, D, F32, pad=0)
    ops.embed_fwd(toks.to(DEV), dense(table, F32, nan_guard=True).data, dense(pos, F32, nan_guard=True).data, so.data)
    check_exact(so, (table[toks] + pos[:L]).reshape(Bn * L, D), "embed_fwd")
    # backward: rows of the batch's tokens / positions are OVERWRITTEN with their sums, every other row keeps what it held
    dx = randn_f32((Bn * L, D), 30)
    sent = 12345.0
    st = out_slab(V, D, F32, pad=0, init=torch.full((V, D), sent))
    sp = out_slab(P, D, F32, pad=0, init=torch.full((P, D), sent))
    live0 = torch.zeros(1, V, dtype=torch.uint8)
    live0[0, 17] = 1                                 # sticky: marks of earlier batches stay
    sl = out_slab(1, V, torch.uint8, pad=0, init=live0)
    ops.embed_bwd(toks.to(DEV), dense(dx, F32, nan_guard=True).data, st.data, sp.data, row_live=sl.data)
    for s in (st, sp, sl):
        s.assert_guards("embed_bwd")
    (rt, rp), (St, Sp) = E.embed_bwd(toks, dx, V, P, F64), E.embed_bwd(toks, dx.abs(), V, P, F64)
    touched = torch.zeros(V, dtype=torch.bool)
    touched[toks.flatten()] = True
    gt, gp = st.get(), sp.get()
    ab = E.abs_coef(Bn * L)
    E.assert_bound(gt[touched].double(), rt[touched], St[touched], 0.0, ab, "embed_bwd dtable")
    assert bool((gt[~touched] == sent).all()), "embed_bwd wrote a table row whose token is not in the batch"
    E.assert_bound(gp[:L].double(), rp[:L], Sp[:L], 0.0, ab, "embed_bwd dpos")
    assert bool((gp[L:] == sent).all()), "embed_bwd wrote a position row >= L"
    want_live = touched.clone()
    want_live[17] = True
    E.assert_exact(sl.get().flatten(), want_live.to(torch.uint8), "row_live")


@pytest.mark.parametrize("D", [8, 264])
def test_eot_gather_scatter_edges(D):
    toks = torch.tensor([[5, 99, 3, 99, 0, 0],       # a tie for the maximum: the first wins
                         [99, 1, 2, 3, 4, 5],        # the maximum at position 0
                         [1, 2, 3, 4, 5, 99],        # ... at L - 1
                         [7, 7, 7, 7, 7, 7]])        # all equal
    want = [1, 0, 5, 0]
    Bn, L = toks.shape
    x = randn_bf((Bn * L, D), 52)
    so, si = out_slab(Bn, D, BF, pad=0), out_slab(1, Bn, torch.int32, pad=0)
    ops.eot_gather(toks.to(DEV), dense(x, BF, nan_guard=True).data, D, so.data, si.data)
    check_exact(si, torch.tensor([want], dtype=torch.int32), "eot_index")
    rows = x.view(Bn, L, D)[torch.arange(Bn), want]
    check_exact(so, rows.to(BF), "eot_gather", ("b", "d"))
    old, g = randn_bf((Bn * L, D), 53), randn_bf((Bn, D), 54)
    sd = out_slab(Bn * L, D, BF, pad=0, init=old)
    ops.eot_scatter_add(si.data, dense(g, BF, nan_guard=True).data, Bn, L, D, sd.data)
    sd.assert_guards("eot_scatter_add")
    got = sd.get().view(Bn, L, D)
    hit = torch.zeros(Bn, L, dtype=torch.bool)
    hit[torch.arange(Bn), want] = True
    E.assert_exact(got[~hit], old.view(Bn, L, D)[~hit].to(BF), "eot_scatter_add: rows that are not the EOT row")
    ref = old.view(Bn, L, D)[hit].double() + g.double()
    E.assert_bound(got[hit].double(), ref, old.view(Bn, L, D)[hit].double().abs() + g.double().abs(), E.REL_BF16, E.ABS_F32, "eot_scatter_add")


@pytest.mark.parametrize("H,W", [(1, 1), (3, 5)])
def test_dynconv_borders(H, W):
    Bn, C_ = 3, 8
    ld = C_ * 9 + 1
    x, wb, dp = randn_bf((Bn, H, W, C_), 55), randn_f32((Bn, ld), 56, 0.05), randn_f32((Bn, H, W), 57)
    sx, sw = dense(x.view(-1, C_), BF, nan_guard=True), dense(wb, F32, nan_guard=True)
    spred = out_slab(Bn, H * W, F32, pad=0)
    ops.dynconv_fwd(sx.data, Bn, H, W, C_, sw.data, spred.data)
    # pred[b, p] = sum_k unfold(x)[b, k, p] w[b, k] + bias[b], k = c*9 + kh*3 + kw, in float64
    xl, wl = x.double().requires_grad_(True), wb.double().requires_grad_(True)
    ref = torch.einsum("bkp,bk->bp", F.unfold(xl.permute(0, 3, 1, 2), 3, padding=1), wl[:, :-1]) + wl[:, -1:]
    (ref * dp.double().view(Bn, H * W)).sum().backward()
    spred.assert_guards("dynconv_fwd")
    E.assert_rows(spred.get(), ref.detach().reshape(Bn, H * W), 1e-4, "dynconv fwd (per image)")
    sdx = out_slab(Bn * H * W, C_, BF, pad=0)
    sdw = out_slab(Bn, ld, F32, pad=0, init=torch.zeros(Bn, ld))
    ops.dynconv_bwd(sx.data, dense(dp.view(Bn, H * W), F32, nan_guard=True).data, Bn, H, W, C_, sw.data, sdx.data, sdw.data)
    sdx.assert_guards("dynconv_bwd dx")
    sdw.assert_guards("dynconv_bwd dwb")
    E.assert_rows(sdx.get().view(Bn, -1), xl.grad.reshape(Bn, -1), 5e-3, "dynconv dx (per image)")
    E.assert_rows(sdw.get(), wl.grad, 1e-4, "dynconv dw (per image)")


@pytest.mark.parametrize("G,H,W,C_", E.POSRESIZE_CASES)
def test_posresize_guarded(G, H, W, C_):
    from cris.pytorch_amd.tables import bicubic_resize_matrix
    T = H * W
    R = torch.from_numpy(bicubic_resize_matrix(G, H, W)).float()
    pos, d, old = randn_f32((G * G + 1, C_), 27), randn_f32((T, C_), 28), randn_f32((G * G + 1, C_), 29)
    sR = dense(R, F32, nan_guard=True)
    so = out_slab(T, C_, F32, pad=0)
    ops.posresize_fwd(sR.data, dense(pos, F32, nan_guard=True).data, T, G, C_, so.data)
    check_linear(so, E.posresize_fwd(R, pos, F64), E.posresize_fwd(R.abs(), pos.abs(), F64), False, G * G, "posresize_fwd")
    sd = out_slab(G * G + 1, C_, F32, pad=0, init=old)
    ops.posresize_bwd(sR.data, dense(d, F32, nan_guard=True).data, T, G, C_, sd.data)
    check_linear(sd, E.posresize_bwd(R, d, old, F64), E.posresize_bwd(R.abs(), d.abs(), old.abs(), F64), False, T + 1, "posresize_bwd")
    E.assert_exact(sd.get()[0], old[0], "posresize_bwd: the class-token row is not touched")


# ----------------------------------------------------------------------------------------------------
# LayerNorm: partial vector slots, the row loop past the grid caps, mean / rstd, wide input rows
# ----------------------------------------------------------------------------------------------------
def _ln_stats(u, C_):
    mean = u.mean(1)
    rstd = 1.0 / torch.sqrt(u.var(1, unbiased=False) + 1e-5)
    return mean, rstd


def _check_ln_stats(smean, srstd, u, what):
    smean.assert_guards(what + " mean")
    srstd.assert_guards(what + " rstd")
    mean, rstd = _ln_stats(u.detach(), u.shape[1])
    gm, gr = smean.get().flatten().double(), srstd.get().flatten().double()
    lim = 1e-5 * u.detach().abs().mean(1)
    bad = ~((gm - mean).abs() <= lim)
    print("%s: max |mean - ref| / mean|x| %.3e, max rel rstd error %.3e" % (
        what, float(((gm - mean).abs() / (u.detach().abs().mean(1) + 1e-30)).max()), float(((gr - rstd).abs() / rstd).max())))
    assert not bool(bad.any()), "%s mean: %s: got %.9g, reference %.9g" % (what, E.first_bad(bad, names=["row"]), float(gm[bad][0]), float(mean[bad][0]))
    bad = ~((gr - rstd).abs() <= 1e-5 * rstd)
    assert not bool(bad.any()), "%s rstd: %s: got %.9g, reference %.9g" % (what, E.first_bad(bad, names=["row"]), float(gr[bad][0]), float(rstd[bad][0]))


@pytest.mark.parametrize("C_,rows", E.LN_CASES)
@pytest.mark.parametrize("variant", ["f32_pos", "relu_drop", "resid_drop"])
def test_layernorm_edges(variant, C_, rows):
    T, ldx, p, seed = E.LN_POS_ROWS, C_ + 8, 0.1, 77
    gamma, beta = randn_f32((C_,), 1) * 0.2 + 1, randn_f32((C_,), 2) * 0.1
    gd, bd = gamma.to(DEV), beta.to(DEV)
    gl, bl = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    smean, srstd = out_slab(1, rows, F32, pad=0), out_slab(1, rows, F32, pad=0)
    wide = dict(pad=8, coff=0)                       # ldx = C + 8 for the input and dx; y / ypos / out_f32 rows are dense by design
    if variant == "f32_pos":                         # fp32 in -> y, ypos; dy + dypos -> fp32 dx, accumulated
        x = randn_f32((rows, C_), 3) * 2 + 0.5
        pos = randn_f32((T, C_), 4)
        sx = sliced(x, F32, nan_guard=True, **wide)
        sy, syp = out_slab(rows, C_, BF, pad=0), out_slab(rows, C_, BF, pad=0)
        ops.ln_fwd(sx.rows, gd, bd, rows, C_, smean.data, srstd.data, ldx=ldx, y=sy.data, ypos=syp.data, pos=pos.to(DEV), pos_rows=T)
        xl = x.double().requires_grad_(True)
        u = xl
        ref = F.layer_norm(u, (C_,), gl, bl, 1e-5)
        _check_ln_stats(smean, srstd, u, "ln f32")
        sy.assert_guards("ln y")
        syp.assert_guards("ln ypos")
        E.assert_rows(sy.get(), ref.detach(), 6e-3, "ln y")
        E.assert_rows(syp.get(), ref.detach() + pos.double().repeat(rows // T + 1, 1)[:rows], 6e-3, "ln ypos")
        dy, dyp = randn_bf((rows, C_), 5), randn_bf((rows, C_), 6)
        (ref * (dy + dyp).double()).sum().backward()
        old = randn_f32((rows, C_), 7)
        sdx = out_slab(rows, C_, F32, init=old, **wide)
        sdg, sdb = out_slab(1, C_, F32, pad=0), out_slab(1, C_, F32, pad=0)
        ops.ln_bwd(sx.rows, gd, smean.data, srstd.data, rows, C_, sdx.rows, ldx=ldx, dy=dy.to(DEV).to(BF), dypos=dyp.to(DEV).to(BF),
                   dgamma=sdg.data, dbeta=sdb.data, dx_accum=True)
        for s, w in ((sdx, "dx"), (sdg, "dgamma"), (sdb, "dbeta")):
            s.assert_guards("ln " + w)
        E.assert_rows(sdx.get().double() - old.double(), xl.grad, 2e-3, "ln dx (accum f32)")
        E.assert_rows(sdg.get(), gl.grad.view(1, C_), 1e-3, "ln dgamma")
        E.assert_rows(sdb.get(), bl.grad.view(1, C_), 1e-3, "ln dbeta")
        return
    dy = randn_bf((rows, C_), 5)
    if variant == "relu_drop":                       # bf16 pre-activation in, relu + input dropout (FFN norm), bf16 dx
        h = randn_bf((rows, C_), 8, 1.5)
        km = keep_mask(seed, 4, rows * C_, p).view(rows, C_).double()
        sx = sliced(h, BF, nan_guard=True, **wide)
        sy = out_slab(rows, C_, BF, pad=0)
        ops.ln_fwd(sx.rows, gd, bd, rows, C_, smean.data, srstd.data, ldx=ldx, y=sy.data, in_relu=True, in_drop=Drop(p, seed, 4))
        xl = h.double().requires_grad_(True)
        u = torch.relu(xl) * km / (1 - p)
        ref = F.layer_norm(u, (C_,), gl, bl, 1e-5)
        _check_ln_stats(smean, srstd, u, "ln(relu,dropout)")
        sy.assert_guards("ln(relu,dropout) y")
        E.assert_rows(sy.get(), ref.detach(), 6e-3, "ln(relu,dropout)")
        (ref * dy.double()).sum().backward()
        sdx = out_slab(rows, C_, BF, **wide)
        ops.ln_bwd(sx.rows, gd, smean.data, srstd.data, rows, C_, sdx.rows, ldx=ldx, dy=dy.to(DEV).to(BF), in_relu=True, in_drop=Drop(p, seed, 4))
        sdx.assert_guards("ln(relu,dropout) dx")
        E.assert_rows(sdx.get(), xl.grad, 8e-3, "ln(relu,dropout) dx")
    else:                                            # bf16 in -> resid + dropout(LN(x)) in fp32 (post-attention norms)
        a, resid = randn_bf((rows, C_), 9), randn_f32((rows, C_), 10)
        km = keep_mask(seed, 1, rows * C_, p).view(rows, C_).double()
        sx = sliced(a, BF, nan_guard=True, **wide)
        so = out_slab(rows, C_, F32, pad=0)
        ops.ln_fwd(sx.rows, gd, bd, rows, C_, smean.data, srstd.data, ldx=ldx, resid=resid.to(DEV), out_f32=so.data, out_drop=Drop(p, seed, 1))
        xl = a.double().requires_grad_(True)
        ref = resid.double() + F.layer_norm(xl, (C_,), gl, bl, 1e-5) * km / (1 - p)
        _check_ln_stats(smean, srstd, xl, "resid + drop(LN)")
        so.assert_guards("resid + drop(LN)")
        E.assert_rows(so.get(), ref.detach(), 2e-3, "resid + drop(LN)")
        do = randn_f32((rows, C_), 12)
        (ref * do.double()).sum().backward()
        sdx = out_slab(rows, C_, BF, **wide)
        ops.ln_bwd(sx.rows, gd, smean.data, srstd.data, rows, C_, sdx.rows, ldx=ldx, dout_f32=do.to(DEV), out_drop=Drop(p, seed, 1))
        sdx.assert_guards("resid-drop LN dx")
        E.assert_rows(sdx.get(), xl.grad, 8e-3, "resid-drop LN dx")


# ====================================================================================================
# C. index paths: large shapes, every element compared, references in torch fp32 on the device
# ====================================================================================================
@pytest.fixture
def device_memory():
    yield
    torch.cuda.empty_cache()


def _dev_randn_bf(shape, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, device=DEV, generator=g).to(BF)


def _bcyx(flat, dims):
    """(b, y, x, cv) of a flat element index over [b][y][x][cv][8]"""
    b, y, x, cv, _ = np.unravel_index(flat, tuple(dims) + (8,))
    return "flat element %d = vector %d = (b=%d, y=%d, x=%d, cv=%d)" % (flat, flat // 8, b, y, x, cv)


def _dev_bound(got, ref, S, what, dims, offset=0):
    """|got - ref| <= 2^-8 |ref| + 2^-20 S on the device; dims: (B, Y, X, CV) of the whole output, offset: flat index of got[0]"""
    err = (got.float() - ref).abs()
    bad = ~(err <= E.REL_BF16 * ref.abs() + E.ABS_F32 * S)
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        assert False, "%s: %d elements out of bound; first at %s: got %.9g, reference %.9g" % (
            what, int(bad.sum()), _bcyx(offset + i, dims), float(got.flatten()[i]), float(ref.flatten()[i]))


def _dev_exact(got, ref, what, dims, offset=0):
    bad = got.view(torch.int16) != ref.view(torch.int16)
    if bool(bad.any()):
        bad = bad.expand(got.shape)
        i = int(bad.flatten().nonzero()[0])
        assert False, "%s: %d elements differ; first at %s: got %.9g, expected %.9g" % (
            what, int(bad.sum()), _bcyx(offset + i, dims), float(got.flatten()[i]), float(ref.expand(got.shape).flatten()[i]))


def test_second_trip_avgpool2_fwd(device_memory):
    s, items = E.STRIDE2_CASES["avgpool2_fwd"]
    Bn, H, W, C_ = s["B"], s["H"], s["W"], s["C"]
    OH, OW = H // 2, W // 2
    x = _dev_randn_bf((Bn, H, W, C_), 60)
    sy = Slab(Bn * OH * OW, C_, BF, DEV)
    ops.avgpool2_fwd(x, Bn, H, W, C_, sy.rows)
    sy.assert_guards("avgpool2_fwd")
    got = sy.data.view(Bn, OH, OW, C_)
    for b in range(Bn):
        xf = x[b].float().view(OH, 2, OW, 2, C_)
        _dev_bound(got[b], xf.sum((1, 3)) * 0.25, xf.abs().sum((1, 3)) * 0.25, "avgpool2_fwd", (Bn, OH, OW, C_ // 8), b * OH * OW * C_)


def test_second_trip_add_bf16(device_memory):
    s, items = E.STRIDE2_CASES["add_bf16"]
    M, C_ = s["M"], s["C"]
    a, b = _dev_randn_bf((M, C_), 61), _dev_randn_bf((M, C_), 62)
    sy = Slab(M, C_, BF, DEV)
    ops.add_bf16(a, sy.rows, M, C_, b=b)
    sy.assert_guards("add_bf16")
    _dev_bound(sy.data, a.float() + b.float(), a.float().abs() + b.float().abs(), "add_bf16", (1, 1, M, C_ // 8))


def test_second_trip_cast_drop(device_memory):
    n = E.STRIDE2_CASES["cast_f32_bf16_drop"][0]["n"]
    p, seed, stream = 0.25, 123, 3
    x = torch.randn(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(63))
    x[x == 0] = 1.0
    sy = Slab(1, n, BF, DEV)
    ops.cast_f32_bf16_drop(x, sy.data, Drop(p, seed, stream))
    sy.assert_guards("cast_f32_bf16_drop")
    keep = dropout_hash.keep_mask_torch(seed, stream, n, p, DEV)
    got = sy.data.flatten()
    wrong = (got != 0) != keep
    assert not bool(wrong.any()), "keep decision of element %d" % int(wrong.nonzero()[0])
    ref = torch.where(keep, x * (1.0 / (1.0 - p)), torch.zeros_like(x))
    err = (got.float() - ref).abs()
    bad = ~(err <= E.REL_BF16 * ref.abs() + E.ABS_F32 * ref.abs())
    assert not bool(bad.any()), "cast_f32_bf16_drop: first bad element %d" % int(bad.nonzero()[0])


@pytest.mark.parametrize("table", ["rcp_top", "div64"])
def test_index_paths_avgpool2_bwd(table, device_memory):
    s, items = (E.RCP_TOP_CASES if table == "rcp_top" else E.DIV64_CASES)["avgpool2_bwd"]
    Bn, H, W, C_ = s["B"], s["H"], s["W"], s["C"]
    OH, OW = H // 2, W // 2
    dy = _dev_randn_bf((Bn, OH, OW, C_), 64)
    sx = Slab(Bn * H * W, C_, BF, DEV)
    ops.avgpool2_bwd(dy, Bn, H, W, C_, sx.rows)
    sx.assert_guards("avgpool2_bwd")
    ref = (dy.float() * 0.25).to(BF)                 # exact
    for b in range(Bn):
        _dev_exact(sx.data.view(Bn, OH, 2, OW, 2, C_)[b], ref[b].view(OH, 1, OW, 1, C_), "avgpool2_bwd", (Bn, H, W, C_ // 8), b * H * W * C_)


def _up2_taps(n_in):
    """source taps of the 2 n_in outputs of a x2 bilinear resize, align_corners=False: src = max(0, (dst + 0.5) / 2 - 0.5)"""
    dst = torch.arange(2 * n_in, device=DEV, dtype=torch.float32)
    src = ((dst + 0.5) * 0.5 - 0.5).clamp_min(0)
    i0 = src.floor().long()
    return i0, (i0 + 1).clamp_max(n_in - 1), src - i0


def _up2_rows(xf, r0, r1, x0, x1, lx, y0, y1, ly):
    """output rows [r0, r1) of the resize of xf [H][W][C] (fp32, on the device)"""
    w = ly[r0:r1].view(-1, 1, 1)
    v = xf[y0[r0:r1]] * (1 - w) + xf[y1[r0:r1]] * w
    lx = lx.view(1, -1, 1)
    return v[:, x0] * (1 - lx) + v[:, x1] * lx


@pytest.mark.parametrize("table", ["rcp_top", "div64"])
def test_index_paths_upsample2_fwd(table, device_memory):
    s, items = (E.RCP_TOP_CASES if table == "rcp_top" else E.DIV64_CASES)["upsample2_fwd"]
    Bn, H, W, C_ = s["B"], s["H"], s["W"], s["C"]
    assert Bn == 1
    x = _dev_randn_bf((H, W, C_), 65)
    sy = Slab(4 * H * W, C_, BF, DEV)
    ops.upsample2_fwd(x, Bn, H, W, C_, sy.rows)
    sy.assert_guards("upsample2_fwd")
    got = sy.data.view(2 * H, 2 * W, C_)
    xf = x.float()
    xa = xf.abs()
    (y0, y1, ly), (x0, x1, lx) = _up2_taps(H), _up2_taps(W)
    for r0 in range(0, 2 * H, 64):
        r1 = min(2 * H, r0 + 64)
        _dev_bound(got[r0:r1], _up2_rows(xf, r0, r1, x0, x1, lx, y0, y1, ly), _up2_rows(xa, r0, r1, x0, x1, lx, y0, y1, ly),
                   "upsample2_fwd", (1, 2 * H, 2 * W, C_ // 8), r0 * 2 * W * C_)


@pytest.mark.parametrize("case", ["window", "square"])
def test_index_paths_stem_im2col(case, device_memory):
    s, items = E.RCP_TOP_CASES["stem_im2col"] if case == "window" else E.STEM_SQUARE_CASE
    Bn, H, W = s["B"], s["H"], s["W"]
    assert Bn == 1
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    img = torch.randn(1, 3, H, W, device=DEV, generator=torch.Generator(device=DEV).manual_seed(66))
    so = Slab(OH * OW, 32, BF, DEV)
    ops.stem_im2col(img, so.data)
    so.assert_guards("stem_im2col")
    got = so.data.view(OH, OW, 32)
    pad = F.pad(img[0].to(BF), (1, 1, 1, 1))          # [3][H + 2][W + 2], zero border
    for k in range(32):                              # column k = ci*9 + kh*3 + kw: the padded image at stride 2 from (kh, kw)
        ci, kh, kw = k // 9, (k % 9) // 3, k % 3
        ref = pad[ci, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2] if k < 27 else torch.zeros(OH, OW, dtype=BF, device=DEV)
        bad = got[:, :, k].view(torch.int16) != ref.contiguous().view(torch.int16)
        if bool(bad.any()):
            i = int(bad.flatten().nonzero()[0])
            assert False, "stem_im2col: column %d: %d pixels differ; first at %s" % (k, int(bad.sum()), _bcyx((i * 32 + k), (1, OH, OW, 4)))
