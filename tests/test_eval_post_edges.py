"""The evaluation kernels of csrc/evalpost.hip beyond square maps, border 0 and letter-box matrices, on the GPU: the cases of
tests/eval_post_edge_cases.py (non-square probability maps, three borders, mirrors, transposes, singular matrices, outputs outside
the source, exact ties at every threshold) through the per-sample kernels (warp_to_original, iou_counts), the three batch kernels
(iou_batch, predict_batch, iou_sweep_batch), the statistics of filter_components and sigmoid_upsample.

Warped values, counts, mask bytes and statistics are compared with oracle/eval_post.py for EQUALITY (the maps are built on the
host and uploaded as they are).  The upsample kernel is compared per element with a float64 reference at float32 coordinates;
the bound 4 r0 is derived in tests/eval_post_edge_cases.py and recomputed here, never typed in.  Every output buffer is
pre-filled with a guard value and every count / statistics table has one unused trailing row; both must come back untouched.
tests/test_eval_post_edges_cpu.py shows that a kernel with any one of fifteen plausible errors fails in a named case."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import components_cases as CC  # noqa: E402
import eval_post_edge_cases as E  # noqa: E402
from cris.pytorch_amd import evalpost, hip  # noqa: E402
from cris.pytorch_amd.evalpost import Components  # noqa: E402
from cris.pytorch_amd.hip import ptr  # noqa: E402
from oracle import eval_post as EP  # noqa: E402

DEV = torch.device("cuda:0")
THR = float(E.THR)
INIT = list(evalpost.PREDICT_INIT)
GUARD_F, GUARD_B, TAIL = -777.25, 0x55, 64
_SHAPES = pytest.mark.parametrize("shape", E.MAP_SHAPES, ids=lambda s: "%dx%d" % s)
_BORDERS = pytest.mark.parametrize("border", E.BORDERS, ids=lambda b: "border%g" % b)
WORST = {}


@functools.lru_cache(maxsize=None)
def _probs(shape):
    return torch.from_numpy(E.maps(*shape).copy()).to(DEV).contiguous()


@functools.lru_cache(maxsize=None)
def _staging(shape):
    masks, entries = E.batch_layout(*shape)
    st = evalpost.EvalStaging(DEV).pack(list(masks), [(e.mat, e.mask, e.map, e.row) for e in entries]).upload()
    assert st.n == len(entries) and len({st.descs[j].mask_off for j in range(st.n)}) == len(masks) < st.n
    return st


def _want(shape, e, border):
    return E.oracle_warp(shape[0], shape[1], e.k, e.map, border)


def _warp_guarded(prob, mat, h, w, border):
    """cris_warp_affine_cubic into a buffer pre-filled with a guard value: h * w floats written, the tail untouched"""
    out = torch.full((h * w + TAIL,), GUARD_F, dtype=torch.float32, device=DEV)
    m = np.ascontiguousarray(np.asarray(mat, np.float64).reshape(6))
    hip.call("cris_warp_affine_cubic", ptr(prob), prob.shape[0], prob.shape[1], m.ctypes.data_as(C.c_void_p), w, h, float(border), ptr(out),
             evalpost._stream())
    got = out.cpu().numpy()
    assert (got[h * w:] == np.float32(GUARD_F)).all()
    return got[:h * w].reshape(h, w)


def _rect(buf, d):
    return buf[d.out_off:d.out_off + d.pitch * d.h_out].reshape(d.h_out, d.pitch)


def _check_masks(st, out_h, want_bytes, what):
    """every descriptor's rectangle equals the oracle's bytes, zero padding included; gaps and tail keep the guard byte"""
    used = np.zeros(out_h.shape[0], bool)
    for j, want in enumerate(want_bytes):
        d = st.descs[j]
        assert (d.h_out, d.pitch) == want.shape
        assert np.array_equal(_rect(out_h, d), want), (what, j)
        assert not used[d.out_off:d.out_off + d.pitch * d.h_out].any()
        used[d.out_off:d.out_off + d.pitch * d.h_out] = True
    assert (out_h[~used] == GUARD_B).all() and (~used).sum() >= TAIL, what


def _iou_launch(shape, border, thr, with_masks=True):
    st, n = _staging(shape), len(E.batch_layout(*shape)[1])
    counts = torch.zeros(n + 1, 2, dtype=torch.int32, device=DEV)          # (one row more than used: it must stay zero)
    out = torch.full((st.out_bytes + TAIL,), GUARD_B, dtype=torch.uint8, device=DEV) if with_masks else None
    evalpost.iou_batch(_probs(shape), st, st.masks, counts, 0, float(np.float32(thr)), out_masks=out, border=border)
    c = counts.cpu().numpy()
    assert not c[n].any()
    return c[:n], None if out is None else out.cpu().numpy()


_column_cache = {}


def _iou_column(shape, border, thr):
    """iou_batch's counts [n, 2] at one threshold, launched once per (shape, border, threshold)"""
    key = (shape, float(border), float(np.float32(thr)))
    if key not in _column_cache:
        _column_cache[key] = _iou_launch(shape, border, thr, with_masks=False)[0]
    return _column_cache[key]


def _predict_launch(shape, border, thr):
    st, n = _staging(shape), len(E.batch_layout(*shape)[1])
    stats = evalpost.new_predict_stats(n + 1, DEV)                         # (one row more than used: it must keep its initial value)
    out = torch.full((st.out_bytes + TAIL,), GUARD_B, dtype=torch.uint8, device=DEV)
    evalpost.predict_batch(_probs(shape), st, stats, 0, float(np.float32(thr)), out_masks=out, border=border)
    s = stats.cpu().numpy()
    assert s[n].tolist() == INIT
    return s[:n], out


# ---- per-sample kernels ----
@_SHAPES
@_BORDERS
def test_per_sample_warp_equals_the_oracle_bit_for_bit(shape, border):
    probs = _probs(shape)
    _, entries = E.batch_layout(*shape)
    for e in entries:                                                      # every descriptor against map 0 and a second map
        d = E.descriptors(*shape)[e.k]
        want = _want(shape, e, border)
        got = evalpost.warp_to_original(probs[e.map], e.mat, (d.h_out, d.w_out), border=border)
        assert got.shape == (d.h_out, d.w_out) and got.dtype == torch.float32
        got = got.cpu().numpy()
        assert got.tobytes() == want.tobytes(), (e.name, e.map, border, float(np.abs(got - want).max()))
        assert _warp_guarded(probs[e.map], e.mat, d.h_out, d.w_out, border).tobytes() == want.tobytes(), (e.name, e.map, border)
        if e.name in E.SINGULAR:
            assert (got == E.maps(*shape)[e.map, 0, 0]).all()


@_SHAPES
@_BORDERS
def test_per_sample_counts_equal_the_oracle(shape, border):
    probs = _probs(shape)
    masks, entries = E.batch_layout(*shape)
    fmasks = [torch.from_numpy(m.astype(np.float32)).to(DEV) for m in masks]
    for e in entries:
        d = E.descriptors(*shape)[e.k]
        warped = evalpost.warp_to_original(probs[e.map], e.mat, (d.h_out, d.w_out), border=border)
        got = evalpost.iou_counts(warped, fmasks[e.mask], THR).cpu().numpy().tolist()
        _, inter, union = EP.iou(_want(shape, e, border), masks[e.mask], E.THR)
        assert got == [inter, union], (e.name, e.map, border)


# ---- the three batch kernels ----
@_SHAPES
@_BORDERS
def test_iou_batch_equals_the_oracle_and_the_per_sample_kernels(shape, border):
    probs = _probs(shape)
    masks, entries = E.batch_layout(*shape)
    counts, out_h = _iou_launch(shape, border, THR)
    _check_masks(_staging(shape), out_h, [E.oracle_mask_bytes(_want(shape, e, border), THR) for e in entries], "iou_batch")
    fmasks = [torch.from_numpy(m.astype(np.float32)).to(DEV) for m in masks]
    for e in entries:
        d = E.descriptors(*shape)[e.k]
        want = E.oracle_counts(_want(shape, e, border), masks[e.mask], THR)
        assert counts[e.row].tolist() == want, (e.name, e.map, border)
        single = evalpost.iou_counts(evalpost.warp_to_original(probs[e.map], e.mat, (d.h_out, d.w_out), border=border), fmasks[e.mask], THR)
        assert counts[e.row].tolist() == single.cpu().numpy().tolist(), (e.name, e.map, border)


@_SHAPES
@_BORDERS
def test_predict_batch_equals_the_oracle_and_iou_batch(shape, border):
    _, entries = E.batch_layout(*shape)
    st = _staging(shape)
    stats, out = _predict_launch(shape, border, THR)
    out_h = out.cpu().numpy()
    _check_masks(st, out_h, [E.oracle_mask_bytes(_want(shape, e, border), THR) for e in entries], "predict_batch")
    assert np.array_equal(out_h, _iou_launch(shape, border, THR)[1])       # iou_batch's bytes, guard bytes included
    empty = 0
    for e in entries:
        v = _want(shape, e, border)
        fg = v > E.THR
        row = [int(fg.sum()), int(np.rint(v[fg] * np.float32(65536)).astype(np.int64).sum())]
        ys, xs = np.nonzero(fg)
        row += [int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1] if fg.any() else INIT[2:]
        assert stats[e.row].tolist() == row == E.oracle_predict_row(v, THR), (e.name, e.map, border, stats[e.row].tolist(), row)
        empty += not fg.any()
        if e.name == "far away":
            d = E.descriptors(*shape)[e.k]
            assert row == (INIT if border != 0.5 else [210, 210 * 32768, 0, 0, d.w_out, d.h_out]), (border, row)
    assert 0 < empty < len(entries)


@_SHAPES
@_BORDERS
def test_sweep_equals_iou_batch_and_the_oracle_in_every_column(shape, border):
    masks, entries = E.batch_layout(*shape)
    st, n = _staging(shape), len(entries)
    for T, thrs in E.SWEEPS.items():
        counts = torch.zeros(n + 1, T, 2, dtype=torch.int32, device=DEV)   # (one row more than used: it must stay zero)
        evalpost.iou_sweep_batch(_probs(shape), st, st.masks, counts, 0, thrs, border=border)
        got = counts.cpu().numpy()
        assert not got[n].any()
        for i, t in enumerate(thrs):
            assert np.array_equal(got[:n, i], _iou_column(shape, border, t)), (T, i, float(t))
        for e in entries:
            want = E.oracle_sweep_counts(_want(shape, e, border), masks[e.mask], thrs)
            assert np.array_equal(got[e.row], want), (T, e.name, e.map, border)


@_SHAPES
@_BORDERS
@pytest.mark.parametrize("spec", [dict(keep="largest", min_area=0), dict(keep="all", min_area=9)], ids=lambda s: "%s-%d" % (s["keep"], s["min_area"]))
def test_filtered_statistics_over_non_square_maps(shape, border, spec):
    _, entries = E.batch_layout(*shape)
    st, n = _staging(shape), len(entries)
    raw_rows, buf = _predict_launch(shape, border, THR)
    buf = buf[:st.out_bytes].clone()
    raw = buf.cpu().numpy()
    labels = evalpost.label_components(buf, st, 8)
    info = torch.zeros(n + 1, 4, dtype=torch.int64, device=DEV)
    stats = evalpost.new_predict_stats(n + 1, DEV)
    evalpost.filter_components(buf, labels, st, Components(**spec), info, 0, probs=_probs(shape), stats=stats, border=border)
    got, table, rows = buf.cpu().numpy(), info.cpu().numpy(), stats.cpu().numpy()
    multi = 0
    for j, e in enumerate(entries):
        d = st.descs[j]
        v = _want(shape, e, border)
        fg = _rect(raw, d)[:, :d.w_out] != 0
        kept, want_info, _ = CC.filter_mask(fg, **spec)
        assert table[e.row].tolist() == want_info and want_info[2] == raw_rows[e.row][0], (e.name, e.map)
        assert np.array_equal(_rect(got, d)[:, :d.w_out], kept.astype(np.uint8) * 255) and not _rect(got, d)[:, d.w_out:].any(), (e.name, e.map)
        assert rows[e.row].tolist() == CC.stats_row(kept, E.q16_of(v)), (e.name, e.map, border)
        multi += want_info[0] > 1
    assert rows[n].tolist() == INIT and not table[n].any() and multi >= 2


# ---- ties ----
@_SHAPES
def test_ties_are_decided_by_strict_comparisons(shape):
    H, W = shape
    masks, entries = E.batch_layout(H, W)
    st = _staging(shape)
    ties = E.maps(H, W)[E.TIES_MAP]
    tied = [(j, e) for j, e in enumerate(entries) if e.map == E.TIES_MAP and e.name in ("identity", "shift")]
    assert [e.name for _, e in tied] == ["identity", "shift"]
    up = lambda t: np.nextafter(np.float32(t), np.float32(np.inf))
    for T, thrs in E.SWEEPS.items():
        counts = torch.zeros(len(entries) + 1, T, 2, dtype=torch.int32, device=DEV)
        evalpost.iou_sweep_batch(_probs(shape), st, st.masks, counts, 0, thrs)
        sweep = counts.cpu().numpy()
        for i in sorted({0, T - 1, T >> 1} & set(range(T))):              # thr[0], thr[T - 1], the binary search's first probe
            t = thrs[i]
            col, out_h = _iou_launch(shape, 0.0, t)
            pred_out = _predict_launch(shape, 0.0, t)[1].cpu().numpy() if t >= 0 else None
            for j, e in tied:
                v = _want(shape, e, 0.0)
                eq, nxt = v == t, v == up(t)
                assert eq.any() and nxt.any(), (T, i, e.name)
                for name, bytes_h in (("iou_batch", out_h), ("predict_batch", pred_out)):
                    if bytes_h is None:
                        continue
                    m = _rect(bytes_h, st.descs[j])[:, :v.shape[1]]
                    assert not m[eq].any(), "%s: a value equal to thr[%d] = %r of T = %d counts as foreground (%s)" % (name, i, float(t), T, e.name)
                    assert (m[nxt] == 255).all(), "%s: the float above thr[%d] = %r of T = %d is background (%s)" % (name, i, float(t), T, e.name)
                gt = int((masks[e.mask] != 0).sum())
                for c in (sweep[e.row, i], col[e.row]):                    # predicted = union + intersection - ground truth
                    assert int(c[0]) + int(c[1]) - gt == int((v > t).sum()) < int((v >= t).sum()), (T, i, e.name, c.tolist())
    # the k + 0.5 products: the score sum is the half-to-even sum, and half-up would differ
    stats, _ = _predict_launch(shape, 0.0, THR)
    for j, e in tied:
        v = _want(shape, e, 0.0)
        fg = v > E.THR
        prod = v[fg].astype(np.float64) * 65536.0
        assert stats[e.row, 1] == int(np.rint(prod).sum()) != int(np.floor(prod + 0.5).sum()), e.name
        assert np.isin(E.half_values(), v).all()
    assert np.array_equal(_want(shape, tied[0][1], 0.0), ties)
    # border == thr: border pixels equal the threshold exactly and are not counted, by any of the three kernels
    j, e = tied[1]
    v = _want(shape, e, E.TIE_BORDER)
    outside = np.ones(v.shape, bool)
    outside[0:H - 5, 7:W + 7] = False
    assert (v[outside] == E.THR).all()
    col, out_h = _iou_launch(shape, E.TIE_BORDER, THR)
    stats, pred_out = _predict_launch(shape, E.TIE_BORDER, THR)
    counts = torch.zeros(len(entries), 1, 2, dtype=torch.int32, device=DEV)
    evalpost.iou_sweep_batch(_probs(shape), st, st.masks, counts, 0, E.SWEEPS[1], border=E.TIE_BORDER)
    want = E.oracle_counts(v, masks[e.mask], THR)
    assert col[e.row].tolist() == want == counts.cpu().numpy()[e.row, 0].tolist()
    for bytes_h in (out_h, pred_out.cpu().numpy()):
        assert np.array_equal(_rect(bytes_h, st.descs[j]), E.oracle_mask_bytes(v, THR)) and not _rect(bytes_h, st.descs[j])[:, :v.shape[1]][outside].any()
    assert stats[e.row].tolist() == E.oracle_predict_row(v, THR) and stats[e.row, 0] == int((v[~outside] > E.THR).sum())


# ---- sigmoid + bicubic upsample ----
def _upsample_guarded(logits, H, W):
    B, h, w = logits.shape
    out = torch.full((B * H * W + TAIL,), GUARD_F, dtype=torch.float32, device=DEV)
    x = torch.from_numpy(logits.copy()).to(DEV).contiguous()
    hip.call("cris_sigmoid_bicubic_up", ptr(x), B, h, w, H, W, ptr(out), evalpost._stream())
    got = out.cpu().numpy()
    assert (got[B * H * W:] == np.float32(GUARD_F)).all()
    return got[:B * H * W].reshape(B, H, W)


@pytest.mark.parametrize("name", [c.name for c in E.upsample_cases()])
def test_sigmoid_upsample_is_within_the_bound_of_the_float64_reference(name):
    c = E.up_case(name)
    bound = E.upsample_bound()
    assert bound == 4.0 * E.upsample_r0()
    got = evalpost.sigmoid_upsample(torch.from_numpy(c.logits.copy())[:, None].to(DEV), c.H, c.W)
    assert tuple(got.shape) == (E.UP_B, c.H, c.W) and got.dtype == torch.float32
    got = got.cpu().numpy()
    assert np.array_equal(got, _upsample_guarded(c.logits, c.H, c.W), equal_nan=True)
    ref = E.upsample_ref64(c.logits, c.H, c.W)
    with np.errstate(invalid="ignore"):
        oracle = E.oracle_upsample(c.logits, c.H, c.W)
    assert np.array_equal(np.isnan(got), np.isnan(oracle)), "%s: the NaN footprint differs from the oracle's" % name
    assert np.array_equal(np.isnan(oracle), np.isnan(ref))
    finite = ~np.isnan(ref)
    assert np.isfinite(got[finite]).all()
    x = E.upsample_ratio(got, ref)
    WORST[name] = x
    print("%s: worst error / bound %.3f (bound %.3e)" % (name, x, bound))
    err = np.abs(got.astype(np.float64) - ref)[finite]
    assert (err <= bound).all(), "%s: |kernel - float64 reference| reaches %.3e, bound %.3e" % (name, err.max(), bound)
    if c.logits.shape[1:] == (c.H, c.W):                                   # the identity size: the float64 sigmoid itself
        assert (np.abs(got.astype(np.float64) - E.sigmoid64(c.logits)) <= bound).all()
    if name == "one NaN":
        assert int(np.isnan(got[E.UP_NAN_AT[0]]).sum()) == E.UP_NAN_FOOTPRINT and np.isnan(got).sum() == E.UP_NAN_FOOTPRINT
    else:
        assert np.isfinite(got).all()


def test_validate_batch_on_non_square_logits():
    """logits 10 x 18 -> (40, 72), three letter-box originals: each IoU equals inter / (union + 1e-6) of the oracle warp of the
    GPU's own upsampled map exactly (no allowance: both sides warp the same probabilities)"""
    H, W = 40, 72
    sizes = [(50, 37), (30, 90), (5, 3)]
    logits = np.stack([np.random.default_rng(400 + b).standard_normal((10, 18)).astype(np.float32) * 3 for b in range(3)])
    dev = torch.from_numpy(logits)[:, None].to(DEV)
    probs = evalpost.sigmoid_upsample(dev, H, W).cpu().numpy()
    mats = [E.letterbox_inverse(oh, ow, H, W) for oh, ow in sizes]
    masks = [(np.random.default_rng(410 + b).random(s) > 0.5).astype(np.float32) for b, s in enumerate(sizes)]
    ious = evalpost.validate_batch(dev, (H, W), mats, sizes, masks)
    for b, (oh, ow) in enumerate(sizes):
        _, inter, union = EP.iou(EP.warp_affine_cubic(probs[b], mats[b], ow, oh), masks[b])
        print("validate_batch %d x %d: IoU %.6f (inter %d, union %d)" % (oh, ow, ious[b], inter, union))
        assert ious[b] == float(inter / (union + 1e-6)) and 0 < inter < union, (b, ious[b], inter, union)


def test_zz_worst_ratios():
    """(runs last in this file) the worst error / bound ratio of the upsample kernel per case"""
    print("\nworst |kernel - float64 reference| / (4 r0) of sigmoid_bicubic_kernel, r0 = %.3e:" % E.upsample_r0())
    for name, x in WORST.items():
        print("  %-22s %.3f" % (name, x))
    if WORST:
        print("  worst of all: %.3f (%s)" % (max(WORST.values()), max(WORST, key=WORST.get)))
