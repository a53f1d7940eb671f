"""Host side of the threshold sweep (csrc/evalpost.hip cris_eval_iou_sweep_batch, evalpost.iou_sweep_batch,
evaluate.sweep_metrics / SweepResult): the ABI bookkeeping of the new symbol, the launcher's rejections before a device is
touched, the metric arithmetic against `metrics` column by column, and the histogram-to-counts algebra of the kernel restated in
numpy against the oracle.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cris_hip.h")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()


def test_symbol_is_declared_bound_and_named_at_abi_8(built):
    from cris.pytorch_amd import hip
    from header_decls import ctype_of, prototypes
    src = open(HEADER).read()
    assert re.search(r"\bint cris_eval_iou_sweep_batch\s*\(", src)
    assert "cris_eval_iou_sweep_batch" in hip.EXPORTS and hip.load().cris_eval_iou_sweep_batch is not None
    res, args = hip._SIGS["cris_eval_iou_sweep_batch"]
    ret, params = prototypes(src)["cris_eval_iou_sweep_batch"]
    assert res is C.c_int and ret == "int" and len(args) == 15
    assert list(args) == [C.c_size_t if p.split()[0] == "size_t" else ctype_of(p) for p in params.split(",")]
    assert hip.ABI_VERSION == 8 == hip.load().cris_abi_version() == int(re.search(r"#define CRIS_ABI_VERSION (\d+)", src).group(1))
    comment = src[src.index("/* CRIS_ABI_VERSION moves"):src.index("#define CRIS_ABI_VERSION")]
    assert "cris_eval_iou_sweep_batch" in comment
    assert comment.index("cris_predict_masks_batch") < comment.index("cris_eval_iou_sweep_batch")    # appended after the last addition
    assert len(re.findall(r"typedef struct \{[^{}]*\} cris_eval_desc;", src)) == 1                   # reused, no new struct
    assert hip.load().cris_sizeof(b"cris_eval_desc") == C.sizeof(hip.EvalDesc) == 88
    # the retained launchers keep their argument lists
    assert len(hip._SIGS["cris_eval_iou_batch"][1]) == 16 and len(hip._SIGS["cris_predict_masks_batch"][1]) == 14


def test_launcher_rejects_bad_arguments_on_the_host(built):
    """cris_eval_iou_sweep_batch checks its operands, the thresholds and every descriptor before it touches the device"""
    from cris.pytorch_amd import hip
    l = hip.load()
    d = (hip.EvalDesc * 1)()
    mat = (C.c_double * 6)(1, 0, 0, 0, 1, 0)
    good = [0.2, 0.35, 0.5]

    def fill(w=5, h=4, map=0, mask_off=0, pitch=None, row=0):
        assert l.cris_eval_desc_fill(C.addressof(d), mat, w, h, map, mask_off, (w + 3) // 4 * 4 if pitch is None else pitch, 0, row) == 0

    def launch(probs=0x1000, host=None, dev=0x2000, n=1, masks=0x3000, mask_bytes=64, thr=good, T=None, counts=0x4000, rows=4,
               border=0.0):
        host = C.addressof(d) if host is None else host
        arr = None if thr is None else (C.c_float * 65)(*thr)
        return l.cris_eval_iou_sweep_batch(probs, 2, 8, 8, host or None, dev, n, masks, mask_bytes, arr, len(thr or []) if T is None else T,
                                           border, counts, rows, None)

    def rejected(msg, **kw):
        assert launch(**kw) != 0
        err = l.cris_last_error()
        assert b"cris_eval_iou_sweep_batch" in err and msg in err, (kw, err)

    fill()
    rejected(b"null operand", probs=None)
    rejected(b"null operand", host=0)
    rejected(b"null operand", dev=None)
    rejected(b"null operand", masks=None)
    rejected(b"null operand", thr=None, T=3)
    rejected(b"null operand", counts=None)
    for T in (0, 65, -1):
        rejected(b"T must be in 1 .. 64", thr=[0.1] * 65, T=T)
    rejected(b"strictly increasing", thr=[0.2, 0.5, 0.35])                          # unsorted
    rejected(b"strictly increasing", thr=[0.2, 0.35, 0.35])                         # a repeated value
    rejected(b"strictly increasing", thr=[0.0, -0.0])
    for bad in (float("nan"), float("inf"), float("-inf")):
        rejected(b"thresholds must be finite", thr=[bad])
        rejected(b"thresholds must be finite", thr=[0.1, bad])
    rejected(b"thresholds must be finite", thr=[float("-inf"), 0.1])
    for n in (0, -1, 65536):
        rejected(b"n must be in 1 .. 65535", n=n)
    rejected(b"bad sizes", rows=0)
    fill(row=4)
    rejected(b"map / row out of range")
    fill(row=-1)
    rejected(b"map / row out of range")
    fill(row=3)
    rejected(b"map / row out of range", rows=3)
    fill(map=2)
    rejected(b"map / row out of range")
    for pitch in (6, 4, 7):
        fill(pitch=pitch)
        rejected(b"pitch must be a multiple of 4")
    fill(w=0)
    rejected(b"bad output size")
    fill(w=46341, h=46341)
    rejected(b"bad output size")
    fill(mask_off=64)                                                               # 8 x 4 bytes at 64 need 96
    rejected(b"mask outside the buffer", mask_bytes=95)
    fill(mask_off=2)
    rejected(b"mask outside the buffer", mask_bytes=1 << 20)                        # misaligned offset
    fill(mask_off=-16)
    rejected(b"mask outside the buffer", mask_bytes=1 << 20)
    fill()
    rejected(b"4-byte aligned", masks=0x3001)
    rejected(b"4-byte aligned", counts=0x4002)


def _table():
    rng = np.random.default_rng(5)
    union = rng.integers(1, 2000, size=(7, 5))
    inter = (union * rng.random((7, 5))).astype(np.int64)
    inter[2], union[2] = 0, 0                                                       # a sample with an empty mask and no prediction
    inter[:, 3], union[:, 3] = inter[:, 1], union[:, 1]                             # columns 1 and 3 tie in every metric
    return np.stack([inter, union], -1).astype(np.int32)


def test_sweep_metrics_equal_metrics_column_by_column():
    from cris.pytorch_amd import evaluate
    counts = _table()
    thr = [0.2, 0.35, 0.5, 0.65, 0.8]
    res = evaluate.sweep_metrics(counts, thr)
    assert res.thresholds.dtype == np.float32 and res.thresholds.tolist() == [float(np.float32(t)) for t in thr]
    assert res.iou.shape == res.overall_iou.shape == (5,) and res.per_sample.shape == (7, 5) and list(res.prec) == list(evaluate.PR_KEYS)
    for i in range(5):
        iou, prec, per = evaluate.metrics(counts[:, i])
        assert res.iou[i] == iou and res.per_sample[:, i].tolist() == per.tolist()
        assert {k: float(v[i]) for k, v in res.prec.items()} == prec
        c = counts[:, i].astype(np.float64)
        assert res.overall_iou[i] == c[:, 0].sum() / (c[:, 1].sum() + 1e-6) == evaluate.overall_iou(counts[:, i])
        assert res.at(thr[i]) == (iou, prec)
    assert res.per_sample[2].tolist() == [0.0] * 5                                  # union 0: 0 / 1e-6
    for metric in ("iou", "overall_iou") + evaluate.PR_KEYS:
        v = res._metric(metric)
        t, best = res.best(metric)
        assert best == v.max() and t == float(res.thresholds[int(np.flatnonzero(v == v.max())[0])])
    # the tie rule: with columns 1 and 3 equal and made the best, the lower threshold is returned
    tie = counts.copy()
    tie[:, [1, 3], 0] = tie[:, [1, 3], 1]                                           # IoU 1 wherever the union is not 0
    r2 = evaluate.sweep_metrics(tie, thr)
    assert r2.iou[1] == r2.iou[3] == r2.iou.max() and r2.best()[0] == float(np.float32(0.35)) and r2.best("Pr@90")[0] == float(np.float32(0.35))
    assert r2.best("overall_iou") == (float(np.float32(0.35)), float(r2.overall_iou[1]))
    # at() looks the float32 value up: the python float 0.35 finds float32(0.35); a value that was not swept does not
    grid = evaluate.sweep_metrics(np.repeat(counts[:, :1], 19, 1), evaluate.sweep_thresholds())
    assert grid.at(0.35) == evaluate.metrics(counts[:, 0])[:2] and grid.at(np.float32(0.35)) == grid.at(0.35)
    with pytest.raises(KeyError):
        grid.at(0.36)
    with pytest.raises(ValueError):
        res.best("Pr@95")
    for bad_counts, bad_thr in ((counts[:, :4], thr), (counts[:, :, 0], thr), (counts[:0], thr), (counts, []), (counts.reshape(35, 2), thr),
                                (counts, [0.2, 0.35, 0.35, 0.5, 0.6]), (counts, [0.2, 0.35, 0.3, 0.5, 0.6]),
                                (counts, [0.2, 0.35, float("nan"), 0.5, 0.6])):
        with pytest.raises(ValueError):
            evaluate.sweep_metrics(bad_counts, bad_thr)
    with pytest.raises(ValueError):
        evaluate.overall_iou(np.zeros((0, 2)))


def test_sweep_thresholds_default_grid():
    from cris.pytorch_amd import evaluate
    t = evaluate.sweep_thresholds()
    assert t.dtype == np.float32 and t.shape == (19,) and (np.diff(t) > 0).all()
    assert t.tolist() == [float(np.float32(s)) for s in ("0.05 0.10 0.15 0.20 0.25 0.30 0.35 0.40 0.45 0.50 0.55 0.60 0.65 0.70 0.75 0.80 "
                                                         "0.85 0.90 0.95").split()]
    assert np.float32(0.35) in t                                                    # the reference's cut is one of them


def test_histogram_to_counts_algebra_equals_the_oracle_at_every_threshold():
    """What the kernel does after the warp, in numpy: k = #{i : value > thr[i]} per pixel, a histogram over (mask bit, k) in which
    the k = 0 bins are left out, suffix sums over k for pred_i / inter_i, union_i = pred_i + gt - inter_i - against
    oracle.eval_post.iou on the same warped map at every threshold (a NaN pixel included: above no threshold)."""
    from oracle import eval_post as EP
    S, oh, ow = 96, 50, 37
    rng = np.random.default_rng(3)
    prob = EP.upsample_bicubic(EP.sigmoid(rng.standard_normal((24, 24)).astype(np.float32) * 3), S, S)
    scale = min(S / oh, S / ow)
    inv = np.array([[1 / scale, 0, -(S - ow * scale) / 2 / scale], [0, 1 / scale, -(S - oh * scale) / 2 / scale]], np.float64)
    warped = EP.warp_affine_cubic(prob, inv, ow, oh)
    warped[7, 11] = np.nan
    mask = (rng.random((oh, ow)) > 0.6).astype(np.uint8) * 255
    mask[0, 0] = 1
    thr = np.array([-0.5, 0.0] + [i / 20 for i in range(1, 20)] + [1.0, 1.5], np.float32)
    T = thr.shape[0]
    with np.errstate(invalid="ignore"):
        k = np.zeros(warped.shape, np.int64)
        for t in thr:                                                               # comparisons of exactly the kernel's form
            k += warped > t
    assert k[7, 11] == 0 and (k[np.isfinite(warped)] >= 1).all() and k.max() == T - 1      # finite values: above -0.5, none above 1.5
    assert len(np.unique(k)) > 10                                                   # the map is not bimodal: the middle bins are used
    m = (mask != 0).astype(np.int64)
    hist = np.zeros((2, T + 1), np.int64)
    np.add.at(hist, (m.ravel(), k.ravel()), 1)
    gt = int(m.sum())
    hist[:, 0] = 0                                                                  # the bins the kernel never counts
    for i in range(T):
        inter = int(hist[1, i + 1:].sum())
        pred = int(hist[:, i + 1:].sum())
        with np.errstate(invalid="ignore"):
            _, want_i, want_u = EP.iou(warped, mask, thr[i])
        assert (inter, pred + gt - inter) == (want_i, want_u), i
    with np.errstate(invalid="ignore"):
        assert EP.iou(warped, mask, thr[0])[1:] == (gt - int(m[7, 11]), oh * ow - 1 + int(m[7, 11]))      # -0.5: every finite pixel predicted
        assert EP.iou(warped, mask, thr[-1])[1:] == (0, gt)                                             # 1.5: nothing predicted
