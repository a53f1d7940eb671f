"""The threshold sweep on the GPU: cris_eval_iou_sweep_batch (csrc/evalpost.hip) against the single-threshold kernel it shares its
per-pixel value with - integer counts, so equality, column by column - and against the CPU oracle on the GPU's own
probabilities; then Evaluator.sweep (cris/pytorch_amd/evaluate.py) against one validate / inference pass per threshold."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

pytest.importorskip("PIL")

from cris.pytorch_amd import arch, evalpost, evaluate, records  # noqa: E402
from oracle import eval_post as EP  # noqa: E402
from test_evaluate_gpu import _Keep, _KeepSegment, _letterbox_inverse, _records, _runner  # noqa: E402
from test_records_gpu import _StandInTokenizer  # noqa: E402

DEV = torch.device("cuda:0")
S = 96
NAN_MAP = 2
THRS = np.array([-0.5, 0.0] + [i / 20 for i in range(1, 20)] + [1.0, 1.5], np.float32)


def _probs():
    """three 24 x 24 logit maps through sigmoid_upsample to 96 x 96: random x 3; constant +40 (sigmoid is exactly 1.0: the warp's
    cubic weights overshoot around 1.0, so `> 1.0` is decided by single ulps); random with one NaN"""
    maps = [np.random.default_rng(20).standard_normal((24, 24)).astype(np.float32) * 3, np.full((24, 24), 40.0, np.float32),
            np.random.default_rng(22).standard_normal((24, 24)).astype(np.float32) * 3]
    maps[NAN_MAP][9, 14] = np.nan
    dev = evalpost.sigmoid_upsample(torch.from_numpy(np.stack(maps))[:, None].to(DEV), S, S)
    host = dev.cpu().numpy()
    # (the fixture, not the kernel under test: the upsample's two 4-tap passes round 1.0 by a few ulps - values on both sides of 1.0)
    assert np.abs(host[1] - 1.0).max() < 4e-6 and (host[1] > 1.0).any() and (host[1] < 1.0).any()
    assert np.isnan(host[NAN_MAP]).any() and np.isfinite(host[0]).all()
    return dev, host


def _kernel_cases():
    """(masks, descriptors (mat, mask, map, row)): 14 descriptors over 3 maps and 9 masks"""
    masks, descs = [], []
    for k, (oh, ow) in enumerate(((1, 1), (5, 3), (50, 37), (75, 101))):          # letter-box originals; the last one is upsampled
        masks.append((np.random.default_rng(30 + k).random((oh, ow)) > 0.5).astype(np.uint8) * 255)
        descs.append((_letterbox_inverse(oh, ow, S), k, k % 2))
    masks[0][0, 0] = 255
    masks[2][3, 5] = 1                                                              # any non-zero byte counts
    descs.append((_letterbox_inverse(75, 101, S), 3, NAN_MAP))
    rot = np.array([[0.9, -0.3, 5.5], [0.25, 1.1, -3.25]], np.float64)              # rotation + shear, 40 x 60 output
    masks.append((np.random.default_rng(7).random((40, 60)) > 0.5).astype(np.uint8) * 255)
    descs += [(rot, 4, 0), (rot, 4, 1)]
    masks.append((np.random.default_rng(8).random((50, 37)) > 0.7).astype(np.uint8) * 255)
    descs += [(_letterbox_inverse(50, 37, S), 5, p) for p in (0, 1, NAN_MAP)]      # three descriptors share ONE mask
    masks += [np.zeros((50, 37), np.uint8), np.full((50, 37), 255, np.uint8)]      # all-zero and all-255 masks
    descs += [(_letterbox_inverse(50, 37, S), 6, 0), (_letterbox_inverse(50, 37, S), 7, 0),
              (_letterbox_inverse(50, 37, S), 6, 1), (_letterbox_inverse(50, 37, S), 7, 1)]
    return masks, [(m, mi, p, row) for row, (m, mi, p) in enumerate(descs)]


def _single(probs_dev, st, rows, thr):
    """a fresh single-threshold table at the float32 value of thr"""
    c = torch.zeros(rows, 2, dtype=torch.int32, device=DEV)
    evalpost.iou_batch(probs_dev, st, st.masks, c, 0, float(np.float32(thr)))
    return c.cpu().numpy()


def test_sweep_kernel_equals_the_single_threshold_kernel_and_the_oracle():
    probs_dev, probs = _probs()
    masks, descs = _kernel_cases()
    n = len(descs)
    st = evalpost.EvalStaging(DEV).pack(masks, descs).upload()
    assert st.descs[7].mask_off == st.descs[8].mask_off == st.descs[9].mask_off
    warped = [None if p == NAN_MAP else EP.warp_affine_cubic(probs[p], mat, masks[mi].shape[1], masks[mi].shape[0])
              for mat, mi, p, _ in descs]                                          # once, for every threshold list
    for thrs in (THRS, np.array([0.35], np.float32), np.linspace(-0.1, 1.1, 64).astype(np.float32)):
        T = len(thrs)
        counts = torch.zeros(n + 1, T, 2, dtype=torch.int32, device=DEV)           # (one row more than used: it must stay zero)
        evalpost.iou_sweep_batch(probs_dev, st, st.masks, counts, 0, thrs)
        got = counts.cpu().numpy()
        evalpost.iou_sweep_batch(probs_dev, st, st.masks, counts, 0, [float(t) for t in thrs])      # +=: a second call doubles
        assert np.array_equal(counts.cpu().numpy(), 2 * got)
        assert not got[n].any()
        for i, t in enumerate(thrs):
            want = _single(probs_dev, st, n + 1, t)
            assert np.array_equal(got[:, i], want), (T, i, float(t), got[:, i].tolist(), want.tolist())
            for k, (mat, mi, p, row) in enumerate(descs):
                if warped[k] is not None:
                    _, inter, union = EP.iou(warped[k], masks[mi], np.float32(t))
                    assert (int(got[row, i, 0]), int(got[row, i, 1])) == (inter, union), (T, i, k)
        print("T = %2d: union per threshold of descriptor 2:" % T, got[2, :, 1].tolist())
    # THRS again: the columns whose counts are known without a warp, and a window into a larger table
    T = len(THRS)
    counts = torch.zeros(n + 6, T, 2, dtype=torch.int32, device=DEV)
    evalpost.iou_sweep_batch(probs_dev, st, st.masks, counts, 4, THRS)
    big = counts.cpu().numpy()
    assert not big[:4].any() and not big[4 + n:].any()
    got = big[4:4 + n]
    for k, (mat, mi, p, row) in enumerate(descs):
        oh, ow = masks[mi].shape
        gt = int((masks[mi] != 0).sum())
        if p != NAN_MAP:
            assert got[row, 0].tolist() == [gt, oh * ow], k                        # -0.5: every pixel is predicted
        assert got[row, -1].tolist() == [0, gt], k                                 # 1.5: none is
        assert (np.diff(got[row, :, 0]) <= 0).all() and (np.diff(got[row, :, 1]) <= 0).all(), k
    assert len({tuple(c) for c in got[2].tolist()}) > 10                            # the random map uses the middle bins
    assert got[4, 0, 1] < 75 * 101                                                  # the NaN reaches the original: above no threshold
    with pytest.raises(ValueError):
        evalpost.iou_sweep_batch(probs_dev, st, st.masks, counts, n + 6, THRS)
    with pytest.raises(ValueError):
        evalpost.iou_sweep_batch(probs_dev, st, st.masks, counts, 0, THRS[:5])     # T of the table and of the list differ
    with pytest.raises(ValueError):
        evalpost.iou_sweep_batch(probs_dev, st, st.masks, counts[:, :, :1], 0, THRS)
    with pytest.raises(evalpost.hip.HipLibraryError, match="row out of range"):
        evalpost.iou_sweep_batch(probs_dev, st, st.masks, counts, 7, THRS)         # the last descriptor's row falls outside
    with pytest.raises(evalpost.hip.HipLibraryError, match="strictly increasing"):
        evalpost.iou_sweep_batch(probs_dev, st, st.masks, counts[:, :2].contiguous(), 0, [0.5, 0.5])


def test_sweep_kernel_grid_stride():
    """300 descriptors of 120 x 160: 4800 groups each need 19 blocks of 256, the launcher's cap at n = 300 is 8, so every block
    strides over its descriptor's groups (and one thread's LDS bins collect several groups)"""
    probs_dev, _ = _probs()
    rng = np.random.default_rng(40)
    masks = [(rng.random((120, 160)) > q).astype(np.uint8) * 255 for q in (0.3, 0.6, 0.9)]
    mats = [_letterbox_inverse(120, 160, S), np.array([[1.6, 0.3, -5.0], [-0.2, 1.3, 12.0]], np.float64),
            np.array([[1.9, 0.0, -10.5], [0.0, 1.4, 1.25]], np.float64)]
    descs = [(mats[k % 3], k % 3, k % 3, k) for k in range(300)]
    st = evalpost.EvalStaging(DEV).pack(masks, descs).upload()
    thrs = evaluate.sweep_thresholds()
    counts = torch.zeros(300, len(thrs), 2, dtype=torch.int32, device=DEV)
    evalpost.iou_sweep_batch(probs_dev, st, st.masks, counts, 0, thrs)
    got = counts.cpu().numpy()
    for i, t in enumerate(thrs):
        assert np.array_equal(got[:, i], _single(probs_dev, st, 300, t)), i
    assert np.array_equal(got[3:], got[:-3]) and got[:3, :, 1].min() > 0            # the triples repeat
    assert len({tuple(c) for c in got[0].tolist()}) > 10


def _per_threshold(model, pipe, thrs, **kw):
    out = []
    for t in thrs:
        ev = evaluate.Evaluator(model, pipe, thr=float(np.float32(t)))
        res = ev.validate(**kw) if pipe.mode == "val" else ev.inference(**kw)
        out.append((res, ev.counts.copy()))
    return out


def test_evaluator_sweep_equals_one_pass_per_threshold():
    recs = _records()
    tok = _StandInTokenizer()
    runner = _runner()
    thrs = [0.2, 0.35, 0.5]
    # validate: ten first sentences, batches of 4 (4 + 4 + padded 2)
    pipe = records.RecordPipeline(96, 9, DEV, mode="val", tokenizer=tok)
    model = _Keep(runner)
    ev = evaluate.Evaluator(model, pipe)
    res = ev.sweep(recs, thrs, split="validate", batch_size=4)
    assert [tuple(l.shape) for l in model.logits] == [(4, 1, 24, 24)] * 3          # exactly 3 model calls of one shape
    assert runner.graph_error is None and len(runner._shapes) == 1
    assert ev.sweep_counts.shape == (10, 3, 2) and res.per_sample.shape == (10, 3) and res.thresholds.dtype == np.float32
    for i, ((iou, prec), counts) in enumerate(_per_threshold(runner, pipe, thrs, records=recs, batch_size=4)):
        assert np.array_equal(ev.sweep_counts[:, i], counts), i
        assert res.at(thrs[i]) == (iou, prec)
    assert res.at(0.35) == evaluate.Evaluator(runner, pipe, thr=0.35).validate(recs, batch_size=4)
    print("validate sweep: IoU", res.iou.tolist(), "overall", res.overall_iou.tolist(), "best", res.best())
    full = ev.sweep_counts.copy()
    sub = ev.sweep(recs, thrs, indices=[7, 2, 9], batch_size=4)                     # a subset in another order, the same evaluator
    assert np.array_equal(ev.sweep_counts, full[[7, 2, 9]]) and np.array_equal(sub.per_sample, res.per_sample[[7, 2, 9]])
    for bad in (dict(split="inference"), dict(split="test"), dict(thresholds=[0.5, 0.2]), dict(thresholds=[]), dict(indices=[])):
        with pytest.raises(ValueError):
            ev.sweep(recs, **bad)
    # inference: all 19 expressions, 4 images per batch, one visual pass per image (`segment`), the default grid
    pipe_t = records.RecordPipeline(96, 9, DEV, mode="test", tokenizer=tok)
    seg = _KeepSegment(runner)
    ev_t = evaluate.Evaluator(seg, pipe_t)
    assert ev_t._segment is not None
    res_t = ev_t.sweep(recs, split="inference", images_per_batch=4)
    assert [tuple(l.shape) for l in seg.logits] == [(8, 1, 24, 24)] * 3
    grid = evaluate.sweep_thresholds()
    assert ev_t.sweep_counts.shape == (19, 19, 2) and np.array_equal(res_t.thresholds, grid)
    for i, ((iou, prec), counts) in enumerate(_per_threshold(runner, pipe_t, grid, records=recs, images_per_batch=4)):
        assert np.array_equal(ev_t.sweep_counts[:, i], counts), i
        assert res_t.at(grid[i]) == (iou, prec)
    with pytest.raises(ValueError):
        ev_t.sweep(recs, split="validate")


def test_module_evaluator_sweep():
    from types import SimpleNamespace as NS
    from cris.pytorch_amd.model import build_segmenter
    from test_module_surface import TINY
    model, _ = build_segmenter(NS(**TINY))
    clip, head = arch.specs_by_name("tiny")
    model.load_state_dict(arch.synthetic_state_dict(clip, head, 0))
    model = model.to(DEV).eval()
    pipe = records.RecordPipeline(64, 9, DEV, mode="val", tokenizer=_StandInTokenizer())
    ev = model.evaluator(pipe)
    recs = _records()[:4]
    res = ev.sweep(recs, [0.2, 0.35, 0.5], batch_size=4)
    for i, t in enumerate([0.2, 0.35, 0.5]):
        one = model.evaluator(pipe, thr=t)
        assert res.at(t) == one.validate(recs, batch_size=4) and np.array_equal(ev.sweep_counts[:, i], one.counts)
