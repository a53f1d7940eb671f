"""Dataset evaluation on the GPU: the batched warp + threshold + IoU kernel (csrc/evalpost.hip cris_eval_iou_batch) against the
CPU oracle on identical probabilities - integer counts, so equality - and against the per-sample kernels it replaces; then
Evaluator.validate / .inference (cris/pytorch_amd/evaluate.py) over synthetic records against the per-sample path on the very
logits the model produced."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

pytest.importorskip("PIL")

from cris.pytorch_amd import arch, evalpost, evaluate, pngdec, records  # noqa: E402
from cris.pytorch_amd.infer import InferenceRunner  # noqa: E402
from oracle import eval_post as EP  # noqa: E402
from test_infer_multi_gpu import _setup  # noqa: E402
from test_records_gpu import _StandInTokenizer, _record  # noqa: E402

DEV = torch.device("cuda:0")
S = 416
THR = 0.35


def _letterbox_inverse(oh, ow, size=S):
    scale = min(size / oh, size / ow)
    bx, by = (size - ow * scale) / 2.0, (size - oh * scale) / 2.0
    return np.array([[1 / scale, 0, -bx / scale], [0, 1 / scale, -by / scale]], np.float64)


def _kernel_cases():
    """(masks, descriptors (mat, mask, map, row), P): every case of one launch, n = 11 descriptors over P = 3 maps"""
    sizes = [(300, 500), (480, 640), (333, 251)]                       # the letter-box sizes of tests/test_eval_post.py
    masks = [(np.random.default_rng(oh).random((oh, ow)) > 0.6).astype(np.uint8) * 255 for oh, ow in sizes]
    descs = [(_letterbox_inverse(oh, ow), i, i) for i, (oh, ow) in enumerate(sizes)]
    rot = np.array([[0.9, -0.3, 20.5], [0.25, 1.1, -7.25]], np.float64)   # the rotation + shear there, 200 x 300 output
    masks.append((np.random.default_rng(7).random((200, 300)) > 0.5).astype(np.uint8) * 255)
    descs.append((rot, 3, 0))
    for oh, ow in ((1, 1), (5, 3)):                                    # a 1 x 1 and a 5 x 3 original
        masks.append(np.full((oh, ow), 255, np.uint8) if oh == 1 else (np.arange(15).reshape(5, 3) % 2 * 255).astype(np.uint8))
        descs.append((_letterbox_inverse(oh, ow), len(masks) - 1, 1))
    masks[-1][0, 0] = 1                                                # any non-zero byte counts (mask / 255. is truthy)
    descs += [(_letterbox_inverse(300, 500), 0, p) for p in (1, 2, 0)]    # n > P: three more maps against ONE shared mask
    masks += [np.zeros((333, 251), np.uint8), np.full((333, 251), 255, np.uint8)]      # all-zero and all-255 masks
    descs += [(_letterbox_inverse(333, 251), len(masks) - 2, 2), (_letterbox_inverse(333, 251), len(masks) - 1, 2)]
    return masks, [(m, mi, p, row) for row, (m, mi, p) in enumerate(descs)], 3


def test_iou_batch_equals_the_oracle_and_the_per_sample_kernels():
    logits = torch.from_numpy(np.stack([np.random.default_rng(10 + b).standard_normal((104, 104)).astype(np.float32) * 3
                                        for b in range(3)]))[:, None]
    probs_dev = evalpost.sigmoid_upsample(logits.to(DEV), S, S)
    probs = probs_dev.cpu().numpy()                                    # the GPU's own probabilities go to both sides
    masks, descs, P = _kernel_cases()
    n = len(descs)
    assert n == 11 and n > P
    st = evalpost.EvalStaging(DEV).pack(masks, descs).upload()
    counts = torch.zeros(n + 1, 2, dtype=torch.int32, device=DEV)      # (one row more than used: it must stay zero)
    out = torch.full((st.out_bytes,), 0x55, dtype=torch.uint8, device=DEV)
    evalpost.iou_batch(probs_dev, st, st.masks, counts, 0, THR, out_masks=out)
    got, out_h = counts.cpu().numpy(), out.cpu().numpy()
    evalpost.iou_batch(probs_dev, st, st.masks, counts, 0, THR)        # the += contract: a second call doubles the counts
    twice = counts.cpu().numpy()
    assert not got[n].any()
    assert st.descs[6].mask_off == st.descs[7].mask_off == st.descs[8].mask_off == st.descs[0].mask_off
    for k, (mat, mi, p, row) in enumerate(descs):
        oh, ow = masks[mi].shape
        warped = EP.warp_affine_cubic(probs[p], mat, ow, oh)
        _, inter, union = EP.iou(warped, masks[mi], THR)
        print("desc %2d  %3d x %3d  map %d  inter %6d union %6d  (kernel %6d %6d)" % (k, oh, ow, p, inter, union, got[row, 0], got[row, 1]))
        assert (int(got[row, 0]), int(got[row, 1])) == (inter, union), k
        d = st.descs[k]
        pred = out_h[d.out_off:d.out_off + d.pitch * oh].reshape(oh, d.pitch)
        assert np.array_equal(pred[:, :ow], (warped > np.float32(THR)).astype(np.uint8) * 255), k      # byte for byte
        assert not pred[:, ow:].any(), k
        # the retained per-sample kernels on the same probabilities
        w_dev = evalpost.warp_to_original(probs_dev[p], mat, (oh, ow))
        c = evalpost.iou_counts(w_dev, torch.from_numpy(masks[mi].astype(np.float32) / 255.0).to(DEV), THR).cpu().numpy()
        assert (int(c[0]), int(c[1])) == (inter, union), k
    assert np.array_equal(twice, 2 * got)
    assert got[9, 0] == 0 and got[10, 0] == got[9, 1] and got[10, 1] == 333 * 251      # all-zero / all-255 masks
    assert got[:n, 1].min() > 0 and got[:3, 0].min() > 0
    # a window into a larger table: row0 moves every row
    big = torch.zeros(n + 5, 2, dtype=torch.int32, device=DEV)
    evalpost.iou_batch(probs_dev, st, st.masks, big, 4, THR)
    big = big.cpu().numpy()
    assert np.array_equal(big[4:4 + n], got[:n]) and not big[:4].any() and not big[4 + n:].any()
    with pytest.raises(ValueError):
        evalpost.iou_batch(probs_dev, st, st.masks, counts, n + 1, THR)
    with pytest.raises(evalpost.hip.HipLibraryError, match="row out of range"):
        evalpost.iou_batch(probs_dev, st, st.masks, counts, 2, THR)    # the last descriptor's row would fall outside the table


SIZES = [(120, 160), (160, 120), (50, 37), (96, 96), (75, 101), (133, 90), (64, 200), (99, 99), (141, 87), (40, 40)]
SIZE, WORD_LEN = 96, 9


def _records():
    rng = np.random.default_rng(0)
    recs = []
    for i, (h, w) in enumerate(SIZES):
        sents = ["the left one", "Woman's umbrella #%d" % i, "zebra closest 2 us"][:i % 3 + 1]
        v, _ = _record(rng, h, w, 2000 + i, sents, quality=90, subsampling=i % 3)
        recs.append(records.load_record(v))
    return recs


def _runner(use_graph=True):
    clip, head, sd = _setup("tiny", SIZE, WORD_LEN)
    return InferenceRunner(clip, head, sd, DEV, use_graph=use_graph)


class _Keep:
    """a model that is only callable (no `segment`) and keeps the logits of every call"""

    def __init__(self, model):
        self.inner, self.logits = model, []

    def __call__(self, img, word):
        out = self.inner(img, word)
        self.logits.append(out.clone())
        return out


class _KeepSegment(_Keep):
    def segment(self, img, word, index):
        out = self.inner.segment(img, word, index)
        self.logits.append(out.clone())
        return out


def test_validate_equals_validate_batch_on_the_same_logits():
    recs = _records()
    tok = _StandInTokenizer()
    pipe = records.RecordPipeline(SIZE, WORD_LEN, DEV, mode="val", tokenizer=tok)
    model = _Keep(_runner())
    ev = evaluate.Evaluator(model, pipe, thr=THR)
    iou, prec = ev.validate(recs, batch_size=4)
    assert [tuple(l.shape) for l in model.logits] == [(4, 1, SIZE // 4, SIZE // 4)] * 3      # 4 + 4 + padded 2: one shape
    assert model.inner.graph_error is None and len(model.inner._shapes) == 1
    want = []
    for b, lo in enumerate(range(0, 10, 4)):
        part = recs[lo:lo + 4]
        _, _, params = pipe(part)
        masks = [pngdec.decode_gray(r["mask"]).numpy().astype(np.float32) / 255.0 for r in part]
        want += evalpost.validate_batch(model.logits[b][:len(part)], (SIZE, SIZE), [p["inverse"] for p in params],
                                        [p["ori_size"] for p in params], masks, thr=THR)
    print("validate per-sample IoU:", " ".join("%.4f" % v for v in ev.per_sample))
    assert ev.per_sample.tolist() == want                                                  # integer counts: exact
    assert ev.counts.shape == (10, 2) and (ev.counts[:, 1] > 0).all()
    m = evaluate.metrics(ev.counts)
    assert iou == m[0] and prec == m[1] and list(prec) == list(evaluate.PR_KEYS)
    # a subset in another order, and a second pass on the same evaluator
    iou2, _ = ev.validate(recs, indices=[7, 2, 9], batch_size=4)
    assert ev.per_sample.tolist() == [want[7], want[2], want[9]] and iou2 == float(np.mean([want[7], want[2], want[9]]))
    with pytest.raises(ValueError):
        ev.inference(recs)


def test_inference_with_one_visual_pass_equals_the_per_expression_fallback():
    """Every sentence of every image (engine.py:152-190), 4 images per batch: 7 -> 8, 8 and 4 -> 8 expressions (a padded last
    image batch too), one graph shape.  `segment` runs the image stage at batch 4 and the expression stage at batch 8; the
    fallback runs `runner(img[index], word)` at batch 8.  WHICH CASE HOLDS: the logits of the two are bit-equal - the expression
    stage issues the same launches at the same batch in both, the gathers copy rows, and the image stage's GEMMs keep the k order
    of every tile variant, so the batch they run at (4 or 8) does not change a value (tests/test_infer_multi_gpu.py measured the
    same on MI355X, tiny and R50).  The test asserts that equality, and with it EXACT per-expression IoUs."""
    recs = _records()
    pipe = records.RecordPipeline(SIZE, WORD_LEN, DEV, mode="test", tokenizer=_StandInTokenizer())
    runner = _runner()
    seg, plain = _KeepSegment(runner), _Keep(runner)
    seen = []
    ev = evaluate.Evaluator(seg, pipe, thr=THR)
    assert ev._segment is not None
    iou, prec = ev.inference(recs, images_per_batch=4, visualize=lambda rec, sent, i, m: seen.append((rec, sent, i, m)))
    per, counts = ev.per_sample.copy(), ev.counts.copy()
    fb = evaluate.Evaluator(plain, pipe, thr=THR)
    assert fb._segment is None
    iou_fb, prec_fb = fb.inference(recs, images_per_batch=4)
    total = sum(len(r["sents"]) for r in recs)
    assert per.shape == (total,) and total == 19
    assert [tuple(l.shape) for l in seg.logits] == [(8, 1, SIZE // 4, SIZE // 4)] * 3 == [tuple(l.shape) for l in plain.logits]
    assert runner.graph_error is None
    for a, b in zip(seg.logits, plain.logits):
        assert torch.equal(a, b)
    print("inference per-expression IoU:", " ".join("%.4f" % v for v in per))
    assert np.array_equal(counts, fb.counts) and per.tolist() == fb.per_sample.tolist()
    assert (iou, prec) == (iou_fb, prec_fb) == evaluate.metrics(counts)[:2]
    # the first sentence of every record is what validate scores
    val = evaluate.Evaluator(_Keep(runner), records.RecordPipeline(SIZE, WORD_LEN, DEV, mode="val", tokenizer=_StandInTokenizer()), thr=THR)
    val.validate(recs, batch_size=5)
    firsts = np.cumsum([0] + [len(r["sents"]) for r in recs])[:-1]
    print("first sentences, inference vs validate:", per[firsts].tolist(), val.per_sample.tolist())
    # the callback: every expression once, in order, with a mask whose pixel counts reproduce the IoU it is given
    assert len(seen) == total
    k = 0
    for r in recs:
        gt = pngdec.decode_gray(r["mask"]).numpy() != 0
        for s in r["sents"]:
            rec, sent, i, m = seen[k]
            assert rec is r and sent == s and m.dtype == np.uint8 and m.shape == gt.shape and set(np.unique(m)) <= {0, 255}
            p = m != 0
            assert i == np.sum(p & gt) / (np.sum(p | gt) + 1e-6) == per[k]
            k += 1


def test_module_evaluator():
    from types import SimpleNamespace as NS
    from cris.pytorch_amd.model import build_segmenter
    from test_module_surface import TINY
    model, _ = build_segmenter(NS(**TINY))
    clip, head = arch.specs_by_name("tiny")
    model.load_state_dict(arch.synthetic_state_dict(clip, head, 0))
    model = model.to(DEV)
    pipe = records.RecordPipeline(64, 9, DEV, mode="val", tokenizer=_StandInTokenizer())
    model.train()
    with pytest.raises(RuntimeError, match="eval"):
        model.evaluator(pipe)
    model.eval()
    ev = model.evaluator(pipe, thr=THR)
    assert isinstance(ev, evaluate.Evaluator) and ev._segment is not None
    recs = _records()[:4]
    iou, prec = ev.validate(recs, batch_size=4)
    img, word, params = pipe(recs)
    keep = model(img, word)
    masks = [pngdec.decode_gray(r["mask"]).numpy().astype(np.float32) / 255.0 for r in recs]
    want = evalpost.validate_batch(keep, (64, 64), [p["inverse"] for p in params], [p["ori_size"] for p in params], masks, thr=THR)
    assert ev.per_sample.tolist() == want and iou == float(np.mean(want))
