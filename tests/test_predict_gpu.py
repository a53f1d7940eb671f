"""Prediction on unlabeled images on the GPU: the batched warp + threshold + statistics kernel (csrc/evalpost.hip
cris_predict_masks_batch) against the CPU oracle on identical probabilities - mask bytes and integer statistics, so equality -
and against cris_eval_iou_batch, whose per-pixel value it shares; then predict.Predictor over synthetic JPEGs against
Evaluator.inference's masks and against numpy on the per-expression warp of the very logits the model produced."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

pytest.importorskip("PIL")

from cris.pytorch_amd import arch, evalpost, evaluate, jpegdec, predict, records  # noqa: E402
from cris.pytorch_amd.infer import InferenceRunner  # noqa: E402
from oracle import eval_post as EP  # noqa: E402
from test_infer_multi_gpu import _setup  # noqa: E402
from test_records_gpu import _StandInTokenizer, _record  # noqa: E402

DEV = torch.device("cuda:0")
S, P = 96, 4
THR = 0.35
INIT = list(evalpost.PREDICT_INIT)
ROT = np.array([[0.9, -0.3, 20.5], [0.25, 1.1, -7.25]], np.float64)      # the rotation + shear of tests/test_evaluate_gpu.py


def _letterbox_inverse(oh, ow, size=S):
    scale = min(size / oh, size / ow)
    bx, by = (size - ow * scale) / 2.0, (size - oh * scale) / 2.0
    return np.array([[1 / scale, 0, -bx / scale], [0, 1 / scale, -by / scale]], np.float64)


# (h, w) of every output and (matrix, shape, map) of every descriptor: n = 9 over P = 4 maps (maps shared), one launch
SHAPES = [(1, 1), (5, 3), (3, 5), (50, 37), (480, 640), (29, 41)]
DESCS = [(None, 0, 0), (None, 1, 1), (None, 2, 2), (None, 3, 2), (None, 4, 0), (ROT, 5, 1), (None, 3, 3), (None, 4, 2), (None, 3, 0)]


def _descs(row_of=lambda k: k):
    return [(_letterbox_inverse(*SHAPES[si]) if mat is None else mat, si, mp, row_of(k)) for k, (mat, si, mp) in enumerate(DESCS)]


@pytest.fixture(scope="module")
def case():
    """the probability maps (device and host copies of the same bits) and the oracle's expectation per descriptor, computed once"""
    logits = torch.from_numpy(np.stack([np.random.default_rng(10 + b).standard_normal((24, 24)).astype(np.float32) * 3 for b in range(2)]))
    rect = torch.full((S, S), 0.05)
    rect[20:60, 30:80] = 0.9                                               # a non-trivial box
    probs_dev = torch.cat([evalpost.sigmoid_upsample(logits[:, None].to(DEV), S, S), rect[None].to(DEV),
                           torch.zeros(1, S, S, device=DEV)]).contiguous()
    probs = probs_dev.cpu().numpy()                                        # the GPU's own probabilities go to both sides
    want = []
    for mat, si, mp, _ in _descs():
        h, w = SHAPES[si]
        v = EP.warp_affine_cubic(probs[mp], mat, w, h)
        fg = v > np.float32(THR)
        area = int(fg.sum())
        q16 = int(np.rint(v[fg] * np.float32(65536)).astype(np.int64).sum())
        ys, xs = np.nonzero(fg)
        box = [int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1] if area else INIT[2:]
        want.append((fg, [area, q16] + box, float(v.min()), float(v.max())))
    return probs_dev, want


def _check_output(st, out_h, want, fill):
    used = np.zeros(out_h.shape[0], bool)
    for k, (fg, _, _, _) in enumerate(want):
        d = st.descs[k]
        h, w = fg.shape
        assert (d.h_out, d.w_out) == (h, w) and d.pitch == (w + 3) // 4 * 4
        rows = out_h[d.out_off:d.out_off + d.pitch * h].reshape(h, d.pitch)
        assert np.array_equal(rows[:, :w], fg.astype(np.uint8) * 255), k   # byte for byte
        assert not rows[:, w:].any(), k                                    # padding bytes are zero
        assert not used[d.out_off:d.out_off + d.pitch * h].any()
        used[d.out_off:d.out_off + d.pitch * h] = True
    assert (out_h[~used] == fill).all() and (~used).sum() >= 64            # gaps between outputs and the tail: untouched


def test_predict_batch_equals_the_oracle(case):
    probs_dev, want = case
    n = len(DESCS)
    assert n > P
    st = evalpost.EvalStaging(DEV, mask_bytes=16).pack_sizes(SHAPES, _descs()).upload()
    stats = evalpost.new_predict_stats(n + 1, DEV)                         # (one row more than used: it must keep its initial value)
    out = torch.full((st.out_bytes + 64,), 0x55, dtype=torch.uint8, device=DEV)
    evalpost.predict_batch(probs_dev, st, stats, 0, THR, out_masks=out)
    got, out_h = stats.cpu().numpy(), out.cpu().numpy()
    evalpost.predict_batch(probs_dev, st, stats, 0, THR)                   # the accumulate contract, statistics only
    twice = stats.cpu().numpy()
    for k, (fg, row, lo, hi) in enumerate(want):
        print("desc %d  %3d x %3d  map %d  warp %.3f .. %.3f  want %s  kernel %s" % (k, fg.shape[0], fg.shape[1], DESCS[k][2], lo, hi, row, got[k].tolist()))
        assert got[k].tolist() == row, k
        assert twice[k].tolist() == [2 * row[0], 2 * row[1]] + row[2:], k  # sums double, the box stays
    assert got[n].tolist() == INIT and twice[n].tolist() == INIT
    _check_output(st, out_h, want, 0x55)
    # the cases are what they were chosen for
    assert want[6][1] == INIT and not want[6][0].any()                     # the zero map: empty mask, untouched box
    assert want[0][0].shape == (1, 1)
    a3 = want[3][1]                                                        # the rectangle at 50 x 37: a box strictly inside
    assert 0 < a3[2] < a3[4] < 37 and 0 < a3[3] < a3[5] < 50 and 0 < a3[0] <= (a3[4] - a3[2]) * (a3[5] - a3[3])
    a7 = want[7][1]                                                        # and at 480 x 640: several blocks, grid-stride,
    assert a7[0] > 256 * 256 and 0 < a7[2] < a7[4] < 640 and 0 < a7[3] < a7[5] < 480 and a7[1] > 2 ** 32      # a sum past 32 bits
    assert want[4][1][0] > 0 and 0 < want[5][1][0] < 29 * 41               # the rotated output: partly foreground
    # a window into a larger table: row0 moves every row, the other rows keep their initial values
    big = evalpost.new_predict_stats(n + 5, DEV)
    evalpost.predict_batch(probs_dev, st, big, 3, THR)
    big = big.cpu().numpy()
    assert np.array_equal(big[3:3 + n], got[:n]) and big[:3].tolist() == [INIT] * 3 and big[3 + n:].tolist() == [INIT] * 2
    # rows in another order inside the launch
    perm = [4, 0, 8, 2, 6, 1, 7, 3, 5]
    st2 = evalpost.EvalStaging(DEV, mask_bytes=16).pack_sizes(SHAPES, _descs(lambda k: perm[k])).upload()
    other = evalpost.new_predict_stats(n, DEV)
    evalpost.predict_batch(probs_dev, st2, other, 0, THR)
    other = other.cpu().numpy()
    assert all(other[perm[k]].tolist() == want[k][1] for k in range(n))
    with pytest.raises(ValueError):
        evalpost.predict_batch(probs_dev, st, stats, n + 1, THR)
    with pytest.raises(evalpost.hip.HipLibraryError, match="row out of range"):
        evalpost.predict_batch(probs_dev, st, stats, 2, THR)               # the last descriptor's row would fall outside the table
    with pytest.raises(ValueError):
        evalpost.predict_batch(probs_dev, st, stats, 0, THR, out_masks=out[:st.out_bytes - 1])


def test_predict_batch_agrees_with_iou_batch(case):
    probs_dev, want = case
    n = len(DESCS)
    st = evalpost.EvalStaging(DEV, mask_bytes=16).pack_sizes(SHAPES, _descs()).upload()
    stats = evalpost.new_predict_stats(n, DEV)
    out = torch.full((st.out_bytes,), 0xAA, dtype=torch.uint8, device=DEV)
    evalpost.predict_batch(probs_dev, st, stats, 0, THR, out_masks=out)
    area = stats[:, 0].cpu().numpy()
    for value in (0, 255):
        ev = evalpost.EvalStaging(DEV).pack([np.full(s, value, np.uint8) for s in SHAPES], _descs()).upload()
        assert ev.out_bytes == st.out_bytes
        counts = torch.zeros(n, 2, dtype=torch.int32, device=DEV)
        ref = torch.full((ev.out_bytes,), 0xAA, dtype=torch.uint8, device=DEV)
        evalpost.iou_batch(probs_dev, ev, ev.masks, counts, 0, THR, out_masks=ref)
        assert torch.equal(out, ref)                                       # the same layout, byte for byte
        counts = counts.cpu().numpy()
        # all-zero masks: union = prediction; all-255 masks: intersection = prediction
        assert np.array_equal(counts[:, 1 if value == 0 else 0], area)
        assert np.array_equal(counts[:, 0 if value == 0 else 1], np.zeros(n) if value == 0 else [h * w for _, si, _ in DESCS for h, w in [SHAPES[si]]])
    assert area.tolist() == [w[1][0] for w in want]
    # statistics only: the same table, nothing written
    only = evalpost.new_predict_stats(n, DEV)
    evalpost.predict_batch(probs_dev, st, only, 0, THR, out_masks=None)
    assert torch.equal(only, stats)


# ---- end to end, tiny model ----
SIZES = [(120, 160), (50, 37), (96, 96), (75, 101), (64, 200)]
SIZE, WORD_LEN = 96, 9
E2E_THR = 0.75          # synthetic weights give probabilities around 0.7 - 0.9: at 0.35 every mask would be the whole image


def _records():
    rng = np.random.default_rng(0)
    recs = []
    for i, (h, w) in enumerate(SIZES):
        sents = ["the left one", "Woman's umbrella #%d" % i, "zebra closest 2 us"][:i % 3 + 1]
        v, _ = _record(rng, h, w, 3000 + i, sents, quality=90, subsampling=i % 3)
        recs.append(records.load_record(v))
    return recs


class _KeepSegment:
    """the runner behind `segment` and `__call__`, keeping the logits of every call"""

    def __init__(self, model):
        self.inner, self.logits = model, []

    def __call__(self, img, word):
        out = self.inner(img, word)
        self.logits.append(out.clone())
        return out

    def segment(self, img, word, index):
        out = self.inner.segment(img, word, index)
        self.logits.append(out.clone())
        return out


def _same(a, b, masks=True):
    assert [len(x) for x in a] == [len(x) for x in b]
    for pa, pb in zip((p for x in a for p in x), (p for x in b for p in x)):
        assert (pa.sentence, pa.area, pa.box, pa.score) == (pb.sentence, pb.area, pb.box, pb.score)
        if masks:
            ma = pa.mask.cpu().numpy() if torch.is_tensor(pa.mask) else pa.mask
            mb = pb.mask.cpu().numpy() if torch.is_tensor(pb.mask) else pb.mask
            assert ma.dtype == np.uint8 and np.array_equal(ma, mb)


def test_predictor_end_to_end(monkeypatch):
    recs = _records()
    files, exprs = [r["img"] for r in recs], [r["sents"] for r in recs]
    assert [len(e) for e in exprs] == [1, 2, 3, 1, 2]
    pipe = records.RecordPipeline(SIZE, WORD_LEN, DEV, mode="test", tokenizer=_StandInTokenizer())
    clip, head, sd = _setup("tiny", SIZE, WORD_LEN)
    runner = InferenceRunner(clip, head, sd, DEV)
    model = _KeepSegment(runner)
    # Evaluator.inference on the same records: same batches (2 + 2 + padded 1), same graph shapes
    seen = []
    evaluate.Evaluator(model, pipe, thr=E2E_THR).inference(recs, images_per_batch=2, visualize=lambda rec, sent, iou, m: seen.append((sent, m)))
    ev_logits, model.logits = model.logits, []
    pr = predict.Predictor(model, pipe, thr=E2E_THR)
    assert pr._segment is not None
    out = pr.predict(files, exprs, images_per_batch=2, masks="host")
    assert [tuple(l.shape) for l in model.logits] == [(8, 1, SIZE // 4, SIZE // 4)] * 3 and runner.graph_error is None
    assert len(runner._shapes) == 1                                        # the evaluator's graph, replayed
    for a, b in zip(ev_logits, model.logits):
        assert torch.equal(a, b)
    flat = [p for x in out for p in x]
    assert [p.sentence for p in flat] == [s for s, _ in seen] == [s for e in exprs for s in e]
    # the warp of the kept logits, per expression, through the per-sample kernel
    k = 0
    for b, lo in enumerate(range(0, len(recs), 2)):
        part = recs[lo:lo + 2]
        _, params = pipe(part)
        probs = evalpost.sigmoid_upsample(model.logits[b], SIZE, SIZE)
        j = 0
        for r, prm in zip(part, params):
            h, w = (int(v) for v in prm["ori_size"])
            for _ in r["sents"]:
                p = flat[k]
                assert isinstance(p.mask, np.ndarray) and p.mask.dtype == np.uint8 and p.mask.shape == (h, w) and p.mask.flags["C_CONTIGUOUS"]
                assert np.array_equal(p.mask, seen[k][1])                  # Evaluator.inference's mask, byte for byte
                v = evalpost.warp_to_original(probs[j], prm["inverse"], (h, w)).cpu().numpy()
                fg = v > np.float32(E2E_THR)
                assert np.array_equal(p.mask, fg.astype(np.uint8) * 255)
                area = int(fg.sum())
                ys, xs = np.nonzero(fg)
                assert p.area == area == int((p.mask != 0).sum())
                assert p.box == ((int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1) if area else None)
                q16 = int(np.rint(v[fg] * np.float32(65536)).astype(np.int64).sum())
                assert p.score == (q16 / (65536.0 * area) if area else 0.0) and isinstance(p.score, float)
                print("expr %2d  %3d x %3d  area %5d  box %s  score %.4f" % (k, h, w, p.area, p.box, p.score))
                k += 1
                j += 1
    assert k == 9 and any(0 < p.area < p.mask.size for p in flat)           # some masks are partial: their boxes say something
    # decoded arrays in place of the files; device masks; statistics only (no output buffer at all)
    arrays = [t.cpu().numpy() for t in jpegdec.decode_batch(files, DEV)]
    _same(pr.predict(arrays, exprs, images_per_batch=2, masks="host"), out)
    _same(pr.predict([torch.from_numpy(a) for a in arrays], exprs, images_per_batch=2, masks="host"), out)
    dev_out = pr.predict(files, exprs, images_per_batch=2, masks="device")
    assert all(torch.is_tensor(p.mask) and p.mask.is_cuda and p.mask.dtype == torch.uint8 for x in dev_out for p in x)
    _same(dev_out, out)
    calls = []
    real = evalpost.predict_batch
    monkeypatch.setattr(evalpost, "predict_batch", lambda *a, **kw: (calls.append(kw.get("out_masks", "missing")), real(*a, **kw))[1])
    none_out = pr.predict(files, exprs, images_per_batch=2, masks=None)
    assert calls == [None] * 3 and all(p.mask is None for x in none_out for p in x)
    _same(none_out, out, masks=False)
    monkeypatch.undo()
    # a single str per image, another batch size, and a model without `segment`
    one = pr.predict(files[:3], [e[0] for e in exprs[:3]], images_per_batch=3)
    assert [len(x) for x in one] == [1, 1, 1]
    plain = predict.Predictor(lambda img, word: runner(img, word), pipe, thr=E2E_THR)
    assert plain._segment is None
    _same(plain.predict(files, exprs, images_per_batch=2), out)


def test_module_predictor():
    from types import SimpleNamespace as NS
    from cris.pytorch_amd.model import build_segmenter
    from test_module_surface import TINY
    model, _ = build_segmenter(NS(**TINY))
    clip, head = arch.specs_by_name("tiny")
    model.load_state_dict(arch.synthetic_state_dict(clip, head, 0))
    model = model.to(DEV)
    pipe = records.RecordPipeline(64, 9, DEV, mode="test", tokenizer=_StandInTokenizer())
    model.train()
    with pytest.raises(RuntimeError, match="eval"):
        model.predictor(pipe)
    model.eval()
    pr = model.predictor(pipe, thr=E2E_THR)
    assert isinstance(pr, predict.Predictor) and pr._segment is not None
    recs = _records()[:3]
    files, exprs = [r["img"] for r in recs], [r["sents"] for r in recs]
    got = pr.predict(files, exprs, images_per_batch=2)
    _same(got, predict.Predictor(model, pipe, thr=E2E_THR).predict(files, exprs, images_per_batch=2))
    assert [len(x) for x in got] == [1, 2, 3] and all(p.mask.shape == SIZES[i] for i, x in enumerate(got) for p in x)
