"""Connected-component clean-up on the GPU (csrc/evalpost.hip cc_* kernels behind evalpost.label_components / filter_components /
mask_iou_batch) against the numpy oracle of tests/components_cases.py.  Every result is an integer, so every
comparison is an equality: canonical labels, filtered mask bytes, the info table, the statistics of the kept pixels, the counts.
Then predict.Predictor and evaluate.Evaluator with a Components spec on the tiny synthetic model, against the oracle applied to the
masks of the plain calls; and with components=None the very library calls of the calls without the keyword."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

pytest.importorskip("PIL")

import components_cases as CC  # noqa: E402
from cris.pytorch_amd import evalpost, evaluate, hip, pngdec, predict, records  # noqa: E402
from cris.pytorch_amd.evalpost import Components  # noqa: E402
from cris.pytorch_amd.infer import InferenceRunner  # noqa: E402
from test_infer_multi_gpu import _setup  # noqa: E402
from test_predict_gpu import DESCS, E2E_THR, S, SHAPES, SIZE, THR, WORD_LEN, _descs, _KeepSegment  # noqa: E402
from test_predict_gpu import _records as _predict_records  # noqa: E402
from test_records_gpu import _StandInTokenizer  # noqa: E402

DEV = torch.device("cuda:0")
IDENT = np.array([[1.0, 0, 0], [0, 1.0, 0]], np.float64)
FILL = 0x7F7F7F7F


def _pack():
    """every case of components_cases in ONE ragged batch, uploaded straight into the packed layout: one descriptor per mask, in
    order, so a mask's bytes sit at its descriptor's out_off"""
    masks = [m for _, m in CC.cases()]
    st = evalpost.EvalStaging(DEV).pack(masks, [(IDENT, i, 0, i) for i in range(len(masks))]).upload()
    assert st.mask_bytes == st.out_bytes and all(st.descs[i].mask_off == st.descs[i].out_off for i in range(st.n))
    return st, masks


@pytest.fixture(scope="module")
def batch():
    return _pack()


def _rect(buf, d):
    return buf[d.out_off:d.out_off + d.pitch * d.h_out].reshape(d.h_out, d.pitch)


@pytest.mark.parametrize("conn", [4, 8])
def test_label_components_equals_the_oracle(batch, conn):
    st, masks = batch
    assert st.n == len(CC.cases()) >= 12
    buf = st.masks.clone()
    out = torch.full((st.out_bytes + 16,), FILL, dtype=torch.int32, device=DEV)
    labels = evalpost.label_components(buf, st, conn, out=out)
    assert labels.shape == (st.out_bytes,) and labels.dtype == torch.int32 and labels.data_ptr() == out.data_ptr()
    got, used = out.cpu().numpy(), np.zeros(st.out_bytes + 16, bool)
    for i, ((name, m), want) in enumerate(zip(CC.cases(), CC.expected_labels(conn))):
        d = st.descs[i]
        h, w = m.shape
        assert (d.h_out, d.w_out, d.pitch) == (h, w, CC.pitch_of(w))
        rows = _rect(got, d)
        n_got, n_want = np.unique(rows[rows >= 0]).size, np.unique(want[want >= 0]).size
        print("conn %d  %-16s %3d x %3d  components %4d (oracle %4d)" % (conn, name, h, w, n_got, n_want))
        assert np.array_equal(rows[:, :w], want), (name, conn)             # canonical labels, exactly
        assert (rows[:, w:] == -1).all(), (name, conn)                      # padding is background
        used[d.out_off:d.out_off + d.pitch * h] = True
    assert (got[~used] == FILL).all()                                       # the gaps between rectangles and the tail: untouched
    assert torch.equal(buf, st.masks)                                       # labelling reads the masks only
    # two descriptors of equal content: equal labels, each relative to its own out_off
    names = [k for k, _ in CC.cases()]
    a, b = st.descs[names.index("random 0.5")], st.descs[names.index("random 0.5 again")]
    assert a.out_off != b.out_off and np.array_equal(_rect(got, a), _rect(got, b))
    # a fresh buffer (out=None) and a second run: the same words
    again = evalpost.label_components(buf, st, conn)
    assert again.shape == (st.out_bytes,)
    assert np.array_equal(again.cpu().numpy()[used[:st.out_bytes]], got[:st.out_bytes][used[:st.out_bytes]])
    with pytest.raises(ValueError, match="connectivity"):
        evalpost.label_components(buf, st, 6)
    with pytest.raises(ValueError, match="out must be"):
        evalpost.label_components(buf, st, conn, out=out[:st.out_bytes - 1])
    with pytest.raises(ValueError, match="masks_u8"):
        evalpost.label_components(buf[:st.out_bytes - 1], st, conn)


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("spec", CC.SPECS, ids=lambda s: "%s-%d" % (s["keep"], s["min_area"]))
def test_filter_components_equals_the_oracle(batch, conn, spec):
    st, masks = batch
    n = st.n
    buf = st.masks.clone()
    labels = evalpost.label_components(buf, st, conn)
    info = torch.zeros(n + 3, 4, dtype=torch.int64, device=DEV)
    evalpost.filter_components(buf, labels, st, Components(connectivity=conn, **spec), info, 2)      # a window: row0 = 2
    got, table = buf.cpu().numpy(), info.cpu().numpy()
    assert table[:2].tolist() == [[0] * 4] * 2 and table[n + 2].tolist() == [0] * 4
    for i, (name, m) in enumerate(CC.cases()):
        kept, want_info, _ = CC.filter_mask(m, connectivity=conn, **spec)
        d = st.descs[i]
        rows = _rect(got, d)
        print("conn %d  %-16s %s  info %s (oracle %s)" % (conn, name, spec, table[2 + i].tolist(), want_info))
        assert table[2 + i].tolist() == want_info, (name, conn, spec)       # n_components, kept_components, raw_area, error = 0
        assert np.array_equal(rows[:, :m.shape[1]], kept.astype(np.uint8) * 255), (name, conn, spec)          # byte for byte
        assert not rows[:, m.shape[1]:].any(), (name, conn, spec)
    assert (table[:, 3] == 0).all()
    evalpost.check_component_info(table)


def test_two_runs_give_identical_labels_masks_and_tables(batch):
    st, _ = batch
    runs = []
    work = None
    for _ in range(2):
        buf = st.masks.clone()
        labels = evalpost.label_components(buf, st, 8, out=torch.zeros(st.out_bytes, dtype=torch.int32, device=DEV))   # (gaps are not written)
        info = torch.zeros(st.n, 4, dtype=torch.int64, device=DEV)
        work = evalpost.filter_work(st, DEV, work)                          # the second run reuses (dirty) scratch
        evalpost.filter_components(buf, labels, st, Components("largest", 3), info, 0, work=work)
        runs.append((labels.clone(), buf, info))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="info"):
        evalpost.filter_components(buf, labels, st, Components("largest"), info, st.n)
    with pytest.raises(hip.HipLibraryError, match="row out of range"):
        evalpost.filter_components(buf, labels, st, Components("largest"), info, 1)
    with pytest.raises(ValueError, match="spec"):
        evalpost.filter_components(buf, labels, st, None, info, 0)
    with pytest.raises(ValueError, match="labels"):
        evalpost.filter_components(buf, labels[:st.out_bytes - 1], st, Components("largest"), info, 0)


# ---- statistics of the kept pixels: the warp cases of tests/test_predict_gpu.py ----
@pytest.fixture(scope="module")
def warp_case():
    """test_predict_gpu's probability maps and descriptors, the predict_batch masks / rows, and the per-pixel q16 values from the
    per-sample warp kernel (warp_to_original), computed once"""
    logits = torch.from_numpy(np.stack([np.random.default_rng(10 + b).standard_normal((24, 24)).astype(np.float32) * 3 for b in range(2)]))
    rect = torch.full((S, S), 0.05)
    rect[20:60, 30:80] = 0.9
    probs = torch.cat([evalpost.sigmoid_upsample(logits[:, None].to(DEV), S, S), rect[None].to(DEV), torch.zeros(1, S, S, device=DEV)]).contiguous()
    st = evalpost.EvalStaging(DEV, mask_bytes=16).pack_sizes(SHAPES, _descs()).upload()
    stats = evalpost.new_predict_stats(len(DESCS), DEV)
    out = torch.zeros(st.out_bytes, dtype=torch.uint8, device=DEV)
    evalpost.predict_batch(probs, st, stats, 0, THR, out_masks=out)
    q16 = []
    for mat, si, mp, _ in _descs():
        v = evalpost.warp_to_original(probs[mp], mat, SHAPES[si]).cpu().numpy()
        q16.append(np.rint(v * np.float32(65536)).astype(np.int64))
    return probs, st, out, stats.cpu().numpy(), q16


@pytest.mark.parametrize("spec", [dict(keep="largest", min_area=0), dict(keep="all", min_area=9), dict(keep="largest", min_area=2000)],
                         ids=lambda s: "%s-%d" % (s["keep"], s["min_area"]))
def test_filtered_statistics(warp_case, spec):
    probs, st, out, raw_rows, q16 = warp_case
    n = len(DESCS)
    buf = out.clone()
    raw = out.cpu().numpy()
    labels = evalpost.label_components(buf, st, 8)
    info = torch.zeros(n, 4, dtype=torch.int64, device=DEV)
    stats = evalpost.new_predict_stats(n + 1, DEV)
    evalpost.filter_components(buf, labels, st, Components(**spec), info, 0, probs=probs, stats=stats)
    got, table, rows = buf.cpu().numpy(), info.cpu().numpy(), stats.cpu().numpy()
    single = multi = 0
    for k in range(n):
        d = st.descs[k]
        fg = _rect(raw, d)[:, :d.w_out] != 0
        kept, want_info, _ = CC.filter_mask(fg, **spec)
        want = CC.stats_row(kept, q16[k])
        print("desc %d  %3d x %3d  %s  info %s  kept row %s  raw row %s" % (k, d.h_out, d.w_out, spec, table[k].tolist(), rows[k].tolist(), raw_rows[k].tolist()))
        assert table[k].tolist() == want_info and want_info[2] == raw_rows[k][0], k
        assert np.array_equal(_rect(got, d)[:, :d.w_out], kept.astype(np.uint8) * 255), k
        assert rows[k].tolist() == want, k                                  # per field, against the oracle on the raw mask
        if want_info[0] == 1 and want_info[1] == 1:
            assert rows[k].tolist() == raw_rows[k].tolist(), k              # one component, kept: predict_batch's row bit for bit
            single += 1
        multi += want_info[0] > 1
    assert rows[n].tolist() == list(evalpost.PREDICT_INIT)
    assert multi >= 2 and (single >= 2 or spec["min_area"] == 2000)           # both kinds are present in these cases
    with pytest.raises(ValueError, match="go together"):
        evalpost.filter_components(buf, labels, st, Components(**spec), info, 0, probs=probs)


def test_mask_iou_batch_reproduces_iou_batch(warp_case):
    probs = warp_case[0]
    n = len(DESCS)
    rng = np.random.default_rng(4)
    gts = []
    for h, w in SHAPES:
        g = np.zeros((h, w), np.uint8)
        g[h // 4:h // 4 + max(h // 2, 1), w // 5:w // 5 + max(w // 2, 1)] = 255
        g[rng.random((h, w)) < 0.05] = 3                                    # (any non-zero byte counts)
        gts.append(g)
    st = evalpost.EvalStaging(DEV).pack(gts, _descs()).upload()
    counts = torch.zeros(n + 2, 2, dtype=torch.int32, device=DEV)
    out = torch.zeros(st.out_bytes, dtype=torch.uint8, device=DEV)
    evalpost.iou_batch(probs, st, st.masks, counts, 1, THR, out_masks=out)
    again = torch.zeros(n + 2, 2, dtype=torch.int32, device=DEV)
    evalpost.mask_iou_batch(out, st, st.masks, again, 1)
    print("iou_batch counts", counts.cpu().numpy().tolist())
    assert torch.equal(again, counts) and int(counts[1:n + 1, 0].sum()) > 0 and counts[0].tolist() == [0, 0] == counts[n + 1].tolist()
    evalpost.mask_iou_batch(out, st, st.masks, again, 1)
    assert torch.equal(again, 2 * counts)                                   # it accumulates
    with pytest.raises(ValueError, match="counts"):
        evalpost.mask_iou_batch(out, st, st.masks, again, n + 2)
    with pytest.raises(hip.HipLibraryError, match="row out of range"):
        evalpost.mask_iou_batch(out, st, st.masks, again, 3)


# ---- end to end, tiny model ----
def _recorded(monkeypatch, fn):
    names = []
    real = hip.call
    monkeypatch.setattr(hip, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    try:
        return fn(), names
    finally:
        monkeypatch.undo()


def _flat(out):
    return [p for x in out for p in x]


def test_predictor_with_components(monkeypatch):
    recs = _predict_records()
    files, exprs = [r["img"] for r in recs], [r["sents"] for r in recs]
    pipe = records.RecordPipeline(SIZE, WORD_LEN, DEV, mode="test", tokenizer=_StandInTokenizer())
    clip, head, sd = _setup("tiny", SIZE, WORD_LEN)
    model = _KeepSegment(InferenceRunner(clip, head, sd, DEV))
    pr = predict.Predictor(model, pipe, thr=E2E_THR)
    plain = _flat(pr.predict(files, exprs, images_per_batch=2, masks="host"))
    assert all(type(p) is predict.Prediction for p in plain)
    # the q16 value of every pixel, from the kept logits through the per-sample warp kernel
    q16, k = [], 0
    for b, lo in enumerate(range(0, len(recs), 2)):
        _, params = pipe(recs[lo:lo + 2])
        probs = evalpost.sigmoid_upsample(model.logits[b], SIZE, SIZE)
        j = 0
        for r, prm in zip(recs[lo:lo + 2], params):
            for _ in r["sents"]:
                v = evalpost.warp_to_original(probs[j], prm["inverse"], prm["ori_size"]).cpu().numpy()
                q16.append(np.rint(v * np.float32(65536)).astype(np.int64))
                j += 1
    for spec in (Components(keep="largest"), Components(keep="all", min_area=30, connectivity=4)):
        got = _flat(pr.predict(files, exprs, images_per_batch=2, masks="host", components=spec))
        none = _flat(pr.predict(files, exprs, images_per_batch=2, masks=None, components=spec))
        dev = _flat(predict.Predictor(model, pipe, thr=E2E_THR, components=spec).predict(files, exprs, images_per_batch=2, masks="device"))
        assert len(got) == len(plain) == 9
        for k, (p, raw) in enumerate(zip(got, plain)):
            assert type(p) is predict.ComponentPrediction and p.sentence == raw.sentence
            kept, info, _ = CC.filter_mask(raw.mask, spec.keep, spec.min_area, spec.connectivity)
            area, score_q16, x0, y0, x1, y1 = CC.stats_row(kept, q16[k])
            print("expr %d  %s  components %d  raw area %d  kept area %d  box %s" % (k, spec, p.n_components, p.raw_area, p.area, p.box))
            assert isinstance(p.mask, np.ndarray) and p.mask.dtype == np.uint8 and np.array_equal(p.mask, kept.astype(np.uint8) * 255)
            assert (p.n_components, p.raw_area) == (info[0], info[2]) and p.raw_area == raw.area
            assert p.area == area and p.box == ((x0, y0, x1, y1) if area else None)
            assert p.score == (score_q16 / (65536.0 * area) if area else 0.0) and isinstance(p.score, float)
            assert none[k].mask is None and none[k][2:] == p[2:] and none[k].sentence == p.sentence       # masks=None: the same statistics
            assert torch.is_tensor(dev[k].mask) and dev[k].mask.is_cuda and np.array_equal(dev[k].mask.cpu().numpy(), p.mask) and dev[k][2:] == p[2:]
    # components=None / a no-op spec / the keyword left out: the same library calls and the same results
    base, base_calls = _recorded(monkeypatch, lambda: pr.predict(files, exprs, images_per_batch=2, masks="host"))
    for value in (None, Components(), "default"):
        out, calls = _recorded(monkeypatch, lambda: pr.predict(files, exprs, images_per_batch=2, masks="host", components=value))
        assert calls == base_calls and "cris_predict_masks_batch" in calls and not any("components" in c for c in calls)
        for a, b in zip(_flat(out), _flat(base)):
            assert type(a) is predict.Prediction and a[2:] == b[2:] and np.array_equal(a.mask, b.mask)
    _, calls = _recorded(monkeypatch, lambda: pr.predict(files, exprs, images_per_batch=2, masks=None, components=Components("largest")))
    assert calls.count("cris_label_components") == calls.count("cris_filter_components") == calls.count("cris_predict_masks_batch") == 3


def test_evaluator_with_components(monkeypatch):
    from test_evaluate_gpu import _Keep, _records, _runner
    recs = _records()
    spec = Components(keep="largest", min_area=5)
    # validate: metrics from the oracle-filtered masks of the very logits the model produced
    pipe = records.RecordPipeline(SIZE, WORD_LEN, DEV, mode="val", tokenizer=_StandInTokenizer())
    model = _Keep(_runner())
    ev = evaluate.Evaluator(model, pipe, thr=E2E_THR)
    iou, prec = ev.validate(recs, batch_size=4, components=spec)
    want, infos = [], []
    for b, lo in enumerate(range(0, len(recs), 4)):
        part = recs[lo:lo + 4]
        _, _, params = pipe(part)
        probs = evalpost.sigmoid_upsample(model.logits[b], SIZE, SIZE)
        for j, (r, prm) in enumerate(zip(part, params)):
            v = evalpost.warp_to_original(probs[j], prm["inverse"], prm["ori_size"]).cpu().numpy()
            kept, info, _ = CC.filter_mask(v > np.float32(E2E_THR), spec.keep, spec.min_area, spec.connectivity)
            gt = pngdec.decode_gray(r["mask"]).numpy() != 0
            want.append([int((kept & gt).sum()), int((kept | gt).sum())])
            infos.append(info)
    print("validate with components: counts", ev.counts.tolist(), "info", ev.component_info.tolist())
    assert ev.counts.tolist() == want and ev.component_info.tolist() == infos
    m = evaluate.metrics(np.array(want))
    assert iou == m[0] and prec == m[1] and ev.per_sample.tolist() == m[2].tolist()
    # components=None and the keyword left out: the same library calls, the same results
    (iou0, prec0), base_calls = _recorded(monkeypatch, lambda: ev.validate(recs, batch_size=4))
    counts0 = ev.counts.copy()
    for value in (None, Components()):
        (iou1, prec1), calls = _recorded(monkeypatch, lambda: ev.validate(recs, batch_size=4, components=value))
        assert calls == base_calls and calls.count("cris_eval_iou_batch") == 3 and not any("components" in c for c in calls)
        assert (iou1, prec1) == (iou0, prec0) and np.array_equal(ev.counts, counts0)
    # inference: the callback sees the FILTERED masks, and the table counts them
    tpipe = records.RecordPipeline(SIZE, WORD_LEN, DEV, mode="test", tokenizer=_StandInTokenizer())
    tev = evaluate.Evaluator(model, tpipe, thr=E2E_THR)
    raw, seen = [], []
    tev.inference(recs[:4], images_per_batch=2, visualize=lambda rec, sent, i, m: raw.append(m))
    tev.inference(recs[:4], images_per_batch=2, visualize=lambda rec, sent, i, m: seen.append((rec, i, m)), components=spec)
    with_cb = tev.counts.copy()
    tev.inference(recs[:4], images_per_batch=2, components=spec)
    assert np.array_equal(tev.counts, with_cb) and len(seen) == len(raw) == with_cb.shape[0]
    for k, ((rec, i, m), r) in enumerate(zip(seen, raw)):
        kept, info, _ = CC.filter_mask(r, spec.keep, spec.min_area, spec.connectivity)
        gt = pngdec.decode_gray(rec["mask"]).numpy() != 0
        assert np.array_equal(m, kept.astype(np.uint8) * 255) and tev.component_info[k].tolist() == info
        assert with_cb[k].tolist() == [int((kept & gt).sum()), int((kept | gt).sum())] and i == float(with_cb[k, 0] / (with_cb[k, 1] + 1e-6))
