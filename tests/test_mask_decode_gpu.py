"""Encoded masks decoded on the GPU (csrc/decode.hip behind evalpost.decode_masks_batch) against rle.decode /
polygon.decode on every case of tests/decode_cases.py - every slot byte for byte with its zero padding, every other byte untouched,
the payload only read, the same bytes from a dirty scratch - and the round trips through the device encoders.  Then the evaluator on
records whose ground truth is RLE, polygons or a mix against the same pass on PNG records (equal integer tables, with every option),
and evaluate.score_results on what predict(..., masks="rle" / "polygon") returned against Evaluator.inference on the same records."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

pytest.importorskip("PIL")

import decode_cases as DC  # noqa: E402
import test_evaluate_gpu as TE  # noqa: E402
import test_predict_gpu as TP  # noqa: E402
from cris.pytorch_amd import evalpost, evaluate, hip, pngdec, polygon, predict, records, rle  # noqa: E402
from cris.pytorch_amd.evalpost import Components, Smooth  # noqa: E402
from test_records_gpu import _StandInTokenizer  # noqa: E402

DEV = torch.device("cuda:0")
IDENT = np.array([[1.0, 0, 0], [0, 1.0, 0]], np.float64)
GAP = 48                # bytes of 255 before every slot (a multiple of 16: the slots keep the staging's alignment)
NEW_CALLS = ("cris_rle_decode", "cris_polygon_fill")


@pytest.fixture(scope="module")
def batch():
    """one ragged batch of every case, RLE and polygon sources alternating while both last: (staging with one descriptor per mask
    and one more that names mask ALIAS's slot, sources, expected masks, names)"""
    r, p = list(zip(DC.rle_sources(), DC.expected_rle())), list(zip(DC.polygon_sources(), DC.expected_polygon()))
    mixed = [x for pair in zip(r, p) for x in pair] + r[len(p):] + p[len(r):]
    names, items, want = [k for (k, _), _ in mixed], [s for (_, s), _ in mixed], [w for _, w in mixed]
    alias = names.index("polygon random 0.02")
    shapes = [w.shape for w in want]
    descs = [(IDENT, i, 0, i) for i in range(len(items))] + [(IDENT, alias, 0, len(items))]
    st = evalpost.EvalStaging(DEV, mask_bytes=16).pack_sizes(shapes, descs)
    off = 0
    for i, (h, w) in enumerate(shapes):                                     # our own slots: a gap of 255 before each
        off += GAP
        st.descs[i].out_off = off
        off += (DC.pitch_of(w) * h + 15) // 16 * 16
    st.descs[len(items)].out_off = st.descs[alias].out_off
    st.out_bytes = off + GAP
    st.upload()
    forms = [evalpost.mask_form(x) for x in items]
    srcs = evalpost.MaskSources(forms, evalpost.desc_slots(st, "out")[:len(items)]).upload(DEV)
    return st, srcs, want, names, alias


def _fresh(st):
    """255 everywhere, 0x7F in every slot"""
    host = np.full(st.out_bytes, 255, np.uint8)
    for i in range(st.n):
        d = st.descs[i]
        host[d.out_off:d.out_off + d.pitch * d.h_out] = 0x7F
    return host


def test_every_slot_equals_the_oracle_and_nothing_else_is_written(batch):
    st, srcs, want, names, alias = batch
    n = len(want)
    assert srcs.n == n == st.n - 1 and srcs.n_rle == len(DC.rle_sources()) and srcs.n_polygon == len(DC.polygon_sources())
    assert srcs.out_bytes <= st.out_bytes - GAP
    before = _fresh(st)
    out = torch.from_numpy(before).to(DEV)
    work = evalpost.decode_work(srcs, DEV)
    assert evalpost.decode_masks_batch(srcs, out, work=work) is out
    got = out.cpu().numpy()
    expect = before.copy()
    for i, (name, m) in enumerate(zip(names, want)):
        d = st.descs[i]
        h, w = m.shape
        assert (d.h_out, d.w_out, d.pitch) == (h, w, DC.pitch_of(w))
        rows = expect[d.out_off:d.out_off + d.pitch * h].reshape(h, d.pitch)
        rows[:, :w] = m
        rows[:, w:] = 0                                                     # the padding EvalStaging.pack would have uploaded
        slot = got[d.out_off:d.out_off + d.pitch * h].reshape(h, d.pitch)
        assert np.array_equal(slot[:, :w], m), name
        assert not slot[:, w:].any(), name
    assert np.array_equal(got, expect)                                      # gaps, alignment bytes and tail keep their 255
    assert (got[:GAP] == 255).all() and (got[-GAP:] == 255).all()
    assert np.array_equal(srcs._keep[1].cpu().numpy(), srcs.blob)           # the payload is only read
    # a second time from a scratch full of ones and an output full of other bytes: the same bytes
    work.fill_(-1)
    again = torch.from_numpy(before ^ 0x33).to(DEV)
    evalpost.decode_masks_batch(srcs, again, work=work)
    again = again.cpu().numpy()
    covered = np.zeros(st.out_bytes, bool)
    for i in range(n):
        d = st.descs[i]
        covered[d.out_off:d.out_off + d.pitch * d.h_out] = True
    assert np.array_equal(again[covered], expect[covered]) and np.array_equal(again[~covered], (before ^ 0x33)[~covered])
    # each kind alone leaves the other kind's slots alone
    for kind, attr in (("rle", "n_polygon"), ("polygon", "n_rle")):
        idx = [i for i, k in enumerate(names) if (k in dict(DC.rle_sources())) == (kind == "rle")]
        part = evalpost.MaskSources([evalpost.mask_form(dict(DC.rle_sources() + DC.polygon_sources())[names[i]]) for i in idx],
                                    [evalpost.desc_slots(st, "out")[i] for i in idx]).upload(DEV)
        assert getattr(part, attr) == 0
        only = torch.from_numpy(before).to(DEV)
        evalpost.decode_masks_batch(part, only)
        only = only.cpu().numpy()
        mine = np.zeros(st.out_bytes, bool)
        for i in idx:
            d = st.descs[i]
            mine[d.out_off:d.out_off + d.pitch * d.h_out] = True
        assert np.array_equal(only[mine], expect[mine]) and np.array_equal(only[~mine], before[~mine]), kind


def test_round_trips_through_the_device_encoders(batch):
    st, srcs, want, names, alias = batch
    out = torch.from_numpy(_fresh(st)).to(DEV)
    evalpost.decode_masks_batch(srcs, out)
    first = out.cpu().numpy()
    # RLE: the masks the device wrote, encoded there (the aliasing descriptor included), decoded again
    runs, totals = evalpost.rle_encode_batch(out, st)
    rles = evalpost.rle_collect(runs, totals, st, masks_u8=out)
    assert len(rles) == st.n
    for name, r, m in zip(names + ["alias"], rles, want + [want[alias]]):
        assert r == rle.encode(m), name                                     # the aliased mask was decoded once and reads the same
    back = torch.from_numpy(_fresh(st) ^ 0x11).to(DEV)
    evalpost.rle_decode_batch(rles, st, back)
    back = back.cpu().numpy()
    for i in range(st.n):
        d = st.descs[i]
        assert np.array_equal(back[d.out_off:d.out_off + d.pitch * d.h_out], first[d.out_off:d.out_off + d.pitch * d.h_out]), i
    # polygons: traced there, filled again
    work = evalpost.polygon_work(st, DEV)
    polys = evalpost.polygon_collect(out, st, evalpost.polygon_count_batch(out, st, work=work), work=work)
    assert len(polys) == st.n and all(np.array_equal(polygon.decode(p), m) for p, m in zip(polys, want + [want[alias]]))
    back = torch.from_numpy(_fresh(st) ^ 0x11).to(DEV)
    evalpost.polygon_fill_batch(polys, st, back)
    back = back.cpu().numpy()
    for i in range(st.n):
        d = st.descs[i]
        assert np.array_equal(back[d.out_off:d.out_off + d.pitch * d.h_out], first[d.out_off:d.out_off + d.pitch * d.h_out]), i
    with pytest.raises(ValueError, match="mask 0 must be a rle of"):
        evalpost.rle_decode_batch(polys, st, back)
    with pytest.raises(ValueError, match="masks for"):
        evalpost.polygon_fill_batch(polys[:-1], st, back)


def test_staging_decodes_into_the_bytes_pack_uploads():
    """EvalStaging.pack_encoded + upload + decode against pack + upload of the host-decoded masks: `masks` byte for byte in every
    slot, through the ground-truth layout, with two descriptors naming one mask; and the bytes each upload copies"""
    pick = ["rle 33x65", "polygon ellipse with a hole 97x131", "simplified 1 45x67", "rle 1x1 full", "polygon width 5", "both triangles",
            "700 counts with zeros"]
    table = dict(DC.rle_sources() + DC.polygon_sources())
    items = [table[k] for k in pick]
    host = [evalpost.mask_to_array(evalpost.mask_form(x)) for x in items]
    plain = (np.random.default_rng(4).random((50, 37)) < 0.5).astype(np.uint8) * 255
    descs = [(IDENT, i, 0, i) for i in range(len(items))] + [(IDENT, 1, 0, len(items)), (IDENT, len(items), 0, len(items) + 1)]
    ref = evalpost.EvalStaging(DEV).pack([plain] + host, [(m, (mi + 1) % (len(items) + 1), mp, row) for m, mi, mp, row in descs]).upload()
    st = evalpost.EvalStaging(DEV, max_descs=2, mask_bytes=16)
    st.pack_encoded([evalpost.mask_form(x) for x in items] + [evalpost.mask_form(plain)], descs).upload()
    assert st.encoded is not None and st.last_upload_bytes == st.mask_base + (37 // 4 * 4 + 4) * 50 + 0 and st.mask_bytes == ref.mask_bytes
    st.masks[(40 * 50 + 15) // 16 * 16:].fill_(0x7F)                        # the device-only slots start dirty
    st.decode()
    got, want = st.masks.cpu().numpy(), ref.masks.cpu().numpy()
    for i in range(st.n):
        a, b = st.descs[i], ref.descs[i]
        assert (a.mask_off, a.out_off, a.pitch, a.h_out, a.w_out) == (b.mask_off, b.out_off, b.pitch, b.h_out, b.w_out)
        assert np.array_equal(got[a.mask_off:a.mask_off + a.pitch * a.h_out], want[a.mask_off:a.mask_off + a.pitch * a.h_out]), i
    assert st.descs[1].mask_off == st.descs[len(items)].mask_off
    # downstream kernels read the decoded slots like uploaded ones
    pred = torch.from_numpy(np.random.default_rng(5).integers(0, 2, st.out_bytes).astype(np.uint8) * 255).to(DEV)
    c1, c2 = (torch.zeros(st.n, 2, dtype=torch.int32, device=DEV) for _ in range(2))
    evalpost.mask_iou_batch(pred, st, st.masks, c1, 0)
    evalpost.mask_iou_batch(pred, ref, ref.masks, c2, 0)
    assert torch.equal(c1, c2) and int(c1[:, 0].sum()) > 0
    # without a host-decoded mask only the tables and the payload go up; a following `pack` is what it always was
    st.pack_encoded([evalpost.mask_form(x) for x in items], descs[:-1]).upload()
    assert st.last_upload_bytes < st.mask_base and st.last_upload_bytes == (st.n * 88 + 15) // 16 * 16 + st.encoded.blob.size
    st.decode()
    got = st.masks.cpu().numpy()
    for i in range(st.n):
        a = st.descs[i]
        h, w = host[i if i < len(items) else 1].shape
        rows = got[a.mask_off:a.mask_off + a.pitch * h].reshape(h, a.pitch)
        assert np.array_equal(rows[:, :w], host[i if i < len(items) else 1]) and not rows[:, w:].any(), i
    st.pack([plain], [(IDENT, 0, 0, 0)]).upload()
    assert st.encoded is None and st.last_upload_bytes == st.mask_base + st.mask_bytes and st.decode() is None


# ---- the evaluator on encoded ground truth ----

def _recorded(monkeypatch, fn):
    names = []
    real = hip.call
    monkeypatch.setattr(hip, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    try:
        return fn(), names
    finally:
        monkeypatch.undo()


@pytest.fixture(scope="module")
def split():
    """the records of tests/test_evaluate_gpu.py four times: PNG ground truth, RLE, polygons, and the three forms mixed"""
    recs = TE._records()
    masks = [pngdec.decode_gray(r["mask"]).numpy() for r in recs]
    as_rle = [dict(r, mask=rle.encode(m)) for r, m in zip(recs, masks)]
    as_poly = [dict(r, mask=polygon.encode(m)) for r, m in zip(recs, masks)]
    mixed = [(recs, as_rle, as_poly)[i % 3][i] for i in range(len(recs))]
    mixed[4] = dict(recs[4], mask=rle.to_json(rle.encode(masks[4])))        # str counts, as a JSON file holds them
    runner = TE._runner()
    _evaluator(runner, "val").validate(recs, batch_size=4)                  # the runner's one-time work (weight packing, graph capture)
    _evaluator(runner, "test").inference(recs, images_per_batch=4)          # happens here, not inside a recorded pass
    return {"png": recs, "rle": as_rle, "polygon": as_poly, "mixed": mixed}, runner


def _evaluator(runner, mode):
    pipe = records.RecordPipeline(TE.SIZE, TE.WORD_LEN, DEV, mode=mode, tokenizer=_StandInTokenizer())
    return evaluate.Evaluator(TE._KeepSegment(runner), pipe, thr=TE.THR)


def _without(names, drop):
    return [c for c in names if not c.startswith(drop)]


@pytest.mark.parametrize("form", ["rle", "polygon", "mixed"])
def test_evaluator_counts_equal_the_png_pass(split, form, monkeypatch):
    sets, runner = split
    val, inf = _evaluator(runner, "val"), _evaluator(runner, "test")
    thr = [0.2, 0.35, 0.6]
    passes = {"validate": lambda recs: (val.validate(recs, batch_size=4), val.counts.copy()),
              "inference": lambda recs: (inf.inference(recs, images_per_batch=4), inf.counts.copy()),
              "sweep": lambda recs: (val.sweep(recs, thresholds=thr, batch_size=4).iou.tolist(), val.sweep_counts.copy()),
              "sweep inference": lambda recs: (inf.sweep(recs, thresholds=thr, split="inference", images_per_batch=4).iou.tolist(), inf.sweep_counts.copy())}
    for name, run in passes.items():
        (want, table), png_calls = _recorded(monkeypatch, lambda: run(sets["png"]))
        (got, counts), calls = _recorded(monkeypatch, lambda: run(sets[form]))
        assert np.array_equal(counts, table) and counts.dtype == table.dtype and got == want, name
        assert table[..., 1].min() > 0 and 0 < table[..., 0].sum()
        assert not any(c in NEW_CALLS for c in png_calls), name            # PNG records: no new entry point
        assert _without(calls, ("cris_rle_decode", "cris_polygon_fill", "cris_png")) == _without(png_calls, ("cris_png",)), name
        kinds = [{"polygon" if "rings" in r["mask"] else "rle" for r in sets[form][lo:lo + 4] if isinstance(r["mask"], dict)} for lo in (0, 4, 8)]
        assert sum(c == "cris_rle_decode" for c in calls) == sum("rle" in k for k in kinds), name       # one call per batch that holds the kind
        assert sum(c == "cris_polygon_fill" for c in calls) == sum("polygon" in k for k in kinds), name
        first = [i for i, c in enumerate(calls) if c in NEW_CALLS][0]
        reader = [i for i, c in enumerate(calls) if c in ("cris_eval_iou_batch", "cris_eval_iou_sweep_batch")][0]
        assert first < reader, name                                         # decoded before the first kernel that reads the masks


def test_evaluator_options_on_mixed_ground_truth(split):
    sets, runner = split
    opts = dict(components=Components(keep="largest"), smooth=Smooth(open=1, close=1), boundary=True)
    for mode, call in (("val", lambda ev, recs: ev.validate(recs, batch_size=4, **opts)), ("test", lambda ev, recs: ev.inference(recs, images_per_batch=4, **opts))):
        ev = _evaluator(runner, mode)
        want = call(ev, sets["png"])
        table, btable, info = ev.counts.copy(), ev.boundary_counts.copy(), ev.component_info.copy()
        for form in ("mixed", "polygon"):
            assert call(ev, sets[form]) == want
            assert np.array_equal(ev.counts, table) and np.array_equal(ev.boundary_counts, btable) and np.array_equal(ev.component_info, info), (mode, form)
        assert btable[:, 1].min() > 0
    bad = [dict(r) for r in sets["rle"]]
    bad[5] = dict(bad[5], mask=rle.encode(np.zeros((3, 3), np.uint8)))
    with pytest.raises(ValueError, match="mask is \\(3, 3\\), image"):
        _evaluator(runner, "val").validate(bad, batch_size=4)


def test_train_pipeline_takes_encoded_ground_truth(split):
    sets, _ = split
    pipe = records.RecordPipeline(TE.SIZE, TE.WORD_LEN, DEV, mode="train", tokenizer=_StandInTokenizer())
    want = pipe(sets["png"][:4], np.random.default_rng(1))
    got = pipe(sets["mixed"][:4], np.random.default_rng(1))
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and float(want[2].sum()) > 0


# ---- the model-free scorer ----

@pytest.fixture(scope="module")
def predicted():
    recs = TP._records()
    pipe = records.RecordPipeline(TP.SIZE, TP.WORD_LEN, DEV, mode="test", tokenizer=_StandInTokenizer())
    clip, head, sd = TP._setup("tiny", TP.SIZE, TP.WORD_LEN)
    model = TP._KeepSegment(TP.InferenceRunner(clip, head, sd, DEV))
    ev = evaluate.Evaluator(model, pipe, thr=TP.E2E_THR)
    ev.inference(recs, images_per_batch=2, boundary=True)
    pr = predict.Predictor(model, pipe, thr=TP.E2E_THR)
    gt = [r["mask"] for r in recs for _ in r["sents"]]                      # PNG bytes, one per expression
    return pr, [r["img"] for r in recs], [r["sents"] for r in recs], gt, ev.counts.copy(), ev.boundary_counts.copy()


def test_score_results_on_a_results_file_equals_inference(predicted):
    pr, files, exprs, gt, counts, bcounts = predicted
    out = pr.predict(files, exprs, images_per_batch=2, masks="rle")
    entries = json.loads(json.dumps(predict.coco_results(out, list(range(len(files))))))
    segs = [e["segmentation"] for e in entries]
    assert len(segs) == 9 == len(gt) and all(isinstance(s["counts"], str) for s in segs)
    res = evaluate.score_results(segs, gt, DEV, boundary=True, batch=4)     # 4 + 4 + 1: three batches
    assert np.array_equal(res.counts, counts) and res.counts.dtype == counts.dtype  # the two launches warp bit for bit alike
    assert np.array_equal(res.boundary_counts, bcounts)
    assert (res.iou, res.prec) == evaluate.metrics(counts)[:2] and res.overall_iou == evaluate.overall_iou(counts)
    assert res.per_sample.tolist() == evaluate.metrics(counts)[2].tolist() and 0 < counts[:, 0].sum() < counts[:, 1].sum()
    assert res.boundary_iou == evaluate.metrics(bcounts)[0] and res.boundary_prec == evaluate.metrics(bcounts)[1]
    plain = evaluate.score_results(segs, gt, DEV)
    assert np.array_equal(plain.counts, counts) and plain.boundary_counts is None and plain.boundary_iou is None
    # ground truth as RLE, arrays on either side, Prediction objects: the same table
    gt_arrays = [pngdec.decode_gray(g).numpy() for g in gt]
    flat = [p for x in out for p in x]
    mixed_pred = [rle.decode(s) if i % 2 else p for i, (s, p) in enumerate(zip(segs, flat))]
    mixed_gt = [rle.encode(g) if i % 3 == 0 else polygon.encode(g) if i % 3 == 1 else g for i, g in enumerate(gt_arrays)]
    assert np.array_equal(evaluate.score_results(mixed_pred, mixed_gt, DEV, batch=5).counts, counts)
    # what is refused, with its index, before the batch's device work
    with pytest.raises(ValueError, match="pair 5: the prediction is"):
        evaluate.score_results(segs, gt_arrays[:5] + [gt_arrays[5][:-1]] + gt_arrays[6:], DEV, batch=4)
    with pytest.raises(ValueError, match="prediction 6: .*sum to"):
        evaluate.score_results(segs[:6] + [dict(segs[6], counts=[1, 2])] + segs[7:], gt, DEV, batch=4)
    with pytest.raises(ValueError, match="ground truth 2: .*flat polygon lists are not accepted"):
        evaluate.score_results(segs, gt[:2] + [[[0, 0, 5, 0, 5, 5]]] + gt[3:], DEV)


def test_score_results_on_polygons(predicted):
    pr, files, exprs, gt, counts, _ = predicted
    exact = [p for x in pr.predict(files, exprs, images_per_batch=2, masks="polygon") for p in x]
    assert all(isinstance(p.mask, dict) and "epsilon" not in p.mask for p in exact)
    assert np.array_equal(evaluate.score_results(exact, gt, DEV, batch=4).counts, counts)
    simple = [p for x in pr.predict(files, exprs, images_per_batch=2, masks="polygon", simplify=1.0) for p in x]
    assert all(p.mask.get("epsilon") == 1.0 for p in simple) and sum(len(r) for p in simple for r in p.mask["rings"]) < sum(len(r) for p in exact for r in p.mask["rings"])
    got = evaluate.score_results(simple, [p.mask for p in exact], DEV).counts
    want = []
    for s, e in zip(simple, exact):
        a, b = polygon.decode(s.mask) != 0, polygon.decode(e.mask) != 0
        want.append([int((a & b).sum()), int((a | b).sum())])
    assert got.tolist() == want and any(i < u for i, u in want)             # what simplify=1.0 costs, in pixels
