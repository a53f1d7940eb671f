"""Mask smoothing on the GPU (csrc/morph.hip cris_morph_masks and csrc/evalpost.hip cris_fill_holes behind evalpost.morph_batch /
dilate_batch / open_batch / close_batch / fill_holes_batch) against the numpy oracle of tests/morph_cases.py: every
byte and every table entry, as equalities; what the launches must leave alone; the algebra of opening and closing on the device.
Then predict.Predictor and evaluate.Evaluator with smooth=Smooth(...) on the tiny synthetic model against the oracle applied to the
masks the same objects return without the spec, and the library calls they issue with and without it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

pytest.importorskip("PIL")

import boundary_cases as BC  # noqa: E402
import components_cases as CC  # noqa: E402
import morph_cases as MC  # noqa: E402
from cris.pytorch_amd import evalpost, evaluate, hip, pngdec, predict, records, rle  # noqa: E402
from cris.pytorch_amd.evalpost import Boundary, Components, Smooth  # noqa: E402
from test_boundary_gpu import _pack, _recorded, _rect  # noqa: E402
from test_evaluate_gpu import SIZE, WORD_LEN, _Keep, _KeepSegment, _records, _runner  # noqa: E402
from test_predict_gpu import E2E_THR  # noqa: E402
from test_records_gpu import _StandInTokenizer  # noqa: E402

DEV = torch.device("cuda:0")
NEW = ("cris_morph_masks", "cris_fill_holes", "cris_fill_holes_work_bytes")
SENTINEL = 0x5A


@pytest.fixture(scope="module")
def batch():
    names = [k for k, _, _ in MC.cases()]
    a = names.index(MC.ALIAS)
    masks = [m for _, m, _ in MC.cases()]
    st, buf, inside = _pack(masks, alias=a)
    radii = [d for _, _, d in MC.cases()] + [MC.cases()[a][2]]
    return st, buf, inside, radii, names + [MC.ALIAS + " (the same rectangle)"], masks + [masks[a]], list(MC.expected()) + [MC.expected()[a]]


def _check_bytes(res, st, names, want, what):
    for i, (name, ref) in enumerate(zip(names, want)):
        assert np.array_equal(_rect(res, st.descs[i]), ref.astype(np.uint8) * 255), (what, name)     # byte for byte


@pytest.mark.parametrize("which", [0, 1, 2], ids=["dilate", "open", "close"])
def test_dilate_open_close_equal_the_oracle(batch, which):
    st, buf, inside, radii, names, masks, exp = batch
    fn = (evalpost.dilate_batch, evalpost.open_batch, evalpost.close_batch)[which]
    assert st.n == len(MC.cases()) + 1 and any(st.descs[i].pitch != st.descs[i].w_out for i in range(st.n))
    want = [e[which] for e in exp]
    before = buf.clone()
    out = torch.full((st.out_bytes + 64,), SENTINEL, dtype=torch.uint8, device=DEV)
    assert fn(buf, st, radii, out=out).data_ptr() == out.data_ptr()
    res = out.cpu().numpy()
    _check_bytes(res, st, names, want, fn.__name__)
    assert (res[~inside] == SENTINEL).all()                                 # padding, gaps and tail keep their fill
    assert torch.equal(buf, before)                                         # the source is only read
    # a fresh zeroed result, dirty scratch: the same bytes
    work = evalpost.morph_work(st, DEV)
    work.fill_(-1)
    again = fn(buf, st, radii, work=work)
    assert again.numel() == st.out_bytes and again.dtype == torch.uint8
    ins = torch.from_numpy(inside[:st.out_bytes]).to(DEV)
    assert torch.equal(again[ins], out[:st.out_bytes][ins]) and int(again[~ins].max()) == 0
    # in place; the padding the source holds (255) stays
    same = buf.clone()
    assert fn(same, st, radii, out=same, work=work) is same
    place = same.cpu().numpy()
    assert np.array_equal(place[inside], res[inside]) and (place[~inside] == 255).all()


def test_mixed_chain_with_per_descriptor_radii(batch):
    st, buf, inside, radii, names, masks, _ = batch
    per = [MC.mixed_ops(i, radii[i]) for i in range(st.n)]
    per[-1] = per[names.index(MC.ALIAS)]                                    # the aliased rectangle: the same chain
    ops = [(per[0][k][0], [per[i][k][1] for i in range(st.n)]) for k in range(4)]
    ops[1] = (ops[1][0], np.asarray(ops[1][1], np.int64))                  # a numpy array of radii is a sequence too
    want = [MC.chain(m, per[i]) for i, m in enumerate(masks)]
    out = torch.full((st.out_bytes + 64,), SENTINEL, dtype=torch.uint8, device=DEV)
    evalpost.morph_batch(buf, st, ops, out=out)
    res = out.cpu().numpy()
    _check_bytes(res, st, names, want, "chain")
    assert (res[~inside] == SENTINEL).all()
    out2 = torch.full((st.out_bytes + 64,), SENTINEL, dtype=torch.uint8, device=DEV)
    evalpost.morph_batch(buf, st, ops, out=out2)
    assert torch.equal(out, out2)                                           # twice: identical bytes
    # a chain of eight, the most the launcher takes, equals two chains of four
    half = evalpost.morph_batch(out, st, ops)
    full = evalpost.morph_batch(buf, st, ops + ops)
    ins = torch.from_numpy(inside[:st.out_bytes]).to(DEV)
    assert torch.equal(full[ins], half[ins])
    _check_bytes(full.cpu().numpy(), st, names, [MC.chain(m, per[i] + per[i]) for i, m in enumerate(masks)], "chain of eight")


def test_algebra_on_the_device(batch):
    """open within M within close; both idempotent"""
    st, buf, inside, radii, names, masks, _ = batch
    ins = torch.from_numpy(inside[:st.out_bytes]).to(DEV)
    m = (buf[:st.out_bytes] != 0) & ins
    op = evalpost.open_batch(buf, st, radii)
    cl = evalpost.close_batch(buf, st, radii)
    assert not bool(((op != 0) & ~m).any()) and not bool((m & ~(cl != 0) & ins).any())
    assert bool(((op != 0) != m).any()) and bool((((cl != 0) & ins) != m).any())
    assert torch.equal(evalpost.open_batch(op, st, radii), op)
    assert torch.equal(evalpost.close_batch(cl, st, radii), cl)


def test_erode_batch_is_unchanged_and_the_chain_gives_its_bytes():
    names = [k for k, _, _ in BC.cases()]
    st, buf, inside = _pack([m for _, m, _ in BC.cases()])
    radii = [d for _, _, d in BC.cases()]
    got = evalpost.erode_batch(buf, st, radii).cpu().numpy()
    _check_bytes(got, st, names, BC.expected(), "erode_batch")
    chain = evalpost.morph_batch(buf, st, [("erode", radii)]).cpu().numpy()
    assert np.array_equal(chain, got)


@pytest.fixture(scope="module")
def hole_batch():
    masks = [m for _, m, _, _ in MC.hole_cases()]
    return [(k, c, a) for k, _, c, a in MC.hole_cases()], masks, MC.expected_holes()


def test_fill_holes_batch_equals_the_oracle(hole_batch):
    keys, masks, exp = hole_batch
    groups = {}
    for i, (_, c, a) in enumerate(keys):
        groups.setdefault((c, a), []).append(i)
    assert len(groups) >= 5
    for (c, a), idx in groups.items():                                      # one launch per (connectivity, cap): a ragged batch each
        st, buf, inside = _pack([masks[i] for i in idx])
        n = st.n
        table = torch.zeros(n + 3, 4, dtype=torch.int64, device=DEV)
        work = evalpost.fill_work(st, DEV)
        work.fill_(-1)                                                      # dirty scratch: the launcher zeroes it
        labels = torch.full((st.out_bytes,), 7, dtype=torch.int32, device=DEV)
        evalpost.fill_holes_batch(buf, st, table, 2, connectivity=c, max_area=a, labels=labels, work=work)
        res = buf.cpu().numpy()
        got = table.cpu().numpy()
        for j, i in enumerate(idx):
            filled, nf, npix, holes = exp[i]
            want = np.where(filled & (masks[i] == 0), 255, masks[i])       # only filled pixels change: bytes of 1 stay 1
            assert np.array_equal(_rect(res, st.descs[j]), want), keys[i]
            assert got[2 + j].tolist() == [nf, npix, holes, 0], (keys[i], got[2 + j].tolist())
        assert (res[~inside] == 255).all()                                  # padding, gaps and tail keep their bytes
        assert not got[:2].any() and not got[2 + n:].any()
        # again on the filled masks: holes above the cap are still there, nothing else is
        table2 = torch.zeros_like(table)
        evalpost.fill_holes_batch(buf, st, table2, 2, connectivity=c, max_area=a)
        assert np.array_equal(buf.cpu().numpy(), res)
        t2 = table2.cpu().numpy()
        assert t2[2:2 + n, :2].sum() == 0 and t2[2:2 + n, 2].tolist() == [exp[i][3] - exp[i][1] for i in idx]
        # twice from the same input: identical bytes and tables
        st3, buf3, _ = _pack([masks[i] for i in idx])
        table3 = torch.zeros_like(table)
        evalpost.fill_holes_batch(buf3, st3, table3, 2, connectivity=c, max_area=a)
        assert torch.equal(buf3, buf) and torch.equal(table3, table)


def test_smooth_batch_is_open_close_fill():
    masks = [m for _, m, _, _ in MC.hole_cases()] + [m for k, m, _ in MC.cases() if k.startswith("blob") or k.startswith("width")]
    spec = Smooth(open=1, close=2, fill_holes=True, max_hole_area=1000, hole_connectivity=4)
    st, buf, inside = _pack(masks)
    info = torch.zeros(st.n, 4, dtype=torch.int64, device=DEV)
    evalpost.smooth_batch(buf, st, spec, info, 0)
    res = buf.cpu().numpy()
    got = info.cpu().numpy()
    for i, m in enumerate(masks):
        mid = MC.closing(MC.opening(m, 1), 2)
        filled, nf, npix, holes = MC.fill_holes(mid, 4, 1000)
        assert np.array_equal(_rect(res, st.descs[i]), filled.astype(np.uint8) * 255), i
        assert got[i].tolist() == [nf, npix, holes, 0]
        assert np.array_equal(filled, MC.smooth(m, 1, 2, True, 1000, 4))
    assert (res[~inside] == 255).all() and 0 < (got[:, 0] > 0).sum() < (got[:, 2] > 0).sum()     # some holes filled, some above the cap


def test_argument_errors(batch):
    st, buf, _, radii, _, _, _ = batch
    with pytest.raises(ValueError, match="masks_u8"):
        evalpost.morph_batch(buf.to(torch.int8), st, [("dilate", 1)])
    with pytest.raises(ValueError, match="out must be"):
        evalpost.dilate_batch(buf, st, 1, out=buf[:st.out_bytes - 1])
    for bad in ([], "dilate", [("dilate", 1)] * 9, [("grow", 1)], [("dilate",)], [("dilate", 0)], [("dilate", 65536)], [("dilate", 1.5)],
                [("dilate", radii[:-1])], [("dilate", True)], [("erode", [[1] * st.n])]):
        with pytest.raises(ValueError, match="morph_batch"):
            evalpost.morph_batch(buf, st, bad)
    info = torch.zeros(st.n, 4, dtype=torch.int64, device=DEV)
    for kw in ({"connectivity": 6}, {"max_area": -1}, {"max_area": 2.5}, {"labels": torch.zeros(st.out_bytes - 1, dtype=torch.int32, device=DEV)}):
        with pytest.raises(ValueError, match="fill_holes_batch"):
            evalpost.fill_holes_batch(buf, st, info, 0, **kw)
    with pytest.raises(ValueError, match="info must be"):
        evalpost.fill_holes_batch(buf, st, info[:, :3], 0)
    with pytest.raises(hip.HipLibraryError, match="row out of range"):
        evalpost.fill_holes_batch(buf, st, info, 1)
    with pytest.raises(hip.HipLibraryError, match="work buffer is too small"):
        hip.call("cris_morph_masks", buf.data_ptr(), st.out_bytes, evalpost.C.addressof(st.descs), st.dev.data_ptr(), st.n,
                 np.array([1], np.int32).ctypes.data_as(evalpost.C.c_void_p), 1, np.asarray(radii, np.int32).ctypes.data_as(evalpost.C.c_void_p),
                 torch.tensor(radii, dtype=torch.int32, device=DEV).data_ptr(), evalpost.morph_work(st, DEV).data_ptr(), 64, buf.data_ptr(),
                 st.out_bytes, None)
    assert not info.cpu().numpy().any()                                     # nothing was launched


# ---- end to end, tiny model ----
SPEC = Smooth(open=1, close=2, fill_holes=True)


def _smoothed(m, spec=SPEC):
    return MC.smooth(m, spec.open, spec.close, spec.fill_holes, spec.max_hole_area, spec.hole_connectivity)


def _flat(out):
    return [p for x in out for p in x]


def test_predictor_with_smooth(monkeypatch):
    from cris.pytorch_amd.infer import InferenceRunner
    from test_infer_multi_gpu import _setup
    from test_predict_gpu import SIZE as PSIZE, WORD_LEN as PWORD, _KeepSegment as PKeep, _records as _predict_records
    recs = _predict_records()
    files, exprs = [r["img"] for r in recs], [r["sents"] for r in recs]
    pipe = records.RecordPipeline(PSIZE, PWORD, DEV, mode="test", tokenizer=_StandInTokenizer())
    clip, head, sd = _setup("tiny", PSIZE, PWORD)
    model = PKeep(InferenceRunner(clip, head, sd, DEV))
    pr = predict.Predictor(model, pipe, thr=E2E_THR)
    plain = _flat(pr.predict(files, exprs, images_per_batch=2, masks="host"))       # (the first call also packs weights and captures graphs)
    _, base_calls = _recorded(monkeypatch, lambda: pr.predict(files, exprs, images_per_batch=2, masks="host"))
    assert all(type(p) is predict.Prediction for p in plain) and pr.smooth_info is None and pr._sm_work is None
    q16 = []                                                                # the q16 value of every pixel, from the kept logits
    for b, lo in enumerate(range(0, len(recs), 2)):
        _, params = pipe(recs[lo:lo + 2])
        probs = evalpost.sigmoid_upsample(model.logits[b], PSIZE, PSIZE)
        j = 0
        for r, prm in zip(recs[lo:lo + 2], params):
            for _ in r["sents"]:
                v = evalpost.warp_to_original(probs[j], prm["inverse"], prm["ori_size"]).cpu().numpy()
                q16.append(np.rint(v * np.float32(65536)).astype(np.int64))
                j += 1
    want = [_smoothed(p.mask) for p in plain]
    assert sum(not np.array_equal(w, p.mask != 0) for w, p in zip(want, plain)) >= 3                    # not vacuous
    below = 0
    for mode in ("host", "device", "rle", None):
        got = _flat(pr.predict(files, exprs, images_per_batch=2, masks=mode, smooth=SPEC))
        assert len(got) == len(plain) == 9 and pr.smooth_info.shape == (9, 2)
        for k, (p, raw, w) in enumerate(zip(got, plain, want)):
            assert type(p) is predict.ComponentPrediction and p.sentence == raw.sentence
            area, score_q16, x0, y0, x1, y1 = CC.stats_row(w, q16[k])
            assert p.area == area == int(w.sum()) and p.box == ((x0, y0, x1, y1) if area else None)
            assert p.score == (score_q16 / (65536.0 * area) if area else 0.0) and isinstance(p.score, float)
            assert p.raw_area == raw.area and p.n_components == CC.filter_mask(w, "all", 0, 8)[1][0]
            filled = MC.fill_holes(MC.closing(MC.opening(raw.mask, 1), 2))
            assert pr.smooth_info[k].tolist() == [filled[1], filled[2]]
            below += int((w & (q16[k] <= np.rint(np.float32(E2E_THR) * np.float32(65536)))).any())
            if mode == "host":
                assert isinstance(p.mask, np.ndarray) and np.array_equal(p.mask, w.astype(np.uint8) * 255)
            elif mode == "device":
                assert torch.is_tensor(p.mask) and p.mask.is_cuda and np.array_equal(p.mask.cpu().numpy(), w.astype(np.uint8) * 255)
            elif mode == "rle":
                assert p.mask == rle.encode(w.astype(np.uint8) * 255)
            else:
                assert p.mask is None
    assert below > 0                                                        # pixels below the threshold were set and scored
    # with a Components spec after it, and the constructor's default
    comp = Components(keep="largest", min_area=5)
    got = _flat(predict.Predictor(model, pipe, thr=E2E_THR, components=comp, smooth=SPEC).predict(files, exprs, images_per_batch=2, masks="host"))
    for k, (p, raw, w) in enumerate(zip(got, plain, want)):
        kept, info, _ = CC.filter_mask(w, comp.keep, comp.min_area, comp.connectivity)
        area, score_q16, x0, y0, x1, y1 = CC.stats_row(kept, q16[k])
        assert np.array_equal(p.mask, kept.astype(np.uint8) * 255) and (p.n_components, p.raw_area) == (info[0], raw.area)
        assert p.area == area and p.box == ((x0, y0, x1, y1) if area else None) and p.score == (score_q16 / (65536.0 * area) if area else 0.0)
    # smooth=None / a no-op spec / the keyword left out, after the spec was used: the library calls recorded before it ever was
    for value in (None, Smooth(), "default"):
        out, calls = _recorded(monkeypatch, lambda: pr.predict(files, exprs, images_per_batch=2, masks="host", smooth=value))
        assert calls == base_calls and not any(c in NEW for c in calls) and pr.smooth_info is None
        for a, b in zip(_flat(out), plain):
            assert type(a) is predict.Prediction and a[2:] == b[2:] and np.array_equal(a.mask, b.mask)
    _, calls = _recorded(monkeypatch, lambda: pr.predict(files, exprs, images_per_batch=2, masks=None, smooth=SPEC))
    per_batch = ["cris_predict_masks_batch", "cris_morph_masks", "cris_fill_holes", "cris_label_components", "cris_filter_components"]
    assert [c for c in calls if c in per_batch] == per_batch * 3


@pytest.fixture(scope="module")
def tiny():
    """records, the evaluator, the library calls of its first pass, and per sample of validate(batch_size=4) the thresholded warp
    (bool) from the model's own logits and the decoded ground truth (bool)"""
    recs = _records()
    pipe = records.RecordPipeline(SIZE, WORD_LEN, DEV, mode="val", tokenizer=_StandInTokenizer())
    model = _Keep(_runner())
    ev = evaluate.Evaluator(model, pipe, thr=E2E_THR)
    base = ev.validate(recs, batch_size=4)                                  # (the first pass also packs weights and captures graphs)
    names, real = [], hip.call
    hip.call = lambda name, *a: (names.append(name), real(name, *a))[1]
    try:
        assert ev.validate(recs, batch_size=4) == base
    finally:
        hip.call = real
    base_counts = ev.counts.copy()
    assert ev.smooth_info is None and ev._sm_work is None
    preds, gts = [], []
    for b, lo in enumerate(range(0, len(recs), 4)):
        part = recs[lo:lo + 4]
        _, _, params = pipe(part)
        probs = evalpost.sigmoid_upsample(model.logits[b], SIZE, SIZE)
        for j, (r, prm) in enumerate(zip(part, params)):
            preds.append(evalpost.warp_to_original(probs[j], prm["inverse"], prm["ori_size"]).cpu().numpy() > np.float32(E2E_THR))
            gts.append(pngdec.decode_gray(r["mask"]).numpy() != 0)
    return recs, model, ev, base, base_counts, names, preds, gts


def _counts(masks, gts):
    return [[int((m & g).sum()), int((m | g).sum())] for m, g in zip(masks, gts)]


def test_validate_with_smooth(tiny, monkeypatch):
    recs, _, ev, base, base_counts, base_calls, preds, gts = tiny
    want = [_smoothed(p) for p in preds]
    assert sum(not np.array_equal(w, p) for w, p in zip(want, preds)) >= 3  # not vacuous
    result = ev.validate(recs, batch_size=4, smooth=SPEC)
    m = evaluate.metrics(np.array(_counts(want, gts)))
    assert ev.counts.tolist() == _counts(want, gts) and result == (m[0], m[1]) and ev.per_sample.tolist() == m[2].tolist()
    fills = [MC.fill_holes(MC.closing(MC.opening(p, 1), 2))[1:3] for p in preds]
    assert ev.smooth_info.tolist() == [list(f) for f in fills]
    # with components: smoothed, then filtered; with boundary: the same final masks
    comp, bspec = Components(keep="largest", min_area=5), Boundary()
    kept = [CC.filter_mask(w, comp.keep, comp.min_area, comp.connectivity)[0] for w in want]
    ev.validate(recs, batch_size=4, smooth=SPEC, components=comp, boundary=True)
    assert ev.counts.tolist() == _counts(kept, gts)
    assert ev.boundary_counts.tolist() == [BC.counts(k, g, bspec.radius(*g.shape)) for k, g in zip(kept, gts)]
    ev.validate(recs, batch_size=4, smooth=SPEC, boundary=True)
    assert ev.counts.tolist() == _counts(want, gts)
    assert ev.boundary_counts.tolist() == [BC.counts(w, g, bspec.radius(*g.shape)) for w, g in zip(want, gts)]
    # only a closing, a subset in another order
    only = Smooth(close=3)
    ev.validate(recs, indices=[7, 2, 9], batch_size=4, smooth=only)
    assert ev.counts.tolist() == _counts([MC.closing(preds[k], 3) for k in (7, 2, 9)], [gts[k] for k in (7, 2, 9)])
    assert ev.smooth_info.tolist() == [[0, 0]] * 3
    # smooth=None after the spec was used: the library calls recorded before it ever was, the same figures, no table
    for kw in ({}, {"smooth": None}, {"smooth": Smooth()}):
        out, calls = _recorded(monkeypatch, lambda: ev.validate(recs, batch_size=4, **kw))
        assert calls == base_calls and not any(c in NEW for c in calls) and out == base and np.array_equal(ev.counts, base_counts)
        assert ev.smooth_info is None
    _, calls = _recorded(monkeypatch, lambda: ev.validate(recs, batch_size=4, smooth=SPEC))
    per_batch = ["cris_eval_iou_batch", "cris_morph_masks", "cris_fill_holes", "cris_mask_iou_batch"]
    assert [c for c in calls if c in per_batch + ["cris_label_components"]] == per_batch * 3
    fresh = evaluate.Evaluator(ev.model, ev.pipe, thr=E2E_THR)
    fresh.validate(recs, batch_size=4)
    assert fresh._sm_work is None and fresh._cc_masks is None and fresh.smooth_info is None     # nothing new is allocated without the spec


def test_inference_with_smooth(tiny, monkeypatch):
    recs, model, _, _, _, _, _, _ = tiny
    tpipe = records.RecordPipeline(SIZE, WORD_LEN, DEV, mode="test", tokenizer=_StandInTokenizer())
    tev = evaluate.Evaluator(_KeepSegment(model.inner), tpipe, thr=E2E_THR)
    seen = []
    tev.inference(recs[:4], images_per_batch=2)
    (base, base_calls) = _recorded(monkeypatch, lambda: tev.inference(recs[:4], images_per_batch=2, visualize=lambda rec, sent, i, m: seen.append((rec, m))))
    base_counts = tev.counts.copy()
    gts = [pngdec.decode_gray(rec["mask"]).numpy() != 0 for rec, _ in seen]
    want = [_smoothed(m) for _, m in seen]
    assert len(want) == sum(len(r["sents"]) for r in recs[:4]) > 4
    got = []
    tev.inference(recs[:4], images_per_batch=2, smooth=SPEC, visualize=lambda rec, sent, i, m: got.append(m))
    assert tev.counts.tolist() == _counts(want, gts) and all(np.array_equal(g, w.astype(np.uint8) * 255) for g, w in zip(got, want))
    assert tev.smooth_info.tolist() == [list(MC.fill_holes(MC.closing(MC.opening(m, 1), 2))[1:3]) for _, m in seen]
    comp, bspec = Components(keep="largest", min_area=5), Boundary()
    kept = [CC.filter_mask(w, comp.keep, comp.min_area, comp.connectivity)[0] for w in want]
    tev.inference(recs[:4], images_per_batch=2, smooth=SPEC, components=comp, boundary=True)
    assert tev.counts.tolist() == _counts(kept, gts)
    assert tev.boundary_counts.tolist() == [BC.counts(k, g, bspec.radius(*g.shape)) for k, g in zip(kept, gts)]
    tev.inference(recs[:4], images_per_batch=2, smooth=SPEC)
    assert tev.counts.tolist() == _counts(want, gts) and tev.boundary_counts is None
    out, calls = _recorded(monkeypatch, lambda: tev.inference(recs[:4], images_per_batch=2, smooth=None, visualize=lambda rec, sent, i, m: None))
    assert calls == base_calls and not any(c in NEW for c in calls) and out == base and np.array_equal(tev.counts, base_counts)
    assert tev.smooth_info is None
