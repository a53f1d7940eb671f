"""Mask erosion and Boundary IoU on the GPU (csrc/morph.hip behind evalpost.erode_batch / boundary_iou_batch) against
the summed-area-table oracle of tests/boundary_cases.py: every byte and every count, as equalities; what the launches must leave
alone.  Then evaluate.Evaluator with boundary=True on the tiny synthetic model against the oracle applied to the model's own logits,
and the library calls a pass issues with and without the spec."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

pytest.importorskip("PIL")

import boundary_cases as BC  # noqa: E402
import components_cases as CC  # noqa: E402
from cris.pytorch_amd import evalpost, evaluate, hip, pngdec, records  # noqa: E402
from cris.pytorch_amd.evalpost import Boundary, Components  # noqa: E402
from test_evaluate_gpu import SIZE, WORD_LEN, _Keep, _KeepSegment, _records, _runner  # noqa: E402
from test_predict_gpu import E2E_THR  # noqa: E402
from test_records_gpu import _StandInTokenizer  # noqa: E402

DEV = torch.device("cuda:0")
IDENT = np.array([[1.0, 0, 0], [0, 1.0, 0]], np.float64)
NEW = ("cris_erode_masks", "cris_boundary_iou_batch", "cris_boundary_work_bytes")


def _rect(buf, d):
    return buf[d.out_off:d.out_off + d.pitch * d.h_out].reshape(d.h_out, d.pitch)[:, :d.w_out]


def _pack(masks, gts=None, alias=None):
    """the masks in one ragged packed buffer at out_off, one descriptor each in order, plus (alias = index) one more descriptor that
    names that mask's rectangle; gts: the ground truth of every mask, packed by the staging at mask_off.  Pitch padding, the gaps
    between rectangles and the tail of the mask buffer are 255: read as pixels they change the result.  -> (staging, buffer, inside),
    inside: True at the bytes of `buffer` that are pixels of a descriptor."""
    descs = [(IDENT, i, 0, i) for i in range(len(masks))] + ([] if alias is None else [(IDENT, alias, 0, len(masks))])
    st = evalpost.EvalStaging(DEV, mask_bytes=16)
    st = st.pack_sizes([m.shape for m in masks], descs) if gts is None else st.pack(gts, descs)
    if alias is not None:
        st.descs[len(masks)].out_off = st.descs[alias].out_off              # (its own slot stays an unused gap)
    st.upload()
    host = np.full(st.out_bytes + 64, 255, np.uint8)
    inside = np.zeros(st.out_bytes + 64, bool)
    for i, m in enumerate(masks):
        d = st.descs[i]
        assert (d.h_out, d.w_out, d.pitch) == (m.shape[0], m.shape[1], BC.pitch_of(m.shape[1]))
        _rect(host, d)[:] = m
        _rect(inside, d)[:] = True
    return st, torch.from_numpy(host).to(DEV), inside


@pytest.fixture(scope="module")
def batch():
    names = [k for k, _, _ in BC.cases()]
    a = names.index(BC.ALIAS)
    st, buf, inside = _pack([m for _, m, _ in BC.cases()], alias=a)
    radii = [d for _, _, d in BC.cases()] + [BC.cases()[a][2]]
    return st, buf, inside, radii, names + [BC.ALIAS + " (the same rectangle)"], list(BC.expected()) + [BC.expected()[a]]


@pytest.mark.parametrize("boundary", [False, True], ids=["erosion", "boundary"])
def test_erode_batch_equals_the_oracle(batch, boundary):
    st, buf, inside, radii, names, want = batch
    assert st.n == len(BC.cases()) + 1 and any(st.descs[i].pitch != st.descs[i].w_out for i in range(st.n))
    before = buf.clone()
    out = torch.full((st.out_bytes + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    got = evalpost.erode_batch(buf, st, radii, out=out, boundary=boundary)
    assert got.data_ptr() == out.data_ptr()
    res = out.cpu().numpy()
    masks = [m for _, m, _ in BC.cases()] + [BC.cases()[names.index(BC.ALIAS)][1]]
    for i, (name, e) in enumerate(zip(names, want)):
        ref = ((masks[i] != 0) & ~e) if boundary else e
        assert np.array_equal(_rect(res, st.descs[i]), ref.astype(np.uint8) * 255), (name, radii[i])     # byte for byte
    assert (res[~inside] == 0x5A).all()                                     # padding, gaps and tail keep their fill
    assert torch.equal(buf, before)                                         # the source is only read
    # radii on the device, a fresh zeroed result, dirty scratch: the same bytes
    work = evalpost.boundary_work(st, DEV)
    work.fill_(-1)
    again = evalpost.erode_batch(buf, st, torch.tensor(radii, dtype=torch.int32, device=DEV), boundary=boundary, work=work)
    assert again.numel() == st.out_bytes and again.dtype == torch.uint8
    assert torch.equal(again[torch.from_numpy(inside[:st.out_bytes]).to(DEV)], out[:st.out_bytes][torch.from_numpy(inside[:st.out_bytes]).to(DEV)])
    assert int(again[torch.from_numpy(~inside[:st.out_bytes]).to(DEV)].max()) == 0
    # in place
    same = buf.clone()
    assert evalpost.erode_batch(same, st, radii, out=same, boundary=boundary, work=work) is same
    place = same.cpu().numpy()
    assert np.array_equal(place[inside], res[inside]) and (place[~inside] == 255).all()


@pytest.fixture(scope="module")
def pair_batch():
    names = [k for k, _, _, _ in BC.pairs()]
    a = names.index(BC.PAIR_ALIAS)
    st, buf, _ = _pack([p for _, p, _, _ in BC.pairs()], gts=[g for _, _, g, _ in BC.pairs()], alias=a)
    radii = [d for _, _, _, d in BC.pairs()] + [BC.pairs()[a][3]]
    return st, buf, radii, names + [BC.PAIR_ALIAS + " (the same rectangle)"], list(BC.expected_counts()) + [BC.expected_counts()[a]]


def test_boundary_iou_batch_equals_the_oracle(pair_batch):
    st, buf, radii, names, want = pair_batch
    n = st.n
    offs = [st.descs[i].mask_off for i in range(n - 1)]
    assert len(set(offs)) == n - 1 and st.descs[n - 1].mask_off == st.descs[names.index(BC.PAIR_ALIAS)].mask_off
    # the staging pads the ground truth's rows with zeros: fill the padding with 255 - read as pixels it would change the counts
    gt = st.masks.clone()
    pad = np.ones(st.mask_bytes, bool)
    for i in range(n - 1):
        d = st.descs[i]
        pad[d.mask_off:d.mask_off + d.pitch * d.h_out].reshape(d.h_out, d.pitch)[:, :d.w_out] = False
    gt[torch.from_numpy(pad).to(DEV)] = 255
    base = torch.arange(2 * (n + 3), dtype=torch.int32, device=DEV).reshape(n + 3, 2) + 5
    table = base.clone()
    before, gt_before = buf.clone(), gt.clone()
    evalpost.boundary_iou_batch(buf, st, gt, radii, table, 2)
    got = (table - base).cpu().numpy()
    for i, name in enumerate(names):
        print("%-40s d %2d  counts %s (oracle %s)" % (name, radii[i], got[2 + i].tolist(), want[i]))
    assert got[2:2 + n].tolist() == want
    assert not got[:2].any() and not got[2 + n:].any()                      # the rows of no descriptor are left alone
    assert torch.equal(buf, before) and torch.equal(gt, gt_before)
    # a second run, scratch filled with -1, radii on the device: the identical table
    work = evalpost.boundary_work(st, DEV)
    work.fill_(-1)
    table2 = base.clone()
    evalpost.boundary_iou_batch(buf, st, gt, torch.tensor(radii, dtype=torch.int32, device=DEV), table2, 2, work=work)
    assert torch.equal(table2, table)
    # the boundary counts are the mask counts of the two boundary images
    bp = evalpost.erode_batch(buf, st, radii, boundary=True)
    for i in range(n - 1):
        p = _rect(bp.cpu().numpy(), st.descs[i]) != 0
        assert [int((p & BC.boundary(BC.pairs()[i][2], radii[i])).sum()), int((p | BC.boundary(BC.pairs()[i][2], radii[i])).sum())] == want[i]


class _ShortBuffer:
    """a staging's descriptors under another out_bytes"""

    def __init__(self, st, out_bytes):
        self.descs, self.dev, self.n, self.out_bytes = st.descs, st.dev, st.n, out_bytes


def test_argument_errors(pair_batch):
    st, buf, radii, _, _ = pair_batch
    table = torch.zeros(st.n, 2, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="masks_u8"):
        evalpost.erode_batch(buf.to(torch.int8), st, radii)
    with pytest.raises(ValueError, match="masks_u8"):
        evalpost.erode_batch(buf[:st.out_bytes - 1], st, radii)
    with pytest.raises(ValueError, match="out must be"):
        evalpost.erode_batch(buf, st, radii, out=buf[:st.out_bytes - 1])
    with pytest.raises(ValueError, match="out must be"):
        evalpost.erode_batch(buf, st, radii, out=torch.zeros(st.out_bytes, dtype=torch.int32, device=DEV))
    for bad in (radii[:-1], radii + [1], [0] + radii[1:], [1.5] * st.n, torch.tensor(radii, dtype=torch.int64, device=DEV),
                torch.tensor(radii[:-1], dtype=torch.int32, device=DEV)):
        with pytest.raises(ValueError, match="radi"):
            evalpost.erode_batch(buf, st, bad)
        with pytest.raises(ValueError, match="radi"):
            evalpost.boundary_iou_batch(buf, st, st.masks, bad, table, 0)
    with pytest.raises(ValueError, match="masks_u8"):
        evalpost.boundary_iou_batch(buf[:st.out_bytes - 1], st, st.masks, radii, table, 0)
    with pytest.raises(ValueError, match="gt_masks_u8"):
        evalpost.boundary_iou_batch(buf, st, st.masks.to(torch.int16), radii, table, 0)
    for bad in (table.to(torch.int64), table[:, :1], torch.zeros(st.n, 3, dtype=torch.int32, device=DEV)):
        with pytest.raises(ValueError, match="counts must be"):
            evalpost.boundary_iou_batch(buf, st, st.masks, radii, bad, 0)
    with pytest.raises(ValueError, match="row0"):
        evalpost.boundary_iou_batch(buf, st, st.masks, radii, table, st.n)
    with pytest.raises(hip.HipLibraryError, match="row out of range"):
        evalpost.boundary_iou_batch(buf, st, st.masks, radii, table, 1)     # the last descriptor's row would fall outside the table
    with pytest.raises(hip.HipLibraryError, match="mask outside the buffer"):
        evalpost.boundary_iou_batch(buf, st, st.masks[:st.mask_bytes - 16], radii, table, 0)
    with pytest.raises(hip.HipLibraryError, match="output outside the buffer"):
        evalpost.erode_batch(buf, _ShortBuffer(st, st.descs[st.n - 2].out_off), radii)
    with pytest.raises(hip.HipLibraryError, match="work buffer is too small"):
        hip.call("cris_erode_masks", buf.data_ptr(), st.out_bytes, evalpost.C.addressof(st.descs), st.dev.data_ptr(), st.n,
                 np.asarray(radii, np.int32).ctypes.data_as(evalpost.C.c_void_p), torch.tensor(radii, dtype=torch.int32, device=DEV).data_ptr(),
                 evalpost.boundary_work(st, DEV).data_ptr(), 64, buf.data_ptr(), st.out_bytes, 0, None)
    assert not table.cpu().numpy().any()                                    # nothing was launched


# ---- end to end, tiny model ----
def _recorded(monkeypatch, fn):
    names = []
    real = hip.call
    monkeypatch.setattr(hip, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    try:
        return fn(), names
    finally:
        monkeypatch.undo()


@pytest.fixture(scope="module")
def tiny():
    """records, the model, and per sample of validate(batch_size=4) the oracle's inputs from the model's own logits: the thresholded
    warp (bool) and the decoded ground truth (bool)"""
    recs = _records()
    pipe = records.RecordPipeline(SIZE, WORD_LEN, DEV, mode="val", tokenizer=_StandInTokenizer())
    model = _Keep(_runner())
    ev = evaluate.Evaluator(model, pipe, thr=E2E_THR)
    base = ev.validate(recs, batch_size=4)
    base_counts = ev.counts.copy()
    assert ev.boundary_counts is None and ev.boundary_iou is None and ev.boundary_prec is None and ev.boundary_per_sample is None
    preds, gts = [], []
    for b, lo in enumerate(range(0, len(recs), 4)):
        part = recs[lo:lo + 4]
        _, _, params = pipe(part)
        probs = evalpost.sigmoid_upsample(model.logits[b], SIZE, SIZE)
        for j, (r, prm) in enumerate(zip(part, params)):
            preds.append(evalpost.warp_to_original(probs[j], prm["inverse"], prm["ori_size"]).cpu().numpy() > np.float32(E2E_THR))
            gts.append(pngdec.decode_gray(r["mask"]).numpy() != 0)
    return recs, pipe, model, ev, base, base_counts, preds, gts


def _check_figures(ev, want):
    m = evaluate.metrics(np.array(want))
    assert ev.boundary_counts.tolist() == want
    assert ev.boundary_iou == m[0] and ev.boundary_prec == m[1] and ev.boundary_per_sample.tolist() == m[2].tolist()


def test_validate_with_boundary(tiny):
    recs, pipe, model, ev, base, base_counts, preds, gts = tiny
    spec = Boundary()
    want = [BC.counts(p, g, spec.radius(*g.shape)) for p, g in zip(preds, gts)]
    for value in (True, spec):
        assert ev.validate(recs, batch_size=4, boundary=value) == base      # (iou, prec) of the masks: unchanged
        assert np.array_equal(ev.counts, base_counts)
        _check_figures(ev, want)
    print("validate boundary counts", want, "boundary IoU %.4f  mask IoU %.4f" % (ev.boundary_iou, base[0]))
    mask_iou = evaluate.metrics(base_counts)[2]
    assert any(u > 0 and b != m for (_, u), b, m in zip(want, ev.boundary_per_sample, mask_iou))       # not vacuous
    # another radius rule, a subset in another order
    wide = Boundary(ratio=0.05, min_radius=4)
    ev.validate(recs, indices=[7, 2, 9], batch_size=4, boundary=wide)
    _check_figures(ev, [BC.counts(preds[k], gts[k], wide.radius(*gts[k].shape)) for k in (7, 2, 9)])
    assert [wide.radius(*gts[k].shape) for k in (2, 9)] == [4, 4] and wide.radius(*gts[7].shape) == 7
    # with the clean-up: the boundaries of the FILTERED masks
    comp = Components(keep="largest", min_area=5)
    kept = [CC.filter_mask(p, comp.keep, comp.min_area, comp.connectivity)[0] for p in preds]
    ev.validate(recs, batch_size=4, components=comp)
    comp_result, comp_counts = (ev.validate(recs, batch_size=4, components=comp), ev.counts.copy())
    assert ev.boundary_counts is None
    assert ev.validate(recs, batch_size=4, components=comp, boundary=True) == comp_result and np.array_equal(ev.counts, comp_counts)
    assert comp_counts.tolist() == [[int((k & g).sum()), int((k | g).sum())] for k, g in zip(kept, gts)]
    _check_figures(ev, [BC.counts(k, g, spec.radius(*g.shape)) for k, g in zip(kept, gts)])
    # a pass without the spec clears the figures
    ev.validate(recs, batch_size=4)
    assert ev.boundary_counts is None and ev.boundary_iou is None and ev.boundary_prec is None and ev.boundary_per_sample is None


def test_inference_with_boundary(tiny):
    recs, _, model, _, _, _, _, _ = tiny
    spec = Boundary()
    tpipe = records.RecordPipeline(SIZE, WORD_LEN, DEV, mode="test", tokenizer=_StandInTokenizer())
    tev = evaluate.Evaluator(_KeepSegment(model.inner), tpipe, thr=E2E_THR)
    seen = []
    base = tev.inference(recs[:4], images_per_batch=2, visualize=lambda rec, sent, i, m: seen.append((rec, m)))
    base_counts = tev.counts.copy()
    assert tev.boundary_counts is None
    want = []
    for rec, m in seen:                                                     # the masks the pass itself produced
        gt = pngdec.decode_gray(rec["mask"]).numpy() != 0
        want.append(BC.counts(m, gt, spec.radius(*gt.shape)))
    assert len(want) == sum(len(r["sents"]) for r in recs[:4]) > 4          # several expressions share one ground truth
    assert tev.inference(recs[:4], images_per_batch=2, boundary=True) == base and np.array_equal(tev.counts, base_counts)
    _check_figures(tev, want)
    again = []
    assert tev.inference(recs[:4], images_per_batch=2, boundary=True, visualize=lambda rec, sent, i, m: again.append(m)) == base
    _check_figures(tev, want)
    assert all(np.array_equal(a, m) for a, (_, m) in zip(again, seen))      # the callback's masks are the unchanged ones
    comp = Components(keep="largest", min_area=5)
    tev.inference(recs[:4], images_per_batch=2, components=comp, boundary=True)
    kept = [CC.filter_mask(m, comp.keep, comp.min_area, comp.connectivity)[0] for _, m in seen]
    gts = [pngdec.decode_gray(rec["mask"]).numpy() != 0 for rec, _ in seen]
    assert tev.counts.tolist() == [[int((k & g).sum()), int((k | g).sum())] for k, g in zip(kept, gts)]
    _check_figures(tev, [BC.counts(k, g, spec.radius(*g.shape)) for k, g in zip(kept, gts)])
    assert any(u > 0 for _, u in want)


def test_library_calls_with_and_without_the_spec(tiny, monkeypatch):
    """cris_boundary_iou_batch (three launches) once per batch, after the last launch that touches the batch's masks"""
    recs, _, _, ev, _, _, _, _ = tiny
    comp = Components(keep="largest", min_area=5)
    plain = ["cris_eval_iou_batch"]
    cleaned = ["cris_eval_iou_batch", "cris_label_components", "cris_filter_components", "cris_mask_iou_batch"]
    for components, post in ((None, plain), (comp, cleaned)):
        _, base = _recorded(monkeypatch, lambda: ev.validate(recs, batch_size=4, components=components))
        _, none = _recorded(monkeypatch, lambda: ev.validate(recs, batch_size=4, components=components, boundary=None))
        assert none == base and not any(c in NEW for c in base) and [c for c in base if c in cleaned] == post * 3
        scratch = (ev._bd_masks, ev._bd_work)
        _, calls = _recorded(monkeypatch, lambda: ev.validate(recs, batch_size=4, components=components, boundary=True))
        want = []
        for c in base:
            want.append(c)
            if c == post[-1]:
                want.append("cris_boundary_iou_batch")
        assert calls == want and calls.count("cris_boundary_iou_batch") == 3 and "cris_erode_masks" not in calls
        _, calls = _recorded(monkeypatch, lambda: ev.validate(recs, batch_size=4, components=components, boundary=True))
        assert calls == want and ev._bd_work is not None                    # the scratch is reused across batches and passes
        if scratch[1] is not None:
            assert ev._bd_work.data_ptr() == scratch[1].data_ptr()
    fresh = evaluate.Evaluator(ev.model, ev.pipe, thr=E2E_THR)
    fresh.validate(recs, batch_size=4)
    assert fresh._bd_masks is None and fresh._bd_work is None               # nothing new is allocated without the spec
