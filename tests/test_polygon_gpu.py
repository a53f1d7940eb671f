"""Polygon tracing on the GPU (csrc/polygon.hip behind evalpost.polygon_count_batch / polygon_collect) against the
per-crack oracle of tests/polygon_cases.py: totals, every ring, every vertex and the ring table, as equalities; what the launches
must leave alone; the buffers' stated sizes; the rounds.  Then predict.Predictor with masks="polygon" on the tiny synthetic model
against its own masks="host" result, the library calls each mask mode issues, and the command line's results file."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

pytest.importorskip("PIL")

import polygon_cases as PC  # noqa: E402
from cris.pytorch_amd import evalpost, hip, polygon, predict, records  # noqa: E402
from cris.pytorch_amd.evalpost import Components, Smooth  # noqa: E402
from cris.pytorch_amd.infer import InferenceRunner  # noqa: E402
from test_infer_multi_gpu import _setup  # noqa: E402
from test_predict_gpu import E2E_THR, SIZE, WORD_LEN, _KeepSegment  # noqa: E402
from test_predict_gpu import _records as _predict_records  # noqa: E402
from test_records_gpu import _StandInTokenizer  # noqa: E402

DEV = torch.device("cuda:0")
IDENT = np.array([[1.0, 0, 0], [0, 1.0, 0]], np.float64)
FILL = 0x7F7F7F7F7F7F7F7F


def _pack(masks, alias=None):
    """the masks in one ragged packed buffer, one descriptor each in order, plus (alias = index) one more descriptor that names
    that mask's rectangle.  Pitch padding, the gaps between rectangles and the tail are 255: read as pixels they change the result."""
    shapes = [m.shape for m in masks]
    descs = [(IDENT, i, 0, i) for i in range(len(masks))] + ([] if alias is None else [(IDENT, alias, 0, len(masks))])
    st = evalpost.EvalStaging(DEV, mask_bytes=16).pack_sizes(shapes, descs)
    if alias is not None:
        st.descs[len(masks)].out_off = st.descs[alias].out_off              # (its own slot stays an unused gap)
    st.upload()
    host = np.full(st.out_bytes + 64, 255, np.uint8)
    for i, m in enumerate(masks):
        d = st.descs[i]
        assert (d.h_out, d.w_out, d.pitch) == (m.shape[0], m.shape[1], PC.pitch_of(m.shape[1]))
        host[d.out_off:d.out_off + d.pitch * d.h_out].reshape(d.h_out, d.pitch)[:, :d.w_out] = m
    return st, torch.from_numpy(host).to(DEV)


def _same(p, q):
    return (p["size"] == q["size"] and p["holes"] == q["holes"] and len(p["rings"]) == len(q["rings"])
            and all(a.dtype == b.dtype == np.int32 and np.array_equal(a, b) for a, b in zip(p["rings"], q["rings"])))


def _filled(words):
    return torch.full((words,), FILL, dtype=torch.int64, device=DEV)


@pytest.fixture(scope="module")
def batch():
    names = [k for k, _ in PC.cases()]
    st, buf = _pack([m for _, m in PC.cases()], alias=names.index(PC.ALIAS))
    want = [PC.expected_dict(i) for i in range(len(names))] + [PC.expected_dict(names.index(PC.ALIAS))]
    return st, buf, names + [PC.ALIAS + " (the same rectangle)"], want


def test_polygon_batch_equals_the_oracle(batch):
    st, buf, names, want = batch
    n = st.n
    assert n == len(PC.cases()) + 1 and st.descs[n - 1].out_off == st.descs[names.index(PC.ALIAS)].out_off
    counts = [sum(len(r) for r in p["rings"]) for p in want]
    need, nrings = sum(counts), sum(len(p["rings"]) for p in want)
    before = buf.clone()
    # sentinel-filled over-allocations of every buffer the launches write
    work_words = (hip.load().cris_polygon_work_bytes(C.addressof(st.descs), n) + 7) // 8
    work = _filled(work_words + 32)
    totals = evalpost.polygon_count_batch(buf, st, work=work[:work_words])
    assert totals.dtype == torch.int64 and totals.shape == (n + 1,) and totals.is_cuda
    t = totals.cpu().numpy()
    for i, name in enumerate(names):
        d = st.descs[i]
        print("%-60s %3d x %3d  vertices %6d (oracle %6d)  rings %5d" % (name, d.h_out, d.w_out, t[i], counts[i], len(want[i]["rings"])))
        assert t[i] == counts[i], name
    assert t[n] == need
    assert (work[work_words:] == FILL).all()
    tw_words, out_words = (hip.load().cris_polygon_trace_work_bytes(need, n) + 7) // 8, 2 + 4 * (need // 4) + need
    bufs = evalpost.PolygonBuffers(trace_work=_filled(tw_words + 32), out=_filled(out_words + 32))
    twork, out = bufs.trace_work, bufs.out
    got = evalpost.polygon_collect(buf, st, totals, work=work[:work_words], buffers=bufs)
    assert bufs.trace_work is twork and bufs.out is out and bufs.spans == (tw_words, out_words)       # reused, not grown
    for name, p, q in zip(names, got, want):
        assert _same(p, q), name                                            # every ring, every vertex
    # the ring table: descriptor, offset, length, 2 A per ring, rings in descriptor then raster order, vertices packed
    table, at = [], 0
    for i, q in enumerate(want):
        for r in q["rings"]:
            table.append([i, at, len(r), PC.oracle_twice_area([tuple(v) for v in r.tolist()])])
            at += len(r)
    assert bufs.table.tolist() == table and len(table) == nrings and at == need
    assert np.array_equal(bufs.vertices, np.concatenate([r for q in want for r in q["rings"]]))
    words = out.cpu().numpy()
    assert words[:2].tolist() == [nrings, need]
    assert (words[2 + 4 * nrings:2 + 4 * (need // 4)] == FILL).all()       # no row beyond the last ring
    assert (words[out_words:] == FILL).all() and (twork[tw_words:] == FILL).all()      # nothing beyond the stated sizes
    assert (work[work_words:] == FILL).all()
    assert torch.equal(buf, before)                                         # the masks are only read
    a, b = names.index("random 0.5"), names.index("random 0.5 again")
    assert st.descs[a].out_off != st.descs[b].out_off and _same(got[a], got[b])
    # a second run with dirty scratch and reused buffers, and one with two more jumping rounds than needed: the same words
    first = words[:out_words].copy()
    for extra in (0, 2):
        twork.fill_(-1)
        out.fill_(-1)
        again = evalpost.polygon_collect(buf, st, totals, work=work[:work_words], buffers=bufs, extra_rounds=extra)
        assert all(_same(p, q) for p, q in zip(again, want))
        now = out.cpu().numpy()
        assert np.array_equal(now[:2 + 4 * nrings], first[:2 + 4 * nrings]) and np.array_equal(now[2 + 4 * (need // 4):out_words], first[2 + 4 * (need // 4):])
        assert (now[out_words:] == -1).all() and (now[2 + 4 * nrings:2 + 4 * (need // 4)] == -1).all()
    # fresh default buffers, the count run again inside collect
    fresh = evalpost.polygon_collect(buf, st, evalpost.polygon_count_batch(buf, st))
    assert all(_same(p, q) for p, q in zip(fresh, want))
    with pytest.raises(ValueError, match="masks_u8"):
        evalpost.polygon_count_batch(buf[:st.out_bytes - 1], st)
    with pytest.raises(ValueError, match="totals must be"):
        evalpost.polygon_collect(buf, st, totals[:n], work=work)
    with pytest.raises(ValueError, match="extra_rounds"):
        evalpost.polygon_collect(buf, st, totals, work=work, extra_rounds=9)
    with pytest.raises(ValueError, match="PolygonBuffers"):
        evalpost.polygon_collect(buf, st, totals, work=work, buffers=(twork, out))


def test_every_comb_alone_crosses_its_round_and_block_edges():
    """one batch per comb, so that the comb's own vertex count fixes the jumping rounds: 2^k - 2, 2^k, 2^k + 2 around one wave, one
    block, one scan chunk and 4096; then the serpentine"""
    bufs = evalpost.PolygonBuffers()
    for m in [PC.comb(v) for v in PC.COMB_SIZES] + [PC.serpentine()]:
        st, buf = _pack([m])
        work = evalpost.polygon_work(st, DEV)
        got = evalpost.polygon_collect(buf, st, evalpost.polygon_count_batch(buf, st, work=work), work=work, buffers=bufs)
        rings, _ = PC.oracle_trace(m)
        assert len(got) == 1 and len(got[0]["rings"]) == 1 == len(rings) and got[0]["rings"][0].tolist() == [list(v) for v in rings[0]], m.shape
        assert bufs.table.tolist() == [[0, 0, len(rings[0]), PC.oracle_twice_area(rings[0])]]


def test_a_batch_of_background_issues_no_trace(monkeypatch):
    st, buf = _pack([np.zeros((5, 7), np.uint8), np.zeros((PC.RB + 1, PC.CG + 1), np.uint8), np.zeros((1, 1), np.uint8)])
    names, real = [], hip.call
    monkeypatch.setattr(hip, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    work = evalpost.polygon_work(st, DEV)
    totals = evalpost.polygon_count_batch(buf, st, work=work)
    bufs = evalpost.PolygonBuffers()
    got = evalpost.polygon_collect(buf, st, totals, work=work, buffers=bufs)
    monkeypatch.undo()
    assert names == ["cris_polygon_count"] and totals.cpu().tolist() == [0, 0, 0, 0]
    assert got == [{"size": [5, 7], "rings": [], "holes": []}, {"size": [PC.RB + 1, PC.CG + 1], "rings": [], "holes": []},
                   {"size": [1, 1], "rings": [], "holes": []}]
    assert bufs.trace_work is None and bufs.out is None                     # nothing was allocated either


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


@pytest.fixture(scope="module")
def tiny():
    recs = _predict_records()
    pipe = records.RecordPipeline(SIZE, WORD_LEN, DEV, mode="test", tokenizer=_StandInTokenizer())
    clip, head, sd = _setup("tiny", SIZE, WORD_LEN)
    model = _KeepSegment(InferenceRunner(clip, head, sd, DEV))
    return predict.Predictor(model, pipe, thr=E2E_THR), [r["img"] for r in recs], [r["sents"] for r in recs]


@pytest.mark.parametrize("smooth", [None, Smooth(open=1, close=1, fill_holes=True)], ids=["raw", "smoothed"])
@pytest.mark.parametrize("spec", [None, Components(keep="largest")], ids=["plain", "largest"])
def test_predictor_polygon_equals_host_masks(tiny, spec, smooth):
    pr, files, exprs = tiny
    host = _flat(pr.predict(files, exprs, images_per_batch=2, masks="host", components=spec, smooth=smooth))
    got = _flat(pr.predict(files, exprs, images_per_batch=2, masks="polygon", components=spec, smooth=smooth))
    assert len(got) == len(host) == 9 and any(0 < p.area < p.mask.size for p in host)
    for k, (p, q) in enumerate(zip(got, host)):
        assert type(p) is type(q) is (predict.Prediction if spec is None and smooth is None else predict.ComponentPrediction)
        h, w = q.mask.shape
        print("expr %d  %3d x %3d  area %5d  box %s  %d rings of %d vertices" % (k, h, w, p.area, p.box, len(p.mask["rings"]),
                                                                                sum(len(r) for r in p.mask["rings"])))
        assert isinstance(p.mask, dict) and p.mask["size"] == [h, w]
        assert np.array_equal(polygon.decode(p.mask), q.mask)               # byte for byte
        assert _same(p.mask, polygon.encode(q.mask))
        assert p[:1] + p[2:] == q[:1] + q[2:]                               # every other field
        assert polygon.area(p.mask) == p.area and polygon.to_bbox(p.mask) == p.box
    entries = predict.coco_results(pr.predict(files[:2], exprs[:2], images_per_batch=2, masks="polygon", components=spec, smooth=smooth), ["a", "b"])
    assert [e["image_id"] for e in entries] == ["a", "b", "b"] and json.loads(json.dumps(entries)) == entries
    for e, q in zip(entries, host):
        assert e["segmentation"] == polygon.to_coco(polygon.encode(q.mask)) and e["area"] == q.area and e["score"] == q.score
        assert e["bbox"] == ([q.box[0], q.box[1], q.box[2] - q.box[0], q.box[3] - q.box[1]] if q.box else [0, 0, 0, 0])


def test_library_calls_of_every_mask_mode(tiny, monkeypatch):
    pr, files, exprs = tiny
    spec = Components(keep="largest")
    plain = ["cris_predict_masks_batch"]
    cleaned = ["cris_predict_masks_batch", "cris_label_components", "cris_filter_components"]
    for components, post in ((None, plain), (spec, cleaned)):
        calls = {}
        for mode in ("host", "device", None, "rle", "polygon"):
            out, calls[mode] = _recorded(monkeypatch, lambda: pr.predict(files, exprs, images_per_batch=2, masks=mode, components=components))
            if mode == "host":
                areas = [[p.area for p in x] for x in out]
        for mode in ("host", "device", None):                               # what they issued before there was an encoder or a tracer
            assert calls[mode] == calls["host"] and not any("rle" in c or "polygon" in c for c in calls[mode]), mode
            assert [c for c in calls[mode] if c in cleaned] == post * 3, mode
        # "rle": the same sequence with ONE encode per batch, after the last launch that writes the masks; no polygon call
        want, seen = [], 0
        for c in calls["host"]:
            want.append(c)
            if c == post[-1]:
                want.append("cris_rle_encode")
                seen += 1
        assert calls["rle"] == want and seen == 3 and calls["rle"].count("cris_rle_encode") == 3
        # "polygon": ONE count per batch at the same place, and one trace per batch that has foreground
        foreground = [any(a > 0 for x in areas[lo:lo + 2] for a in x) for lo in range(0, len(areas), 2)]
        assert len(foreground) == 3 and any(foreground)
        want, batch = [], 0
        for c in calls["host"]:
            want.append(c)
            if c == post[-1]:
                want += ["cris_polygon_count"] + ["cris_polygon_trace"] * foreground[batch]
                batch += 1
        assert calls["polygon"] == want and batch == 3 and not any("rle" in c for c in calls["polygon"])


def test_command_line_writes_the_polygon_file(tmp_path):
    from PIL import Image
    image = tmp_path / "street.jpg"
    image.write_bytes(_predict_records()[0]["img"])
    prefix, path = str(tmp_path / "out" / "m"), str(tmp_path / "res" / "polygons.json")
    args = ["--synthetic", "tiny", "--size", "96", "--thr", str(E2E_THR), "--image", str(image), "--expr", "the left one", "--expr", "zebra closest 2 us"]
    out = predict.main(args + ["--out-prefix", prefix, "--polygon-json", path])
    with open(path) as f:
        entries = json.load(f)
    assert len(entries) == len(out) == 2 and [e["sentence"] for e in entries] == ["the left one", "zebra closest 2 us"]
    for j, (e, p) in enumerate(zip(entries, out)):
        png = np.array(Image.open("%s_%d.png" % (prefix, j)))
        assert list(e) == ["image_id", "sentence", "segmentation", "bbox", "area", "score"] and e["image_id"] == "street.jpg"
        full = polygon.encode(png)
        assert e["segmentation"] == polygon.to_coco(full) and np.array_equal(png, p.mask)
        rings = [np.array(r, np.int32).reshape(-1, 2) for r in e["segmentation"]]
        filled = polygon.decode({"size": list(png.shape), "rings": rings, "holes": [False] * len(rings)})
        # the file holds the outer rings: it decodes to the PNG where the mask has no holes, and to the PNG with its holes filled otherwise
        holes = [r for r, hole in zip(full["rings"], full["holes"]) if hole]
        if not holes:
            assert np.array_equal(filled, png)
        assert np.array_equal(polygon.decode(dict(full, rings=rings + holes, holes=[False] * len(rings) + [True] * len(holes))), png)
        assert e["area"] == p.area == int((png != 0).sum()) and e["score"] == p.score
    # the file alone, under a chosen id, holes filled on the device so that every entry decodes to the mask itself
    only = predict.main(args + ["--polygon-json", str(tmp_path / "only.json"), "--image-id", "42", "--keep", "largest", "--fill-holes"])
    with open(tmp_path / "only.json") as f:
        again = json.load(f)
    assert not (tmp_path / "None_0.png").exists() and [e["image_id"] for e in again] == ["42", "42"]
    for p, e in zip(only, again):
        assert isinstance(p, predict.ComponentPrediction) and polygon.area(p.mask) == e["area"] and not any(p.mask["holes"])
        assert e["segmentation"] == polygon.to_coco(p.mask) and int((polygon.decode(p.mask) != 0).sum()) == e["area"]
