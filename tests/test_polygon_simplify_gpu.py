"""Douglas-Peucker simplification of traced rings on the GPU (csrc/simplify.hip behind evalpost.polygon_collect(..., simplify=epsilon);
DESIGN.md 9b) against the recursive oracle of tests/simplify_cases.py: every ring, every vertex, the ring table and the header as
equalities at every epsilon; what the launches must leave alone; the buffers' stated sizes; a rerun over dirty scratch.  Then the
library calls with and without `simplify`, and predict.Predictor with masks="polygon", simplify=1.0 on the tiny synthetic model
against polygon.simplify of its own unsimplified result, `coco_results` and the command line's results file."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

pytest.importorskip("PIL")

import polygon_cases as PC  # noqa: E402
import simplify_cases as SC  # noqa: E402
from cris.pytorch_amd import evalpost, hip, polygon, predict  # noqa: E402
from cris.pytorch_amd.evalpost import Components, Smooth  # noqa: E402
from test_polygon_gpu import DEV, FILL, _filled, _flat, _pack, _recorded, tiny  # noqa: E402,F401
from test_predict_gpu import E2E_THR  # noqa: E402
from test_predict_gpu import _records as _predict_records  # noqa: E402

NAMES = [k for k, _ in SC.cases()]


@pytest.fixture(scope="module")
def batch():
    st, buf = _pack([m for _, m in SC.cases()], alias=NAMES.index(PC.ALIAS))
    return st, buf, list(range(len(NAMES))) + [NAMES.index(PC.ALIAS)]


def test_simplified_batch_equals_the_oracle_at_every_epsilon(batch):
    st, buf, case_of = batch
    n = st.n
    assert n == len(SC.cases()) + 1
    traced = [SC.traced_dict(i) for i in case_of]
    need, nrings = sum(len(r) for p in traced for r in p["rings"]), sum(len(p["rings"]) for p in traced)
    ring_cap = need // 4
    before = buf.clone()
    work = evalpost.polygon_work(st, DEV)
    totals = evalpost.polygon_count_batch(buf, st, work=work)
    lib = hip.load()
    tw_words, out_words = (lib.cris_polygon_trace_work_bytes(need, n) + 7) // 8, 2 + 4 * ring_cap + need
    sw_words, so_words = (lib.cris_polygon_simplify_work_bytes(need, ring_cap) + 7) // 8, 4 + 5 * ring_cap + need
    # sentinel-filled over-allocations of every buffer the launches write
    bufs = evalpost.PolygonBuffers(trace_work=_filled(tw_words + 32), out=_filled(out_words + 32), simplify_work=_filled(sw_words + 32),
                                   simplified=_filled(so_words + 32))
    held = (bufs.trace_work, bufs.out, bufs.simplify_work, bufs.simplified)
    plain = evalpost.polygon_collect(buf, st, totals, work=work, buffers=bufs)
    assert all(SC.same(p, q) for p, q in zip(plain, traced)) and bufs.spans == (tw_words, out_words) and bufs.header is None
    traced_words = bufs.out[:out_words].cpu().numpy().copy()                # what the trace leaves: the simplifier's input
    assert (bufs.simplify_work == FILL).all() and (bufs.simplified == FILL).all()      # simplify=None touches neither
    flat_rings = [r for p in traced for r in p["rings"]]
    for eps in SC.EPSILONS:
        want = [SC.expected(eps)[i] for i in case_of]
        got = evalpost.polygon_collect(buf, st, totals, work=work, buffers=bufs, simplify=eps)
        assert all(a is b for a, b in zip((bufs.trace_work, bufs.out, bufs.simplify_work, bufs.simplified), held))     # reused, not grown
        assert bufs.spans == (tw_words, out_words, sw_words, so_words)
        for i, p, q in zip(case_of, got, want):
            assert SC.same(p, q), (NAMES[i], eps)                           # every ring, every vertex, the holes, epsilon
        # the table: descriptor, offset, length, 2 A of the simplified ring, hole flag of the traced ring; vertices packed in ring order
        table, at = [], 0
        for d, q in enumerate(want):
            for r, hole in zip(q["rings"], q["holes"]):
                table.append([d, at, len(r), PC.oracle_twice_area([tuple(v) for v in r.tolist()]), int(hole)])
                at += len(r)
        kept_rings = len(table)
        rounds = []
        polygon.simplify_kept(flat_rings, int(4 * eps), rounds)
        print("epsilon %5.2f  %5d rings of %6d vertices -> %5d rings of %6d vertices, %2d rounds" % (eps, nrings, need, kept_rings, at, rounds[0]))
        assert bufs.table.tolist() == table
        assert np.array_equal(bufs.vertices, np.concatenate([r for q in want for r in q["rings"]] + [np.zeros((0, 2), np.int32)]))
        assert bufs.header.tolist() == [kept_rings, at, nrings, rounds[0], need]
        words = bufs.simplified.cpu().numpy()
        assert words[:4].tolist() == [kept_rings, at, nrings, rounds[0]]
        assert (words[4 + 5 * kept_rings:4 + 5 * ring_cap] == FILL).all()   # no row beyond the last ring
        assert (words[4 + 5 * ring_cap + at:] == FILL).all()                # no vertex beyond the last kept one, nothing beyond the stated size
        assert (bufs.simplify_work[sw_words:] == FILL).all() and (bufs.trace_work[tw_words:] == FILL).all() and (bufs.out[out_words:] == FILL).all()
        assert torch.equal(buf, before)                                     # the masks are only read
        assert np.array_equal(bufs.out[:out_words].cpu().numpy(), traced_words)       # ... and so are the traced rings, table and header
        # a second run over dirty scratch and outputs, the buffers reused: the same words
        first = words.copy()
        for b in held:
            b.fill_(-1)
        again = evalpost.polygon_collect(buf, st, totals, work=work, buffers=bufs, simplify=eps)
        assert all(SC.same(p, q) for p, q in zip(again, want))
        now = bufs.simplified.cpu().numpy()
        assert np.array_equal(now[:4 + 5 * kept_rings], first[:4 + 5 * kept_rings])
        assert np.array_equal(now[4 + 5 * ring_cap:4 + 5 * ring_cap + at], first[4 + 5 * ring_cap:4 + 5 * ring_cap + at])
        assert (now[4 + 5 * kept_rings:4 + 5 * ring_cap] == -1).all() and (now[4 + 5 * ring_cap + at:] == -1).all()
        assert (bufs.simplify_work[sw_words:] == -1).all()
        for b in held:
            b.fill_(FILL)
    # fresh default buffers, the count run again inside collect
    fresh = evalpost.polygon_collect(buf, st, evalpost.polygon_count_batch(buf, st), simplify=2)
    assert all(SC.same(p, SC.expected(2)[i]) for i, p in zip(case_of, fresh))
    with pytest.raises(ValueError, match="multiple of 0.25"):
        evalpost.polygon_collect(buf, st, totals, work=work, simplify=0.3)


def test_every_comb_alone_crosses_the_wave_and_lds_edges():
    """one batch per ring: 2 below, at and above the wave / block switch (256) and the LDS capacity (4096) among the combs, the
    serpentine, the rectangle at its equality and the anchor tie"""
    bufs = evalpost.PolygonBuffers()
    masks = [PC.comb(v) for v in PC.COMB_SIZES] + [PC.serpentine(), SC.rectangle(), SC.anchor_tie()]
    assert {SC.WAVE_RING - 2, SC.WAVE_RING, SC.WAVE_RING + 2, SC.LDS_RING - 2, SC.LDS_RING, SC.LDS_RING + 2} <= set(PC.COMB_SIZES)
    for m in masks:
        st, buf = _pack([m])
        work = evalpost.polygon_work(st, DEV)
        totals = evalpost.polygon_count_batch(buf, st, work=work)
        rings, _ = PC.oracle_trace(m)
        assert len(rings) == 1
        for eps in (0.25, 1, 2, 11.75, 12):
            got = evalpost.polygon_collect(buf, st, totals, work=work, buffers=bufs, simplify=eps)
            want = SC.oracle_simplify(rings, [False], m.shape, eps)
            assert len(got) == 1 and SC.same(got[0], want), (m.shape, eps)
            rounds = []
            polygon.simplify_kept([np.array(rings[0], np.int32)], int(4 * eps), rounds)
            kept = sum(len(r) for r in want["rings"])
            assert bufs.header.tolist() == [len(want["rings"]), kept, 1, rounds[0], len(rings[0])]
            assert bufs.table.tolist() == [[0, 0, kept, PC.oracle_twice_area([tuple(v) for v in r.tolist()]), 0] for r in want["rings"]]


def test_a_side_above_32767_is_refused_before_any_device_work(monkeypatch):
    st, buf = _pack([np.zeros((1, 32768), np.uint8)])
    names, real = [], hip.call
    monkeypatch.setattr(hip, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    work = evalpost.polygon_work(st, DEV)
    totals = evalpost.polygon_count_batch(buf, st, work=work)
    bufs = evalpost.PolygonBuffers()
    with pytest.raises(ValueError, match="<= 32767"):
        evalpost.polygon_collect(buf, st, totals, work=work, buffers=bufs, simplify=1)
    assert evalpost.polygon_collect(buf, st, totals, work=work, buffers=bufs) == [{"size": [1, 32768], "rings": [], "holes": []}]      # unsimplified: as before
    monkeypatch.undo()
    assert names == ["cris_polygon_count"] and bufs.simplify_work is None and bufs.simplified is None


def test_a_batch_of_background_issues_no_trace_and_no_simplify(monkeypatch):
    st, buf = _pack([np.zeros((5, 7), np.uint8), np.zeros((PC.RB + 1, PC.CG + 1), np.uint8)])
    names, real = [], hip.call
    monkeypatch.setattr(hip, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    work = evalpost.polygon_work(st, DEV)
    totals = evalpost.polygon_count_batch(buf, st, work=work)
    bufs = evalpost.PolygonBuffers()
    got = evalpost.polygon_collect(buf, st, totals, work=work, buffers=bufs, simplify=1.0)
    monkeypatch.undo()
    assert names == ["cris_polygon_count"]
    assert got == [{"size": [5, 7], "rings": [], "holes": [], "epsilon": 1.0}, {"size": [PC.RB + 1, PC.CG + 1], "rings": [], "holes": [], "epsilon": 1.0}]
    assert bufs.trace_work is None and bufs.out is None and bufs.simplify_work is None and bufs.simplified is None     # nothing was allocated


def test_library_calls_with_and_without_simplify(tiny, monkeypatch):  # noqa: F811
    pr, files, exprs = tiny
    pr.predict(files, exprs, images_per_batch=2, masks="host")              # (the model's first call packs its weights)
    for components in (None, Components(keep="largest")):
        base, calls = _recorded(monkeypatch, lambda: pr.predict(files, exprs, images_per_batch=2, masks="polygon", components=components))
        none, calls_none = _recorded(monkeypatch, lambda: pr.predict(files, exprs, images_per_batch=2, masks="polygon", components=components, simplify=None))
        assert calls_none == calls and not any("simplify" in c for c in calls) and calls.count("cris_polygon_trace") >= 1    # exactly today's calls
        assert pr._pg_buffers.simplify_work is None and pr._pg_buffers.simplified is None and pr.simplify_info is None       # ... and allocations
        out, with_eps = _recorded(monkeypatch, lambda: pr.predict(files, exprs, images_per_batch=2, masks="polygon", components=components, simplify=1.0))
        want = []
        for c in calls:
            want.append(c)
            if c == "cris_polygon_trace":
                want.append("cris_polygon_simplify")                        # one after each trace, nothing else changes
        assert with_eps == want and with_eps.count("cris_polygon_simplify") == calls.count("cris_polygon_trace")
        pr._pg_buffers = None


@pytest.mark.parametrize("post", [(None, None), (Components(keep="largest"), None), (None, Smooth(open=1, close=1, fill_holes=True))],
                         ids=["plain", "largest", "smoothed"])
def test_predictor_simplified_polygons_equal_the_host_simplifier(tiny, post):  # noqa: F811
    pr, files, exprs = tiny
    spec, smooth = post
    exact = _flat(pr.predict(files, exprs, images_per_batch=2, masks="polygon", components=spec, smooth=smooth))
    got = _flat(pr.predict(files, exprs, images_per_batch=2, masks="polygon", components=spec, smooth=smooth, simplify=1.0))
    assert len(got) == len(exact) == 9 and any(p.mask["rings"] for p in exact)
    before = (sum(len(p.mask["rings"]) for p in exact), sum(len(r) for p in exact for r in p.mask["rings"]))
    after = (sum(len(p.mask["rings"]) for p in got), sum(len(r) for p in got for r in p.mask["rings"]))
    print("rings, vertices: %s exact -> %s at epsilon 1" % (before, after))
    assert pr.simplify_info == before and after[1] < before[1]
    for p, q in zip(got, exact):
        assert type(p) is type(q) and "epsilon" not in q.mask
        assert SC.same(p.mask, polygon.simplify(q.mask, 1.0))               # the device equals the host route it replaces
        assert p[:1] + p[2:] == q[:1] + q[2:]                               # every other field: area, box and score are the mask's own
        assert polygon.validate(p.mask) == tuple(q.mask["size"])
    out = pr.predict(files[:2], exprs[:2], images_per_batch=2, masks="polygon", components=spec, smooth=smooth, simplify=1.0)
    entries = predict.coco_results(out, ["a", "b"])
    assert [e["image_id"] for e in entries] == ["a", "b", "b"] and json.loads(json.dumps(entries)) == entries
    for e, p, q in zip(entries, _flat(out), exact):
        assert e["segmentation"] == polygon.to_coco(polygon.simplify(q.mask, 1.0)) and e["area"] == q.area and e["score"] == q.score
    # the constructor's default applies to polygons alone; the call's None overrides it
    pr2 = predict.Predictor(pr.model, pr.pipe, thr=E2E_THR, components=spec, smooth=smooth, simplify=1.0)
    assert all(SC.same(p.mask, g.mask) for p, g in zip(_flat(pr2.predict(files, exprs, images_per_batch=2, masks="polygon")), got))
    assert all(SC.same(p.mask, q.mask) for p, q in zip(_flat(pr2.predict(files, exprs, images_per_batch=2, masks="polygon", simplify=None)), exact))
    assert all(isinstance(p.mask, np.ndarray) for p in _flat(pr2.predict(files, exprs, images_per_batch=2, masks="host")))
    with pytest.raises(ValueError, match="only with masks='polygon'"):
        pr.predict(files, exprs, images_per_batch=2, masks="rle", simplify=1.0)


def test_command_line_writes_the_simplified_polygon_file(tmp_path, capsys):
    image = tmp_path / "street.jpg"
    image.write_bytes(_predict_records()[0]["img"])
    args = ["--synthetic", "tiny", "--size", "96", "--thr", str(E2E_THR), "--image", str(image), "--expr", "the left one", "--expr", "zebra closest 2 us"]
    exact = predict.main(args + ["--polygon-json", str(tmp_path / "exact.json")])
    capsys.readouterr()
    path = str(tmp_path / "res" / "simplified.json")
    out = predict.main(args + ["--polygon-json", path, "--simplify", "1"])
    line = capsys.readouterr().out.strip().splitlines()[-1]
    with open(path) as f:
        entries = json.load(f)
    assert len(entries) == len(out) == 2 and [e["sentence"] for e in entries] == ["the left one", "zebra closest 2 us"]
    for e, p, q in zip(entries, out, exact):
        assert list(e) == ["image_id", "sentence", "segmentation", "bbox", "area", "score"] and e["image_id"] == "street.jpg"
        assert SC.same(p.mask, polygon.simplify(q.mask, 1.0)) and e["segmentation"] == polygon.to_coco(p.mask)
        assert e["area"] == p.area == q.area and e["score"] == p.score == q.score
    before = (sum(len(p.mask["rings"]) for p in exact), sum(len(r) for p in exact for r in p.mask["rings"]))
    after = (sum(len(p.mask["rings"]) for p in out), sum(len(r) for p in out for r in p.mask["rings"]))
    assert line == "%s\t2 expressions\tepsilon 1\t%d rings of %d vertices before\t%d rings of %d vertices after" % ((path,) + before + after)
