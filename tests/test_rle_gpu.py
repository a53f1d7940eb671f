"""COCO run-length encoding on the GPU (csrc/rle.hip behind evalpost.rle_encode_batch / rle_collect) against the
per-pixel oracle of tests/rle_cases.py: totals, every transition position and every string, as equalities; what the launch must
leave alone; the capacity rule.  Then predict.Predictor with masks="rle" on the tiny synthetic model against its own masks="host"
result, the library calls each mask mode issues, and the command line's results file."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

pytest.importorskip("PIL")

import rle_cases as RC  # noqa: E402
from cris.pytorch_amd import evalpost, hip, predict, records, rle  # noqa: E402
from cris.pytorch_amd.evalpost import Components  # noqa: E402
from cris.pytorch_amd.infer import InferenceRunner  # noqa: E402
from test_infer_multi_gpu import _setup  # noqa: E402
from test_predict_gpu import E2E_THR, SIZE, WORD_LEN, _KeepSegment  # noqa: E402
from test_predict_gpu import _records as _predict_records  # noqa: E402
from test_records_gpu import _StandInTokenizer  # noqa: E402

DEV = torch.device("cuda:0")
IDENT = np.array([[1.0, 0, 0], [0, 1.0, 0]], np.float64)
FILL = 0x7F7F7F7F


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
        assert (d.h_out, d.w_out, d.pitch) == (m.shape[0], m.shape[1], RC.pitch_of(m.shape[1]))
        host[d.out_off:d.out_off + d.pitch * d.h_out].reshape(d.h_out, d.pitch)[:, :d.w_out] = m
    return st, torch.from_numpy(host).to(DEV)


@pytest.fixture(scope="module")
def batch():
    names = [k for k, _ in RC.cases()]
    st, buf = _pack([m for _, m in RC.cases()], alias=names.index(RC.ALIAS))
    want = list(RC.expected()) + [RC.expected()[names.index(RC.ALIAS)]]
    return st, buf, names + [RC.ALIAS + " (the same rectangle)"], want


class _ShortBuffer:
    """a staging's descriptors under another out_bytes"""

    def __init__(self, st, out_bytes):
        self.descs, self.dev, self.n, self.out_bytes = st.descs, st.dev, st.n, out_bytes


def test_rle_encode_batch_equals_the_oracle(batch):
    st, buf, names, want = batch
    n = st.n
    assert n == len(RC.cases()) + 1 and st.descs[n - 1].out_off == st.descs[names.index(RC.ALIAS)].out_off
    pixels = evalpost.rle_pixels(st)
    need = sum(len(P) for P, _, _ in want)
    before = buf.clone()
    store = torch.full((pixels + 16,), FILL, dtype=torch.int32, device=DEV)
    runs, totals = evalpost.rle_encode_batch(buf, st, runs=store)
    assert runs.data_ptr() == store.data_ptr() and totals.dtype == torch.int64 and totals.shape == (n + 1,) and totals.is_cuda
    t, words = totals.cpu().numpy(), store.cpu().numpy().view(np.uint32)
    at = 0
    for i, (name, (P, counts, _)) in enumerate(zip(names, want)):
        d = st.descs[i]
        print("%-36s %3d x %3d  positions %6d (oracle %6d)" % (name, d.h_out, d.w_out, t[i], len(P)))
        assert t[i] == len(P), name
        assert words[at:at + len(P)].tolist() == P, name                    # every position, in order, packed
        at += len(P)
    assert t[n] == need == at
    assert (words[need:] == FILL).all() and need < pixels                   # nothing past the last position
    assert torch.equal(buf, before)                                         # the masks are only read
    a, b = names.index("random 0.5"), names.index("random 0.5 again")
    assert st.descs[a].out_off != st.descs[b].out_off and want[a] == want[b]
    # a second run into a fresh default buffer, dirty scratch reused: the same words
    work = evalpost.rle_work(st, DEV)
    work.fill_(-1)
    runs2, totals2 = evalpost.rle_encode_batch(buf, st, work=work)
    assert runs2.numel() == pixels and torch.equal(totals2, totals) and torch.equal(runs2[:need], store[:need])
    # the read: two copies, the strings of the whole batch
    got = evalpost.rle_collect(runs, totals, st)
    assert got == [{"size": [st.descs[i].h_out, st.descs[i].w_out], "counts": s} for i, (_, _, s) in enumerate(want)]
    for (name, m), r in zip(RC.cases(), got):
        assert r == rle.encode(m) and np.array_equal(rle.decode(r), (m != 0).astype(np.uint8) * 255), name
    with pytest.raises(ValueError, match="masks_u8"):
        evalpost.rle_encode_batch(buf[:st.out_bytes - 1], st)
    with pytest.raises(ValueError, match="runs must be"):
        evalpost.rle_encode_batch(buf, st, runs=store.to(torch.int64))
    with pytest.raises(hip.HipLibraryError, match="output outside the buffer"):
        short = _ShortBuffer(st, out_bytes=st.descs[n - 2].out_off)             # the library checks every rectangle against mask_bytes
        evalpost.rle_encode_batch(buf, short, runs=store)


def test_capacity_rule():
    yy, xx = np.mgrid[0:45, 0:67]
    board = (((yy + xx + 1) & 1) * 255).astype(np.uint8)                    # h odd, (0, 0) foreground: every pixel a transition
    boards = [255 - board[:33, :5], np.zeros((3, 3), np.uint8), board[:40, :64], board]
    st, buf = _pack(boards)
    P = [RC.oracle_positions(m) for m in boards]
    need = sum(len(p) for p in P)
    assert [len(p) for p in P] == [33 * 5 - 1, 0, 40 * 64 - 63, 45 * 67]    # (h even: a column's top continues the run above)
    cap = need // 2 + 3                                                     # ends inside the last board's list
    assert sum(len(p) for p in P[:3]) < cap < need
    store = torch.full((need + 64,), FILL, dtype=torch.int32, device=DEV)
    runs, totals = evalpost.rle_encode_batch(buf, st, runs=store[:cap])
    t, words = totals.cpu().numpy(), store.cpu().numpy().view(np.uint32)
    assert t.tolist() == [len(p) for p in P] + [need]                       # the true totals, whatever fitted
    assert (words[cap:] == FILL).all()                                      # nothing at or beyond runs + run_words
    assert words[:cap].tolist() == [v for p in P for v in p][:cap]          # every position that fits its slot
    with pytest.raises(RuntimeError, match="pass masks_u8"):
        evalpost.rle_collect(runs, totals, st)
    got = evalpost.rle_collect(runs, totals, st, masks_u8=buf)              # grows the buffer and encodes once more
    assert got == [rle.encode(m) for m in boards]
    assert (store.cpu().numpy().view(np.uint32)[cap:] == FILL).all()
    # a buffer of one word: the first position alone
    one = torch.full((8,), FILL, dtype=torch.int32, device=DEV)
    _, totals = evalpost.rle_encode_batch(buf, st, runs=one[:1])
    assert int(totals[-1]) == need and one.cpu().numpy().tolist() == [P[0][0]] + [FILL] * 7 and P[0][0] == 1


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


@pytest.mark.parametrize("spec", [None, Components(keep="largest")], ids=["plain", "largest"])
def test_predictor_rle_equals_host_masks(tiny, spec):
    pr, files, exprs = tiny
    host = _flat(pr.predict(files, exprs, images_per_batch=2, masks="host", components=spec))
    got = _flat(pr.predict(files, exprs, images_per_batch=2, masks="rle", components=spec))
    assert len(got) == len(host) == 9 and any(0 < p.area < p.mask.size for p in host)
    for k, (p, q) in enumerate(zip(got, host)):
        assert type(p) is type(q) is (predict.Prediction if spec is None else predict.ComponentPrediction)
        h, w = q.mask.shape
        print("expr %d  %3d x %3d  area %5d  box %s  %d bytes of RLE" % (k, h, w, p.area, p.box, len(p.mask["counts"])))
        assert isinstance(p.mask, dict) and p.mask["size"] == [h, w] and isinstance(p.mask["counts"], bytes)
        assert np.array_equal(rle.decode(p.mask), q.mask)                   # byte for byte
        assert p.mask == rle.encode(q.mask)
        assert p[:1] + p[2:] == q[:1] + q[2:]                               # every other field
        assert rle.area(p.mask) == p.area and rle.to_bbox(p.mask) == p.box
    entries = predict.coco_results(pr.predict(files[:2], exprs[:2], images_per_batch=2, masks="rle", components=spec), ["a", "b"])
    assert [e["image_id"] for e in entries] == ["a", "b", "b"] and json.loads(json.dumps(entries)) == entries
    for e, q in zip(entries, host):
        assert np.array_equal(rle.decode(e["segmentation"]), q.mask) and e["area"] == q.area and e["score"] == q.score
        assert e["bbox"] == ([q.box[0], q.box[1], q.box[2] - q.box[0], q.box[3] - q.box[1]] if q.box else [0, 0, 0, 0])


def test_library_calls_of_every_mask_mode(tiny, monkeypatch):
    pr, files, exprs = tiny
    spec = Components(keep="largest")
    plain = ["cris_predict_masks_batch"]
    cleaned = ["cris_predict_masks_batch", "cris_label_components", "cris_filter_components"]
    for components, post in ((None, plain), (spec, cleaned)):
        calls = {}
        for mode in ("host", "device", None, "rle"):
            _, calls[mode] = _recorded(monkeypatch, lambda: pr.predict(files, exprs, images_per_batch=2, masks=mode, components=components))
        for mode in ("host", "device", None):                               # what they issued before there was an encoder
            assert calls[mode] == calls["host"] and not any("rle" in c for c in calls[mode]), mode
            assert [c for c in calls[mode] if c in cleaned] == post * 3, mode
        # "rle": the same sequence with ONE encode per batch, after the last launch that writes the masks
        want, seen = [], 0
        for c in calls["host"]:
            want.append(c)
            if c == post[-1]:
                want.append("cris_rle_encode")
                seen += 1
        assert calls["rle"] == want and seen == 3 and calls["rle"].count("cris_rle_encode") == 3


def test_command_line_writes_the_results_file(tmp_path):
    from PIL import Image
    image = tmp_path / "street.jpg"
    image.write_bytes(_predict_records()[0]["img"])
    prefix, path = str(tmp_path / "out" / "m"), str(tmp_path / "res" / "results.json")
    args = ["--synthetic", "tiny", "--size", "96", "--thr", str(E2E_THR), "--image", str(image), "--expr", "the left one", "--expr", "zebra closest 2 us"]
    out = predict.main(args + ["--out-prefix", prefix, "--rle-json", path])
    with open(path) as f:
        entries = json.load(f)
    assert len(entries) == len(out) == 2 and [e["sentence"] for e in entries] == ["the left one", "zebra closest 2 us"]
    for j, (e, p) in enumerate(zip(entries, out)):
        png = np.array(Image.open("%s_%d.png" % (prefix, j)))
        assert list(e) == ["image_id", "sentence", "segmentation", "bbox", "area", "score"] and e["image_id"] == "street.jpg"
        assert np.array_equal(rle.decode(e["segmentation"]), png) and np.array_equal(png, p.mask)
        assert e["area"] == p.area == int((png != 0).sum()) and e["score"] == p.score
    # the file alone, under a chosen id
    only = predict.main(args + ["--rle-json", str(tmp_path / "only.json"), "--image-id", "42", "--keep", "largest"])
    with open(tmp_path / "only.json") as f:
        again = json.load(f)
    assert not (tmp_path / "None_0.png").exists() and [e["image_id"] for e in again] == ["42", "42"]
    assert all(isinstance(p, predict.ComponentPrediction) and rle.area(p.mask) == e["area"] for p, e in zip(only, again))
