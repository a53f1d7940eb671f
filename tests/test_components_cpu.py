"""Host side of the connected-component clean-up (evalpost.Components, csrc/evalpost.hip cris_label_components /
cris_filter_components / cris_mask_iou_batch): the spec's validation, the test oracle against scipy, the argument checks
of predict / validate that run before any device work, the launchers' rejections through the library, and the ABI bookkeeping of the
new symbols.  No GPU."""
import ctypes as C
import os
import re
from types import SimpleNamespace as NS

import numpy as np
import pytest

import components_cases as CC
from test_predict_cpu import _NoDevice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cris_hip.h")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()


def test_spec_validation_and_noop_is_none():
    from cris.pytorch_amd.evalpost import Components, components_spec
    s = Components()
    assert (s.keep, s.min_area, s.connectivity) == ("all", 0, 8) and s.is_noop
    s = Components(keep="largest", min_area=np.int64(7), connectivity=4)
    assert (s.keep, s.min_area, s.connectivity) == ("largest", 7, 4) and type(s.min_area) is int and not s.is_noop
    assert s == Components("largest", 7, 4) and s != Components("largest", 7, 8) and hash(s) == hash(Components("largest", 7, 4))
    assert "largest" in repr(s) and "7" in repr(s)
    with pytest.raises(AttributeError):
        s.keep = "all"
    for kw in (dict(keep="biggest"), dict(keep=None), dict(keep="Largest"), dict(min_area=-1), dict(min_area=2.0), dict(min_area="3"),
               dict(min_area=True), dict(min_area=None), dict(connectivity=6), dict(connectivity="8"), dict(connectivity=None),
               dict(connectivity=True)):
        with pytest.raises(ValueError, match="Components"):
            Components(**kw)
    # a spec that filters nothing is no spec
    assert components_spec(None) is None
    assert components_spec(Components()) is None and components_spec(Components("all", 1, 4)) is None
    assert components_spec(Components("all", 2)) == Components("all", 2)
    assert components_spec(Components("largest")) == Components("largest") and components_spec(Components("largest", 1)) is not None
    for bad in ("largest", 8, dict(keep="largest"), ("largest", 0, 8), True):
        with pytest.raises(ValueError, match="components"):
            components_spec(bad)


def test_oracle_on_small_masks_by_hand():
    m = np.array([[1, 0, 0, 1, 1],
                  [0, 1, 0, 0, 1],
                  [0, 0, 0, 0, 0],
                  [9, 9, 0, 0, 1]], np.uint8)                              # w = 5: pitch 8
    l8, l4 = CC.label(m, 8), CC.label(m, 4)
    assert l8.tolist() == [[0, -1, -1, 3, 3], [-1, 0, -1, -1, 3], [-1] * 5, [24, 24, -1, -1, 28]]
    assert l4.tolist() == [[0, -1, -1, 3, 3], [-1, 9, -1, -1, 3], [-1] * 5, [24, 24, -1, -1, 28]]
    assert CC.label(m, 8, pitch=5)[3].tolist() == [15, 15, -1, -1, 19]
    kept, info, _ = CC.filter_mask(m, "largest", 0, 8)
    assert info == [4, 1, 8, 0] and kept.sum() == 3 and kept[0, 3] and kept[1, 4]            # areas 2, 3, 2, 1
    kept, info, _ = CC.filter_mask(m, "largest", 0, 4)
    assert info == [5, 1, 8, 0] and kept.sum() == 3
    kept, info, _ = CC.filter_mask(m, "all", 2, 8)
    assert info == [4, 3, 8, 0] and kept.sum() == 7 and not kept[3, 4]
    kept, info, _ = CC.filter_mask(m, "largest", 4, 8)
    assert info == [4, 0, 8, 0] and not kept.any() and CC.stats_row(kept) == CC.PREDICT_INIT    # nothing survives: the empty row
    # the tie rule: equal areas -> the lowest canonical label
    t = np.array([[0, 0, 1, 1], [1, 1, 0, 0]], np.uint8)
    kept, info, _ = CC.filter_mask(t, "largest", 0, 4)
    assert info == [2, 1, 4, 0] and kept.tolist() == [[False, False, True, True], [False] * 4]
    assert CC.stats_row(kept, np.full((2, 4), 10, np.int64)) == [2, 20, 2, 0, 4, 1]
    with pytest.raises(ValueError):
        CC.label(m, 6)


def test_the_cases_are_what_they_were_chosen_for():
    cases = dict(CC.cases())
    n = {c: [CC.components(l)[0].size for l in CC.expected_labels(c)] for c in (4, 8)}
    names = [k for k, _ in CC.cases()]
    count = lambda name, c: n[c][names.index(name)]                        # noqa: E731
    assert count("empty", 4) == count("empty", 8) == 0 and count("full", 4) == 1
    assert cases["full"].shape[0] > 32 and cases["full"].shape[1] > 64      # several tiles in both directions
    assert [cases[k].shape for k in ("1x1", "1x37", "37x1")] == [(1, 1), (1, 37), (37, 1)]
    for w in (5, 6, 7):
        assert cases["width %d" % w].shape[1] == w != CC.pitch_of(w) and count("width %d" % w, 8) == 6       # the runs stay apart
    assert count("checkerboard", 8) == 1 and count("checkerboard", 4) == int((cases["checkerboard"] != 0).sum())
    assert count("spiral", 4) == count("spiral", 8) == 1 and count("comb", 4) == 1 and cases["spiral"].shape == (150, 200)
    assert count("stairs", 8) == 2 and count("stairs", 4) == 140
    assert count("tie", 8) == 3 and count("specks", 8) == 5
    areas = CC.components(CC.expected_labels(8)[names.index("tie")])
    assert sorted(areas[1].tolist()) == [11, 12, 12]
    assert CC.filter_mask(cases["tie"], "largest")[0][4, 36] and not CC.filter_mask(cases["tie"], "largest")[0][5, 2]      # the earlier row wins
    assert sorted(CC.components(CC.expected_labels(8)[names.index("specks")])[1].tolist()) == [1, 2, 3, 4, 5]
    assert CC.filter_mask(cases["specks"], "all", 3)[1] == [5, 3, 15, 0]    # below min_area goes, exactly min_area stays
    assert np.array_equal(cases["random 0.5"], cases["random 0.5 again"]) and count("random 0.3", 4) > 1000
    assert 10 <= len(names) <= 20


def test_oracle_equals_scipy_on_every_case():
    ndimage = pytest.importorskip("scipy.ndimage")
    for conn in (4, 8):
        structure = ndimage.generate_binary_structure(2, 1 if conn == 4 else 2)
        for (name, m), want in zip(CC.cases(), CC.expected_labels(conn)):
            lab, n = ndimage.label(m != 0, structure=structure)
            h, w = m.shape
            index = np.arange(h)[:, None] * CC.pitch_of(w) + np.arange(w)[None, :]
            assert np.array_equal(want >= 0, lab > 0), (name, conn)
            roots, areas = CC.components(want)
            assert roots.size == n, (name, conn)
            if n == 0:
                continue
            first = ndimage.minimum(index, lab, index=np.arange(1, n + 1)).astype(np.int64)       # first pixel in raster order
            assert np.array_equal(want[lab > 0], first[lab[lab > 0] - 1]), (name, conn)
            order = np.argsort(first)
            assert np.array_equal(roots, first[order]), (name, conn)
            assert np.array_equal(areas, ndimage.sum(m != 0, lab, index=np.arange(1, n + 1)).astype(np.int64)[order]), (name, conn)
            for spec in CC.SPECS:
                kept, info, _ = CC.filter_mask(m, connectivity=conn, **spec)
                ok = areas >= spec["min_area"]
                cand = roots[ok]
                if spec["keep"] == "largest" and cand.size:
                    best = areas[ok].max()
                    cand = cand[areas[ok] == best][:1]                     # (roots ascend: the first is the lowest label)
                assert info == [n, cand.size, int((m != 0).sum()), 0], (name, conn, spec)
                assert np.array_equal(kept, np.isin(want, cand) & (want >= 0)), (name, conn, spec)


def test_predict_and_validate_reject_bad_components_before_any_device_work():
    from cris.pytorch_amd import evalpost, evaluate, predict
    for bad in ("largest", 8, dict(keep="largest")):
        with pytest.raises(ValueError, match="components"):
            predict.Predictor(NS(), _NoDevice(), components=bad)
    p = predict.Predictor(NS(), _NoDevice(), thr=0.35, components=evalpost.Components())
    assert p.components is None                                             # a no-op spec is no spec
    p = predict.Predictor(NS(), _NoDevice(), thr=0.35, components=evalpost.Components("largest"))
    assert p.components == evalpost.Components("largest")
    jpg = b"\xff\xd8\xff\xe0fake"
    for bad in ("largest", "Default", 4, ("largest",), evalpost.Components):
        with pytest.raises(ValueError, match="components"):
            p.predict([jpg], ["a"], components=bad)
    with pytest.raises(ValueError, match="no images"):                      # the other checks still come before the device
        p.predict([], [], components=evalpost.Components("largest"))
    assert p._ring is None and p._cc_masks is None and p._cc_labels is None and p._cc_work is None
    assert predict._check_components("default", p.components) is p.components
    assert predict._check_components(None, p.components) is None and predict._check_components(evalpost.Components("all", 1), p.components) is None
    assert predict.ComponentPrediction._fields == ("sentence", "mask", "area", "box", "score", "n_components", "raw_area")
    assert predict.ComponentPrediction._fields[:5] == predict.Prediction._fields
    # the evaluator: the spec is checked first, before the pipeline's mode is even looked at
    ev = evaluate.Evaluator.__new__(evaluate.Evaluator)
    ev.pipe = _NoDevice("val")
    for call in (ev.validate, ev.inference):
        for bad in ("largest", 8, evalpost.Components):
            with pytest.raises(ValueError, match="components"):
                call([{}], components=bad)
    with pytest.raises(ValueError, match="mode 'test'"):
        ev.inference([{}], components=evalpost.Components("largest"))
    # the CLI's flags build the spec
    with pytest.raises(SystemExit):
        predict.main(["--image", "x.jpg", "--expr", "a", "--out-prefix", "p", "--keep", "biggest"])
    with pytest.raises(SystemExit):
        predict.main(["--image", "x.jpg", "--expr", "a", "--out-prefix", "p", "--connectivity", "6"])
    with pytest.raises(SystemExit):
        predict.main(["--image", "x.jpg", "--expr", "a", "--out-prefix", "p", "--min-area", "-2"])


def test_op_level_functions_check_their_arguments_first():
    import torch
    from cris.pytorch_amd import evalpost
    st = NS(out_bytes=64, n=1)
    cpu = torch.zeros(64, dtype=torch.uint8)
    for fn, args in ((evalpost.label_components, (cpu, st)), (evalpost.filter_components, (cpu, None, st, evalpost.Components("largest"), None, 0)),
                     (evalpost.mask_iou_batch, (cpu, st, cpu, None, 0))):
        with pytest.raises(RuntimeError, match="GPU only"):
            fn(*args)
    table = evalpost.check_component_info(np.array([[3, 1, 50, 0], [0, 0, 0, 0]]))
    assert table.shape == (2, 4)
    with pytest.raises(RuntimeError, match="iteration cap"):
        evalpost.check_component_info(np.array([[3, 1, 50, 0], [1, 0, 5, 1]]))
    assert evalpost.INFO_FIELDS == ("n_components", "kept_components", "raw_area", "error")


def test_launchers_reject_bad_arguments_on_the_host(built):
    """cris_label_components, cris_filter_components and cris_mask_iou_batch check their operands and every descriptor before any launch"""
    from cris.pytorch_amd import hip
    l = hip.load()
    d = (hip.EvalDesc * 1)()
    mat = (C.c_double * 6)(1, 0, 0, 0, 1, 0)

    def fill(w=5, h=4, map=0, pitch=None, out_off=0, row=0, mask_off=0):
        assert l.cris_eval_desc_fill(C.addressof(d), mat, w, h, map, mask_off, (w + 3) // 4 * 4 if pitch is None else pitch, out_off, row) == 0

    def label(masks=0x1000, mask_bytes=64, host=None, dev=0x2000, n=1, conn=8, labels=0x3000, words=64):
        host = C.addressof(d) if host is None else host
        return l.cris_label_components(masks, mask_bytes, host or None, dev, n, conn, labels, words, None)

    def filt(masks=0x1000, mask_bytes=64, labels=0x3000, words=64, host=None, dev=0x2000, n=1, largest=1, min_area=0, work=0x5000, work_bytes=1 << 12,
             info=0x4000, rows=4, probs=None, P=2, border=0.0, stats=None, stat_rows=4):
        host = C.addressof(d) if host is None else host
        return l.cris_filter_components(masks, mask_bytes, labels, words, host or None, dev, n, largest, min_area, work, work_bytes, info, rows,
                                        probs, P, 8, 8, border, stats, stat_rows, None)

    def iou(pred=0x1000, pred_bytes=64, host=None, dev=0x2000, n=1, gt=0x6000, gt_bytes=64, counts=0x7000, rows=4):
        host = C.addressof(d) if host is None else host
        return l.cris_mask_iou_batch(pred, pred_bytes, host or None, dev, n, gt, gt_bytes, counts, rows, None)

    def rejected(fn, name, msg, **kw):
        assert fn(**kw) != 0, (name, msg, kw)
        err = l.cris_last_error()
        assert name in err and msg in err, (kw, err)

    every = ((label, b"cris_label_components"), (filt, b"cris_filter_components"), (iou, b"cris_mask_iou_batch"))
    for fn, name in every:
        buf = "pred_bytes" if fn is iou else "mask_bytes"
        for pitch in (6, 4, 7):                                             # not a multiple of 4; below w_out; both
            fill(pitch=pitch)
            rejected(fn, name, b"pitch must be a multiple of 4")
        fill(w=0)
        rejected(fn, name, b"bad output size")
        fill(w=46341, h=46341)
        rejected(fn, name, b"bad output size")
        fill(out_off=64)                                                    # 8 x 4 bytes at 64 need 96
        rejected(fn, name, b"output outside the buffer", **{buf: 95, "words": 95} if fn is not iou else {buf: 95})
        fill(out_off=2)
        rejected(fn, name, b"output outside the buffer")
        fill(out_off=-16)
        rejected(fn, name, b"output outside the buffer")
        fill()
        rejected(fn, name, b"null operand", host=0)
        rejected(fn, name, b"null operand", dev=None)
        for n in (0, -1, 65536):
            rejected(fn, name, b"n must be in 1 .. 65535", n=n)
    fill()
    # labels
    rejected(label, b"cris_label_components", b"null operand", masks=None)
    rejected(label, b"cris_label_components", b"null operand", labels=None)
    for conn in (0, 6, -8, 5):
        rejected(label, b"cris_label_components", b"connectivity must be 4 or 8", conn=conn)
    rejected(label, b"cris_label_components", b"one word per mask byte", words=63)        # a label buffer shorter than out_bytes
    rejected(label, b"cris_label_components", b"aligned", masks=0x1002)
    rejected(label, b"cris_label_components", b"aligned", labels=0x3004)
    # filter
    for k in ("masks", "labels", "work", "info"):
        rejected(filt, b"cris_filter_components", b"null operand", **{k: None})
    rejected(filt, b"cris_filter_components", b"keep_largest must be 0 or 1", largest=2)
    rejected(filt, b"cris_filter_components", b"min_area >= 0", min_area=-1)
    rejected(filt, b"cris_filter_components", b"one word per mask byte", words=63)
    need = l.cris_filter_components_work_bytes(64, 1)
    assert need == 64 * 4 + 8 and l.cris_filter_components_work_bytes(61, 3) == 248 + 24
    rejected(filt, b"cris_filter_components", b"work buffer is too small", work_bytes=need - 1)
    rejected(filt, b"cris_filter_components", b"bad sizes", rows=0)
    rejected(filt, b"cris_filter_components", b"aligned", info=0x4004)
    rejected(filt, b"cris_filter_components", b"aligned", work=0x5008)
    rejected(filt, b"cris_filter_components", b"probs and stats go together", probs=0x8000)
    rejected(filt, b"cris_filter_components", b"probs and stats go together", stats=0x9000)
    rejected(filt, b"cris_filter_components", b"border must be finite", probs=0x8000, stats=0x9000, border=float("nan"))
    rejected(filt, b"cris_filter_components", b"aligned", probs=0x8000, stats=0x9004)
    for row, kw in ((4, {}), (-1, {}), (2, dict(probs=0x8000, stats=0x9000, stat_rows=2))):   # row0 inside BOTH tables
        fill(row=row)
        rejected(filt, b"cris_filter_components", b"row out of range", **kw)
    fill(map=2)
    rejected(filt, b"cris_filter_components", b"map out of range", probs=0x8000, stats=0x9000)
    # mask IoU
    fill()
    for k in ("pred", "gt", "counts"):
        rejected(iou, b"cris_mask_iou_batch", b"null operand", **{k: None})
    rejected(iou, b"cris_mask_iou_batch", b"bad sizes", rows=0)
    rejected(iou, b"cris_mask_iou_batch", b"aligned", gt=0x6001)
    fill(row=4)
    rejected(iou, b"cris_mask_iou_batch", b"row out of range")
    fill(mask_off=48)
    rejected(iou, b"cris_mask_iou_batch", b"mask outside the buffer")
    fill(mask_off=6)
    rejected(iou, b"cris_mask_iou_batch", b"mask outside the buffer")


def test_symbols_are_declared_bound_and_named_at_abi_8(built):
    from cris.pytorch_amd import hip
    src = open(HEADER).read()
    plain = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = {m.group(2): (m.group(1), [d.strip() for d in m.group(3).split(",")])
              for m in re.finditer(r"\b(int|size_t)\s+(cris_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", plain)}

    def ctype_of(decl):
        if "*" in decl:
            return C.c_void_p
        return {"int": C.c_int, "size_t": C.c_size_t, "float": C.c_float}[decl.split()[0]]
    new = {"cris_label_components": 9, "cris_filter_components": 21, "cris_mask_iou_batch": 10, "cris_filter_components_work_bytes": 2}
    for name, nargs in new.items():
        assert re.search(r"\b(int|size_t) %s\s*\(" % name, src), name
        assert name in hip.EXPORTS and getattr(hip.load(), name) is not None
        res, args = hip._SIGS[name]
        assert len(args) == nargs and args == [ctype_of(d) for d in protos[name][1]], name
        assert res is (C.c_size_t if name.endswith("work_bytes") else C.c_int) and protos[name][0] == ("size_t" if res is C.c_size_t else "int")
    assert hip.ABI_VERSION == 8 == hip.load().cris_abi_version() == int(re.search(r"#define CRIS_ABI_VERSION (\d+)", src).group(1))
    comment = src[src.index("/* CRIS_ABI_VERSION moves"):src.index("#define CRIS_ABI_VERSION")]
    assert all(name in comment for name in new)
    assert comment.index("cris_attn_plan") < comment.index("cris_label_components")          # appended after the last addition
    assert len(re.findall(r"typedef struct \{[^{}]*\} cris_eval_desc;", src)) == 1            # reused, no new struct
    assert hip.load().cris_sizeof(b"cris_eval_desc") == C.sizeof(hip.EvalDesc) == 88
    # the launchers beside them keep their argument lists
    assert len(hip._SIGS["cris_eval_iou_batch"][1]) == 16 and len(hip._SIGS["cris_predict_masks_batch"][1]) == 14
    assert len(hip._SIGS["cris_eval_iou_sweep_batch"][1]) == 15
