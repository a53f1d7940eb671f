"""Host side of the COCO run-length encoding (cris/pytorch_amd/rle.py; csrc/rle.hip cris_rle_encode / cris_rle_work_bytes;
DESIGN.md 9b): the string format against the fixtures, encode / decode against the per-pixel oracle of tests/rle_cases.py on every
case, area and box from the runs, the validation errors, the launcher's rejections through the library, the new mask mode's argument
check and `coco_results`.  Every comparison is an equality.  No GPU."""
import ctypes as C
import json
import os
import re
from types import SimpleNamespace as NS

import numpy as np
import pytest

import rle_cases as RC
from cris.pytorch_amd import rle
from test_predict_cpu import _NoDevice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cris_hip.h")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()


def test_string_fixtures_in_both_directions():
    for counts, s in RC.STRINGS:
        assert rle.counts_to_string(counts) == s == RC.oracle_string(counts), counts
        assert rle.string_to_counts(s).tolist() == counts == rle.string_to_counts(s.decode()).tolist(), s
    assert RC.STRINGS[3][1] == bytes([ord("P"), ord("P"), 92, ord("9")]) and len(RC.STRINGS[3][1]) == 4
    assert rle.counts_to_string([]) == b"" and rle.string_to_counts(b"").tolist() == []
    m, P, counts, s = RC.MASK_FIXTURE
    assert RC.oracle_positions(m) == P and RC.oracle_counts(m) == counts
    assert rle.positions_to_counts(P, 3, 3).tolist() == counts
    assert rle.encode(m) == {"size": [3, 3], "counts": s}
    # the table of the definitions
    assert rle.positions_to_counts([], 4, 5).tolist() == [20] and rle.positions_to_counts([0], 4, 5).tolist() == [0, 20]
    assert rle.positions_to_counts([0, 7], 4, 5).tolist() == [0, 7, 13]
    for bad in ([3, 3], [5, 2], [-1], [20]):
        with pytest.raises(ValueError, match="positions"):
            rle.positions_to_counts(bad, 4, 5)
    # large differences in both directions: seven groups at the most
    big = [2 ** 31 - 1, 1, 0, 2 ** 31 - 1, 2 ** 31 - 1, 0, 5]
    assert rle.counts_to_string(big) == RC.oracle_string(big) and rle.string_to_counts(rle.counts_to_string(big)).tolist() == big


def test_encode_and_decode_equal_the_oracle_on_every_case():
    from cris.pytorch_amd import evalpost
    assert (RC.RB, RC.CG) == (evalpost.RLE_RB, evalpost.RLE_CG)
    names = [k for k, _ in RC.cases()]
    assert len(set(names)) == len(names) >= 20
    sizes, packed, totals = [], [], []
    for (name, m), (P, counts, s) in zip(RC.cases(), RC.expected()):
        h, w = m.shape
        r = rle.encode(m)
        assert r == {"size": [h, w], "counts": s}, name
        assert sum(counts) == h * w and rle.positions_to_counts(P, h, w).tolist() == counts, name
        back = rle.decode(r)
        assert back.dtype == np.uint8 and back.shape == (h, w) and back.flags["C_CONTIGUOUS"], name
        assert np.array_equal(back, (m != 0).astype(np.uint8) * 255), name
        assert np.array_equal(rle.decode({"size": [h, w], "counts": counts}), back), name           # uncompressed counts
        assert np.array_equal(rle.decode({"size": (h, w), "counts": s.decode()}), back), name       # str counts
        assert rle.encode(m != 0) == r and rle.encode(m.astype(np.float32)) == r, name
        # area and box from the runs, against numpy on the decoded mask
        ys, xs = np.nonzero(back)
        assert rle.area(r) == int((back != 0).sum()), name
        assert rle.to_bbox(r) == ((int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1) if xs.size else None), name
        assert rle.to_json(r) == {"size": [h, w], "counts": s.decode()} and json.loads(json.dumps(rle.to_json(r))) == rle.to_json(r)
        sizes.append((h, w))
        packed += P
        totals.append(len(P))
    # the whole batch in one pass, as the device delivers it
    got = rle.strings_from_positions(np.array(packed, np.uint32), totals, sizes)
    assert got == [{"size": [h, w], "counts": s} for (h, w), (_, _, s) in zip(sizes, RC.expected())]
    with pytest.raises(ValueError, match="add up"):
        rle.strings_from_positions(np.array(packed[:-1], np.uint32), totals, sizes)
    with pytest.raises(ValueError, match="ascend"):
        rle.strings_from_positions(np.array([5, 5], np.uint32), [2], [(4, 4)])
    with pytest.raises(ValueError, match="ascend"):
        rle.strings_from_positions(np.array([3, 16], np.uint32), [2], [(4, 4)])


def test_the_cases_are_what_they_were_chosen_for():
    cases, exp = dict(RC.cases()), dict(zip((k for k, _ in RC.cases()), RC.expected()))
    assert exp["1x1 background"][1] == [1] and exp["1x1 foreground"][1] == [0, 1]
    assert cases["1x7"].shape == (1, 7) and cases["7x1"].shape == (7, 1) and exp["7x1"][0][0] == 0
    assert [cases["width %d" % w].shape[1] for w in (3, 4, 5)] == [3, 4, 5] and [RC.pitch_of(w) for w in (3, 4, 5)] == [4, 4, 8]
    assert [cases["height %d" % h].shape[0] for h in (31, 32, 33, 67)] == [RC.RB - 1, RC.RB, RC.RB + 1, 2 * RC.RB + 3]
    assert [cases["width %d" % w].shape for w in (63, 64, 65)] == [(RC.RB + 2, RC.CG - 1), (RC.RB + 2, RC.CG), (RC.RB + 2, RC.CG + 1)]
    assert exp["all background"][0] == [] and exp["all background"][1] == [37 * 10]
    assert exp["all foreground"][0] == [0] and exp["all foreground"][1] == [0, 37 * 10]
    assert exp["checkerboard"][0] == list(range(37 * 70))                   # the maximum: one transition per pixel
    assert exp["first pixel foreground"][0][0] == 0 and exp["first pixel foreground"][1][0] == 0
    j, h = cases["column joins and breaks"], RC.RB + 1
    assert j[-1, 0] and j[0, 1] and j[-1, 1] and not j[0, 2]
    assert exp["column joins and breaks"][0] == [h - 2, h + 3, 2 * h - 1, 2 * h]         # nothing at (1, 0) = h; a transition at (2, 0) = 2 h
    assert sorted(set(cases["bytes 1 and 128"].ravel().tolist())) == [0, 1, 128]
    assert np.array_equal(cases["random 0.5"], cases["random 0.5 again"]) and cases["blob 480x640"].shape == (480, 640)
    assert 1000 < len(exp["blob 480x640"][0]) < 480 * 640 // 50 and cases["blob 480x640"][-1, 60]
    assert RC.ALIAS in cases


def test_validation_errors():
    good = rle.encode(RC.MASK_FIXTURE[0])
    with pytest.raises(ValueError, match="sum to"):
        rle.decode({"size": [3, 3], "counts": [2, 5, 3]})
    with pytest.raises(ValueError, match="sum to"):
        rle.decode({"size": [3, 4], "counts": good["counts"]})
    with pytest.raises(ValueError, match="negative count"):
        rle.decode({"size": [3, 3], "counts": [4, -1, 6]})
    with pytest.raises(ValueError, match="negative count"):
        rle.decode({"size": [3, 3], "counts": RC.oracle_string([4, -1, 6])})                      # a string that decodes to a negative count
    with pytest.raises(ValueError, match="negative|lie in"):
        rle.counts_to_string([3, -2])
    big = rle.counts_to_string([307200])
    with pytest.raises(ValueError, match="continuation"):                   # a truncated string: it ends inside a count
        rle.string_to_counts(big[:-1])
    with pytest.raises(ValueError, match="sum to"):                         # truncated at a count's end: the pixels no longer add up
        rle.decode({"size": [3, 3], "counts": good["counts"][:-1]})
    with pytest.raises(ValueError, match="continuation"):                   # a last group that announces another
        rle.string_to_counts(b"25" + bytes([48 + 0x22]))
    with pytest.raises(ValueError, match="alphabet"):
        rle.string_to_counts(b"25 ")
    with pytest.raises(ValueError, match="alphabet"):
        rle.string_to_counts(b"25p")                                        # chr(112): one past the alphabet
    with pytest.raises(ValueError, match="groups"):
        rle.string_to_counts(bytes([48 + 0x21] * 7 + [48]))
    with pytest.raises(ValueError, match="ASCII"):
        rle.string_to_counts("25é")
    with pytest.raises(ValueError, match="2\\^31"):
        rle.decode({"size": [65536, 32768], "counts": [2 ** 31]})
    for bad in ({"size": [3, 3]}, {"counts": [9]}, [3, 3], {"size": [3.0, 3], "counts": [9]}, {"size": [3], "counts": [9]},
                {"size": [3, 3], "counts": [4.5, 4.5]}, {"size": [3, 3], "counts": [[9]]}, {"size": [3, 3], "counts": 9}):
        with pytest.raises(ValueError):
            rle.decode(bad)
    with pytest.raises(ValueError, match="2-D"):
        rle.encode(np.zeros((2, 2, 2)))
    assert rle.to_bbox({"size": [3, 3], "counts": [9]}) is None and rle.area({"size": [3, 3], "counts": [9]}) == 0


def test_launcher_rejects_bad_arguments_on_the_host(built):
    """cris_rle_encode checks its operands and every descriptor before any launch; cris_rle_work_bytes is host arithmetic"""
    from cris.pytorch_amd import hip
    l = hip.load()
    d = (hip.EvalDesc * 2)()
    mat = (C.c_double * 6)(1, 0, 0, 0, 1, 0)

    def fill(i=0, w=5, h=4, pitch=None, out_off=0):
        assert l.cris_eval_desc_fill(C.addressof(d[i]), mat, w, h, 0, 0, (w + 3) // 4 * 4 if pitch is None else pitch, out_off, 0) == 0

    def encode(masks=0x1000, mask_bytes=64, host=None, dev=0x2000, n=1, work=0x5000, work_bytes=1 << 12, runs=0x3000, run_words=64, totals=0x4000):
        host = C.addressof(d) if host is None else host
        return l.cris_rle_encode(masks, mask_bytes, host or None, dev, n, work, work_bytes, runs, run_words, totals, None)

    def rejected(msg, **kw):
        assert encode(**kw) != 0, (msg, kw)
        err = l.cris_last_error()
        assert b"cris_rle_encode" in err and msg in err, (kw, err)

    fill()
    for k in ("masks", "dev", "work", "runs", "totals"):
        rejected(b"null operand", **{k: None})
    rejected(b"null operand", host=0)
    for n in (0, -1, 65536):
        rejected(b"n must be in 1 .. 65535", n=n)
    for pitch in (6, 4, 7):                                                 # not a multiple of 4; below w_out; both
        fill(pitch=pitch)
        rejected(b"pitch must be a multiple of 4")
    for w, h in ((0, 4), (5, 0), (-3, 4), (46341, 46341)):
        fill(w=w, h=h)
        rejected(b"bad output size")
    fill(out_off=64)                                                        # 8 x 4 bytes at 64 need 96
    rejected(b"output outside the buffer", mask_bytes=95)
    fill(out_off=-16)
    rejected(b"output outside the buffer")
    fill(h=9)                                                               # 72 bytes in a buffer of 64
    rejected(b"output outside the buffer")
    fill()
    rejected(b"aligned", work=0x5004)
    rejected(b"aligned", runs=0x3002)
    rejected(b"aligned", totals=0x4004)
    # the work buffer: per descriptor the batch's largest w * ceil(h / 32) words, then 8 bytes per descriptor
    host = C.addressof(d)
    assert l.cris_rle_work_bytes(host, 1) == 5 * 1 * 4 + 4 + 8             # (rounded up to 8 bytes)
    fill(1, w=7, h=33)
    assert l.cris_rle_work_bytes(host, 2) == 2 * 14 * 4 + 16
    assert l.cris_rle_work_bytes(host, 0) == 0 and l.cris_rle_work_bytes(None, 2) == 0 and l.cris_rle_work_bytes(host, -3) == 0
    need = l.cris_rle_work_bytes(host, 2)
    fill(1, w=7, h=33, out_off=32)
    rejected(b"work buffer is too small", n=2, mask_bytes=32 + 8 * 33, work_bytes=need - 1)
    fill(1, w=7, h=33, pitch=6)
    rejected(b"pitch must be a multiple of 4", n=2, mask_bytes=1 << 12)     # the second descriptor is checked too
    # the second of two entries is looked at only when n says so
    fill(1, w=0)
    rejected(b"bad output size", n=2)


def test_symbols_are_declared_bound_and_named_at_abi_8(built):
    from cris.pytorch_amd import hip
    src = open(HEADER).read()
    plain = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = {m.group(2): (m.group(1), [x.strip() for x in m.group(3).split(",")])
              for m in re.finditer(r"\b(int|size_t)\s+(cris_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", plain)}

    def ctype_of(decl):
        if "*" in decl:
            return C.c_void_p
        return {"int": C.c_int, "size_t": C.c_size_t}[decl.split()[0]]
    for name, nargs, res in (("cris_rle_work_bytes", 2, C.c_size_t), ("cris_rle_encode", 11, C.c_int)):
        assert name in hip.EXPORTS and getattr(hip.load(), name) is not None
        got_res, args = hip._SIGS[name]
        assert got_res is res and protos[name][0] == ("size_t" if res is C.c_size_t else "int")
        assert len(args) == nargs and args == [ctype_of(x) for x in protos[name][1]], name
    assert hip.ABI_VERSION == 8 == hip.load().cris_abi_version() == int(re.search(r"#define CRIS_ABI_VERSION (\d+)", src).group(1))
    comment = src[src.index("/* CRIS_ABI_VERSION moves"):src.index("#define CRIS_ABI_VERSION")]
    assert comment.index("cris_mask_iou_batch") < comment.index("cris_rle_encode") and "cris_rle_work_bytes" in comment
    assert len(re.findall(r"typedef struct \{[^{}]*\} cris_eval_desc;", src)) == 1 and hip.load().cris_sizeof(b"cris_eval_desc") == 88
    # a translation unit of its own, last in the list: the other kernels are compiled from unchanged files
    from cris.pytorch_amd.csrc import build
    assert build.SOURCES[-1] == "rle.hip" and "evalpost.hip" in build.SOURCES
    assert "rle_" not in open(os.path.join(ROOT, "cris", "pytorch_amd", "csrc", "evalpost.hip")).read()


def test_mask_mode_and_op_level_checks_come_before_any_device_work():
    import torch
    from cris.pytorch_amd import evalpost, predict
    assert predict.MASK_MODES == ("host", "device", "rle", None)
    jpg = b"\xff\xd8\xff\xe0fake"
    assert predict._check_inputs([jpg], ["a"], 8, "rle")[0] == "bytes"
    for bad in ("RLE", "png", "Rle", b"rle", 0):
        with pytest.raises(ValueError, match="'host', 'device', 'rle' or None"):
            predict._check_inputs([jpg], ["a"], 8, bad)
    p = predict.Predictor(NS(), _NoDevice(), thr=0.35)
    with pytest.raises(ValueError, match="no images"):
        p.predict([], [], masks="rle")
    assert p._ring is None and p._cc_masks is None and p._rle_runs is None and p._rle_work is None
    st = NS(out_bytes=64, n=1)
    with pytest.raises(RuntimeError, match="GPU only"):
        evalpost.rle_encode_batch(torch.zeros(64, dtype=torch.uint8), st)
    with pytest.raises(SystemExit):                                         # neither PNGs nor a results file
        predict.main(["--image", "x.jpg", "--expr", "a"])


def test_coco_results_from_hand_made_predictions():
    from cris.pytorch_amd.predict import ComponentPrediction, Prediction, coco_results
    m = np.zeros((6, 8), np.uint8)
    m[2:5, 3:7] = 255
    empty = np.zeros((6, 8), np.uint8)
    out = [[Prediction("the box", rle.encode(m), 12, (3, 2, 7, 5), 0.875), Prediction("nothing", rle.encode(empty), 0, None, 0.0)],
           [ComponentPrediction("kept", rle.encode(m), np.int64(12), (3, 2, 7, 5), 0.5, 2, 14)]]
    got = coco_results(out, [17, "img_b"])
    assert [e["image_id"] for e in got] == [17, 17, "img_b"] and [e["sentence"] for e in got] == ["the box", "nothing", "kept"]
    assert list(got[0]) == ["image_id", "sentence", "segmentation", "bbox", "area", "score"]
    assert got[0]["bbox"] == [3, 2, 4, 3] and got[0]["area"] == 12 and got[0]["score"] == 0.875
    assert got[1]["bbox"] == [0, 0, 0, 0] and got[1]["area"] == 0 and got[1]["segmentation"] == {"size": [6, 8], "counts": "`1"}
    back = json.loads(json.dumps(got))                                      # json-ready as it stands
    assert back == got and type(got[2]["area"]) is int
    for e, want in zip(back, (m, empty, m)):
        assert np.array_equal(rle.decode(e["segmentation"]), want)
        assert rle.area(e["segmentation"]) == e["area"]
    assert rle.to_bbox(back[0]["segmentation"]) == (3, 2, 7, 5)
    assert "sentence" not in coco_results(out, [1, 2], expressions=False)[0]
    with pytest.raises(ValueError, match="image ids"):
        coco_results(out, [1])
    with pytest.raises(ValueError, match="masks='rle'"):
        coco_results([[Prediction("a", m, 12, (3, 2, 7, 5), 0.5)]], [1])
    with pytest.raises(ValueError, match="masks='rle'"):
        coco_results([[Prediction("a", None, 12, (3, 2, 7, 5), 0.5)]], [1])
