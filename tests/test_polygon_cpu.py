"""Host side of the polygon masks (cris/pytorch_amd/polygon.py; csrc/polygon.hip cris_polygon_count / cris_polygon_trace and
their work-size functions; csrc/polygon_core.h): encode against the per-crack oracle of tests/polygon_cases.py on every
case, the invariants of the format, area / box / COCO form, the validation errors, the per-vertex header run on the CPU under
sanitizers, the launchers' rejections through the library, the new mask mode's argument check and `coco_results`.  Every comparison
is an equality.  No GPU."""
import ctypes as C
import json
import os
import re
import subprocess
from types import SimpleNamespace as NS

import numpy as np
import pytest

import polygon_cases as PC
from cris.pytorch_amd import polygon
from test_predict_cpu import _NoDevice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cris_hip.h")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()


def _same(p, q):
    return (p["size"] == q["size"] and p["holes"] == q["holes"] and len(p["rings"]) == len(q["rings"])
            and all(a.dtype == b.dtype == np.int32 and np.array_equal(a, b) for a, b in zip(p["rings"], q["rings"])))


def test_the_cases_cover_the_shapes_the_kernels_branch_on():
    from cris.pytorch_amd import evalpost
    assert (PC.RB, PC.CG, PC.CHUNK) == (evalpost.POLYGON_RB, evalpost.POLYGON_CG, evalpost.POLYGON_CHUNK)
    src = open(os.path.join(ROOT, "cris", "pytorch_amd", "csrc", "polygon.hip")).read()
    for name, value in (("PG_RB", PC.RB), ("PG_CG", PC.CG), ("PG_CHUNK", PC.CHUNK)):
        assert int(re.search(r"#define %s (\d+)" % name, src).group(1)) == value
    shapes = {m.shape for _, m in PC.cases()}
    rows, cols = {h + 1 for h, _ in shapes}, {w + 1 for _, w in shapes}    # vertex rows and columns
    for k in (1, 2):
        assert {k * PC.RB - 1, k * PC.RB, k * PC.RB + 1} <= rows and {k * PC.CG - 1, k * PC.CG, k * PC.CG + 1} <= cols
    assert {pitch - w for w in (3, 4, 5) for pitch in [PC.pitch_of(w)]} == {1, 0, 3}
    counts = {sum(len(r) for r in rings) for rings, _ in PC.expected()}
    for k in (6, 8, 10, 12):                                                # one wave, one block, one scan chunk, 4096: a single ring each
        assert {2 ** k - 2, 2 ** k, 2 ** k + 2} <= counts
    assert 2 ** 10 == PC.CHUNK
    for v in PC.COMB_SIZES:
        rings, _ = PC.oracle_trace(PC.comb(v))
        assert len(rings) == 1 and len(rings[0]) == v
    rings, _ = PC.oracle_trace(PC.serpentine())
    assert len(rings) == 1 and PC.serpentine().shape == (64, 64)
    names = [k for k, _ in PC.cases()]
    board = PC.cases()[names.index("checkerboard odd")][1]
    h, w = board.shape
    assert h % 2 == 1 and sum(len(r) for r in PC.expected()[names.index("checkerboard odd")][0]) == 4 * ((h * w + 1) // 2)
    assert PC.cases()[names.index("blob 480x640")][1].shape == (480, 640)


def test_encode_equals_the_oracle_and_the_invariants_hold():
    for i, (name, m) in enumerate(PC.cases()):
        rings, _ = PC.expected()[i]
        want, got = PC.expected_dict(i), polygon.encode(m)
        assert _same(got, want), name
        h, w = m.shape
        fg = int((m != 0).sum())
        assert polygon.validate(got) == (h, w), name
        areas = [PC.oracle_twice_area(r) for r in rings]
        assert sum(areas) == 2 * fg and all(a != 0 and a % 2 == 0 for a in areas), name           # the area identity, exactly
        assert got["holes"] == [a < 0 for a in areas], name
        assert [polygon.twice_area(r) for r in got["rings"]] == areas, name
        assert np.array_equal(PC.oracle_decode(rings, h, w), (m != 0).astype(np.uint8) * 255), name   # even-odd round trip, per pixel
        assert np.array_equal(polygon.decode(got), (m != 0).astype(np.uint8) * 255), name            # and vectorised
        starts = [(r[0][1], r[0][0]) for r in rings]
        assert starts == sorted(starts), name                               # the rings in raster order of their starts
        for r, a in zip(rings, areas):
            assert len(r) >= 4 and len(r) % 2 == 0, name
            assert (r[0][1], r[0][0]) == min((y, x) for x, y in r) and r.count(r[0]) == 1, name    # raster-first, visited once
            (x0, y0), (x1, y1) = r[0], r[1]
            assert ((x1 > x0 and y1 == y0) if a > 0 else (x1 == x0 and y1 > y0)), name              # outer: east; hole: south
            for j in range(len(r)):                                          # alternating axis-parallel edges
                (xa, ya), (xb, yb) = r[j], r[(j + 1) % len(r)]
                assert (ya == yb and xa != xb) if j % 2 == (0 if a > 0 else 1) else (xa == xb and ya != yb), name
        assert sum(len(r) for r in rings) <= 2 * (h + 1) * (w + 1)
        # area and box agree with numpy on the mask
        assert polygon.area(got) == fg, name
        ys, xs = np.nonzero(m)
        assert polygon.to_bbox(got) == ((int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1) if fg else None), name


def test_corner_visit_lists_pair_up_as_the_device_assumes():
    """entries 2 k and 2 k + 1 of the row-major list are the ends of one horizontal ring edge, of the column-major list of one
    vertical edge: the fact csrc/polygon.hip links the rings with, on the oracle's own visits"""
    for i, (name, m) in enumerate(PC.cases()):
        rings, visits = PC.expected()[i]
        bits = {(v[0], v[1]) + PC.oracle_visit_bits(v) for v in visits}
        assert len(bits) == len(visits) == sum(len(r) for r in rings), name
        x, y, he, vs, outv = polygon.corner_visits(m)
        mine = list(zip(x.tolist(), y.tolist(), he.tolist(), vs.tolist(), outv.tolist()))
        assert mine == sorted(bits, key=lambda v: (v[1], v[0], v[2])), name
        assert len(mine) % 2 == 0
        for a, b in zip(mine[0::2], mine[1::2]):
            assert a[1] == b[1] and a[0] < b[0] and (a[2], b[2]) == (1, 0) and a[4] != b[4], name
        cols = sorted(mine, key=lambda v: (v[0], v[1], v[3]))
        for a, b in zip(cols[0::2], cols[1::2]):
            assert a[0] == b[0] and a[1] < b[1] and (a[3], b[3]) == (1, 0) and a[4] != b[4], name


def test_polygon_core_header_under_sanitizers_equals_the_oracle(tmp_path):
    """csrc/polygon_core.h - the header the HIP kernels include - compiled by g++ into tests/polygon_core_probe.cpp with the address
    and undefined-behaviour sanitizers and run as a child process on the small cases: both corner-visit lists against the oracle"""
    exe, data = str(tmp_path / "polygon_core_probe"), str(tmp_path / "masks.txt")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "polygon_core_probe.cpp")])
    small = [i for i, (_, m) in enumerate(PC.cases()) if m.size <= PC.SMALL]
    assert len(small) >= 12
    with open(data, "w") as f:
        f.write("%d\n" % len(small))
        for i in small:
            m = PC.cases()[i][1]
            f.write("%d %d\n" % m.shape + "".join("".join("1" if v else "0" for v in row) + "\n" for row in m.tolist()))
    r = subprocess.run([exe, data], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-2000:]
    blocks = out.split("mask ")[1:]
    assert len(blocks) == len(small)
    for k, (i, block) in enumerate(zip(small, blocks)):
        name = PC.cases()[i][0]
        lines = block.splitlines()
        visits = {(v[0], v[1]) + PC.oracle_visit_bits(v) for v in PC.expected()[i][1]}
        assert lines[0].split() == [str(k), str(len(visits))], name
        got = {"R": [], "C": []}
        for line in lines[1:]:
            got[line[0]].append(tuple(int(v) for v in line.split()[1:]))
        assert got["R"] == sorted(visits, key=lambda v: (v[1], v[0], v[2])), name
        assert got["C"] == sorted(visits, key=lambda v: (v[0], v[1], v[3])), name


def test_coco_form_with_and_without_holes():
    names = [k for k, _ in PC.cases()]
    p = polygon.encode(PC.cases()[names.index("island in a hole")][1])
    assert p["holes"] == [False, True, False] and [len(r) for r in p["rings"]] == [4, 4, 4]
    assert polygon.to_coco(p) == [[1, 1, 11, 1, 11, 10, 1, 10], [5, 5, 7, 5, 7, 6, 5, 6]]
    assert polygon.to_coco(p, holes=True) == [[1, 1, 11, 1, 11, 10, 1, 10], [3, 3, 3, 8, 9, 8, 9, 3], [5, 5, 7, 5, 7, 6, 5, 6]]
    assert json.loads(json.dumps(polygon.to_coco(p, holes=True))) == polygon.to_coco(p, holes=True)
    assert "Smooth(fill_holes=True)" in polygon.to_coco.__doc__ and "holes" in polygon.to_coco.__doc__
    empty = polygon.encode(np.zeros((3, 4), np.uint8))
    assert empty == {"size": [3, 4], "rings": [], "holes": []} and polygon.to_coco(empty) == [] and polygon.to_bbox(empty) is None
    assert polygon.area(empty) == 0 and not polygon.decode(empty).any() and polygon.decode(empty).shape == (3, 4)
    one = polygon.encode(np.full((1, 1), 7, np.uint8))
    assert polygon.to_coco(one) == [[0, 0, 1, 0, 1, 1, 0, 1]] and polygon.decode(one).tolist() == [[255]]


def test_validate_rejects_malformed_input_before_work():
    sq = np.array([[0, 0], [2, 0], [2, 2], [0, 2]], np.int32)
    good = {"size": [3, 4], "rings": [sq], "holes": [False]}
    assert polygon.validate(good) == (3, 4)

    def bad(match, **kw):
        p = dict(good, **kw)
        for fn in (polygon.validate, polygon.decode, polygon.area, polygon.to_bbox, polygon.to_coco):
            with pytest.raises(ValueError, match=match):
                fn(p)

    for p in (None, [sq], {"size": [3, 4], "rings": [sq]}, {"size": [3, 4], "holes": [False]}):
        with pytest.raises(ValueError, match="expected"):
            polygon.validate(p)
    bad("size must be", size=[3])
    bad("size must be", size=[3.0, 4])
    bad("size must be", size=[-1, 4])
    bad("size must be", size=[True, 4])
    bad("<= 2\\^28", size=[2 ** 14, 2 ** 14])
    bad("one length", holes=[])
    bad("one length", rings=sq)
    bad("must be a bool", holes=[0])
    bad("int32 array", rings=[sq.astype(np.int64)])
    bad("int32 array", rings=[sq.tolist()])
    bad("int32 array", rings=[sq.reshape(-1)])
    bad("even number >= 4", rings=[sq[:2]])
    bad("even number >= 4", rings=[np.concatenate([sq, sq[:1]])])
    bad("leaves", rings=[sq - 1])
    bad("leaves", rings=[sq + np.array([3, 0], np.int32)])
    bad("leaves", rings=[sq + np.array([0, 2], np.int32)])
    bad("axis-parallel", rings=[np.array([[0, 0], [2, 1], [2, 2], [0, 2]], np.int32)])
    bad("axis-parallel", rings=[np.array([[0, 0], [0, 0], [2, 2], [0, 2]], np.int32)])
    bad("collinear", rings=[np.array([[0, 0], [1, 0], [2, 0], [2, 2], [1, 2], [0, 2]], np.int32)])
    for shape in ((2, 3, 4), (5,)):
        with pytest.raises(ValueError, match="2-d"):
            polygon.encode(np.zeros(shape, np.uint8))


def test_from_rings_slices_and_checks():
    verts = np.array([[0, 0], [1, 0], [1, 1], [0, 1], [2, 2], [3, 2], [3, 3], [2, 3]], np.int32)
    table = np.array([[0, 0, 4, 2], [2, 4, 4, 2]], np.int64)
    got = polygon.from_rings(verts, table, [(4, 4), (2, 2), (4, 4)])
    assert [len(p["rings"]) for p in got] == [1, 0, 1] and got[1] == {"size": [2, 2], "rings": [], "holes": []}
    assert np.array_equal(got[2]["rings"][0], verts[4:]) and got[2]["rings"][0].dtype == np.int32
    for row in ([3, 0, 4, 2], [0, 6, 4, 2], [0, 0, 2, 2], [0, -1, 4, 2], [0, 0, 4, 0]):
        with pytest.raises(RuntimeError, match="ring row"):
            polygon.from_rings(verts, np.array([row], np.int64), [(4, 4)] * 3)


def test_launchers_reject_bad_arguments_on_the_host(built):
    """cris_polygon_count / cris_polygon_trace check their operands and every descriptor before any launch; the two work-size
    functions are host arithmetic"""
    from cris.pytorch_amd import hip
    l = hip.load()
    d = (hip.EvalDesc * 2)()
    mat = (C.c_double * 6)(1, 0, 0, 0, 1, 0)

    def fill(i=0, w=5, h=4, pitch=None, out_off=0):
        assert l.cris_eval_desc_fill(C.addressof(d[i]), mat, w, h, 0, 0, (w + 3) // 4 * 4 if pitch is None else pitch, out_off, 0) == 0

    def count(masks=0x1000, mask_bytes=64, host=None, dev=0x2000, n=1, work=0x5000, work_bytes=1 << 12, totals=0x4000):
        host = C.addressof(d) if host is None else host
        return l.cris_polygon_count(masks, mask_bytes, host or None, dev, n, work, work_bytes, totals, None)

    def trace(masks=0x1000, mask_bytes=64, host=None, dev=0x2000, n=1, work=0x5000, work_bytes=1 << 12, totals=0x4000, total=8, most=8,
              extra=0, twork=0x6000, twork_bytes=1 << 12, vertices=0x7000, vertex_cap=8, rings=0x8000, ring_cap=2, header=0x9000):
        host = C.addressof(d) if host is None else host
        return l.cris_polygon_trace(masks, mask_bytes, host or None, dev, n, work, work_bytes, totals, total, most, extra, twork,
                                    twork_bytes, vertices, vertex_cap, rings, ring_cap, header, None)

    def rejected(fn, msg, **kw):
        assert fn(**kw) != 0, (msg, kw)
        err = l.cris_last_error()
        assert fn.__name__.encode() in err and b"cris_polygon_" in err and msg in err, (kw, err)

    fill()
    for k in ("masks", "dev", "work", "totals"):
        rejected(count, b"null operand", **{k: None})
        rejected(trace, b"null operand", **{k: None})
    for k in ("twork", "vertices", "rings", "header"):
        rejected(trace, b"null operand", **{k: None})
    for fn in (count, trace):
        rejected(fn, b"null operand", host=0)
        for n in (0, -1, 65536):
            rejected(fn, b"n must be in 1 .. 65535", n=n)
        for pitch in (6, 4, 7):                                             # not a multiple of 4; below w_out; both
            fill(pitch=pitch)
            rejected(fn, b"pitch must be a multiple of 4")
        for w, h in ((0, 4), (5, 0), (-3, 4), (2 ** 14, 2 ** 14)):          # (h + 1) * (w + 1) > 2^28
            fill(w=w, h=h)
            rejected(fn, b"bad output size")
        fill(out_off=64)                                                    # a rectangle outside mask_bytes: 8 x 4 bytes at 64 need 96
        rejected(fn, b"output outside the buffer", mask_bytes=95)
        fill(out_off=-16)
        rejected(fn, b"output outside the buffer")
        fill(h=9)                                                           # 72 bytes in a buffer of 64
        rejected(fn, b"output outside the buffer")
        fill()
        rejected(fn, b"aligned", work=0x5004)
        rejected(fn, b"aligned", totals=0x4004)
    rejected(trace, b"aligned", twork=0x6004)
    rejected(trace, b"aligned", vertices=0x7002)
    rejected(trace, b"aligned", rings=0x8004)
    rejected(trace, b"aligned", header=0x9004)
    for total in (0, -2, 7, 2 ** 30 + 2):
        rejected(trace, b"total_vertices must be even", total=total)
    for most in (0, 2, 10):
        rejected(trace, b"max_vertices_per_mask", most=most)
    for extra in (-1, 9):
        rejected(trace, b"extra_rounds", extra=extra)
    # the count's work buffer: per descriptor the batch's largest (h + 1) * ceil((w + 1) / 64) and (w + 1) * ceil((h + 1) / 32) words,
    # each part rounded up to 8 bytes, then 8 bytes per descriptor
    host = C.addressof(d)
    assert l.cris_polygon_work_bytes(host, 1) == (5 * 4 + 4) + 6 * 4 + 8
    fill(1, w=70, h=33)
    assert l.cris_polygon_work_bytes(host, 2) == 2 * 34 * 2 * 4 + 2 * 71 * 2 * 4 + 16
    assert l.cris_polygon_work_bytes(host, 0) == 0 and l.cris_polygon_work_bytes(None, 2) == 0 and l.cris_polygon_work_bytes(host, -3) == 0
    need = l.cris_polygon_work_bytes(host, 2)
    fill(1, w=70, h=33, out_off=32)
    for fn in (count, trace):
        rejected(fn, b"work buffer is too small", n=2, mask_bytes=32 + 72 * 33, work_bytes=need - 1)
    fill(1, w=70, h=33, pitch=70)
    rejected(count, b"pitch must be a multiple of 4", n=2, mask_bytes=1 << 14)         # the second descriptor is checked too
    fill(1, w=0)
    rejected(count, b"bad output size", n=2)                               # ... and only when n says so
    # the trace's work buffer: nine words per vertex (each plane rounded up to 8 bytes), one 64-bit word per PG_CHUNK vertices
    assert l.cris_polygon_trace_work_bytes(8, 1) == 9 * 32 + 8
    assert l.cris_polygon_trace_work_bytes(1026, 3) == 9 * 4104 + 16
    assert [l.cris_polygon_trace_work_bytes(t, 1) for t in (0, -4, 2 ** 30 + 2)] == [0, 0, 0] and l.cris_polygon_trace_work_bytes(8, 0) == 0
    fill()
    rejected(trace, b"trace work buffer is too small", twork_bytes=9 * 32 + 7)


def test_symbols_are_declared_bound_and_named_at_abi_8(built):
    from cris.pytorch_amd import hip
    src = open(HEADER).read()
    plain = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = {m.group(2): (m.group(1), [x.strip() for x in m.group(3).split(",")])
              for m in re.finditer(r"\b(int|size_t)\s+(cris_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", plain)}

    def ctype_of(decl):
        if "*" in decl:
            return C.c_void_p
        return C.c_longlong if decl.startswith("long long") else {"int": C.c_int, "size_t": C.c_size_t}[decl.split()[0]]
    for name, nargs, res in (("cris_polygon_work_bytes", 2, C.c_size_t), ("cris_polygon_trace_work_bytes", 2, C.c_size_t),
                             ("cris_polygon_count", 9, C.c_int), ("cris_polygon_trace", 19, C.c_int)):
        assert name in hip.EXPORTS and getattr(hip.load(), name) is not None
        got_res, args = hip._SIGS[name]
        assert got_res is res and protos[name][0] == ("size_t" if res is C.c_size_t else "int")
        assert len(args) == nargs and args == [ctype_of(x) for x in protos[name][1]], name
    assert hip.ABI_VERSION == 8 == hip.load().cris_abi_version()
    comment = src[src.index("/* CRIS_ABI_VERSION moves"):src.index("#define CRIS_ABI_VERSION")]
    assert comment.index("cris_rle_encode") < comment.index("cris_polygon_count") and "cris_polygon_trace_work_bytes" in comment
    from cris.pytorch_amd.csrc import build
    assert "polygon.hip" in build.SOURCES and len(set(build.SOURCES)) == len(build.SOURCES)
    rle_src = open(os.path.join(ROOT, "cris", "pytorch_amd", "csrc", "rle.hip")).read()
    assert "polygon" not in rle_src and "pg_" not in rle_src               # the RLE path is untouched


def test_mask_mode_and_op_level_checks_come_before_any_device_work():
    import torch
    from cris.pytorch_amd import evalpost, predict
    assert predict.POLYGON_MODE == "polygon" and "polygon" not in predict.MASK_MODES
    jpg = b"\xff\xd8\xff\xe0fake"
    assert predict._check_inputs([jpg], ["a"], 8, "polygon")[0] == "bytes"
    for bad in ("Polygon", "polygons", "poly", b"polygon", 0):
        with pytest.raises(ValueError, match="masks must be .*'polygon'"):
            predict._check_inputs([jpg], ["a"], 8, bad)
    p = predict.Predictor(NS(), _NoDevice(), thr=0.35)
    with pytest.raises(ValueError, match="no images"):
        p.predict([], [], masks="polygon")
    assert p._ring is None and p._cc_masks is None and p._pg_work is None and p._pg_buffers is None
    st = NS(out_bytes=64, n=1)
    for fn, args in ((evalpost.polygon_count_batch, ()), (evalpost.polygon_collect, (torch.zeros(2, dtype=torch.int64),))):
        with pytest.raises(RuntimeError, match="GPU only"):
            fn(torch.zeros(64, dtype=torch.uint8), st, *args)
    with pytest.raises(SystemExit):                                         # neither PNGs nor a results file
        predict.main(["--image", "x.jpg", "--expr", "a"])


def test_coco_results_from_hand_made_polygon_predictions():
    from cris.pytorch_amd import rle
    from cris.pytorch_amd.predict import ComponentPrediction, Prediction, coco_results
    m = np.zeros((6, 8), np.uint8)
    m[2:5, 3:7] = 255
    holed = m.copy()
    holed[3, 4] = 0
    empty = np.zeros((6, 8), np.uint8)
    out = [[Prediction("the box", polygon.encode(m), 12, (3, 2, 7, 5), 0.875), Prediction("nothing", polygon.encode(empty), 0, None, 0.0)],
           [ComponentPrediction("holed", polygon.encode(holed), np.int64(11), (3, 2, 7, 5), 0.5, 2, 14)]]
    got = coco_results(out, [17, "img_b"])
    assert [e["image_id"] for e in got] == [17, 17, "img_b"] and [e["sentence"] for e in got] == ["the box", "nothing", "holed"]
    assert list(got[0]) == ["image_id", "sentence", "segmentation", "bbox", "area", "score"]
    assert got[0]["segmentation"] == [[3, 2, 7, 2, 7, 5, 3, 5]] and got[0]["bbox"] == [3, 2, 4, 3] and got[0]["area"] == 12 and got[0]["score"] == 0.875
    assert got[1]["segmentation"] == [] and got[1]["bbox"] == [0, 0, 0, 0] and got[1]["area"] == 0
    assert got[2]["segmentation"] == [[3, 2, 7, 2, 7, 5, 3, 5]] and got[2]["area"] == 11          # the outer ring alone: COCO has no holes
    assert json.loads(json.dumps(got)) == got and type(got[2]["area"]) is int
    assert "sentence" not in coco_results(out, [1, 2], expressions=False)[0]
    # RLE results and the errors are what they were
    mixed = coco_results([[Prediction("r", rle.encode(m), 12, (3, 2, 7, 5), 0.5)]], [1])
    assert mixed[0]["segmentation"] == rle.to_json(rle.encode(m))
    with pytest.raises(ValueError, match="image ids"):
        coco_results(out, [1])
    with pytest.raises(ValueError, match="masks='rle'"):
        coco_results([[Prediction("a", m, 12, (3, 2, 7, 5), 0.5)]], [1])
