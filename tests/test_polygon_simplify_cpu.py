"""Host side of the Douglas-Peucker simplifier of polygon masks (cris/pytorch_amd/polygon.simplify; csrc/simplify.hip
cris_polygon_simplify and its work-size function; csrc/simplify_core.h): the vectorised numpy restatement against the
recursive oracle of tests/simplify_cases.py on every case and epsilon, the Douglas-Peucker invariant in exact integers, decode /
area / box of simplified dicts against a per-pixel oracle, the validation rules, the shared header run on the CPU under sanitizers,
the launcher's rejections through the library and the argument checks of every entry point.  Every comparison is an equality.
No GPU."""
import ctypes as C
import os
import re
import subprocess
from types import SimpleNamespace as NS

import numpy as np
import pytest

import polygon_cases as PC
import simplify_cases as SC
from cris.pytorch_amd import polygon
from test_predict_cpu import _NoDevice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cris_hip.h")
NAMES = [k for k, _ in SC.cases()]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()


def _ring_of(name):
    rings, _ = SC.traced()[NAMES.index(name)]
    assert len(rings) == 1
    return rings[0]


def test_the_cases_cover_the_paths_and_the_figures_of_the_definition():
    from cris.pytorch_amd import evalpost
    assert (SC.WAVE_RING, SC.LDS_RING, SC.MAX_SIDE) == (evalpost.POLYGON_SIMPLIFY_WAVE, evalpost.POLYGON_SIMPLIFY_LDS, polygon.MAX_SIMPLIFY_SIDE)
    src = open(os.path.join(ROOT, "cris", "pytorch_amd", "csrc", "simplify.hip")).read()
    core = open(os.path.join(ROOT, "cris", "pytorch_amd", "csrc", "simplify_core.h")).read()
    for text, name, value in ((src, "SP_WAVE_RING", SC.WAVE_RING), (src, "SP_LDS_RING", SC.LDS_RING), (core, "SP_MAX_SIDE", SC.MAX_SIDE), (core, "SP_MAX_Q", 256)):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == value
    assert '#include "simplify_core.h"' in src and "2^62" in core and "2^47" in core          # the bound stands where the predicate is written
    assert NAMES[:len(PC.cases())] == [k for k, _ in PC.cases()]                               # the tracer's cases as they are
    lengths = {len(r) for rings, _ in SC.traced() for r in rings}
    for edge in (SC.WAVE_RING, SC.LDS_RING):                                                   # 2 below, at and 2 above either switch
        assert {edge - 2, edge, edge + 2} <= lengths and {edge - 2, edge, edge + 2} <= set(PC.COMB_SIZES)
    assert SC.EPSILONS == (0.25, 1, 2, 12, 64)
    # the comb of 4098 vertices.  Between its two ring neighbours a stair-step vertex has c = a b and len2 = a^2 + b^2 for edge
    # lengths a, b >= 1, and 16 a^2 b^2 > a^2 + b^2: at epsilon 0.25 the definition keeps every vertex.  Half of them go at 1.
    comb = _ring_of("comb 4098")
    assert [len(SC.oracle_kept(comb, q)) for q in (1, 4, 8, 256)] == [4098, 2049, 3, 2]
    i = NAMES.index("comb 4098")
    assert [[len(r) for r in SC.expected(e)[i]["rings"]] for e in (0.25, 1, 2, 64)] == [[4098], [2049], [3], []]
    # the 20 x 15 rectangle: the corners lie exactly 12 from the diagonal - kept at 11.75, dropped at 12 (strict), so the ring goes
    rect = _ring_of("rectangle 20x15")
    assert rect == [(0, 0), (20, 0), (20, 15), (0, 15)] and 16 * (20 * 15) ** 2 == 48 ** 2 * (20 ** 2 + 15 ** 2)
    assert SC.oracle_kept(rect, 47) == [0, 1, 2, 3] and SC.oracle_kept(rect, 48) == [0, 2]
    assert SC.expected(12)[NAMES.index("rectangle 20x15")]["rings"] == []
    assert [len(r) for r in polygon.simplify(SC.traced_dict(NAMES.index("rectangle 20x15")), 11.75)["rings"]] == [4]
    # two vertices equally far from v_0: the smaller index is the anchor
    tie = _ring_of("anchor tie")
    assert tie == [(0, 0), (4, 0), (4, 3), (3, 3), (3, 4), (0, 4)] and SC.oracle_kept(tie, 256) == [0, 2]
    # every unit square goes at epsilon >= 0.75 and stays below
    unit = [(0, 0), (1, 0), (1, 1), (0, 1)]
    assert [len(SC.oracle_kept(unit, q)) for q in (1, 2, 3, 4)] == [4, 4, 2, 2]
    # the largest side
    assert {SC.cases()[NAMES.index(k)][1].shape for k in ("row of 32767", "column of 32767")} == {(1, 32767), (32767, 1)}
    assert max(v[0] for r in SC.traced()[NAMES.index("row of 32767")][0] for v in r) == 32767


def test_simplify_equals_the_oracle_and_the_invariant_holds():
    for eps in SC.EPSILONS:
        q = int(4 * eps)
        want = SC.expected(eps)
        for i, name in enumerate(NAMES):
            traced = SC.traced_dict(i)
            before = [r.copy() for r in traced["rings"]]
            got = polygon.simplify(traced, eps)
            assert SC.same(got, want[i]), (name, eps)                          # rings, holes, order, epsilon
            assert got["epsilon"] == float(eps) and type(got["epsilon"]) is float and polygon.validate(got) == tuple(traced["size"])
            assert "epsilon" not in traced and all(np.array_equal(a, b) for a, b in zip(before, traced["rings"]))     # the input is only read
            kept = polygon.simplify_kept(traced["rings"], q)
            out = 0
            for r, hole, idx in zip(traced["rings"], traced["holes"], kept):
                k = r.shape[0]
                assert idx[0] == 0 and (np.diff(idx) > 0).all() and idx[-1] < k and idx.size >= 2
                if idx.size >= 3:
                    assert np.array_equal(got["rings"][out], r[idx]) and got["holes"][out] == hole
                    out += 1
                # Douglas-Peucker: every traced vertex lies within epsilon of the line of the kept segment that spans it
                v = np.concatenate([r, r[:1]]).astype(np.int64)
                ends = np.append(idx, k)
                seg = np.searchsorted(ends, np.arange(k + 1), side="right") - 1
                seg = np.minimum(seg, ends.size - 2)
                a, b = v[ends[seg]], v[ends[seg + 1]]
                cross = (b[:, 0] - a[:, 0]) * (v[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (v[:, 0] - a[:, 0])
                len2 = ((b - a) ** 2).sum(axis=1)
                assert int(np.abs(cross).max()) < 2 ** 29 and int(len2.max()) < 2 ** 31 and int(len2.min()) > 0     # the 64-bit bound
                assert (16 * cross * cross <= q * q * len2).all(), (name, eps)
            assert out == len(got["rings"])


def test_rounds_are_what_the_middle_tie_rule_promises():
    """the depth a round-synchronous kernel pays for: rounds of polygon.simplify_kept = the deepest recursion + 1"""
    rounds = []
    polygon.simplify_kept([np.array(_ring_of("comb 4098"), np.int32)], 4, rounds)
    polygon.simplify_kept([np.array(_ring_of("serpentine"), np.int32)], 4, rounds)
    print("rounds at epsilon 1: comb 4098 %d, serpentine %d" % tuple(rounds))
    assert rounds[0] <= 24 and rounds[1] <= 14                                  # ceil(log2) growth, not 2048 and 34


def test_decode_area_and_box_of_simplified_dicts_equal_the_per_pixel_oracle():
    small = [i for i, (_, m) in enumerate(SC.cases()) if m.size <= PC.SMALL]
    assert len(small) >= 12
    odd = 0
    for eps in (0.25, 1, 2):
        for i in small:
            p = SC.expected(eps)[i]
            h, w = p["size"]
            assert np.array_equal(polygon.decode(p), SC.oracle_decode_general(p["rings"], h, w)), (NAMES[i], eps)
            twice = sum(PC.oracle_twice_area([tuple(v) for v in r.tolist()]) for r in p["rings"])
            got = polygon.area(p)
            assert got == twice / 2 and type(got) is (float if twice % 2 else int), (NAMES[i], eps)
            odd += twice % 2
            pts = [tuple(v) for r in p["rings"] for v in r.tolist()]
            box = (min(x for x, _ in pts), min(y for _, y in pts), max(x for x, _ in pts), max(y for _, y in pts)) if pts else None
            assert polygon.to_bbox(p) == box
            assert polygon.to_coco(p) == [[int(c) for c in r.reshape(-1)] for r, hole in zip(p["rings"], p["holes"]) if not hole]
            assert len(polygon.to_coco(p, holes=True)) == len(p["rings"])
    assert odd > 0                                                              # a float area was met
    # at 0.25 the small cases keep every vertex, so the general fill gives the mask itself back
    for i in small:
        m = SC.cases()[i][1]
        assert sum(len(r) for r in SC.expected(0.25)[i]["rings"]) == sum(len(r) for r in SC.traced()[i][0])
        assert np.array_equal(polygon.decode(SC.expected(0.25)[i]), (m != 0).astype(np.uint8) * 255), NAMES[i]
    # a triangle by hand: (0, 0), (4, 0), (0, 4) covers the pixel centres left of x + y = 4; those ON the diagonal, a right-hand edge, are outside
    tri = {"size": [4, 4], "rings": [np.array([[0, 0], [4, 0], [0, 4]], np.int32)], "holes": [False], "epsilon": 1.0}
    assert (polygon.decode(tri) != 0).astype(int).tolist() == [[1, 1, 1, 0], [1, 1, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0]]
    assert polygon.area(tri) == 8 and type(polygon.area(tri)) is int and polygon.to_bbox(tri) == (0, 0, 4, 4)
    tri["rings"] = [np.array([[0, 0], [3, 0], [0, 3]], np.int32)]
    assert polygon.area(tri) == 4.5 and type(polygon.area(tri)) is float


def test_validate_accepts_and_rejects_simplified_dicts_as_specified():
    tri = np.array([[0, 0], [4, 1], [1, 3]], np.int32)
    good = {"size": [3, 4], "rings": [tri], "holes": [True], "epsilon": 1.5}
    assert polygon.validate(good) == (3, 4)
    flat = dict(good, rings=[np.array([[0, 0], [2, 0], [4, 0]], np.int32)])    # 2 A = 0 is allowed
    assert polygon.validate(flat) == (3, 4) and polygon.area(flat) == 0 and not polygon.decode(flat).any()

    def bad(match, **kw):
        p = dict(good, **kw)
        for fn in (polygon.validate, polygon.decode, polygon.area, polygon.to_bbox, polygon.to_coco):
            with pytest.raises(ValueError, match=match):
                fn(p)

    for eps in (1, "1", None, True, np.float32(1.0)):
        bad("epsilon of a simplified mask must be a float", epsilon=eps)
    for eps in (0.0, 0.1, 0.3, 64.25, -1.0, float("nan"), float("inf")):
        bad("multiple of 0.25", epsilon=eps)
    bad(">= 3", rings=[tri[:2]])
    bad("leaves", rings=[tri + np.array([1, 0], np.int32)])
    bad("leaves", rings=[tri + np.array([0, 1], np.int32)])
    bad("leaves", rings=[tri - 1])
    bad("no length", rings=[np.array([[0, 0], [0, 0], [4, 1], [1, 3]], np.int32)])
    bad("no length", rings=[np.array([[0, 0], [4, 1], [1, 3], [0, 0]], np.int32)])     # the closing edge
    bad("int32 array", rings=[tri.astype(np.int64)])
    bad("must be a bool", holes=[1])
    bad("one length", holes=[])
    bad("size must be", size=[3])
    # without the key the same rings are no traced polygon: the dict is checked exactly as before
    traced = {k: v for k, v in good.items() if k != "epsilon"}
    with pytest.raises(ValueError, match="even number >= 4"):
        polygon.validate(traced)
    sq = np.array([[0, 0], [2, 0], [2, 2], [0, 2]], np.int32)
    plain = {"size": [3, 4], "rings": [sq], "holes": [False]}
    assert polygon.validate(plain) == (3, 4) and polygon.area(plain) == 4 and type(polygon.area(plain)) is int
    assert polygon.decode(plain).tolist() == [[255, 255, 0, 0], [255, 255, 0, 0], [0, 0, 0, 0]]
    with pytest.raises(ValueError, match="axis-parallel"):
        polygon.validate(dict(plain, rings=[np.array([[0, 0], [2, 1], [2, 2], [0, 2]], np.int32)]))
    assert polygon.validate(dict(plain, epsilon=0.25)) == (3, 4)                # ... and with it as a general polygon


def test_simplify_checks_its_arguments_before_any_work():
    sq = np.array([[0, 0], [2, 0], [2, 2], [0, 2]], np.int32)
    plain = {"size": [3, 4], "rings": [sq], "holes": [False]}
    for eps in (0, 0.1, 0.26, 64.25, 65, -1, None, "1", True, float("nan")):
        with pytest.raises(ValueError, match="multiple of 0.25"):
            polygon.simplify(plain, eps)
    assert [polygon.check_epsilon(e) for e in (0.25, 1, 2.0, 12, 64, np.float32(0.75), np.int64(3))] == [1, 4, 8, 48, 256, 3, 12]
    with pytest.raises(ValueError, match="simplified already"):
        polygon.simplify(dict(plain, epsilon=1.0), 1)
    with pytest.raises(ValueError, match="even number >= 4"):
        polygon.simplify(dict(plain, rings=[sq[:3]]), 1)
    # a side of 32767 is simplified, one of 32768 refused with the limit named
    for size in ([1, 32768], [32768, 1]):
        with pytest.raises(ValueError, match="<= 32767"):
            polygon.simplify({"size": size, "rings": [], "holes": []}, 1)
    for name in ("row of 32767", "column of 32767"):
        i = NAMES.index(name)
        assert SC.same(polygon.simplify(SC.traced_dict(i), 2), SC.expected(2)[i])
    empty = polygon.simplify({"size": [3, 4], "rings": [], "holes": []}, 1)
    assert empty == {"size": [3, 4], "rings": [], "holes": [], "epsilon": 1.0} and polygon.to_bbox(empty) is None and polygon.area(empty) == 0


def test_simplify_from_rings_slices_and_checks():
    verts = np.array([[0, 0], [4, 0], [0, 4], [2, 2], [3, 2], [3, 3], [2, 3]], np.int32)
    table = np.array([[0, 0, 3, 16, 0], [2, 3, 4, -2, 1]], np.int64)
    got = polygon.simplify_from_rings(verts, table, [(4, 4), (2, 2), (4, 4)], 0.5)
    assert [len(p["rings"]) for p in got] == [1, 0, 1] and got[1] == {"size": [2, 2], "rings": [], "holes": [], "epsilon": 0.5}
    assert np.array_equal(got[0]["rings"][0], verts[:3]) and got[0]["holes"] == [False] and got[2]["holes"] == [True]
    assert got[2]["rings"][0].dtype == np.int32 and all(polygon.validate(p) for p in got)
    for row in ([3, 0, 3, 2, 0], [0, 5, 3, 2, 0], [0, 0, 2, 2, 0], [0, -1, 3, 2, 0], [0, 0, 3, 2, 2]):
        with pytest.raises(RuntimeError, match="ring row"):
            polygon.simplify_from_rings(verts, np.array([row], np.int64), [(4, 4)] * 3, 0.5)
    with pytest.raises(ValueError, match="multiple of 0.25"):
        polygon.simplify_from_rings(verts, table, [(4, 4)] * 3, 0.3)
    # from_rings is what it was
    four = polygon.from_rings(verts[3:], np.array([[0, 0, 4, 2]], np.int64), [(4, 4)])
    assert "epsilon" not in four[0] and np.array_equal(four[0]["rings"][0], verts[3:])


def test_simplify_core_header_under_sanitizers_equals_the_oracle(tmp_path):
    """csrc/simplify_core.h - the header the HIP kernels include - compiled by g++ into tests/simplify_core_probe.cpp with the
    address and undefined-behaviour sanitizers and run as a child process: the rings of the small cases at every epsilon, and
    rectangles at the largest coordinates the 64-bit bound admits"""
    exe, data = str(tmp_path / "simplify_core_probe"), str(tmp_path / "rings.txt")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "simplify_core_probe.cpp")])
    small = [i for i, (_, m) in enumerate(SC.cases()) if m.size <= PC.SMALL]
    jobs = [(r, int(4 * eps)) for eps in SC.EPSILONS for i in small for r in SC.traced()[i][0]]
    jobs += [(_ring_of(name), q) for name in ("comb 258", "serpentine", "rectangle 20x15") for q in (1, 4, 47, 48)]
    far = [(0, 0), (32767, 0), (32767, 8191), (0, 8191)]                       # (h + 1) (w + 1) = 2^28: |cross| = 2 h w, the largest there is
    jobs += [(far, q) for q in (1, 256)] + [([(0, 0), (8191, 0), (8191, 32767), (0, 32767)], q) for q in (1, 256)]
    assert len(jobs) >= 100
    with open(data, "w") as f:
        f.write("%d\n" % len(jobs))
        for r, q in jobs:
            f.write("%d %d\n" % (len(r), q) + "".join("%d %d\n" % v for v in r))
    r = subprocess.run([exe, data], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-2000:]
    lines = out.splitlines()
    assert len(lines) == 2 * len(jobs)
    for k, (ring, q) in enumerate(jobs):
        want = SC.oracle_kept(ring, q)
        assert lines[2 * k].split() == ["ring", str(k), str(len(want))], (k, q)
        assert [int(v) for v in lines[2 * k + 1].split()] == want, (k, q)


def test_launcher_rejects_bad_arguments_on_the_host(built):
    """cris_polygon_simplify checks its operands and every descriptor before any launch; the work size is host arithmetic"""
    from cris.pytorch_amd import hip
    l = hip.load()
    d = (hip.EvalDesc * 2)()
    mat = (C.c_double * 6)(1, 0, 0, 0, 1, 0)

    def fill(i=0, w=5, h=4):
        assert l.cris_eval_desc_fill(C.addressof(d[i]), mat, w, h, 0, 0, (w + 3) // 4 * 4, 0, 0) == 0

    def simplify(vertices=0x1000, rings=0x2000, header=0x3000, total=8, ring_cap=2, q=4, host=None, n=1, work=0x5000, work_bytes=1 << 12,
                 out_vertices=0x6000, out_vertex_cap=8, out_rings=0x7000, out_ring_cap=2, out_header=0x8000):
        host = C.addressof(d) if host is None else host
        return l.cris_polygon_simplify(vertices, rings, header, total, ring_cap, q, host or None, n, work, work_bytes, out_vertices,
                                       out_vertex_cap, out_rings, out_ring_cap, out_header, None)

    def rejected(msg, **kw):
        assert simplify(**kw) != 0, (msg, kw)
        err = l.cris_last_error()
        assert b"cris_polygon_simplify" in err and msg in err, (kw, err)

    fill()
    for k in ("vertices", "rings", "header", "work", "out_vertices", "out_rings", "out_header"):
        rejected(b"null operand", **{k: None})
    rejected(b"null operand", host=0)
    for k, v in (("rings", 0x2004), ("header", 0x3004), ("work", 0x5004), ("out_rings", 0x7004), ("out_header", 0x8004), ("vertices", 0x1002),
                 ("out_vertices", 0x6002)):
        rejected(b"aligned", **{k: v})
    for q in (0, -1, 257, 1024):
        rejected(b"q = 4 * epsilon must be in 1 .. 256", q=q)
    for total in (0, 3, -8, 2 ** 30 + 1):
        rejected(b"total_vertices must be in 4 .. 2^30", total=total)
    for cap in (0, -1, 2 ** 28 + 1):
        rejected(b"ring_cap must be in 1 .. 2^28", ring_cap=cap)
    for n in (0, -1, 65536):
        rejected(b"n must be in 1 .. 65535", n=n)
    rejected(b"out_vertex_cap must be >= total_vertices", out_vertex_cap=7)
    rejected(b"out_vertex_cap must be >= total_vertices", out_ring_cap=1)
    # the size limit: a side of 32767 passes this check (and fails the next one, the work size), 32768 is refused by name
    fill(w=32767, h=1)
    rejected(b"work buffer is too small", work_bytes=0)
    fill(w=1, h=32767)
    rejected(b"work buffer is too small", work_bytes=0)
    for w, h in ((32768, 1), (1, 32768), (0, 4), (5, -1)):
        fill(w=w, h=h)
        rejected(b"h_out and w_out must be in 1 .. 32767")
    fill()
    fill(1, w=32768, h=2)
    rejected(b"h_out and w_out must be in 1 .. 32767", n=2)                     # the second descriptor is checked too
    assert simplify(n=1, work_bytes=0) != 0 and b"work buffer" in l.cris_last_error()       # ... and only when n says so
    # the work buffer: 4 64-bit words per ring row, one rank word per vertex, one staged word and one 64-bit key slot per position
    # (a ring has one position more than vertices), each part rounded up to 8 bytes
    assert l.cris_polygon_simplify_work_bytes(8, 2) == 64 + 32 + 40 + 80
    assert l.cris_polygon_simplify_work_bytes(1026, 256) == 8192 + 4104 + 5128 + 10256
    assert l.cris_polygon_simplify_work_bytes(5, 1) == 32 + 24 + 24 + 48
    assert [l.cris_polygon_simplify_work_bytes(t, 1) for t in (0, 3, -4, 2 ** 30 + 1)] == [0, 0, 0, 0]
    assert [l.cris_polygon_simplify_work_bytes(8, c) for c in (0, -1, 2 ** 28 + 1)] == [0, 0, 0]
    rejected(b"work buffer is too small", work_bytes=64 + 32 + 40 + 80 - 1)


def test_symbols_are_declared_bound_and_the_abi_stays_8(built):
    from cris.pytorch_amd import hip
    src = open(HEADER).read()
    plain = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = {m.group(2): (m.group(1), [x.strip() for x in m.group(3).split(",")])
              for m in re.finditer(r"\b(int|size_t)\s+(cris_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", plain)}

    def ctype_of(decl):
        if "*" in decl:
            return C.c_void_p
        return C.c_longlong if decl.startswith("long long") else {"int": C.c_int, "size_t": C.c_size_t}[decl.split()[0]]
    for name, nargs, res in (("cris_polygon_simplify_work_bytes", 2, C.c_size_t), ("cris_polygon_simplify", 16, C.c_int)):
        assert name in hip.EXPORTS and getattr(hip.load(), name) is not None
        got_res, args = hip._SIGS[name]
        assert got_res is res and protos[name][0] == ("size_t" if res is C.c_size_t else "int")
        assert len(args) == nargs and args == [ctype_of(x) for x in protos[name][1]], name
    assert hip.ABI_VERSION == 8 == hip.load().cris_abi_version()
    comment = src[src.index("/* CRIS_ABI_VERSION moves"):src.index("#define CRIS_ABI_VERSION")]
    assert comment.index("cris_polygon_trace_work_bytes") < comment.index("cris_polygon_simplify / cris_polygon_simplify_work_bytes")
    from cris.pytorch_amd.csrc import build
    assert "simplify.hip" in build.SOURCES and build.SOURCES[-1] == "rle.hip" and len(set(build.SOURCES)) == len(build.SOURCES)
    pg = open(os.path.join(ROOT, "cris", "pytorch_amd", "csrc", "polygon.hip")).read()
    assert "simplify" not in pg and "sp_" not in pg                             # the tracer is untouched


def test_argument_checks_come_before_any_device_work(capsys):
    import torch
    from cris.pytorch_amd import evalpost, predict
    jpg = b"\xff\xd8\xff\xe0fake"
    # polygon_collect: a bad epsilon is refused before the tensors are even looked at; a good one reaches the device check
    st = NS(out_bytes=64, n=1)
    for eps in (0.1, 0, 65, "1", True):
        with pytest.raises(ValueError, match="multiple of 0.25"):
            evalpost.polygon_collect(torch.zeros(64, dtype=torch.uint8), st, torch.zeros(2, dtype=torch.int64), simplify=eps)
    with pytest.raises(RuntimeError, match="GPU only"):
        evalpost.polygon_collect(torch.zeros(64, dtype=torch.uint8), st, torch.zeros(2, dtype=torch.int64), simplify=1.0)
    # Predictor and predict
    for eps in (0.1, 0, 65, "1", True):
        with pytest.raises(ValueError, match="multiple of 0.25"):
            predict.Predictor(NS(), _NoDevice(), simplify=eps)
    assert predict.Predictor(NS(), _NoDevice()).simplify is None and predict.Predictor(NS(), _NoDevice(), simplify=2).simplify == 2.0
    p = predict.Predictor(NS(), _NoDevice(), thr=0.35, simplify=1)
    for mode in ("host", "device", "rle", None):
        with pytest.raises(ValueError, match="simplify is valid only with masks='polygon'"):
            p.predict([jpg], ["a"], masks=mode, simplify=1.0)
        assert predict._check_simplify("default", 1.0, mode) is None            # the constructor's applies to polygons alone
    assert predict._check_simplify("default", 1.0, "polygon") == 1.0 and predict._check_simplify("default", None, "polygon") is None
    assert predict._check_simplify(None, 1.0, "polygon") is None and predict._check_simplify(0.25, None, "polygon") == 0.25
    for eps in (0.1, 64.5, "x", False):
        with pytest.raises(ValueError, match="multiple of 0.25"):
            p.predict([jpg], ["a"], masks="polygon", simplify=eps)
    with pytest.raises(ValueError, match="no images"):
        p.predict([], [], masks="polygon", simplify=1.0)
    assert p._ring is None and p._cc_masks is None and p._pg_work is None and p._pg_buffers is None     # nothing was allocated
    # the command line: --simplify needs --polygon-json and a valid epsilon, both before the device is looked for
    for args, msg in ((["--out-prefix", "x", "--simplify", "1"], "only with --polygon-json"), (["--rle-json", "x.json", "--simplify", "1"], "only with --polygon-json"),
                      (["--polygon-json", "x.json", "--simplify", "0.3"], "multiple of 0.25"), (["--polygon-json", "x.json", "--simplify", "65"], "multiple of 0.25")):
        with pytest.raises(SystemExit) as e:
            predict.main(["--image", "x.jpg", "--expr", "a"] + args)
        assert e.value.code == 2 and msg in capsys.readouterr().err
