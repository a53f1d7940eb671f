"""Host side of the mask decoders (csrc/decode.hip cris_rle_decode / cris_polygon_fill / cris_mask_decode_work_bytes, csrc/decode_core.h;
evalpost.mask_form / MaskSources / decode_masks_batch / EvalStaging.pack_encoded, records.mask_array, evaluate.score_results;
DESIGN.md 9b): the restatements the kernels use against rle.decode / polygon.decode on every case of tests/decode_cases.py, the
kernels' own arithmetic compiled for the CPU and run under the sanitizers, every mask form, the validators, the source table's
layout, the staging's host arithmetic, the ABI pins and the launchers' rejections through the library.  Every comparison is an
equality.  No GPU."""
import ctypes as C
import io
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import decode_cases as DC
from cris.pytorch_amd import polygon, rle
from test_predict_cpu import _NoDevice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cris_hip.h")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()


def test_the_cases_cover_what_they_claim():
    names = [k for k, _ in DC.masks()]
    assert names[:len(DC.RC.cases())] == [k for k, _ in DC.RC.cases()]                  # every mask of rle_cases, unchanged
    shapes = {m.shape for _, m in DC.masks()}
    assert {(1, 1), (1, 130), (130, 1), (7, 5), (33, 64), (33, 65), (45, 67), (97, 131), (35, 66), (480, 640)} <= shapes
    assert {DC.pitch_of(w) - w for _, w in shapes} == {0, 1, 2, 3}
    frame = dict(DC.masks())["touches all four sides"]
    v = np.concatenate(polygon.encode(frame)["rings"])
    assert v[:, 0].max() == frame.shape[1] and v[:, 1].max() == frame.shape[0] and v.min() == 0
    hole = polygon.encode(dict(DC.masks())["ellipse with a hole 97x131"])
    assert hole["holes"] == [False, True]
    assert any(len(r["counts"]) > 256 for _, r in DC.rle_sources() if isinstance(r["counts"], list))
    assert any(isinstance(r["counts"], str) for _, r in DC.rle_sources())
    assert len(DC.polygon_sources()) >= 4 * len(DC.masks()) + 10


def test_searchsorted_restatement_equals_rle_decode_on_every_case():
    for (name, r), want in zip(DC.rle_sources(), DC.expected_rle()):
        h, w, counts = rle._parts(r)
        assert want.shape == (h, w) and want.dtype == np.uint8
        assert np.array_equal(DC.searchsorted_decode(h, w, counts), want), name
    assert DC.expected_rle()[[k for k, _ in DC.rle_sources()].index("1x1 [0, 1]")].tolist() == [[255]]
    for (name, m), want in zip(DC.masks(), DC.expected_rle()):                           # and the oracle inverts the encoder
        assert np.array_equal(want, (m != 0).astype(np.uint8) * 255), name


def test_scalar_fill_with_the_floor_equals_polygon_decode_on_every_case():
    floors = 0
    for (name, p), want in zip(DC.polygon_sources(), DC.expected_polygon()):
        h, w = p["size"]
        assert np.array_equal(DC.scalar_fill(h, w, p["rings"]), want), name
        if "epsilon" not in p:                                              # the traced form needs no rule of its own
            assert np.array_equal(polygon._decode_general(p["rings"], h, w), want), name
    for (name, m), (k, p), want in zip(DC.masks(), DC.polygon_sources()[::1 + len(DC.EPSILONS)], DC.expected_polygon()[::1 + len(DC.EPSILONS)]):
        assert k == "polygon " + name and np.array_equal(want, (m != 0).astype(np.uint8) * 255), name
    # the cases do reach a negative numerator that the divisor does not divide: truncation would differ there
    for _, p in DC.polygon_sources():
        for r in p["rings"]:
            r = r.astype(np.int64)
            for (ax, ay), (bx, by) in zip(r.tolist(), np.roll(r, -1, axis=0).tolist()):
                if by < ay:
                    ax, ay, bx, by = bx, by, ax, ay
                for py in range(ay, by):
                    a, b = (by - ay) - (2 * py + 1 - 2 * ay) * (bx - ax), 2 * (by - ay)
                    floors += a < 0 and a % b != 0
    assert floors > 100
    empty = DC.expected_polygon()[[k for k, _ in DC.polygon_sources()].index("two identical rings")]
    assert not empty.any()
    assert DC._trunc_div(-3, 2) == -1 and -3 // 2 == -2 and DC._trunc_div(3, 2) == 1 and DC._trunc_div(-4, 2) == -2


def _write_probe_input(path):
    with open(path, "w") as f:
        f.write("%d\n" % (len(DC.rle_sources()) + len(DC.polygon_sources())))
        for _, r in DC.rle_sources():
            h, w, counts = rle._parts(r)
            f.write("R %d %d %d %s\n" % (h, w, counts.size, " ".join(str(int(c)) for c in counts)))
        for _, p in DC.polygon_sources():
            h, w = p["size"]
            f.write("P %d %d %d" % (h, w, len(p["rings"])))
            for r in p["rings"]:
                f.write(" %d %s" % (r.shape[0], " ".join(str(int(v)) for v in r.reshape(-1))))
            f.write("\n")


def test_decode_core_under_the_sanitizers_equals_the_oracles(tmp_path):
    """csrc/decode_core.h - the header the HIP kernels include - compiled by g++ into tests/decode_core_probe.cpp with the address and
    undefined-behaviour sanitizers and run as a child process on every case: the scan, the upper-bound search, the crossings with their
    floor, the toggles, the prefix parity with its carry and the dword stores, in exact-size vectors"""
    exe, data = str(tmp_path / "decode_core_probe"), str(tmp_path / "cases.txt")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "decode_core_probe.cpp")])
    _write_probe_input(data)
    r = subprocess.run([exe, data], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = io.StringIO(r.stdout.decode())
    names = [k for k, _ in DC.rle_sources()] + [k for k, _ in DC.polygon_sources()]
    for i, (name, want) in enumerate(zip(names, DC.expected_rle() + DC.expected_polygon())):
        h, w = want.shape
        assert lines.readline().split() == ["mask", str(i), str(h), str(w), str(DC.pitch_of(w))], name
        rows = [lines.readline().rstrip("\n") for _ in range(h)]
        padded = np.zeros((h, DC.pitch_of(w)), np.uint8)
        padded[:, :w] = want != 0
        assert rows == ["".join("01"[v] for v in row) for row in padded.tolist()], name  # the zero padding included
    assert lines.readline() == ""


def _png(mask):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(mask).save(buf, format="PNG")
    return buf.getvalue()


def test_mask_array_and_mask_form_take_every_form():
    pytest.importorskip("PIL")
    from cris.pytorch_amd import evalpost, records
    from cris.pytorch_amd.predict import Prediction
    m = dict(DC.masks())["ellipse with a hole 97x131"]
    r, p = rle.encode(m), polygon.encode(m)
    s = polygon.simplify(p, 1.0)
    forms = {"png": _png(m), "rle bytes": r, "rle str": rle.to_json(r), "rle list": {"size": [97, 131], "counts": rle._parts(r)[2].tolist()},
             "polygon": p}
    for name, f in forms.items():
        got = records.mask_array({"mask": f, "seg_id": 5})
        got = got.numpy() if torch.is_tensor(got) else got
        assert got.dtype == np.uint8 and np.array_equal(got, m), name
        kind, h, w, _ = evalpost.mask_form(f)
        assert (h, w) == (97, 131) and kind == {"png": "array", "polygon": "polygon"}.get(name, "rle"), name
        assert np.array_equal(evalpost.mask_to_array(evalpost.mask_form(f)), m), name
    assert torch.is_tensor(records.mask_array({"mask": forms["png"]}))                   # PNG records: what pngdec returns, as before
    assert np.array_equal(records.mask_array({"mask": s}), polygon.decode(s))
    assert evalpost.mask_form(m)[0] == "array" and evalpost.mask_form(torch.from_numpy(m))[3].data_ptr() == torch.from_numpy(m).data_ptr()
    assert evalpost.mask_form(Prediction("a", rle.to_json(r), 1, None, 0.5))[0] == "rle"
    assert evalpost.mask_form(Prediction("a", m, 1, None, 0.5))[0] == "array"
    assert evalpost.MASK_KINDS == ("array", "rle", "polygon")


def test_validators_refuse_bad_input_before_any_work():
    from cris.pytorch_amd import evalpost, records
    m = np.zeros((4, 6), np.uint8)
    bad = [({"size": [4, 6], "counts": [23]}, "sum to 23"), ({"size": [4, 6], "counts": [25, -1]}, "negative"),
           ({"size": [4, 6], "counts": "\x7f"}, "alphabet"), ({"size": [4], "counts": [4]}, "expected"),
           ({"size": [4, 6], "rings": [np.array([[0, 0], [7, 0], [7, 4], [0, 4]], np.int32)], "holes": [False]}, "leaves"),
           ({"size": [4, 6], "rings": [np.array([[0, 0], [3, 3], [0, 3]], np.int32)], "holes": [False]}, "even number"),
           ({"size": [4, 6], "rings": [np.array([[0, 0], [3, 3]], np.int32)], "holes": [False], "epsilon": 1.0}, ">= 3"),
           ({"size": [4, 6], "rings": [], "holes": [True]}, "one length"),
           ([[0, 0, 4, 0, 4, 4]], "flat polygon lists are not accepted"), ([0, 0, 4, 0, 4, 4], "exchange RLE"),
           (m.astype(np.float32), "uint8"), (m[0], "uint8"), (b"not a png", ""), (None, "expected a uint8 array"), (7, "expected")]
    for value, msg in bad:
        with pytest.raises(ValueError, match="entry 3: .*" + msg):
            evalpost.mask_form(value, "entry 3")
        if not isinstance(value, (bytes, np.ndarray)):
            with pytest.raises(ValueError, match="record 9: mask"):
                records.mask_array({"mask": value, "seg_id": 9})
    ok = evalpost.mask_form({"size": [4, 6], "counts": [24]})
    for forms, slots, msg in (([], [], "1 .. 65535"), ([ok], [], "one slot per mask"), ([ok], [(0, 6)], "pitch"), ([ok], [(0, 4)], "pitch"),
                              ([ok], [(2, 8)], "offset"), ([ok], [(-4, 8)], "offset"), ([evalpost.mask_form(m)], [(0, 8)], "RLE or a polygon"),
                              ([evalpost.mask_form({"size": [0, 6], "counts": []})], [(0, 8)], "positive size")):
        with pytest.raises(ValueError, match="MaskSources: .*" + msg):
            evalpost.MaskSources(forms, slots)
    srcs = evalpost.MaskSources([ok], [(0, 8)])
    cpu = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(ValueError, match="srcs must be"):
        evalpost.decode_masks_batch([ok], cpu)
    with pytest.raises(ValueError, match="holds every slot"):
        evalpost.decode_masks_batch(srcs, cpu[:31])
    with pytest.raises(ValueError, match="holds every slot"):
        evalpost.decode_masks_batch(srcs, cpu.to(torch.int32))
    with pytest.raises(RuntimeError, match="GPU only"):
        evalpost.decode_masks_batch(srcs, cpu)
    with pytest.raises(ValueError, match="srcs must be"):
        evalpost.decode_work(None, "cpu")
    with pytest.raises(ValueError, match="layout"):
        evalpost.desc_slots(None, "gt")


def test_mask_sources_layout(built):
    """the packing helper: one block of bytes holding the source table, the ring table, the vertices and the counts"""
    from cris.pytorch_amd import evalpost, hip
    assert C.sizeof(hip.MaskSrc) == 40 == hip.load().cris_sizeof(b"cris_mask_src") and hip.STRUCTS["cris_mask_src"] is hip.MaskSrc
    assert (hip.MASK_RLE, hip.MASK_POLYGON) == (0, 1)
    m = dict(DC.masks())["ellipse with a hole 97x131"]
    tri = dict(DC.polygon_sources())["both triangles"]
    items = [rle.encode(m), polygon.encode(m), {"size": [3, 7], "counts": [0, 4, 6, 11, 0, 0]}, tri, polygon.encode(np.zeros((5, 5), np.uint8))]
    forms = [evalpost.mask_form(x) for x in items]
    slots = [(0, 132), (12816, 132), (25632, 8), (25664, 8), (25712, 8)]
    s = evalpost.MaskSources(forms, slots)
    assert (s.n, s.n_rle, s.n_polygon, s.n_rings, s.out_bytes) == (5, 2, 3, 4, 25712 + 40) and s.blob.dtype == np.uint8
    assert s.rings_off == 200 and s.vertices_off == 200 + 24 * 4 and s.counts_off == s.vertices_off + 8 * s.n_vertices
    assert s.blob.size == (s.counts_off + 4 * s.n_counts + 7) // 8 * 8 and s.host_addr is None and s.dev_addr is None
    table = (hip.MaskSrc * 5).from_buffer_copy(s.blob[:200].tobytes())
    counts = s.blob[s.counts_off:s.counts_off + 4 * s.n_counts].view(np.uint32)
    rings = s.blob[s.rings_off:s.rings_off + 24 * s.n_rings].view(np.int64).reshape(-1, 3)
    verts = s.blob[s.vertices_off:s.vertices_off + 8 * s.n_vertices].view(np.int32).reshape(-1, 2)
    c0 = rle._parts(items[0])[2]
    assert [(t.dst_off, t.pitch, t.h, t.w, t.kind) for t in table] == [(0, 132, 97, 131, 0), (12816, 132, 97, 131, 1), (25632, 8, 3, 7, 0),
                                                                         (25664, 8, 6, 7, 1), (25712, 8, 5, 5, 1)]
    assert [(t.pay_off, t.pay_len) for t in table] == [(0, c0.size), (0, 2), (c0.size, 6), (2, 2), (4, 0)]
    assert counts.tolist() == c0.tolist() + [0, 4, 6, 11, 0, 0]
    want_rings = items[1]["rings"] + tri["rings"]
    assert rings[:, 0].tolist() == [1, 1, 3, 3] and rings[:, 2].tolist() == [r.shape[0] for r in want_rings]
    assert rings[:, 1].tolist() == np.cumsum([0] + [r.shape[0] for r in want_rings[:-1]]).tolist()
    assert np.array_equal(verts, np.concatenate(want_rings))
    l = hip.load()
    # the scratch: n slots of the largest of ceil(counts / 2) and h * ceil(w / 64) 64-bit words
    assert l.cris_mask_decode_work_bytes(s.blob.ctypes.data_as(C.c_void_p), 5) == 5 * 8 * max(97 * 3, (c0.size + 1) // 2)
    only = evalpost.MaskSources(forms[2:3], [(0, 8)])
    assert l.cris_mask_decode_work_bytes(only.blob.ctypes.data_as(C.c_void_p), 1) == 8 * 3
    assert l.cris_mask_decode_work_bytes(None, 1) == 0 and l.cris_mask_decode_work_bytes(s.blob.ctypes.data_as(C.c_void_p), 0) == 0
    assert l.cris_mask_decode_work_bytes(s.blob.ctypes.data_as(C.c_void_p), 65536) == 0
    with pytest.raises(ValueError, match="8-byte aligned"):
        s.place(s.blob.ctypes.data + 4, 0x1000)
    assert s.place(s.blob.ctypes.data, 0x1000).dev_addr == 0x1000


def test_staging_packs_encoded_masks_next_to_the_tables(built):
    """EvalStaging.pack_encoded on the host: host-decoded masks first, the same slots `pack` computes, sources and payload below
    mask_base, and an upload that ends with the last host-decoded mask - or with the payload"""
    from cris.pytorch_amd import evalpost, hip
    rng = np.random.default_rng(2)
    masks = [(rng.random((h, w)) < 0.5).astype(np.uint8) * 255 for h, w in ((9, 5), (33, 65), (7, 12), (20, 3))]
    ident = np.array([[1.0, 0, 0], [0, 1.0, 0]])
    descs = [(ident, 0, 0, 0), (ident, 1, 0, 1), (ident, 1, 1, 2), (ident, 2, 0, 3), (ident, 3, 0, 4)]
    given = [rle.encode(masks[0]), masks[1], polygon.encode(masks[2]), torch.from_numpy(masks[3])]
    forms = [evalpost.mask_form(x) for x in given]
    st = evalpost.EvalStaging(None, max_descs=4, mask_bytes=64).pack_encoded(forms, descs)
    ref = evalpost.EvalStaging(None).pack([masks[1], masks[3], masks[0], masks[2]], [(ident, {0: 2, 1: 0, 2: 3, 3: 1}[mi], mp, row) for _, mi, mp, row in descs])
    assert (st.n, st.mask_bytes, st.out_bytes) == (ref.n, ref.mask_bytes, ref.out_bytes) == (5, st.mask_bytes, st.out_bytes)
    for i in range(5):
        a, b = st.descs[i], ref.descs[i]
        assert (a.mask_off, a.out_off, a.pitch, a.h_out, a.w_out, a.row, a.map) == (b.mask_off, b.out_off, b.pitch, b.h_out, b.w_out, b.row, b.map)
    assert st.descs[1].mask_off == st.descs[2].mask_off == 0                             # two descriptors, one mask, decoded once
    srcs, end = st._pending
    host_bytes = 33 * 68 + (20 * 4 + 15) // 16 * 16 + (-(33 * 68) % 16)
    assert end == st.mask_base + host_bytes and (srcs.n, srcs.n_rle, srcs.n_polygon) == (2, 1, 1)
    assert np.array_equal(st._bytes[st.mask_base:st.mask_base + host_bytes], ref._bytes[ref.mask_base:ref.mask_base + host_bytes])
    aux = (5 * C.sizeof(hip.EvalDesc) + 15) // 16 * 16
    assert srcs.host_addr == st.host.data_ptr() + aux and aux + srcs.blob.size <= st.mask_base and st.max_descs > 5
    assert np.array_equal(st._bytes[aux:aux + srcs.blob.size], srcs.blob)
    table = (hip.MaskSrc * 2).from_buffer_copy(srcs.blob[:80].tobytes())
    assert [(t.dst_off, t.kind) for t in table] == [(st.descs[0].mask_off, 0), (st.descs[3].mask_off, 1)]
    # no host-decoded mask at all: the upload is the tables and the payload only
    st.pack_encoded([forms[0], forms[2]], [(ident, 0, 0, 0), (ident, 1, 0, 1)])
    srcs, end = st._pending
    assert end == (2 * C.sizeof(hip.EvalDesc) + 15) // 16 * 16 + srcs.blob.size < st.mask_base and st.mask_bytes > 0
    # host-decoded masks only: `pack`'s bytes, and nothing to decode
    st.pack_encoded([forms[1], forms[3]], [(ident, 0, 0, 0), (ident, 1, 0, 1)])
    assert st._pending == (None, st.mask_base + st.mask_bytes)


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
    for name, nargs, res in (("cris_mask_decode_work_bytes", 2, C.c_size_t), ("cris_rle_decode", 10, C.c_int), ("cris_polygon_fill", 14, C.c_int)):
        assert name in hip.EXPORTS and getattr(hip.load(), name) is not None
        got_res, args = hip._SIGS[name]
        assert got_res is res and protos[name][0] == ("size_t" if res is C.c_size_t else "int")
        assert len(args) == nargs and args == [ctype_of(x) for x in protos[name][1]], name
    assert hip.ABI_VERSION == 8 == hip.load().cris_abi_version() == int(re.search(r"#define CRIS_ABI_VERSION (\d+)", src).group(1))
    comment = src[src.index("/* CRIS_ABI_VERSION moves"):src.index("#define CRIS_ABI_VERSION")]
    assert comment.index("cris_polygon_simplify") < comment.index("cris_rle_decode") < comment.index("cris_mask_decode_work_bytes")
    assert "cris_polygon_fill" in comment and "cris_mask_src" in comment
    for name, value in (("CRIS_MASK_RLE", 0), ("CRIS_MASK_POLYGON", 1)):
        assert re.search(r"#define %s %d\b" % (name, value), src), name
    assert hip.load().cris_sizeof(b"cris_eval_desc") == 88


def test_launchers_reject_bad_arguments_on_the_host(built):
    """both launchers check their operands, the whole table and the payload's extent before any launch"""
    from cris.pytorch_amd import hip
    l = hip.load()
    t = (hip.MaskSrc * 2)()
    rings = (C.c_longlong * 9)(0, 0, 4, 0, 4, 3, 1, 7, 3)

    def fill(i=0, kind=0, h=4, w=5, pitch=8, dst_off=0, pay_off=0, pay_len=2):
        t[i].kind, t[i].h, t[i].w, t[i].pitch, t[i].dst_off, t[i].pay_off, t[i].pay_len = kind, h, w, pitch, dst_off, pay_off, pay_len

    def rdec(host=None, dev=0x1000, n=1, counts=0x2000, words=8, work=0x3000, work_bytes=1 << 12, out=0x4000, out_bytes=64):
        host = C.addressof(t) if host is None else host
        return l.cris_rle_decode(host or None, dev, n, counts, words, work, work_bytes, out, out_bytes, None)

    def pfill(host=None, dev=0x1000, n=1, verts=0x2000, pairs=10, rh=None, rd=0x5000, rows=3, stride=3, work=0x3000, work_bytes=1 << 12,
              out=0x4000, out_bytes=64):
        host = C.addressof(t) if host is None else host
        rh = C.addressof(rings) if rh is None else rh
        return l.cris_polygon_fill(host or None, dev, n, verts, pairs, rh or None, rd, rows, stride, work, work_bytes, out, out_bytes, None)

    def rejected(fn, msg, **kw):
        assert fn(**kw) != 0, (msg, kw)
        err = l.cris_last_error()
        assert (b"cris_rle_decode" if fn is rdec else b"cris_polygon_fill") in err and msg in err, (kw, err)

    fill()
    for k in ("dev", "counts", "work", "out"):
        rejected(rdec, b"null operand", **{k: None})
    rejected(rdec, b"null operand", host=0)
    for k in ("dev", "verts", "rd", "work", "out"):
        rejected(pfill, b"null operand", **{k: None})
    for k in ("host", "rh"):
        rejected(pfill, b"null operand", **{k: 0})
    for fn in (rdec, pfill):
        fill(kind=0 if fn is rdec else 1)
        for n in (0, -1, 65536):
            rejected(fn, b"n must be in 1 .. 65535", n=n)
        rejected(fn, b"aligned", work=0x3004)
        rejected(fn, b"aligned", out=0x4002)
        rejected(fn, b"aligned", dev=0x1004)
        for pitch in (6, 4, 7):
            fill(kind=t[0].kind, pitch=pitch)
            rejected(fn, b"pitch must be a multiple of 4")
        for h, w in ((0, 5), (4, 0), (-3, 5), (46341, 46341)):
            fill(kind=t[0].kind, h=h, w=w, pitch=(max(w, 1) + 3) // 4 * 4)
            rejected(fn, b"bad size")
        fill(kind=t[0].kind, dst_off=-8)
        rejected(fn, b"slot outside the buffer")
        fill(kind=t[0].kind, dst_off=2)
        rejected(fn, b"slot outside the buffer")
        fill(kind=t[0].kind, h=9)                                           # 72 bytes in a buffer of 64
        rejected(fn, b"slot outside the buffer")
        fill(kind=t[0].kind, dst_off=32)
        rejected(fn, b"slot outside the buffer", out_bytes=63)
        fill(kind=5)
        rejected(fn, b"kind must be")
        fill(kind=t[0].kind if t[0].kind < 2 else 0, pay_len=-1)
        rejected(fn, b"negative payload")
        fill(kind=0 if fn is rdec else 1)
        fill(1, kind=1 if fn is rdec else 0, pitch=6)                       # a bad row of the OTHER kind is refused as well
        rejected(fn, b"pitch must be a multiple of 4", n=2)
    # the payload's extent and the work buffer
    fill(kind=0, pay_off=3, pay_len=6)
    rejected(rdec, b"counts outside the payload", words=8)
    fill(kind=0, pay_len=100)
    rejected(rdec, b"the work buffer is too small", words=100, work_bytes=8 * 50 - 1)
    fill(kind=0)
    fill(1, kind=1, h=33, w=65, pitch=68, dst_off=32, pay_len=0)            # the largest slot of EITHER kind sizes every slot
    rejected(rdec, b"the work buffer is too small", n=2, out_bytes=32 + 68 * 33, work_bytes=2 * 8 * 66 - 1)
    assert l.cris_mask_decode_work_bytes(C.addressof(t), 2) == 2 * 8 * 66
    rejected(rdec, b"aligned", counts=0x2002)
    rejected(pfill, b"aligned", verts=0x2004)
    for stride in (2, 9):
        rejected(pfill, b"ring_stride must be in 3 .. 8", stride=stride)
    fill(kind=1, pay_off=2, pay_len=2)
    rejected(pfill, b"ring rows outside the table")
    fill(kind=1, pay_off=0, pay_len=3)                                      # the third row names mask 1
    rejected(pfill, b"names another mask")
    fill(kind=1, pay_len=2)
    rejected(pfill, b"vertices outside the payload", pairs=6)
    rings[4] = 5                                                            # a gap between the two rings of one mask
    rejected(pfill, b"must follow each other")
    rings[4] = 4
    rings[5] = 0
    rejected(pfill, b"vertices outside the payload")                        # a ring of no vertices
    rings[5] = 3
    fill(kind=1, h=16384, w=16384, pitch=16384, pay_len=2)                  # 2^28 pixels, 16385^2 corners
    rejected(pfill, b"(h + 1) * (w + 1)", out_bytes=1 << 30)


def test_entry_points_check_their_arguments_before_any_device_work():
    from cris.pytorch_amd import evaluate
    m = np.zeros((4, 6), np.uint8)
    r = rle.encode(m)
    for bad, msg in (((([r], [r, r], "cuda"), {}), "equally long"), ((([], [], "cuda"), {}), "non-empty"),
                     ((([r], [r], "cuda"), {"batch": 0}), "batch must be"), ((([r], [r], "cuda"), {"batch": 2.5}), "batch must be"),
                     ((([r], [r], "cuda"), {"boundary": 3}), "score_results: boundary")):
        with pytest.raises(ValueError, match=msg):
            evaluate.score_results(*bad[0], **bad[1])
    with pytest.raises(RuntimeError, match="GPU only"):
        evaluate.score_results([r], [r], "cpu")
    ev = evaluate.Evaluator.__new__(evaluate.Evaluator)
    ev.pipe = _NoDevice("val")
    png, params = b"\x89PNG....", [{"mask_dir": "5.png", "ori_size": np.array([4, 6])}] * 2
    seen = []
    ev._masks = lambda recs, prm: seen.append(len(recs)) or ["decoded"] * len(recs)
    assert ev._ground_truth([{"mask": png}, {"mask": bytearray(png)}], params) == (["decoded"] * 2, False) and seen == [2]
    forms, encoded = ev._ground_truth([{"mask": r}, {"mask": polygon.encode(m)}], params)
    assert encoded and [f[:3] for f in forms] == [("rle", 4, 6), ("polygon", 4, 6)] and seen == [2]
    with pytest.raises(ValueError, match="record 5.png: mask is \\(3, 6\\), image \\(4, 6\\)"):
        ev._ground_truth([{"mask": r}, {"mask": rle.encode(m[:3])}], params)
    with pytest.raises(ValueError, match="record 5.png: .*sum to"):
        ev._ground_truth([{"mask": {"size": [4, 6], "counts": [7]}}], params[:1])
    res = evaluate.ScoreResult(np.array([[5, 10], [0, 4], [9, 10]]), np.array([[1, 2], [0, 1], [3, 4]]))
    assert (res.iou, res.prec, res.overall_iou) == (*evaluate.metrics(res.counts)[:2], evaluate.overall_iou(res.counts))
    assert res.boundary_iou == evaluate.metrics(res.boundary_counts)[0] and res.per_sample.shape == (3,) and res.boundary_per_sample.shape == (3,)
    assert evaluate.ScoreResult(res.counts).boundary_counts is None
