"""Host side of Boundary IoU (evalpost.Boundary / boundary_spec / boundary_radii; csrc/morph.hip cris_erode_masks /
cris_boundary_iou_batch / cris_boundary_work_bytes): the oracle of tests/boundary_cases.py against scipy on every case,
the pinned radii, the spec's validation, the ABI pins, the launchers' rejections through the library, the evaluator's argument
check, and the kernels' per-word arithmetic (csrc/morph_core.h) run on the CPU against a per-pixel loop.  Every comparison is an
equality.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import boundary_cases as BC
from cris.pytorch_amd.evalpost import Boundary
from test_predict_cpu import _NoDevice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cris_hip.h")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()


def test_oracle_equals_scipy_on_every_case():
    ndimage = pytest.importorskip("scipy.ndimage")
    square = np.ones((3, 3), bool)
    nonempty = 0
    for (name, m, d), want in zip(BC.cases(), BC.expected()):
        got = ndimage.binary_erosion(m != 0, structure=square, iterations=d, border_value=0)
        assert np.array_equal(want, got), name
        assert np.array_equal(BC.boundary(m, d), (m != 0) & ~got), name
        nonempty += bool(want.any())
    assert nonempty >= 20 and len(BC.cases()) - nonempty >= 20              # both kinds are well represented
    for (name, p, g, d), want in zip(BC.pairs(), BC.expected_counts()):
        bp = (p != 0) & ~ndimage.binary_erosion(p != 0, structure=square, iterations=d, border_value=0)
        bg = (g != 0) & ~ndimage.binary_erosion(g != 0, structure=square, iterations=d, border_value=0)
        assert want == [int((bp & bg).sum()), int((bp | bg).sum())], name
    # the definition by hand: a 5 x 7 block, d = 1 -> its 3 x 5 inside; d = 2 -> the middle row's 3 pixels
    m = np.zeros((9, 11), np.uint8)
    m[2:7, 2:9] = 1
    assert BC.erode(m, 1).sum() == 15 and BC.erode(m, 1)[3:6, 3:8].all() and BC.erode(m, 2).sum() == 3 and not BC.erode(m, 3).any()
    assert BC.erode(np.ones((5, 7)), 2).sum() == 3 and not BC.erode(np.ones((4, 7)), 2).any()   # outside the image is background


def test_word_arithmetic_of_the_kernels_equals_a_per_pixel_loop(tmp_path):
    """csrc/morph_core.h - the header the HIP kernels include - compiled by g++ into tests/morph_core_probe.cpp with the address and
    undefined-behaviour sanitizers: row pass and column pass against per-pixel loops; an index outside a plane ends the run"""
    exe = str(tmp_path / "morph_core_probe")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "morph_core_probe.cpp")])
    r = subprocess.run([exe, "900"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode()
    assert r.returncode == 0 and out.startswith("ok "), out[-2000:]
    assert int(out.split()[1]) > 5_000_000                                  # bits compared


def test_pinned_radii_and_the_spec():
    from cris.pytorch_amd import evalpost
    spec = Boundary()
    assert (spec.ratio, spec.min_radius) == (0.02, 1)
    for (h, w), d in BC.PINNED:
        assert spec.radius(h, w) == d == BC.radius(h, w), (h, w)
    assert Boundary(0.02, 3).radius(15, 20) == 3 and Boundary(1.0).radius(3, 4) == 5 and Boundary(ratio=0.5, min_radius=2).radius(1, 1) == 2
    assert Boundary(1, 1) == Boundary(1.0) and hash(Boundary(0.02)) == hash(Boundary()) and Boundary(0.03) != Boundary() != Boundary(0.02, 2)
    assert Boundary() != (0.02, 1) and len({Boundary(), Boundary(0.02, 1), Boundary(0.1)}) == 2
    assert repr(Boundary(0.05, 4)) == "Boundary(ratio=0.05, min_radius=4)" and eval(repr(spec), {"Boundary": Boundary}) == spec
    with pytest.raises(AttributeError, match="immutable"):
        spec.ratio = 0.1
    for bad in (0, -0.02, 1.5, float("nan"), float("inf"), "0.02", None, True):
        with pytest.raises(ValueError, match="ratio"):
            Boundary(bad)
    for bad in (0, -1, 1.0, "1", None, True):
        with pytest.raises(ValueError, match="min_radius"):
            Boundary(0.02, bad)
    with pytest.raises(ValueError, match="positive"):
        spec.radius(0, 5)
    assert evalpost.boundary_spec(None, "x") is None and evalpost.boundary_spec(True, "x") == Boundary()
    assert evalpost.boundary_spec(Boundary(0.1), "x") == Boundary(0.1)
    for bad in (False, 1, 0.02, "x", Boundary, (0.02, 1)):
        with pytest.raises(ValueError, match="here: boundary must be None, True or an evalpost.Boundary"):
            evalpost.boundary_spec(bad, "here: boundary")
    from types import SimpleNamespace as NS
    st = NS(n=3, descs=[NS(h_out=480, w_out=640), NS(h_out=75, w_out=100), NS(h_out=1, w_out=1)])
    r = evalpost.boundary_radii(st, spec)
    assert r.dtype == np.int32 and r.tolist() == [16, 2, 1]
    with pytest.raises(ValueError, match="spec"):
        evalpost.boundary_radii(st, True)


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
    for name, nargs, res in (("cris_boundary_work_bytes", 2, C.c_size_t), ("cris_erode_masks", 13, C.c_int), ("cris_boundary_iou_batch", 14, C.c_int)):
        assert name in hip.EXPORTS and getattr(hip.load(), name) is not None
        got_res, args = hip._SIGS[name]
        assert got_res is res and protos[name][0] == ("size_t" if res is C.c_size_t else "int")
        assert len(args) == nargs and args == [ctype_of(x) for x in protos[name][1]], name
    assert hip.ABI_VERSION == 8 == hip.load().cris_abi_version() == int(re.search(r"#define CRIS_ABI_VERSION (\d+)", src).group(1))
    comment = src[src.index("/* CRIS_ABI_VERSION moves"):src.index("#define CRIS_ABI_VERSION")]
    assert comment.index("cris_rle_encode") < comment.index("cris_erode_masks") < comment.index("cris_boundary_iou_batch")
    assert "cris_boundary_work_bytes" in comment
    assert hip.load().cris_sizeof(b"cris_eval_desc") == 88
    # a translation unit of its own, before rle.hip (which stays last)
    from cris.pytorch_amd.csrc import build
    assert build.SOURCES[-1] == "rle.hip" and "morph.hip" in build.SOURCES[:-1] and len(set(build.SOURCES)) == len(build.SOURCES)
    assert "morph_" not in open(os.path.join(ROOT, "cris", "pytorch_amd", "csrc", "evalpost.hip")).read()


def test_launchers_reject_bad_arguments_on_the_host(built):
    """both launchers check their operands, every radius and every descriptor before any launch; the work size is host arithmetic"""
    from cris.pytorch_amd import hip
    l = hip.load()
    d = (hip.EvalDesc * 2)()
    radii = (C.c_int * 2)(1, 1)
    mat = (C.c_double * 6)(1, 0, 0, 0, 1, 0)

    def fill(i=0, w=5, h=4, pitch=None, out_off=0, mask_off=0, row=0):
        assert l.cris_eval_desc_fill(C.addressof(d[i]), mat, w, h, 0, mask_off, (w + 3) // 4 * 4 if pitch is None else pitch, out_off, row) == 0

    def erode(masks=0x1000, mask_bytes=64, host=None, dev=0x2000, n=1, rh=None, rd=0x3000, work=0x5000, work_bytes=1 << 12, out=0x6000,
              out_bytes=64, boundary=0):
        host = C.addressof(d) if host is None else host
        rh = C.addressof(radii) if rh is None else rh
        return l.cris_erode_masks(masks, mask_bytes, host or None, dev, n, rh or None, rd, work, work_bytes, out, out_bytes, boundary, None)

    def biou(pred=0x1000, pred_bytes=64, host=None, dev=0x2000, n=1, gt=0x7000, gt_bytes=64, rh=None, rd=0x3000, work=0x5000, work_bytes=1 << 12,
             counts=0x8000, rows=4):
        host = C.addressof(d) if host is None else host
        rh = C.addressof(radii) if rh is None else rh
        return l.cris_boundary_iou_batch(pred, pred_bytes, host or None, dev, n, gt, gt_bytes, rh or None, rd, work, work_bytes, counts, rows, None)

    def rejected(fn, msg, **kw):
        assert fn(**kw) != 0, (msg, kw)
        err = l.cris_last_error()
        assert (b"cris_erode_masks" if fn is erode else b"cris_boundary_iou_batch") in err and msg in err, (kw, err)

    fill()
    for k in ("masks", "dev", "rd", "work", "out"):
        rejected(erode, b"null operand", **{k: None})
    for k in ("pred", "dev", "gt", "rd", "work", "counts"):
        rejected(biou, b"null operand", **{k: None})
    for fn in (erode, biou):
        rejected(fn, b"null operand", host=0)
        rejected(fn, b"null operand", rh=0)
        for n in (0, -1, 65536):
            rejected(fn, b"n must be in 1 .. 65535", n=n)
        rejected(fn, b"aligned", work=0x5004)
        rejected(fn, b"aligned", rd=0x3002)
        for bad in (0, -3):                                                 # a radius of 0
            radii[0] = bad
            rejected(fn, b"every radius must be >= 1")
        radii[0] = 1
        for pitch in (6, 4, 7):
            fill(pitch=pitch)
            rejected(fn, b"pitch must be a multiple of 4")
        for w, h in ((0, 4), (5, 0), (-3, 4), (46341, 46341)):
            fill(w=w, h=h)
            rejected(fn, b"bad output size")
        fill(out_off=-16)                                                   # a rectangle outside the buffer
        rejected(fn, b"output outside the buffer")
        fill(h=9)                                                           # 72 bytes in a buffer of 64
        rejected(fn, b"output outside the buffer")
        fill()
    rejected(erode, b"boundary must be 0 or 1", boundary=2)
    rejected(erode, b"output outside the buffer", out_bytes=31)             # inside the source, outside `out`
    fill(out_off=64)
    rejected(erode, b"output outside the buffer", mask_bytes=95, out_bytes=96)
    fill(mask_off=48)
    rejected(biou, b"mask outside the buffer")
    fill(mask_off=-4)
    rejected(biou, b"mask outside the buffer")
    for row in (4, -1):
        fill(row=row)
        rejected(biou, b"row out of range")
    fill()
    rejected(biou, b"bad sizes", rows=0)
    rejected(biou, b"aligned", counts=0x8002)
    # the work buffer: four planes of n slots of the batch's largest h * ceil(w / 64) 64-bit words
    host = C.addressof(d)
    assert l.cris_boundary_work_bytes(host, 1) == 4 * 8 * 1 * 4
    fill(1, w=65, h=33, out_off=32, mask_off=32)
    assert l.cris_boundary_work_bytes(host, 2) == 4 * 8 * 2 * 66
    assert l.cris_boundary_work_bytes(host, 0) == 0 and l.cris_boundary_work_bytes(None, 2) == 0 and l.cris_boundary_work_bytes(host, -3) == 0
    need, big = l.cris_boundary_work_bytes(host, 2), 32 + 68 * 33
    rejected(biou, b"work buffer is too small", n=2, pred_bytes=big, gt_bytes=big, work_bytes=need - 1)
    rejected(erode, b"work buffer is too small", n=2, mask_bytes=big, out_bytes=big, work_bytes=need // 2 - 1)
    radii[1] = 0                                                            # the second of two entries is looked at only when n says so
    rejected(biou, b"every radius must be >= 1", n=2, pred_bytes=big, gt_bytes=big)
    rejected(erode, b"every radius must be >= 1", n=2, mask_bytes=big, out_bytes=big)
    fill(1, w=0)
    radii[1] = 1
    rejected(erode, b"bad output size", n=2)


def test_evaluator_and_ops_check_their_arguments_before_any_device_work():
    import torch
    from types import SimpleNamespace as NS
    from cris.pytorch_amd import evalpost, evaluate
    ev = evaluate.Evaluator.__new__(evaluate.Evaluator)
    ev.pipe = _NoDevice("val")
    for call in (ev.validate, ev.inference):
        for bad in ("x", 0.02, False, evalpost.Boundary):
            with pytest.raises(ValueError, match="boundary must be None, True"):
                call([{}], boundary=bad)
    with pytest.raises(ValueError, match="mode 'test'"):                    # a good spec: the next check is the pipeline's mode
        ev.inference([{}], boundary=True)
    st = NS(out_bytes=64, n=1)
    with pytest.raises(RuntimeError, match="GPU only"):
        evalpost.erode_batch(torch.zeros(64, dtype=torch.uint8), st, [1])
    with pytest.raises(RuntimeError, match="GPU only"):
        evalpost.boundary_iou_batch(torch.zeros(64, dtype=torch.uint8), st, torch.zeros(64, dtype=torch.uint8), [1], None, 0)
