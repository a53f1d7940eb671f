"""Host side of mask smoothing (evalpost.Smooth / smooth_spec; csrc/morph.hip cris_morph_masks, csrc/evalpost.hip cris_fill_holes /
cris_fill_holes_work_bytes): the oracle of tests/morph_cases.py against scipy on every case, the kernels' per-word
arithmetic (csrc/morph_core.h) run on the CPU against per-pixel loops, the spec's validation, the ABI pins, the launchers'
rejections through the library, and the entry points' argument checks.  Every comparison is an equality.  No GPU."""
import ctypes as C
import os
import re
import subprocess
from types import SimpleNamespace as NS

import numpy as np
import pytest

import morph_cases as MC
from cris.pytorch_amd.evalpost import Smooth
from test_predict_cpu import _NoDevice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cris_hip.h")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()


def test_oracle_equals_scipy_on_every_case():
    ndimage = pytest.importorskip("scipy.ndimage")
    for (name, m, d), (dil, op, cl) in zip(MC.cases(), MC.expected()):
        fg = m != 0
        sq = np.ones((3, 3), bool)                                         # d iterations of the 3 x 3 square: the (2 d + 1)-square
        assert np.array_equal(dil, ndimage.binary_dilation(fg, structure=sq, iterations=d)), name
        assert np.array_equal(MC.erode(m, d), ndimage.binary_erosion(fg, structure=sq, iterations=d, border_value=0)), name
        assert np.array_equal(MC.erode_clipped(m, d), ndimage.binary_erosion(fg, structure=sq, iterations=d, border_value=1)), name
        assert np.array_equal(op, ndimage.binary_opening(fg, structure=sq, iterations=d)), name
        assert np.array_equal(cl, ndimage.binary_erosion(dil, structure=sq, iterations=d, border_value=1)), name
        assert np.array_equal(dil, ~MC.erode_clipped(~fg, d)), name          # D = not E' not
        assert np.array_equal(MC.opening(op, d), op) and np.array_equal(MC.closing(cl, d), cl), name       # idempotent
    # the deliberate difference from scipy's default closing: an object at the border survives here
    k = [k for k, _, _ in MC.cases()].index("flush top-left")
    m = MC.cases()[k][1] != 0
    assert (m & ~ndimage.binary_closing(m, structure=np.ones((5, 5), bool))).any() and (MC.expected()[k][2] & m).sum() == m.sum() > 0
    # and one case with the full square as the structure, as the definitions state it
    name, m, d = MC.cases()[[k for k, _, _ in MC.cases()].index("blob r 3")]
    full = np.ones((2 * d + 1, 2 * d + 1), bool)
    assert np.array_equal(MC.opening(m, d), ndimage.binary_opening(m != 0, structure=full))
    assert np.array_equal(MC.closing(m, d), ndimage.binary_erosion(ndimage.binary_dilation(m != 0, structure=full), structure=full, border_value=1))
    for (name, m, c, a), (filled, nf, npix, holes) in zip(MC.hole_cases(), MC.expected_holes()):
        lab, n = ndimage.label(m == 0, structure=np.ones((3, 3), int) if c == 8 else None)
        want, cnt = m != 0, [0, 0, 0]
        for i in range(1, n + 1):
            comp = lab == i
            if comp[0].any() or comp[-1].any() or comp[:, 0].any() or comp[:, -1].any():
                continue
            cnt[2] += 1
            if a is None or comp.sum() <= a:
                want = want | comp
                cnt[0] += 1
                cnt[1] += int(comp.sum())
        assert np.array_equal(filled, want) and [nf, npix, holes] == cnt, name
        if c == 4 and a is None:
            assert np.array_equal(filled, ndimage.binary_fill_holes(m != 0)), name


def test_word_arithmetic_of_dilation_and_clipped_erosion_equals_per_pixel_loops(tmp_path):
    """csrc/morph_core.h - the header the HIP kernels include - compiled by g++ into tests/morph_ops_probe.cpp with the address and
    undefined-behaviour sanitizers and run as a child process: the row and column passes of D and E' against per-pixel loops at the
    widths and radii of the cases; an index outside a plane, or a bit at x >= w in a row word, ends the run"""
    exe = str(tmp_path / "morph_ops_probe")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "morph_ops_probe.cpp")])
    r = subprocess.run([exe, "250"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode()
    assert r.returncode == 0 and out.startswith("ok "), out[-2000:]
    assert int(out.split()[1]) > 5_000_000                                  # bits compared


def test_the_spec():
    from cris.pytorch_amd import evalpost
    s = Smooth()
    assert (s.open, s.close, s.fill_holes, s.max_hole_area, s.hole_connectivity) == (0, 0, False, None, 4) and s.is_noop and s.ops == ()
    assert not Smooth(open=1).is_noop and not Smooth(close=1).is_noop and not Smooth(fill_holes=True).is_noop
    assert Smooth(hole_connectivity=8).is_noop
    assert Smooth(open=2, close=3).ops == (("erode", 2), ("dilate", 2), ("dilate", 3), ("erode_clipped", 3))      # open, then close
    assert Smooth(close=1).ops == (("dilate", 1), ("erode_clipped", 1)) and Smooth(fill_holes=True).ops == ()
    assert Smooth(1, 2, True, 9, 8) == Smooth(open=1, close=2, fill_holes=True, max_hole_area=9, hole_connectivity=8)
    assert hash(Smooth(1, 2)) == hash(Smooth(np.int64(1), 2)) and Smooth(1) != Smooth(0, 1) and Smooth(1) != (1, 0, False, None, 4)
    assert len({Smooth(1), Smooth(1, 0), Smooth(1, fill_holes=True)}) == 2
    assert repr(Smooth(1, 2, True, 30, 8)) == "Smooth(open=1, close=2, fill_holes=True, max_hole_area=30, hole_connectivity=8)"
    assert eval(repr(Smooth(3, fill_holes=True)), {"Smooth": Smooth}) == Smooth(3, fill_holes=True)
    with pytest.raises(AttributeError, match="immutable"):
        s.open = 2
    for bad in (-1, 1.0, "1", None, True, 65536):
        with pytest.raises(ValueError, match="open"):
            Smooth(open=bad)
        with pytest.raises(ValueError, match="close"):
            Smooth(close=bad)
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="fill_holes"):
            Smooth(fill_holes=bad)
    for bad in (0, -3, 2.5, "9", True):
        with pytest.raises(ValueError, match="max_hole_area"):
            Smooth(fill_holes=True, max_hole_area=bad)
    with pytest.raises(ValueError, match="needs fill_holes"):
        Smooth(open=1, max_hole_area=5)
    for bad in (6, "4", None, True):
        with pytest.raises(ValueError, match="hole_connectivity"):
            Smooth(hole_connectivity=bad)
    assert evalpost.smooth_spec(None, "x") is None and evalpost.smooth_spec(Smooth(), "x") is None          # a spec that does nothing is no spec
    assert evalpost.smooth_spec(Smooth(close=2), "x") == Smooth(close=2)
    for bad in (True, 1, "open", Smooth, (1, 1), dict(open=1)):
        with pytest.raises(ValueError, match="here: smooth must be None or an evalpost.Smooth"):
            evalpost.smooth_spec(bad, "here: smooth")
    assert evalpost.MORPH_OPS == {"erode": 0, "dilate": 1, "erode_clipped": 2} and evalpost.MORPH_MAX_OPS == 8
    assert evalpost.FILL_FIELDS == ("holes_filled", "pixels_filled", "holes", "error")
    codes, radii = evalpost._morph_ops("f", [("dilate", 2), ("erode", [1, 2, 3])], 3)
    assert codes.tolist() == [1, 0] and radii.tolist() == [[2, 2, 2], [1, 2, 3]] and radii.dtype == np.int32 == codes.dtype


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
    for name, nargs, res in (("cris_morph_masks", 14, C.c_int), ("cris_fill_holes_work_bytes", 1, C.c_size_t), ("cris_fill_holes", 14, C.c_int)):
        assert name in hip.EXPORTS and getattr(hip.load(), name) is not None
        got_res, args = hip._SIGS[name]
        assert got_res is res and protos[name][0] == ("size_t" if res is C.c_size_t else "int")
        assert len(args) == nargs and args == [ctype_of(x) for x in protos[name][1]], name
    assert hip.ABI_VERSION == 8 == hip.load().cris_abi_version() == int(re.search(r"#define CRIS_ABI_VERSION (\d+)", src).group(1))
    comment = src[src.index("/* CRIS_ABI_VERSION moves"):src.index("#define CRIS_ABI_VERSION")]
    assert comment.index("cris_boundary_iou_batch") < comment.index("cris_morph_masks") < comment.index("cris_fill_holes")
    assert "cris_fill_holes_work_bytes" in comment
    for name, value in (("CRIS_MORPH_ERODE", 0), ("CRIS_MORPH_DILATE", 1), ("CRIS_MORPH_ERODE_CLIPPED", 2), ("CRIS_MORPH_MAX_OPS", 8)):
        assert re.search(r"#define %s %d\b" % (name, value), src), name
    assert hip.load().cris_sizeof(b"cris_eval_desc") == 88
    assert hip.load().cris_fill_holes_work_bytes(10) == 40 and hip.load().cris_fill_holes_work_bytes(13) == 56


def test_launchers_reject_bad_arguments_on_the_host(built):
    """both launchers check their operands, every operation, every radius and every descriptor before any launch"""
    from cris.pytorch_amd import hip
    l = hip.load()
    d = (hip.EvalDesc * 2)()
    ops = (C.c_int * 8)(1, 2, 0, 1, 1, 1, 1, 1)
    radii = (C.c_int * 16)(*([1] * 16))
    mat = (C.c_double * 6)(1, 0, 0, 0, 1, 0)

    def fill(i=0, w=5, h=4, pitch=None, out_off=0, mask_off=0, row=0):
        assert l.cris_eval_desc_fill(C.addressof(d[i]), mat, w, h, 0, mask_off, (w + 3) // 4 * 4 if pitch is None else pitch, out_off, row) == 0

    def morph(masks=0x1000, mask_bytes=64, host=None, dev=0x2000, n=1, oh=None, n_ops=2, rh=None, rd=0x3000, work=0x5000, work_bytes=1 << 12,
              out=0x6000, out_bytes=64):
        host = C.addressof(d) if host is None else host
        oh = C.addressof(ops) if oh is None else oh
        rh = C.addressof(radii) if rh is None else rh
        return l.cris_morph_masks(masks, mask_bytes, host or None, dev, n, oh or None, n_ops, rh or None, rd, work, work_bytes, out, out_bytes, None)

    def holes(masks=0x1000, mask_bytes=64, host=None, dev=0x2000, n=1, conn=4, max_area=-1, labels=0x4000, label_words=64, work=0x5000,
              work_bytes=1 << 12, info=0x8000, rows=4):
        host = C.addressof(d) if host is None else host
        return l.cris_fill_holes(masks, mask_bytes, host or None, dev, n, conn, max_area, labels, label_words, work, work_bytes, info, rows, None)

    def rejected(fn, msg, **kw):
        assert fn(**kw) != 0, (msg, kw)
        err = l.cris_last_error()
        assert (b"cris_morph_masks" if fn is morph else b"cris_fill_holes") in err and msg in err, (kw, err)

    fill()
    for k in ("masks", "dev", "rd", "work", "out"):
        rejected(morph, b"null operand", **{k: None})
    for k in ("host", "oh", "rh"):
        rejected(morph, b"null operand", **{k: 0})
    for k in ("masks", "dev", "labels", "work", "info"):
        rejected(holes, b"null operand", **{k: None})
    rejected(holes, b"null operand", host=0)
    for fn in (morph, holes):
        for n in (0, -1, 65536):
            rejected(fn, b"n must be in 1 .. 65535", n=n)
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
    for n_ops in (0, -1, 9):
        rejected(morph, b"n_ops must be in 1 .. 8", n_ops=n_ops)
    for bad in (3, -1):
        ops[1] = bad
        rejected(morph, b"every operation must be 0")
        ops[1] = 2
    ops[7] = 5                                                              # the last of eight
    rejected(morph, b"every operation must be 0", n_ops=8)
    ops[7] = 1
    for bad in (0, -3, 65536, 1 << 30):
        radii[1] = bad                                                      # the radius of the second operation
        rejected(morph, b"every radius must be in 1 .. 65535")
        radii[1] = 1
    rejected(morph, b"aligned", work=0x5004)
    rejected(morph, b"aligned", rd=0x3002)
    rejected(morph, b"output outside the buffer", out_bytes=31)             # inside the source, outside `out`
    fill(out_off=64)
    rejected(morph, b"output outside the buffer", mask_bytes=95, out_bytes=96)
    fill()
    # the work buffer: two planes of n slots of the batch's largest h * ceil(w / 64) 64-bit words, half of the boundary's four
    fill(1, w=65, h=33, out_off=32)
    need, big = l.cris_boundary_work_bytes(C.addressof(d), 2) // 2, 32 + 68 * 33
    assert need == 2 * 8 * 2 * 66
    rejected(morph, b"work buffer is too small", n=2, mask_bytes=big, out_bytes=big, work_bytes=need - 1)
    radii[3] = 0                                                            # operation 1, descriptor 1: read only when n says so
    rejected(morph, b"every radius must be in 1 .. 65535", n=2, mask_bytes=big, out_bytes=big)
    radii[3] = 1
    # hole filling
    rejected(holes, b"connectivity must be 4 or 8", conn=6)
    rejected(holes, b"max_area must be >= 0", max_area=-2)
    rejected(holes, b"bad sizes", rows=0)
    rejected(holes, b"aligned", masks=0x1002)
    rejected(holes, b"aligned", labels=0x4004)
    rejected(holes, b"aligned", work=0x5008)
    rejected(holes, b"aligned", info=0x8004)
    rejected(holes, b"label buffer must hold one word per mask byte", label_words=63)
    rejected(holes, b"work buffer is too small", work_bytes=255)
    for row in (4, -1):
        fill(row=row)
        rejected(holes, b"row out of range")
    fill(out_off=2)
    rejected(holes, b"output outside the buffer", mask_bytes=128, label_words=128)      # out_off must be 4-byte aligned for the labeller
    fill()


def test_entry_points_reject_a_bad_smooth_before_any_device_work():
    import torch
    from cris.pytorch_amd import evalpost, evaluate, predict
    for bad in ("open", 2, dict(open=1), Smooth):
        with pytest.raises(ValueError, match="Predictor: smooth"):
            predict.Predictor(NS(), _NoDevice(), smooth=bad)
    p = predict.Predictor(NS(), _NoDevice(), thr=0.35, smooth=Smooth())
    assert p.smooth is None and p.smooth_info is None                       # a no-op spec is no spec
    p = predict.Predictor(NS(), _NoDevice(), thr=0.35, smooth=Smooth(close=2))
    assert p.smooth == Smooth(close=2) and p.components is None
    jpg = b"\xff\xd8\xff\xe0fake"
    for bad in ("open", "Default", 4, (1, 2), Smooth):
        with pytest.raises(ValueError, match="predict: smooth"):
            p.predict([jpg], ["a"], smooth=bad)
    with pytest.raises(ValueError, match="no images"):                      # the other checks still come before the device
        p.predict([], [], smooth=Smooth(open=1, fill_holes=True))
    assert p._ring is None and p._cc_masks is None and p._cc_labels is None and p._cc_work is None and p._sm_work is None
    assert predict._check_smooth("default", p.smooth) is p.smooth and predict._check_smooth(None, p.smooth) is None
    assert predict._check_smooth(Smooth(hole_connectivity=8), p.smooth) is None
    ev = evaluate.Evaluator.__new__(evaluate.Evaluator)
    ev.pipe = _NoDevice("val")
    for call in (ev.validate, ev.inference):
        for bad in ("close", 1, True, Smooth):
            with pytest.raises(ValueError, match="smooth must be None or an evalpost.Smooth"):
                call([{}], smooth=bad)
    with pytest.raises(ValueError, match="mode 'test'"):                    # a good spec: the next check is the pipeline's mode
        ev.inference([{}], smooth=Smooth(close=1))
    for flags in (["--open", "-1"], ["--close", "x"], ["--max-hole-area", "5"], ["--fill-holes", "--max-hole-area", "0"]):
        with pytest.raises(SystemExit):
            predict.main(["--image", "x.jpg", "--expr", "a", "--out-prefix", "p"] + flags)
    st = NS(out_bytes=64, n=1)
    cpu = torch.zeros(64, dtype=torch.uint8)
    for fn, args in ((evalpost.morph_batch, (cpu, st, [("dilate", 1)])), (evalpost.dilate_batch, (cpu, st, 1)), (evalpost.open_batch, (cpu, st, 1)),
                     (evalpost.close_batch, (cpu, st, 1)), (evalpost.fill_holes_batch, (cpu, st, None, 0))):
        with pytest.raises(RuntimeError, match="GPU only"):
            fn(*args)
    with pytest.raises(ValueError, match="spec must be"):
        evalpost.smooth_batch(cpu, st, None, None, 0)
