"""Host side of prediction on unlabeled images (cris/pytorch_amd/predict.py, evalpost.EvalStaging.pack_sizes,
csrc/evalpost.hip cris_predict_masks_batch): the batch plan, the argument checks that run before a device is touched, the
launcher's rejections through the library, and the ABI bookkeeping of the new symbol.  No GPU."""
import ctypes as C
import os
import re
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cris_hip.h")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()


def _inv(i):
    return np.array([[1.2 + 0.1 * i, 0.0, -3.5], [0.0, 1.2 + 0.1 * i, 2.25 - i]], np.float64)


def test_plan_predict_mapping_and_padding():
    from cris.pytorch_amd import predict
    invs = [_inv(i) for i in range(3)]
    plans = predict.plan_predict([1, 3, 2], images_per_batch=2, inverses=invs)
    assert len(plans) == 2
    a, b = plans
    # batch 0: images 0, 1 with 1 + 3 expressions, padded to 8 by repeating the last expression's image
    assert (a.lo, a.n, a.image_index) == (0, 2, [0, 1])
    assert a.index == [0, 1, 1, 1, 1, 1, 1, 1] and len(a.descs) == 4               # padding entries get no descriptor
    assert [(i, k, row) for _, i, k, row in a.descs] == [(0, 0, 0), (1, 1, 1), (1, 2, 2), (1, 3, 3)]
    assert a.descs[0][0] is invs[0] and all(d[0] is invs[1] for d in a.descs[1:])
    # batch 1: ONE image (the last batch is short: its image is repeated), 2 expressions -> 8
    assert (b.lo, b.n, b.image_index) == (2, 1, [0, 0])
    assert b.index == [0] * 8 and len(b.descs) == 2
    assert [(i, k, row) for _, i, k, row in b.descs] == [(0, 0, 4), (0, 1, 5)] and all(d[0] is invs[2] for d in b.descs)
    assert [d[3] for p in plans for d in p.descs] == [0, 1, 2, 3, 4, 5]             # rows of the whole call, in order
    # expression count already a multiple of 8: nothing is added; without inverses the slot stays None
    (p,) = predict.plan_predict([3, 5], images_per_batch=8)
    assert p.index == [0] * 3 + [1] * 5 and len(p.descs) == 8 and p.image_index == [0, 1] + [1] * 6
    assert all(d[0] is None for d in p.descs)
    (p,) = predict.plan_predict([2], images_per_batch=1, multiple=3)
    assert p.index == [0, 0, 0] and p.image_index == [0]
    for bad in ([], [1, 0], [2, -1]):
        with pytest.raises(ValueError):
            predict.plan_predict(bad)
    with pytest.raises(ValueError):
        predict.plan_predict([1, 2], inverses=invs)
    with pytest.raises(ValueError):
        predict.plan_predict([1], images_per_batch=0)


class _NoDevice:
    """a pipeline any use of which (beyond mode / device) is an error: the argument checks must come first"""

    def __init__(self, mode="test"):
        self.mode, self.device = mode, torch.device("cpu")

    def __getattr__(self, name):
        raise AssertionError("touched %s before the arguments were checked" % name)


def test_predictor_argument_errors_before_any_device_work():
    from cris.pytorch_amd import predict
    model = NS()
    for mode in ("val", "train"):
        with pytest.raises(ValueError, match="mode 'test'"):
            predict.Predictor(model, _NoDevice(mode))
    for thr in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="thr"):
            predict.Predictor(model, _NoDevice(), thr=thr)
    p = predict.Predictor(model, _NoDevice(), thr=0.35)          # (NS(): not even callable)
    jpg, arr = b"\xff\xd8\xff\xe0fake", np.zeros((4, 5, 3), np.uint8)
    cases = [
        (([jpg, jpg], ["a"]), {}, "2 images but 1 expression"),
        (([], []), {}, "no images"),
        (([jpg], [""]), {}, "non-empty"),
        (([jpg], [[]]), {}, "non-empty"),
        (([jpg], [["a", "  "]]), {}, "non-empty"),
        (([jpg], [["a", 3]]), {}, "non-empty"),
        (([jpg], [None]), {}, "non-empty"),
        (([jpg], ["a"]), dict(masks="cpu"), "masks must be"),
        (([jpg], ["a"]), dict(masks="Host"), "masks must be"),
        (([jpg], ["a"]), dict(images_per_batch=0), "images_per_batch"),
        (([jpg, arr], ["a", "b"]), {}, "one kind per call"),
        (([arr.astype(np.float32)], ["a"]), {}, "uint8 RGB"),
        (([arr[:, :, 0]], ["a"]), {}, "uint8 RGB"),
        (([torch.zeros(4, 5, 4, dtype=torch.uint8)], ["a"]), {}, "uint8 RGB"),
        ((["file.jpg"], ["a"]), {}, "uint8 RGB"),
    ]
    for args, kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            p.predict(*args, **kw)
    assert p._ring is None                                                          # nothing was allocated
    # the accepted forms pass the checks (and only then reach the pipeline)
    for images, exprs in (([jpg], ["a"]), ([arr], [["a", "b"]]), ([torch.zeros(4, 5, 3, dtype=torch.uint8)], [("a",)])):
        kind, _, e = predict._check_inputs(images, exprs, 8, None)
        assert kind == ("bytes" if images[0] is jpg else "array") and all(isinstance(x, list) for x in e)


def test_module_predictor_is_eval_only():
    from cris.pytorch_amd.model import build_segmenter
    from test_module_surface import TINY
    model, _ = build_segmenter(NS(**TINY))
    model.train()
    with pytest.raises(RuntimeError, match="eval"):
        model.predictor(_NoDevice())
    model.eval()
    from cris.pytorch_amd import predict
    pr = model.predictor(_NoDevice(), thr=0.5)
    assert isinstance(pr, predict.Predictor) and pr.thr == 0.5 and pr._segment is not None
    with pytest.raises(ValueError, match="mode 'test'"):
        model.predictor(_NoDevice("val"))


def test_pack_sizes_fills_descriptors_without_masks(built):
    from cris.pytorch_amd import evalpost, predict
    from oracle import eval_post as EP
    shapes = [(33, 25), (5, 3), (1, 1)]
    invs = [_inv(i) for i in range(3)]
    (plan,) = predict.plan_predict([2, 1, 3], images_per_batch=4, inverses=invs)
    st = evalpost.EvalStaging(None, max_descs=2, mask_bytes=16)                     # too small on purpose: pack_sizes grows it
    st.pack_sizes(shapes, plan.descs)
    assert st.n == 6 and st.max_descs >= 6 and st.mask_bytes == 0
    want_off = 0
    for k, (inv, i, mp, row) in enumerate(plan.descs):
        d, (h, w) = st.descs[k], shapes[i]
        assert (d.w_out, d.h_out, d.map, d.row, d.mask_off) == (w, h, k, k, 0)
        assert d.pitch == (w + 3) // 4 * 4 and d.out_off == want_off and d.out_off % 16 == 0
        assert np.array_equal(np.array(d.m[:]).reshape(2, 3), EP.invert_affine(inv))
        want_off += (d.pitch * h + 15) // 16 * 16
    assert st.out_bytes == want_off
    # the same sizes through pack() (with masks) give the same pitches, output offsets and out_bytes
    masks = [np.zeros(s, np.uint8) for s in shapes]
    ref = evalpost.EvalStaging(None).pack(masks, plan.descs)
    assert ref.out_bytes == st.out_bytes
    assert [(ref.descs[k].pitch, ref.descs[k].out_off) for k in range(6)] == [(st.descs[k].pitch, st.descs[k].out_off) for k in range(6)]


def test_new_predict_stats_rows():
    from cris.pytorch_amd import evalpost
    t = evalpost.new_predict_stats(3, "cpu")
    assert t.dtype == torch.int64 and t.shape == (3, 6) and t.is_contiguous()
    assert t.tolist() == [[0, 0, 2 ** 31 - 1, 2 ** 31 - 1, 0, 0]] * 3
    assert evalpost.PREDICT_FIELDS == ("area", "score_q16", "x_min", "y_min", "x_end", "y_end")
    with pytest.raises(ValueError):
        evalpost.new_predict_stats(0, "cpu")


def test_launcher_rejects_bad_arguments_on_the_host(built):
    """cris_predict_masks_batch checks its operands and every descriptor before it touches the device"""
    from cris.pytorch_amd import hip
    l = hip.load()
    d = (hip.EvalDesc * 1)()
    mat = (C.c_double * 6)(1, 0, 0, 0, 1, 0)

    def fill(w=5, h=4, map=0, pitch=None, out_off=0, row=0):
        assert l.cris_eval_desc_fill(C.addressof(d), mat, w, h, map, 0, (w + 3) // 4 * 4 if pitch is None else pitch, out_off, row) == 0

    def launch(probs=0x1000, host=None, dev=0x2000, n=1, thr=0.35, stats=0x4000, rows=4, out=None, out_bytes=0, border=0.0):
        host = C.addressof(d) if host is None else host
        return l.cris_predict_masks_batch(probs, 2, 8, 8, host or None, dev, n, thr, border, stats, rows, out, out_bytes, None)

    def rejected(msg, **kw):
        assert launch(**kw) != 0
        err = l.cris_last_error()
        assert b"cris_predict_masks_batch" in err and msg in err, (kw, err)

    fill(row=4)
    rejected(b"row out of range")
    fill(row=-1)
    rejected(b"row out of range")
    fill(map=2)
    rejected(b"map out of range")
    fill(map=-1)
    rejected(b"map out of range")
    for pitch in (6, 4, 7):                                                         # not a multiple of 4; below w_out; both
        fill(pitch=pitch)
        rejected(b"pitch must be a multiple of 4")
    fill(w=0)
    rejected(b"bad output size")
    fill(w=46341, h=46341)                                                          # w_out * h_out >= 2^31
    rejected(b"bad output size")
    fill(out_off=64)                                                                # 8 x 4 bytes at 64 need 96
    rejected(b"output outside the buffer", out=0x5000, out_bytes=95)
    fill(out_off=2)
    rejected(b"output outside the buffer", out=0x5000, out_bytes=1 << 20)           # misaligned
    fill(out_off=-16)
    rejected(b"output outside the buffer", out=0x5000, out_bytes=1 << 20)
    fill()
    for thr in (-0.35, float("nan"), float("inf"), -0.0 - 1e-30):
        rejected(b"thr must be finite and >= 0", thr=thr)
    rejected(b"border must be finite", border=float("nan"))
    rejected(b"null operand", probs=None)
    rejected(b"null operand", host=0)
    rejected(b"null operand", dev=None)
    rejected(b"null operand", stats=None)
    for n in (0, -1, 65536):
        rejected(b"n must be in 1 .. 65535", n=n)
    rejected(b"bad sizes", rows=0)
    rejected(b"aligned", stats=0x4004)
    rejected(b"aligned", out=0x5002, out_bytes=1 << 20)


def test_symbol_is_declared_bound_and_named_at_abi_8(built):
    from cris.pytorch_amd import hip
    src = open(HEADER).read()
    assert re.search(r"\bint cris_predict_masks_batch\s*\(", src)
    assert "cris_predict_masks_batch" in hip.EXPORTS and hip.load().cris_predict_masks_batch is not None
    res, args = hip._SIGS["cris_predict_masks_batch"]
    assert res is C.c_int and len(args) == 14
    assert hip.ABI_VERSION == 8 == hip.load().cris_abi_version() == int(re.search(r"#define CRIS_ABI_VERSION (\d+)", src).group(1))
    comment = src[src.index("/* CRIS_ABI_VERSION moves"):src.index("#define CRIS_ABI_VERSION")]
    assert "cris_predict_masks_batch" in comment
    assert comment.index("cris_preprocess_batch_aug") < comment.index("cris_predict_masks_batch")     # appended after the last addition
    assert len(re.findall(r"typedef struct \{[^{}]*\} cris_eval_desc;", src)) == 1                   # reused, no new struct
    assert hip.load().cris_sizeof(b"cris_eval_desc") == C.sizeof(hip.EvalDesc) == 88
