"""Training-time augmentation of the GPU input pipeline, host side (no GPU): the `Augment` spec, the map from uniforms to
per-sample parameters, the matrix, the left / right swap of a mirrored sentence, the host-side argument checks of the two new
launchers and the numpy restatement of the colour arithmetic at its identity."""
import ctypes as C
import math

import numpy as np
import pytest

import augment_cases as ac
from cris.pytorch_amd import hip, inputpipe, records
from cris.pytorch_amd.inputpipe import Augment, AugmentParams, augment_matrix, augment_params
from oracle import input_pipe as ip


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return hip.load()


# ---- Augment ---------------------------------------------------------------------------------------------------------------

def test_defaults_are_the_identity_and_normalise_to_none():
    assert Augment() == Augment(scale=(1.0, 1.0), translate=0.0, rotate=0.0, hflip=0.0, brightness=0.0, contrast=0.0, saturation=0.0)
    assert Augment.normalized(None) is None and Augment.normalized(Augment()) is None
    assert Augment.normalized(Augment(scale=(1, 1))) is None                       # ints are accepted and compare equal
    a = Augment(scale=(0.8, 1.25), translate=0.1, rotate=10.0, brightness=0.2, contrast=0.2, saturation=0.2)
    assert Augment.normalized(a) is a
    with pytest.raises(ValueError):
        Augment.normalized({"rotate": 3})
    with pytest.raises(Exception):
        a.rotate = 5.0                                                              # frozen


@pytest.mark.parametrize("field,value", [
    ("scale", (0.0, 1.0)), ("scale", (-1.0, 1.0)), ("scale", (1.2, 1.1)), ("scale", (1.0, math.inf)), ("scale", (math.nan, 1.0)),
    ("scale", 1.0), ("scale", (1.0, 1.0, 1.0)),
    ("translate", -0.1), ("translate", 1.0), ("translate", math.nan),
    ("rotate", -1.0), ("rotate", 180.5), ("rotate", math.inf),
    ("hflip", -0.01), ("hflip", 1.01), ("hflip", math.nan),
    ("brightness", -0.1), ("brightness", 1.1), ("brightness", math.inf),
    ("contrast", -0.1), ("contrast", 1.1), ("contrast", math.nan),
    ("saturation", -0.1), ("saturation", 1.1), ("saturation", "0.2"), ("saturation", True)])
def test_bad_values_raise_and_name_the_field(field, value):
    with pytest.raises(ValueError, match=r"Augment\.%s\b" % field):
        Augment(**{field: value})


def test_limits_of_the_ranges_are_accepted():
    Augment(scale=(1e-3, 1e-3), translate=0.0, rotate=0.0, hflip=0.0)
    Augment(scale=(0.5, 4.0), translate=0.999, rotate=180.0, hflip=1.0, brightness=1.0, contrast=1.0, saturation=1.0)


# ---- augment_params --------------------------------------------------------------------------------------------------------

def test_one_draw_of_B_by_8_feeds_the_parameters():
    """(that RecordPipeline makes exactly one such draw, before the sentence draws: tests/test_augment_gpu.py)"""
    aug = Augment(scale=(0.8, 1.25), translate=0.1, rotate=10.0, hflip=0.5, brightness=0.2, contrast=0.3, saturation=0.4)
    S_h, S_w = 36, 52
    u = np.random.default_rng(3).random((6, 8))
    ps = augment_params(aug, u, (S_h, S_w))
    assert len(ps) == 6
    for r, p in zip(u, ps):
        assert p.scale == 0.8 + r[0] * (1.25 - 0.8)
        assert p.tx == (2 * r[1] - 1) * 0.1 * S_w and p.ty == (2 * r[2] - 1) * 0.1 * S_h
        assert p.angle == (2 * r[3] - 1) * 10.0
        assert p.flip == bool(r[4] < 0.5)
        for got, ui, knob in ((p.fb, r[5], 0.2), (p.fc, r[6], 0.3), (p.fs, r[7], 0.4)):
            assert isinstance(got, np.float32) and got == np.float32(1 + (2 * ui - 1) * knob)         # float64, rounded once
    with pytest.raises(ValueError):
        augment_params(aug, np.zeros((6, 7)), (S_h, S_w))


def test_a_knob_at_zero_gives_exactly_one():
    aug = Augment(rotate=5.0)                                    # everything else at its default
    for p in augment_params(aug, np.random.default_rng(0).random((64, 8)), (416, 416)):
        assert p.fb == 1.0 and p.fc == 1.0 and p.fs == 1.0 and p.scale == 1.0 and p.tx == 0.0 and p.ty == 0.0 and p.flip is False
    for p in augment_params(Augment(brightness=0.5), np.random.default_rng(1).random((64, 8)), (416, 416)):
        assert p.fc == 1.0 and p.fs == 1.0 and p.angle == 0.0 and not p.geometric


def test_ranges_are_hit_at_the_ends_of_the_unit_interval():
    aug = Augment(scale=(0.5, 2.0), translate=0.25, rotate=30.0, hflip=0.5, brightness=0.2, contrast=0.4, saturation=1.0)
    one = np.nextafter(1.0, 0.0)
    lo, hi = augment_params(aug, np.array([[0.0] * 8, [one] * 8]), (40, 80))
    assert lo.scale == 0.5 and lo.tx == -20.0 and lo.ty == -10.0 and lo.angle == -30.0 and lo.flip is True
    assert (lo.fb, lo.fc, lo.fs) == (np.float32(0.8), np.float32(0.6), np.float32(0.0))
    assert hi.flip is False
    assert math.isclose(hi.scale, 2.0, rel_tol=1e-15) and hi.scale <= 2.0
    assert math.isclose(hi.tx, 20.0, rel_tol=1e-15) and math.isclose(hi.ty, 10.0, rel_tol=1e-15) and math.isclose(hi.angle, 30.0, rel_tol=1e-15)
    assert (hi.fb, hi.fc, hi.fs) == (np.float32(1.2), np.float32(1.4), np.float32(2.0))


# ---- augment_matrix --------------------------------------------------------------------------------------------------------

SHAPES = [((480, 640), (416, 416)), ((37, 50), (36, 52)), ((50, 37), (36, 52)), ((1, 1), (36, 52)), ((333, 500), (416, 416))]


def test_identity_parameters_give_the_letter_box_matrix_exactly():
    for size, inp in SHAPES:
        assert np.array_equal(augment_matrix(size, inp, AugmentParams()), inputpipe.get_transform_mat(size, inp)[0])
        assert np.array_equal(augment_matrix(size, inp, AugmentParams(fb=0.5, fc=1.5, fs=0.0)), ip.get_transform_mat(size, inp)[0])
    assert augment_matrix((480, 640), (416, 416), AugmentParams()).dtype == np.float64


def _apply(M, pts):
    return np.asarray(pts, np.float64) @ M[:, :2].T + M[:, 2]


def test_scale_two_keeps_the_centre_fixed():
    for size, inp in SHAPES:
        L = inputpipe.get_transform_mat(size, inp)[0]
        M = augment_matrix(size, inp, AugmentParams(scale=2.0))
        c = np.array([inp[1] / 2., inp[0] / 2.])
        src_c = np.linalg.solve(L[:, :2], c - L[:, 2])                 # the source point the letter-box puts on the centre
        assert np.allclose(_apply(M, [src_c]), c, atol=1e-9)
        p = src_c + np.array([0.25, -0.5])
        assert np.allclose(_apply(M, [p]) - c, 2.0 * (_apply(L, [p]) - c), atol=1e-9)


def test_flip_mirrors_the_letter_boxed_image():
    for size, inp in SHAPES:
        L = inputpipe.get_transform_mat(size, inp)[0]
        M = augment_matrix(size, inp, AugmentParams(flip=True))
        pts = np.array([[0., 0.], [size[1], 0.], [0.3 * size[1], 0.9 * size[0]]])
        a, b = _apply(L, pts), _apply(M, pts)
        assert np.allclose(b[:, 0], inp[1] - a[:, 0], atol=1e-9) and np.allclose(b[:, 1], a[:, 1], atol=1e-9)


def test_general_case_against_an_independent_composition():
    size, inp = (37, 50), (36, 52)
    p = AugmentParams(scale=0.7, angle=17.0, tx=3.5, ty=-2.25, flip=True)
    M = augment_matrix(size, inp, p)
    L = inputpipe.get_transform_mat(size, inp)[0]
    cx, cy, a = inp[1] / 2., inp[0] / 2., math.radians(17.0)
    for pt in ([0., 0.], [50., 37.], [12.5, 30.25]):
        x, y = _apply(L, [pt])[0]                                       # letter-box
        x, y = x - cx, y - cy                                           # to the centre
        x, y = -0.7 * x, 0.7 * y                                        # mirror + zoom
        x, y = math.cos(a) * x - math.sin(a) * y, math.sin(a) * x + math.cos(a) * y
        want = (x + cx + 3.5, y + cy - 2.25)
        assert np.allclose(_apply(M, [pt])[0], want, atol=1e-9)
    assert abs(np.linalg.det(M[:, :2]) + 0.49 * np.linalg.det(L[:, :2])) < 1e-9       # a mirror: the determinant changes sign


def test_library_inverse_of_augmented_matrices_is_the_oracles(lib):
    """rotated and mirrored matrices go through the same cris_invert_affine / warp as the letter-box: the restated warp
    (oracle.input_pipe.warp_affine_u8) accepts them as it is, and a mirror really reverses the picture"""
    from oracle.eval_post import invert_affine
    for p in (AugmentParams(scale=0.6, angle=17.0), AugmentParams(scale=1.7), AugmentParams(tx=10.4, ty=-7.2), AugmentParams(flip=True),
              AugmentParams(scale=0.7, angle=-163.0, tx=1.0, flip=True)):
        for size in ac.SIZES:
            M = augment_matrix(size, ac.INPUT_SIZE, p)
            m, inv = np.ascontiguousarray(M.reshape(6)), np.zeros(6, np.float64)
            hip.call("cris_invert_affine", m.ctypes.data_as(C.c_void_p), inv.ctypes.data_as(C.c_void_p))
            assert np.array_equal(inv.reshape(2, 3), invert_affine(M))
    img = ac.image(37, 50, 0)
    S_h, S_w = ac.INPUT_SIZE
    a = ip.warp_affine_u8(img, augment_matrix((37, 50), ac.INPUT_SIZE, AugmentParams()), S_w, S_h, ip.INTER_CUBIC, ip.BORDER_RGB)
    b = ip.warp_affine_u8(img, augment_matrix((37, 50), ac.INPUT_SIZE, AugmentParams(flip=True)), S_w, S_h, ip.INTER_CUBIC, ip.BORDER_RGB)
    # x -> S_w - x puts pixel centre x on S_w - x: columns 1 .. S_w-1 reversed, to within the rounding of the 1/32-pixel grid
    d = np.abs(b[:, 1:].astype(int) - a[:, :0:-1].astype(int))
    assert d.mean() < 1.0 and np.percentile(d, 99) <= 8


# ---- swap_left_right -------------------------------------------------------------------------------------------------------

def test_swap_left_right():
    s = records.swap_left_right
    assert s("the left one") == "the right one"
    assert s("Leftmost zebra") == "rightmost zebra"
    assert s("right-hand cup") == "left-hand cup"
    assert s("bright sky") == "bright sky" and s("upright cleft") == "upright cleft"
    assert s("LEFT of the RIGHT one") == "right of the left one"
    for t in ("the left one", "Leftmost zebra", "right-hand cup", "bright sky", "left of the right one"):
        assert s(s(t)) == t.lower()
    assert "spatial" in Augment.__doc__ and "heuristic" in Augment.__doc__


def test_record_pipeline_refuses_augmentation_outside_training():
    aug = Augment(rotate=5.0)
    for mode in ("val", "test"):
        with pytest.raises(ValueError, match="train"):
            records.RecordPipeline(416, 17, "cpu", mode=mode, tokenizer=object(), augment=aug)


# ---- the launchers' host-side checks ---------------------------------------------------------------------------------------

def _descs(addresses, h=4, w=4):
    d = (hip.SampleDesc * len(addresses))()
    for i, a in enumerate(addresses):
        d[i].img, d[i].H, d[i].W = a, h, w
    return d


def test_gray_sum_argument_validation_without_gpu(lib):
    fake, sums = C.c_void_p(0x10000), C.c_void_p(0x20000)              # never dereferenced: every case is refused before the launch
    good = _descs([0x30000, 0x40000])
    for args, word in (((None, fake, 2, sums, None), b"null pointer"), ((good, None, 2, sums, None), b"null pointer"),
                       ((good, fake, 2, None, None), b"null pointer"), ((good, fake, 0, sums, None), b"n must be"),
                       ((good, fake, -3, sums, None), b"n must be"), ((_descs([0x30000, 0x40001]), fake, 2, sums, None), b"4-byte aligned"),
                       ((_descs([0x30002]), fake, 1, sums, None), b"4-byte aligned"), ((_descs([0x30000, 0]), fake, 2, sums, None), b"null image"),
                       ((_descs([0x30000], h=0), fake, 1, sums, None), b"positive"), ((good, fake, 2, C.c_void_p(0x20004), None), b"8-byte aligned")):
        assert lib.cris_gray_sum_batch(*args) != 0
        msg = lib.cris_last_error()
        assert b"cris_gray_sum_batch" in msg and word in msg, msg


def test_preprocess_batch_aug_argument_validation_without_gpu(lib):
    p = [C.c_void_p(0x10000 + 0x1000 * i) for i in range(12)]
    border = (C.c_ubyte * 3)(123, 117, 104)
    norm = (C.c_float * 6)(*ip.MEAN, *ip.STD)

    def args(**kw):
        a = dict(samples=p[0], n=2, S_h=36, S_w=52, lin=p[1], cub=p[2], lut=p[3], lutm=p[4], border=border, factors=p[5], sums=p[6], unit=p[7],
                 norm=norm, img=p[8], mask=p[9], stream=None)
        a.update(kw)
        return list(a.values())

    cases = [(dict(samples=None), b"null pointer"), (dict(factors=None), b"null pointer"), (dict(unit=None), b"null pointer"),
             (dict(norm=None), b"null pointer"), (dict(img=None), b"null pointer"), (dict(border=None), b"null pointer"),
             (dict(n=0), b"n must be"), (dict(n=-1), b"n must be"), (dict(S_h=0), b"output size"),
             (dict(factors=C.c_void_p(0x15002)), b"aligned"), (dict(sums=C.c_void_p(0x16004)), b"aligned"),
             (dict(norm=(C.c_float * 6)(0.5, 0.5, 0.5, 0.25, 0.0, 0.25)), b"std > 0")]
    for kw, word in cases:
        assert lib.cris_preprocess_batch_aug(*args(**kw)) != 0
        msg = lib.cris_last_error()
        assert b"cris_preprocess_batch_aug" in msg and word in msg, (kw, msg)


def test_new_symbols_are_bound_and_the_plain_entry_point_is_what_it_was():
    assert "cris_gray_sum_batch" in hip.EXPORTS and "cris_preprocess_batch_aug" in hip.EXPORTS
    P, I = C.c_void_p, C.c_int
    assert hip._SIGS["cris_preprocess_batch"] == (I, [P, I, I, I, P, P, P, P, P, P, P, P])
    assert hip._SIGS["cris_preprocess_batch_aug"][1][:9] == hip._SIGS["cris_preprocess_batch"][1][:9]


# ---- the numpy restatement of the colour steps -----------------------------------------------------------------------------

def test_colour_reference_with_all_factors_one_is_convert_image():
    for seed, (h, w) in enumerate(ac.SIZES):
        v = ac.image(h, w, 10 + seed)
        for gsum in (0, ac.gray_sum(v), 65280 * h * w):
            assert np.array_equal(ac.colour(v, gsum, h, w, 1, 1, 1), ip.convert_image(v))
    full = np.arange(256, dtype=np.uint8).repeat(3).reshape(16, 16, 3)              # every 8-bit value in every channel
    assert np.array_equal(ac.colour(full, ac.gray_sum(full), 16, 16, 1, 1, 1), ip.convert_image(full))


def test_colour_reference_anchors():
    v = ac.image(37, 50, 0)
    H, W = v.shape[:2]
    gs = ac.gray_sum(v)
    mean, std = ip.MEAN[:, None, None], ip.STD[:, None, None]
    black = ac.colour(v, gs, H, W, 0, 1, 1)                                        # brightness 0: black
    assert np.array_equal(black, np.broadcast_to(((np.float32(0) - mean) / std).astype(np.float32), black.shape))
    flat = ac.colour(v, gs, H, W, 1, 0, 1)                                         # contrast 0: the mean luminance everywhere
    m = np.float32(np.float64(gs) / (65280.0 * H * W))
    assert np.array_equal(flat, np.broadcast_to(((m - mean) / std).astype(np.float32), flat.shape))
    gray = ac.colour(v, gs, H, W, 1, 1, 0) * std + mean                            # saturation 0: three equal channels
    assert np.abs(gray[0] - gray[1]).max() < 1e-6 and np.abs(gray[0] - gray[2]).max() < 1e-6
    assert ac.gray_sum(np.full((512, 512, 3), 255, np.uint8)) == 512 * 512 * 65280 > 2 ** 32
