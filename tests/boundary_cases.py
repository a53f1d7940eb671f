"""Cases and an independent oracle for the mask erosion and the Boundary IoU counts (csrc/morph.hip behind evalpost.erode_batch /
boundary_iou_batch).  The oracle is plain numpy over a summed-area table - a pixel survives the erosion by d iff its
(2 d + 1)-square lies inside the image and sums to (2 d + 1)^2 - and shares nothing with the kernels' bit planes.  The cases are the
smallest shapes at which a word-packed, haloed kernel can go wrong: widths around the 64-bit word (with and without pitch padding),
heights around the window, radii around the word.  Every shape is <= 200 x 200."""
import functools
import math

import numpy as np

WIDTHS = (1, 3, 63, 64, 65, 127, 129, 200)      # 65 and 129: pitch != w
RADII = (1, 2, 31, 32, 33, 63, 64, 65)          # around the 64-bit word
# radius(h, w) at the defaults, pinned (75 x 100: 2.5 rounds to even)
PINNED = (((480, 640), 16), ((427, 640), 15), ((75, 100), 2), ((375, 500), 12), ((45, 60), 2), ((15, 20), 1), ((1, 1), 1), ((3000, 4000), 100))


def pitch_of(w):
    return (w + 3) // 4 * 4


def radius(h, w, ratio=0.02, min_radius=1):
    return max(int(round(ratio * math.sqrt(h * h + w * w))), min_radius)


def erode(fg, d):
    """E_d: True where every pixel of [y - d, y + d] x [x - d, x + d] lies inside the image and is foreground (!= 0)"""
    fg = np.asarray(fg) != 0
    h, w = fg.shape
    k = 2 * d + 1
    out = np.zeros((h, w), bool)
    if d < 1:
        raise ValueError("erode: d must be >= 1")
    if k > h or k > w:
        return out
    sat = np.zeros((h + 1, w + 1), np.int64)
    sat[1:, 1:] = fg.astype(np.int64).cumsum(0).cumsum(1)
    win = sat[k:, k:] - sat[:-k, k:] - sat[k:, :-k] + sat[:-k, :-k]          # entry (y, x): the window centred at (y + d, x + d)
    out[d:h - d, d:w - d] = win == k * k
    return out


def boundary(fg, d):
    """B_d = M & ~E_d(M)"""
    fg = np.asarray(fg) != 0
    return fg & ~erode(fg, d)


def counts(pred, gt, d):
    """[|B_d(pred) & B_d(gt)|, |B_d(pred) | B_d(gt)|]"""
    p, g = boundary(pred, d), boundary(gt, d)
    return [int((p & g).sum()), int((p | g).sum())]


def _u8(m):
    return np.asarray(m).astype(np.uint8) * 255


def _holes(h, w):
    """a full mask with single-pixel holes at a corner, on each edge, and at x = 63 and x = 64"""
    m = np.ones((h, w), bool)
    for y, x in ((0, 0), (0, w // 2), (h - 1, w // 3), (h // 2, 0), (h // 3, w - 1), (h // 2, 63), (h // 2 + 9, 64)):
        m[y, x] = False
    return m


RANDOM = (((40, 65), 3, 0.97), ((33, 130), 2, 0.95), ((9, 200), 4, 0.99), ((70, 129), 5, 0.999))     # (shape, d, density)


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, uint8 mask, d)] - one ragged batch"""
    rng = np.random.default_rng(11)
    out = []
    k = 0
    for d in RADII:
        for h in (1, 2 * d, 2 * d + 1, 2 * d + 2):
            for w in (WIDTHS[k % len(WIDTHS)], 199 if WIDTHS[k % len(WIDTHS)] == 200 else 200):      # every width meets every kind of height; the second holds every window
                m = np.ones((h, w), bool)
                for _ in range(2):                                          # nearly full: two holes
                    m[rng.integers(h), rng.integers(w)] = False
                out.append(("d %d  %d x %d" % (d, h, w), _u8(m), d))
            k += 1
    for w in WIDTHS:                                                        # every width at a radius its window fits in (or not: 1, 3)
        out.append(("width %d" % w, _u8(rng.random((7, w)) < 0.98), 2))
    out.append(("window wider than the image", np.full((30, 9), 255, np.uint8), 5))              # 2 d + 1 = 11 > 9: empty
    out.append(("window higher than the image", np.full((8, 90), 255, np.uint8), 4))             # 2 d + 1 = 9 > 8: empty
    out.append(("full", np.full((50, 150), 255, np.uint8), 7))
    out.append(("empty", np.zeros((50, 150), np.uint8), 7))
    out.append(("holes", _u8(_holes(60, 140)), 3))
    out.append(("holes, wide radius", _u8(_holes(150, 200)), 33))
    corner = np.ones((130, 200), bool)
    corner[0, 0] = False
    out.append(("corner hole, radius of one word", _u8(corner), 64))        # the window reaches exactly one whole word to either side
    out.append(("bytes 1 and 128", np.where(rng.random((40, 70)) < 0.98, np.where(rng.random((40, 70)) < 0.5, 1, 128), 0).astype(np.uint8), 2))
    for (h, w), d, p in RANDOM:
        out.append(("random %g  %d x %d" % (p, h, w), _u8(rng.random((h, w)) < p), d))
    return out


ALIAS = "holes"             # the packed batch ends with one more descriptor that names this case's rectangle (same radius)


@functools.lru_cache(maxsize=None)
def expected():
    """per case the eroded mask (bool) from the oracle, computed once"""
    return [erode(m, d) for _, m, d in cases()]


def _disc(h, w, cy, cx, r):
    yy, xx = np.mgrid[0:h, 0:w]
    return (yy - cy) ** 2 + (xx - cx) ** 2 < r * r


@functools.lru_cache(maxsize=None)
def pairs():
    """[(name, pred, gt, d)]: prediction and ground truth of one size whose boundaries partly overlap (or do not exist)"""
    rng = np.random.default_rng(12)
    out = [("shifted discs", _u8(_disc(120, 160, 60, 80, 40)), _u8(_disc(120, 160, 63, 85, 40)), radius(120, 160)),
           ("disc and ragged disc", _u8(_disc(99, 129, 50, 64, 35) | (rng.random((99, 129)) < 0.01)), _u8(_disc(99, 129, 50, 64, 35)), 3),
           ("same mask", _u8(_disc(75, 100, 40, 50, 30)), _u8(_disc(75, 100, 40, 50, 30)), radius(75, 100)),
           ("both empty", np.zeros((20, 65), np.uint8), np.zeros((20, 65), np.uint8), 1),
           ("empty prediction", np.zeros((45, 60), np.uint8), _u8(_disc(45, 60, 20, 30, 15)), radius(45, 60)),
           ("full and nearly full", np.full((131, 200), 255, np.uint8), _u8(_holes(131, 200)), 65),
           ("window does not fit", _u8(rng.random((15, 20)) < 0.7), _u8(rng.random((15, 20)) < 0.7), 9),
           ("one row", _u8(rng.random((1, 129)) < 0.6), _u8(rng.random((1, 129)) < 0.6), 1)]
    for (h, w), d, p in RANDOM:
        out.append(("random %g  %d x %d" % (p, h, w), _u8(rng.random((h, w)) < p), _u8(rng.random((h, w)) < p), d))
    return out


PAIR_ALIAS = "shifted discs"


@functools.lru_cache(maxsize=None)
def expected_counts():
    return [counts(p, g, d) for _, p, g, d in pairs()]


# what the cases were chosen for, checked once at import
def _check():
    names = [k for k, _, _ in cases()]
    assert len(set(names)) == len(names)
    exp = dict(zip(names, expected()))
    shape = {k: m.shape for k, m, _ in cases()}
    for (h, w), d, p in RANDOM:                                             # neither empty nor full: the erosion has an inside edge
        e = exp["random %g  %d x %d" % (p, h, w)]
        assert 0 < int(e.sum()) < (h - 2 * d) * (w - 2 * d), ((h, w), d, int(e.sum()))
    assert not exp["window wider than the image"].any() and not exp["window higher than the image"].any() and not exp["empty"].any()
    full = np.zeros((50, 150), bool)
    full[7:43, 7:143] = True
    assert np.array_equal(exp["full"], full)                                # the inner rectangle: the boundary is a frame of width d
    assert exp["holes, wide radius"].any() and exp["holes"].any()
    assert int(exp["corner hole, radius of one word"].sum()) == 2 * 72 - 1 and not exp["corner hole, radius of one word"][64, 64]
    for d in RADII:
        wide = [k for k in names if k.startswith("d %d  %d x " % (d, 2 * d)) and shape[k][1] >= 199]
        assert wide and not any(exp[k].any() for k in wide)                 # one row short of the window: empty at every width
    assert {m.shape[1] for _, m, _ in cases()} >= set(WIDTHS)
    assert all(max(m.shape) <= 200 for _, m, _ in cases()) and all(max(p.shape) <= 200 for _, p, _, _ in pairs())
    c = dict(zip((k for k, _, _, _ in pairs()), expected_counts()))
    assert 0 < c["shifted discs"][0] < c["shifted discs"][1] and 0 < c["disc and ragged disc"][0] < c["disc and ragged disc"][1]
    assert c["same mask"][0] == c["same mask"][1] > 0 and c["both empty"] == [0, 0] and c["empty prediction"][0] == 0 < c["empty prediction"][1]


_check()
