"""Cases and oracles for the mask decoders (csrc/decode.hip behind evalpost.decode_masks_batch, csrc/decode_core.h): numpy only.
The oracle of every case is rle.decode / polygon.decode - the definitions - computed once.  The shapes are the smallest at which
the kernels can take another path: pitch padding of 0 .. 3 bytes, one word of the bit plane and the first bit of the next, more
counts than one chunk of the scan, masks of more dwords than one block."""
import functools

import numpy as np

import rle_cases as RC
from cris.pytorch_amd import polygon, rle

EPSILONS = (0.25, 1.0, 4.0)


def _ellipse_with_hole(h=97, w=131):
    yy, xx = np.mgrid[0:h, 0:w]
    m = ((xx - 64) / 50.0) ** 2 + ((yy - 47) / 35.0) ** 2 < 1.0
    m &= ~((xx - 70) ** 2 + (yy - 45) ** 2 < 13 ** 2)
    return m.astype(np.uint8) * 255


@functools.lru_cache(maxsize=None)
def masks():
    """[(name, uint8 mask)]: every mask of rle_cases.cases(), then the sizes this decoder adds"""
    rng = np.random.default_rng(11)
    rand = lambda h, w, p: (rng.random((h, w)) < p).astype(np.uint8) * 255                       # noqa: E731
    out = list(RC.cases())
    out += [("1x1 empty", np.zeros((1, 1), np.uint8)), ("1x1 full", np.full((1, 1), 255, np.uint8)),
            ("1x130", rand(1, 130, 0.5)), ("130x1", rand(130, 1, 0.5)), ("7x5", rand(7, 5, 0.5)),
            ("33x64", rand(33, 64, 0.4)), ("33x65", rand(33, 65, 0.4)), ("45x67", rand(45, 67, 0.3)),
            ("ellipse with a hole 97x131", _ellipse_with_hole())]
    yy, xx = np.mgrid[0:35, 0:66]
    out.append(("checkerboard 35x66", (((yy + xx) & 1) * 255).astype(np.uint8)))                  # h odd, (0, 0) background
    frame = np.zeros((21, 30), np.uint8)
    frame[:, :3] = frame[:, -2:] = frame[:2, :] = frame[-4:, :] = 255                             # touches all four sides: vertices at x = w, y = h
    frame[8:12, 10:20] = 255
    out.append(("touches all four sides", frame))
    return out


def _general(h, w, rings):
    """a dict of general integer rings: the form polygon.simplify returns"""
    rings = [np.asarray(r, np.int32).reshape(-1, 2) for r in rings]
    return {"size": [h, w], "rings": rings, "holes": [polygon.twice_area(r) < 0 for r in rings], "epsilon": 0.25}


@functools.lru_cache(maxsize=None)
def rle_sources():
    """[(name, RLE dict)]: every mask's rle.encode, then counts nobody's encoder writes - runs of length zero in the middle and at the
    end, all background as [h * w], all foreground as [0, h * w], and more counts than one 256-chunk of the scan with zeros among them"""
    out = [("rle " + name, rle.encode(m)) for name, m in masks()]
    out += [("zero runs in the middle", {"size": [5, 4], "counts": [3, 0, 2, 4, 0, 0, 5, 0, 0, 6]}),
            ("zero runs at the end", {"size": [3, 7], "counts": [0, 4, 6, 11, 0, 0]}),
            ("leading zeros", {"size": [4, 4], "counts": [0, 0, 0, 5, 0, 3, 8]}),
            ("[h * w]", {"size": [6, 9], "counts": [54]}), ("[0, h * w]", {"size": [6, 9], "counts": [0, 54]}),
            ("1x1 [0, 1]", {"size": [1, 1], "counts": [0, 1]}), ("1x1 [1]", {"size": [1, 1], "counts": [1]})]
    rng = np.random.default_rng(3)
    c = rng.integers(0, 4, 700)
    c[rng.random(700) < 0.3] = 0
    h = 29
    w = -(-int(c.sum()) // h)
    c[-1] += h * w - int(c.sum())
    out.append(("700 counts with zeros", {"size": [h, w], "counts": c.tolist()}))
    out.append(("str counts", rle.to_json(rle.encode(masks()[-1][1]))))
    return out


@functools.lru_cache(maxsize=None)
def polygon_sources():
    """[(name, polygon dict)]: every mask's polygon.encode and polygon.simplify of it at EPSILONS, then general rings written by hand
    that exercise the floor of the crossing (edges leaning both ways, a sliver one row high and w wide), two identical rings (the
    empty mask), a ring that runs along the frame, and random integer polygons (self-intersecting: even-odd is defined for them)"""
    out = []
    for name, m in masks():
        p = polygon.encode(m)
        out.append(("polygon " + name, p))
        for eps in EPSILONS:
            out.append(("simplified %g %s" % (eps, name), polygon.simplify(p, eps)))
    tri, mirror = [(0, 0), (4, 4), (0, 4)], [(7, 0), (3, 4), (7, 4)]
    out += [("triangle leaning right", _general(6, 7, [tri])), ("triangle leaning left", _general(6, 7, [mirror])),
            ("both triangles", _general(6, 7, [tri, mirror])),
            ("sliver right", _general(5, 7, [[(0, 2), (7, 3), (0, 3)]])), ("sliver left", _general(5, 7, [[(7, 2), (0, 3), (7, 3)]])),
            ("sliver 130 wide", _general(3, 130, [[(0, 1), (130, 2), (0, 2)]])),
            ("steep and shallow", _general(40, 67, [[(1, 0), (66, 7), (60, 40), (33, 3), (2, 39)]])),
            ("two identical rings", _general(9, 9, [[(1, 1), (8, 2), (4, 8)], [(1, 1), (8, 2), (4, 8)]])),
            ("the frame itself", _general(8, 12, [[(0, 0), (12, 0), (12, 8), (0, 8)]])),
            ("diamond with a hole", _general(33, 65, [[(32, 0), (65, 16), (32, 33), (0, 16)], [(32, 8), (16, 16), (32, 25), (48, 16)]]))]
    rng = np.random.default_rng(19)
    for k in range(6):
        h, w = int(rng.integers(2, 70)), int(rng.integers(2, 140))
        rings = []
        for _ in range(int(rng.integers(1, 4))):
            n = int(rng.integers(3, 10))
            while True:
                r = np.stack([rng.integers(0, w + 1, n), rng.integers(0, h + 1, n)], 1)
                if (np.roll(r, -1, axis=0) != r).any(axis=1).all():
                    break
            rings.append(r)
        out.append(("random polygons %d" % k, _general(h, w, rings)))
    return out


@functools.lru_cache(maxsize=None)
def expected_rle():
    return [rle.decode(r) for _, r in rle_sources()]


@functools.lru_cache(maxsize=None)
def expected_polygon():
    return [polygon.decode(p) for _, p in polygon_sources()]


def searchsorted_decode(h, w, counts):
    """the restatement the device uses: pixel i = x * h + y is foreground iff the number of run ends <= i is odd"""
    ends = np.cumsum(np.asarray(counts, np.int64))
    i = np.arange(h * w, dtype=np.int64)
    v = (np.searchsorted(ends, i, side="right") & 1).astype(np.uint8) * 255
    return np.ascontiguousarray(v.reshape(w, h).T)


def _trunc_div(a, b):
    """C++'s integer division: towards zero"""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b > 0) else -q


def scalar_fill(h, w, rings):
    """csrc/decode_core.h's rule, one edge and one row at a time in Python integers: the truncating division of C++ followed by the
    floor correction, toggles XORed into rows of bits, the inclusive prefix parity read out"""
    rows = [0] * h
    for r in rings:
        r = [(int(x), int(y)) for x, y in np.asarray(r).tolist()]
        for (ax, ay), (bx, by) in zip(r, r[1:] + r[:1]):
            if ay == by:
                continue
            if by < ay:
                ax, ay, bx, by = bx, by, ax, ay
            dx, dy = bx - ax, by - ay
            for py in range(max(ay, 0), min(by, h)):
                num = (2 * py + 1 - 2 * ay) * dx
                a, b = dy - num, 2 * dy
                q = _trunc_div(a, b)
                if a % b != 0 and a < 0:                                    # Python's % has the divisor's sign: != 0 iff C++'s is
                    q -= 1
                px = min(max(ax - q, 0), w)
                if px < w:
                    rows[py] ^= 1 << px
    out = np.zeros((h, w), np.uint8)
    for y, bits in enumerate(rows):
        parity = 0
        for x in range(w):
            parity ^= (bits >> x) & 1
            out[y, x] = 255 * parity
    return out


def pitch_of(w):
    return (w + 3) // 4 * 4
