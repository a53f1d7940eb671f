"""Cases and an independent oracle for the Douglas-Peucker simplifier of traced rings (cris/pytorch_amd/polygon.simplify on the host,
csrc/simplify.hip behind evalpost.polygon_collect(..., simplify=epsilon) on the device; DESIGN.md 9b states the definition).  The
oracle is the plain recursion of that definition - Python ints, one ring and one segment at a time - written apart from the
round-synchronous numpy and HIP code so that they check each other, plus a per-pixel even-odd decode of general polygons in
exact fractions.  The traced rings it starts from are those of the per-crack oracle of polygon_cases.py."""
import functools
from fractions import Fraction

import numpy as np

import polygon_cases as PC

EPSILONS = (0.25, 1, 2, 12, 64)
WAVE_RING, LDS_RING = 256, 4096     # evalpost.POLYGON_SIMPLIFY_WAVE / POLYGON_SIMPLIFY_LDS (csrc/simplify.hip); the CPU test compares them
MAX_SIDE = 32767                    # polygon.MAX_SIMPLIFY_SIDE


def oracle_kept(ring, q):
    """ring: [(x, y), ...] from its raster-first vertex; q = 4 epsilon -> the sorted indices the definition keeps"""
    k = len(ring)
    pts = list(ring) + [ring[0]]                                            # v_k = v_0
    x0, y0 = ring[0]
    a = min(range(k), key=lambda i: (-((ring[i][0] - x0) ** 2 + (ring[i][1] - y0) ** 2), i))
    kept = {0, a}

    def split(i, j):
        if j - i < 2:
            return
        (xi, yi), (xj, yj) = pts[i], pts[j]
        dx, dy = xj - xi, yj - yi
        len2 = dx * dx + dy * dy
        assert len2 > 0
        best = None
        for m in range(i + 1, j):
            c = abs(dx * (pts[m][1] - yi) - dy * (pts[m][0] - xi))
            order = (-c, abs(2 * m - (i + j)), m)                          # greatest c, nearest the middle, smallest m
            if best is None or order < best:
                best = order
        c, m = -best[0], best[2]
        if 16 * c * c > q * q * len2:                                       # strict: on equality the whole interior goes
            kept.add(m)
            split(i, m)
            split(m, j)

    split(0, a)
    split(a, k)
    return sorted(kept)


def oracle_simplify(rings, holes, size, epsilon):
    """the traced rings of one mask ([(x, y)] lists) -> the simplified dict the definition asks for"""
    q = int(4 * epsilon)
    assert q == 4 * epsilon and 1 <= q <= 256
    out = {"size": list(size), "rings": [], "holes": [], "epsilon": q / 4.0}
    for r, hole in zip(rings, holes):
        idx = oracle_kept(r, q)
        if len(idx) >= 3:
            out["rings"].append(np.array([r[i] for i in idx], np.int32).reshape(-1, 2))
            out["holes"].append(bool(hole))
    return out


def oracle_decode_general(rings, h, w):
    """even-odd filling of general polygons sampled at pixel centres, one pixel and one edge at a time in exact fractions: the
    centre (px + 1/2, py + 1/2) is inside iff an odd number of edges crosses its row (half-open in y: y0 <= cy < y1 or the
    reverse) at or left of it, so that a row is filled over [left crossing, right crossing)"""
    out = np.zeros((h, w), np.uint8)
    half = Fraction(1, 2)
    edges = []
    for r in rings:
        pts = [tuple(int(c) for c in v) for v in r]
        edges += [(pts[i], pts[(i + 1) % len(pts)]) for i in range(len(pts))]
    for py in range(h):
        cy = py + half
        crossing = []
        for (xa, ya), (xb, yb) in edges:
            if (ya <= cy) != (yb <= cy):
                crossing.append(xa + (cy - ya) * Fraction(xb - xa, yb - ya))
        for px in range(w):
            if sum(1 for x in crossing if x <= px + half) & 1:
                out[py, px] = 255
    return out


def rectangle():
    """20 wide, 15 high: from the start corner the far corner is the anchor and the two others lie exactly 20 * 15 / 25 = 12 from
    the diagonal - kept at epsilon 11.75, dropped at 12 (the strict test), which leaves 2 vertices: the ring is removed"""
    return np.full((15, 20), 255, np.uint8)


def anchor_tie():
    """a 4 x 4 square without its last pixel: (4, 3) and (3, 4) are both 5 from (0, 0); the smaller index, (4, 3), is the anchor"""
    m = np.full((4, 4), 255, np.uint8)
    m[3, 3] = 0
    return m


def strip(side, tall):
    """one pixel wide, `side` long, foreground but for a gap: rings whose coordinates reach `side`"""
    m = np.full((1, side), 255, np.uint8)
    m[0, 7:9] = 0
    return np.ascontiguousarray(m.T) if tall else m


@functools.lru_cache(maxsize=None)
def extra_cases():
    return [("rectangle 20x15", rectangle()), ("anchor tie", anchor_tie()), ("row of 32767", strip(MAX_SIDE, False)),
            ("column of 32767", strip(MAX_SIDE, True))]


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, uint8 mask)]: polygon_cases.cases() as they are, then the simplifier's own"""
    return list(PC.cases()) + extra_cases()


@functools.lru_cache(maxsize=None)
def traced():
    """per case (rings as [(x, y)] lists, holes) from the per-crack oracle, computed once"""
    out = [PC.expected()[i][0] for i in range(len(PC.cases()))] + [PC.oracle_trace(m)[0] for _, m in extra_cases()]
    return [(rings, [PC.oracle_twice_area(r) < 0 for r in rings]) for rings in out]


def traced_dict(i):
    rings, holes = traced()[i]
    return {"size": list(cases()[i][1].shape), "rings": [np.array(r, np.int32).reshape(-1, 2) for r in rings], "holes": list(holes)}


@functools.lru_cache(maxsize=None)
def expected(epsilon):
    """per case the simplified dict from the oracle, computed once per epsilon"""
    return [oracle_simplify(rings, holes, cases()[i][1].shape, epsilon) for i, (rings, holes) in enumerate(traced())]


def same(p, q):
    return (p["size"] == q["size"] and p["holes"] == q["holes"] and len(p["rings"]) == len(q["rings"]) and p.get("epsilon") == q.get("epsilon")
            and type(p.get("epsilon")) is type(q.get("epsilon"))
            and all(a.dtype == b.dtype == np.int32 and np.array_equal(a, b) for a, b in zip(p["rings"], q["rings"])))
