"""Cases and an independent oracle for mask smoothing (csrc/morph.hip cris_morph_masks and csrc/evalpost.hip cris_fill_holes behind
evalpost.morph_batch / dilate_batch / open_batch / close_batch / fill_holes_batch).  The oracle is plain numpy: a
summed-area table over the mask padded by the radius - zeros for the dilation D and the erosion E, ones for the clipped erosion E' -
and for the holes a flood fill per background component with an area table.  It shares nothing with the kernels' bit planes or
their union-find.  Every shape is <= 200 x 200.

What "neither empty nor full" can ask: open_r is non-empty only when the mask holds a (2 r + 1)-square, and close_r is not full only
when a clipped window of the background stays clear of D_r(M), which reaches r beyond the square: together 4 r + 3 pixels along one
axis.  Within 200 pixels that is r <= 49, so the blob cases (BLOB_RADII), for which all of it is asserted at import, stop at 33; the
grid of every width, height and radius holds such a blob wherever it is satisfiable (`satisfiable`: h >= 2 r + 1 and w >= 4 r + 5,
which leaves room for a speck beside the square) and all of it is asserted there too; the rest of the grid - a height of 1 or 2 r
empties every opening by definition, a narrow width or a radius of 63 .. 65 fills every closing that keeps an opening - is checked
against the definitions instead (open within the mask within close, the window that does not fit)."""
import functools

import numpy as np

WIDTHS = (1, 3, 63, 64, 65, 127, 129, 200)      # 65 and 129: pitch != w
RADII = (1, 2, 31, 32, 33, 63, 64, 65)          # around the 64-bit word
BLOB_RADII = (1, 2, 3, 31, 32, 33)


def pitch_of(w):
    return (w + 3) // 4 * 4


def _window_sum(fg, d, pad):
    """per pixel the sum of the (2 d + 1)-square around it, the image continued by `pad` (0 or 1)"""
    if d < 1:
        raise ValueError("the radius must be >= 1")
    h, w = fg.shape
    p = np.full((h + 2 * d, w + 2 * d), pad, np.int64)
    p[d:d + h, d:d + w] = fg
    sat = np.zeros((h + 2 * d + 1, w + 2 * d + 1), np.int64)
    sat[1:, 1:] = p.cumsum(0).cumsum(1)
    k = 2 * d + 1
    return sat[k:, k:] - sat[:-k, k:] - sat[k:, :-k] + sat[:-k, :-k]


def dilate(m, d):
    """D_d: OR over the square clipped to the image"""
    return _window_sum(np.asarray(m) != 0, d, 0) > 0


def erode(m, d):
    """E_d: the whole square inside the image and foreground (background outside)"""
    return _window_sum(np.asarray(m) != 0, d, 0) == (2 * d + 1) ** 2


def erode_clipped(m, d):
    """E'_d: AND over the square clipped to the image (foreground outside)"""
    return _window_sum(np.asarray(m) != 0, d, 1) == (2 * d + 1) ** 2


def opening(m, d):
    return dilate(erode(m, d), d)


def closing(m, d):
    return erode_clipped(dilate(m, d), d)


OPS = {"erode": erode, "dilate": dilate, "erode_clipped": erode_clipped}


def chain(m, ops):
    """ops: [(name, radius)] applied in order"""
    m = np.asarray(m) != 0
    for name, d in ops:
        m = OPS[name](m, int(d))
    return m


def fill_holes(m, connectivity=4, max_area=None):
    """-> (filled mask, holes filled, pixels filled, holes): flood fill of every background component, an area and a frame flag per
    component; the holes are the components that own no pixel of the outer frame"""
    fg = np.asarray(m) != 0
    h, w = fg.shape
    seen = fg.copy()
    out = fg.copy()
    steps = ((0, 1), (0, -1), (1, 0), (-1, 0)) + (((1, 1), (1, -1), (-1, 1), (-1, -1)) if connectivity == 8 else ())
    table = []                                                              # (area, touches the frame, pixels)
    for y0 in range(h):
        for x0 in range(w):
            if seen[y0, x0]:
                continue
            seen[y0, x0] = True
            stack, pixels, frame = [(y0, x0)], [], False
            while stack:
                y, x = stack.pop()
                pixels.append((y, x))
                frame |= y == 0 or y == h - 1 or x == 0 or x == w - 1
                for dy, dx in steps:
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < h and 0 <= xx < w and not seen[yy, xx]:
                        seen[yy, xx] = True
                        stack.append((yy, xx))
            table.append((len(pixels), frame, pixels))
    holes = filled = npix = 0
    for area, frame, pixels in table:
        if frame:
            continue
        holes += 1
        if max_area is None or area <= max_area:
            filled += 1
            npix += area
            for y, x in pixels:
                out[y, x] = True
    return out, filled, npix, holes


def smooth(m, open=0, close=0, fill=False, max_hole_area=None, hole_connectivity=4):
    """the fixed order of evalpost.Smooth: open, close, fill holes"""
    m = np.asarray(m) != 0
    if open:
        m = opening(m, open)
    if close:
        m = closing(m, close)
    if fill:
        m = fill_holes(m, hole_connectivity, max_hole_area)[0]
    return m


def _u8(m, value=255):
    return np.asarray(m).astype(np.uint8) * np.uint8(value)


def _ragged(h, w, rng):
    """rectangles with specks around them and pin-holes in them"""
    m = np.zeros((h, w), bool)
    for _ in range(3):
        y0, x0 = int(rng.integers(h)), int(rng.integers(w))
        m[y0:y0 + 1 + int(rng.integers(max(h * 2 // 3, 1))), x0:x0 + 1 + int(rng.integers(max(w * 2 // 3, 1)))] = True
    flip = rng.random((h, w)) < 0.02
    return m ^ flip


def satisfiable(h, w, r):
    """an h x w image can hold a mask whose opening and closing by r differ from it and are neither empty nor full (_grid_blob)"""
    return h >= 2 * r + 1 and w >= 4 * r + 5


def _grid_blob(h, w, r):
    """the smallest such mask for a grid shape: a block of all rows and 2 r + 2 columns with its corner pixel missing (the closing
    fills it, a square beside it still fits), a speck one column off the block (the opening removes it), and on the right r + 1
    columns that no dilation reaches (the closing leaves them)"""
    k = 2 * r + 1
    m = np.zeros((h, w), bool)
    m[:, :k + 1] = True
    m[0, 0] = False
    m[h - 1, k + 2] = True
    return m


def _blob(r):
    """one blob that holds the (2 r + 1)-square, a pin-hole in it, a one-pixel bridge out of it to a second, thin blob, a speck beside
    it, and room on the right for a window of the background: open removes bridge, thin blob and speck, close fills the pin-hole"""
    k = 2 * r + 1
    h, w = k + 8, 4 * r + 14
    m = np.zeros((h, w), bool)
    m[2:2 + k + 2, 1:1 + k + 3] = True                                      # rows [2, k + 4), columns [1, k + 4)
    m[3, 2] = False                                                         # the pin-hole: one pixel in from the blob's corner, so that squares beside it still fit
    m[2 + r, k + 4:k + 7] = True                                            # the bridge, one pixel thick
    m[1 + r:4 + r, k + 7:k + 9] = True                                      # the thin blob at its end: 3 x 2
    m[0, k + 6] = True                                                      # the speck
    return m


EDGES = {"top": (slice(0, 3), slice(20, 50)), "bottom": (slice(27, 30), slice(20, 50)), "left": (slice(8, 22), slice(0, 3)),
         "right": (slice(8, 22), slice(64, 67)), "top-left": (slice(0, 3), slice(0, 3)), "top-right": (slice(0, 3), slice(64, 67)),
         "bottom-left": (slice(27, 30), slice(0, 3)), "bottom-right": (slice(27, 30), slice(64, 67))}
EDGE_RADIUS = 2                                                             # 2 r + 1 = 5 > the objects' thickness of 3


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, uint8 mask, r)] - one ragged batch; every case is dilated, opened and closed with its r"""
    rng = np.random.default_rng(21)
    out = []
    k = 0
    for d in RADII:
        for h in (1, 2 * d, 2 * d + 1, 2 * d + 2):
            for w in (WIDTHS[k % len(WIDTHS)], 199 if WIDTHS[k % len(WIDTHS)] == 200 else 200):      # every width meets every kind of height
                out.append(("d %d  %d x %d" % (d, h, w), _u8(_grid_blob(h, w, d) if satisfiable(h, w, d) else _ragged(h, w, rng)), d))
            k += 1
    for w in WIDTHS:
        out.append(("width %d" % w, _u8(_grid_blob(9, w, 2) if satisfiable(9, w, 2) else _ragged(9, w, rng)), 2))
    for r in BLOB_RADII:
        out.append(("blob r %d" % r, _u8(_blob(r)), r))
    for name, (ys, xs) in EDGES.items():
        m = np.zeros((30, 67), bool)
        m[ys, xs] = True
        out.append(("flush " + name, _u8(m), EDGE_RADIUS))
    out.append(("full", np.full((50, 150), 255, np.uint8), 7))
    out.append(("empty", np.zeros((50, 150), np.uint8), 7))
    out.append(("one pixel, set", np.full((1, 1), 255, np.uint8), 1))
    out.append(("one pixel, clear", np.zeros((1, 1), np.uint8), 3))
    b = _blob(2)
    out.append(("bytes 1 and 128", np.where(b, np.where(rng.random(b.shape) < 0.5, 1, 128), 0).astype(np.uint8), 2))
    return out


ALIAS = "blob r 2"          # the packed batch ends with one more descriptor that names this case's rectangle (same radii)


@functools.lru_cache(maxsize=None)
def expected():
    """per case (dilation, opening, closing) as bool arrays, computed once"""
    return [(dilate(m, d), opening(m, d), closing(m, d)) for _, m, d in cases()]


def mixed_ops(i, d):
    """the mixed chain of descriptor i of the batch: four operations, per-descriptor radii"""
    return (("dilate", 1 + i % 3), ("erode_clipped", d), ("erode", 1 + (i // 3) % 2), ("dilate", d))


def _ring(h, w, y0, y1, x0, x1, t=2):
    """a frame of thickness t around the background rectangle [y0, y1) x [x0, x1)"""
    m = np.zeros((h, w), bool)
    m[y0 - t:y1 + t, x0 - t:x1 + t] = True
    m[y0:y1, x0:x1] = False
    return m


@functools.lru_cache(maxsize=None)
def hole_cases():
    """[(name, uint8 mask, background connectivity, max_area)]"""
    rng = np.random.default_rng(22)
    out = []
    out.append(("hole across the tile borders", _u8(_ring(70, 75, 10, 60, 12, 68)), 4, None))     # spans x = 32, 64 and y = 32
    notch = np.zeros((20, 30), bool)
    notch[0:15, 5:25] = True
    notch[0:10, 12:15] = False                                              # open to row 0: no hole
    out.append(("notch open to the frame", _u8(notch), 4, None))
    diag = np.zeros((12, 14), bool)
    diag[2:9, 2:9] = True
    diag[4:7, 4:7] = False                                                  # a pocket ...
    diag[7, 7] = False                                                      # (at 4 a hole of its own)
    diag[8, 8] = False                                                      # ... that leaves through the corner, diagonally
    diag[7, 8] = diag[8, 7] = True
    out.append(("diagonal pocket, 4", _u8(diag), 4, None))
    out.append(("diagonal pocket, 8", _u8(diag), 8, None))
    island = _ring(40, 44, 6, 34, 6, 38)
    island[15:22, 18:26] = True
    island[17, 20] = False                                                  # a hole inside the island inside the hole
    out.append(("island inside a hole", _u8(island), 4, None))
    two = np.ones((12, 20), bool)
    two[0] = two[-1] = False
    two[3:5, 3:6] = False                                                   # 6 pixels
    two[3:5, 10:13] = False
    two[5, 10] = False                                                      # 7 pixels
    out.append(("areas of A and A + 1", _u8(two), 4, 6))
    out.append(("areas, no cap", _u8(two), 4, None))
    out.append(("areas, cap below both", _u8(two), 4, 5))
    touch = _ring(20, 24, 4, 16, 4, 20, t=4)                                # the ring reaches the frame on every side
    touch[10, 0:4] = False                                                  # the pocket reaches column 0 in one pixel
    out.append(("pocket touching the frame in one pixel", _u8(touch), 4, None))
    line = np.ones((9, 1), bool)
    line[3:5] = False
    out.append(("width 1", _u8(line), 4, None))
    out.append(("height 1", _u8(line.T.copy()), 8, None))
    out.append(("full", np.full((33, 65), 255, np.uint8), 4, None))
    out.append(("empty", np.zeros((33, 65), np.uint8), 4, None))
    blobs = _ring(100, 129, 20, 80, 20, 110, t=9)
    blobs[20:80, 60:70] = True                                              # two chambers
    blobs ^= rng.random(blobs.shape) < 0.01                                 # pin-holes in the walls, specks in the chambers
    out.append(("chambers with pin-holes, 4", _u8(blobs), 4, None))
    out.append(("chambers with pin-holes, 8, cap 3", np.where(blobs, 1, 0).astype(np.uint8), 8, 3))
    return out


@functools.lru_cache(maxsize=None)
def expected_holes():
    """per hole case (filled mask, holes filled, pixels filled, holes)"""
    return [fill_holes(m, c, a) for _, m, c, a in hole_cases()]


# what the cases were chosen for, checked once at import
def _check():
    names = [k for k, _, _ in cases()]
    assert len(set(names)) == len(names)
    exp = dict(zip(names, expected()))
    mask = {k: m != 0 for k, m, _ in cases()}
    rad = {k: d for k, _, d in cases()}
    for k in names:
        dil, op, cl = exp[k]
        m = mask[k]
        assert not (op & ~m).any() and not (m & ~cl).any() and not (cl & ~dil).any(), k          # open in M in close in D
        h, w = m.shape
        if 2 * rad[k] + 1 > min(h, w):
            assert not op.any(), k                                          # the square fits nowhere
    full_property = ["blob r %d" % r for r in BLOB_RADII] + ["bytes 1 and 128"] + [
        k for k in names if (k.startswith("d ") or k.startswith("width ")) and satisfiable(mask[k].shape[0], mask[k].shape[1], rad[k])]
    assert len(full_property) >= 7 + 5 * 2 + 6                              # + radii 1 .. 33 at heights 2 r + 1, 2 r + 2 and the wide width, + the widths >= 13
    for k in full_property:                                                 # open != input != close, neither result empty or full
        _, op, cl = exp[k]
        assert op.any() and not op.all() and cl.any() and not cl.all() and (op != mask[k]).any() and (cl != mask[k]).any(), k
    for r in BLOB_RADII:
        k = "blob r %d" % r
        _, op, cl = exp[k]
        assert (2 * r + 1) ** 2 <= op.sum() < mask[k].sum() < cl.sum(), k
    k = "bytes 1 and 128"
    assert exp[k][1].any() and not exp[k][2].all() and set(np.unique(cases()[names.index(k)][1])) == {0, 1, 128}
    for name in EDGES:                                                      # close keeps the object at the border, open removes it
        k = "flush " + name
        assert mask[k].any() and not exp[k][1].any() and not (mask[k] & ~exp[k][2]).any() and not exp[k][2].all(), k
    assert all(e.all() for e in exp["full"]) and not any(e.any() for e in exp["empty"])
    one = exp["one pixel, set"]                                             # E of a 1 x 1 image is empty, D and E' see the pixel alone
    assert one[0].all() and not one[1].any() and one[2].all() and not any(e.any() for e in exp["one pixel, clear"])
    changed = sum(bool((exp[k][1] != mask[k]).any()) + bool((exp[k][2] != mask[k]).any()) for k in names if k.startswith("d "))
    assert changed >= len(RADII) * 8                                        # the grid is not a list of fixed points
    assert {m.shape[1] for _, m, _ in cases()} >= set(WIDTHS) and all(max(m.shape) <= 200 for _, m, _ in cases())
    hn = [k for k, _, _, _ in hole_cases()]
    assert len(set(hn)) == len(hn) and all(max(m.shape) <= 200 for _, m, _, _ in hole_cases())
    got = {k: (int((f & ~(m != 0)).sum()), a, b, c) for (k, m, _, _), (f, a, b, c) in zip(hole_cases(), expected_holes())}
    assert all(v[0] == v[2] for v in got.values())
    assert got["hole across the tile borders"][1:] == (1, 50 * 56, 1) and got["notch open to the frame"][1:] == (0, 0, 0)
    assert got["diagonal pocket, 4"][1:] == (2, 10, 2) and got["diagonal pocket, 8"][1:] == (0, 0, 0)
    assert got["island inside a hole"][1:] == (2, 28 * 32 - 7 * 8 + 1, 2)
    assert got["areas of A and A + 1"][1:] == (1, 6, 2) and got["areas, no cap"][1:] == (2, 13, 2) and got["areas, cap below both"][1:] == (0, 0, 2)
    assert got["pocket touching the frame in one pixel"][1:] == (0, 0, 0) and got["width 1"][1:] == (0, 0, 0) == got["height 1"][1:]
    assert got["full"][1:] == (0, 0, 0) == got["empty"][1:]
    assert got["chambers with pin-holes, 4"][1] > 3 and 0 < got["chambers with pin-holes, 8, cap 3"][1] < got["chambers with pin-holes, 8, cap 3"][3]


_check()
