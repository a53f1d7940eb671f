"""Polygon form of binary masks on the host: numpy only, no device.

    p = polygon.encode(mask)         {"size": [h, w], "rings": [int32 [k, 2] of (x, y), ...], "holes": [bool, ...]}
    m = polygon.decode(p)            uint8 [h, w] of 0 / 255
    json.dump(polygon.to_coco(p), f) COCO's list-of-polygons segmentation (outer rings)

The format, all of it integer geometry (DESIGN.md 9b states it in full):
  - vertices are pixel CORNERS, integer (x, y) with 0 <= x <= w, 0 <= y <= h; pixel (px, py) is the square [px, px + 1] x [py, py + 1];
    a mask's foreground is byte != 0, outside the image is background;
  - a crack is a unit edge between a foreground pixel and a background pixel (or the outside), directed with the foreground on the
    RIGHT of travel (y grows downwards); at its end a ring continues with the first existing crack among turn right, straight, turn
    left - at a saddle vertex (10/01) both visits turn right, so the traced foreground is 4-connected;
  - a ring is the cyclic list of the vertices at which the direction changes, from its raster-first vertex (minimum y, then x), which
    an outer ring leaves heading east and a hole heading south; it has an even number >= 4 of vertices, horizontal and vertical edges
    alternating, and no collinear vertex;
  - with 2 A = sum x_i y_i+1 - x_i+1 y_i outer rings have A > 0 (clockwise on screen), holes A < 0 ("holes"); the areas of a mask's
    rings sum to its foreground pixels; even-odd filling of all rings sampled at pixel centres gives the mask back;
  - the rings of a mask are ordered by the raster order of their start vertices.  An empty mask has "rings": [].

`encode` is the format's vectorised restatement and the CPU route the device tracer replaces (csrc/polygon.hip behind
evalpost.polygon_count_batch / polygon_collect delivers the packed vertices and the ring table; `from_rings` slices them)."""
import numpy as np

MAX_VERTICES = 2 ** 28      # (h + 1) * (w + 1) must not exceed it (a corner visit is one 32-bit word on the device)


def _check_size(h, w):
    if isinstance(h, bool) or isinstance(w, bool) or not isinstance(h, (int, np.integer)) or not isinstance(w, (int, np.integer)):
        raise ValueError("polygon: size must be two integers, got %r" % ((h, w),))
    h, w = int(h), int(w)
    if h < 0 or w < 0 or (h + 1) * (w + 1) > MAX_VERTICES:
        raise ValueError("polygon: size must be non-negative with (h + 1) * (w + 1) <= 2^28, got %r" % ((h, w),))
    return h, w


def twice_area(ring):
    """2 A = sum x_i y_i+1 - x_i+1 y_i of one ring, as a Python int"""
    r = np.asarray(ring, np.int64)
    n = np.roll(r, -1, axis=0)
    return int((r[:, 0] * n[:, 1] - n[:, 0] * r[:, 1]).sum())


def validate(poly):
    """-> (h, w); raises ValueError before any work unless `poly` is a polygon mask: the dict's keys and types, int32 [k, 2] rings
    with k even and >= 4, every vertex inside [0, w] x [0, h], edges axis-parallel, non-degenerate and alternating between
    horizontal and vertical (hence no collinear vertex), and one bool per ring in "holes"."""
    if not isinstance(poly, dict) or "size" not in poly or "rings" not in poly or "holes" not in poly:
        raise ValueError("polygon: expected {'size': [h, w], 'rings': [...], 'holes': [...]}, got %r" % (type(poly).__name__,))
    size = poly["size"]
    if not isinstance(size, (list, tuple)) or len(size) != 2:
        raise ValueError("polygon: size must be [h, w], got %r" % (size,))
    h, w = _check_size(*size)
    rings, holes = poly["rings"], poly["holes"]
    if not isinstance(rings, (list, tuple)) or not isinstance(holes, (list, tuple)) or len(rings) != len(holes):
        raise ValueError("polygon: rings and holes must be lists of one length")
    for k, (r, hole) in enumerate(zip(rings, holes)):
        if not isinstance(hole, (bool, np.bool_)):
            raise ValueError("polygon: holes[%d] must be a bool" % k)
        if not isinstance(r, np.ndarray) or r.dtype != np.int32 or r.ndim != 2 or r.shape[1] != 2:
            raise ValueError("polygon: rings[%d] must be an int32 array [k, 2]" % k)
        if r.shape[0] < 4 or r.shape[0] % 2:
            raise ValueError("polygon: rings[%d] has %d vertices, a ring has an even number >= 4" % (k, r.shape[0]))
        if int(r.min()) < 0 or int(r[:, 0].max()) > w or int(r[:, 1].max()) > h:
            raise ValueError("polygon: rings[%d] leaves [0, %d] x [0, %d]" % (k, w, h))
        step = np.roll(r, -1, axis=0).astype(np.int64) - r
        horizontal, vertical = (step[:, 0] != 0) & (step[:, 1] == 0), (step[:, 0] == 0) & (step[:, 1] != 0)
        if not (horizontal | vertical).all():
            raise ValueError("polygon: rings[%d] has an edge that is not axis-parallel (or has no length)" % k)
        if (horizontal == np.roll(horizontal, -1)).any():
            raise ValueError("polygon: rings[%d] has a collinear vertex (horizontal and vertical edges must alternate)" % k)
    return h, w


def _jump(succ):
    """pointer jumping over the cyclic lists `succ`: -> (label, dist) per element, the smallest index of its cycle and the steps
    from the element to it (0 at the smallest itself).  A strictly smaller label wins, so the first occurrence is kept."""
    n = succ.size
    label, dist, hop = np.arange(n, dtype=np.int64), np.zeros(n, np.int64), 1
    while hop < n:
        l2 = label[succ]
        take = l2 < label
        dist = np.where(take, hop + dist[succ], dist)
        label = np.where(take, l2, label)
        succ = succ[succ]
        hop *= 2
    return label, dist


def corner_visits(mask):
    """The corner visits of a mask in row-major vertex order (a saddle's west-connected copy first) -> int64 arrays
    (x, y, he, vs, outv): the vertex, whether the visit's horizontal crack is the east one, its vertical crack the south one, and
    whether the ring leaves on the vertical crack.  What csrc/polygon_core.h computes per vertex, for all vertices at once."""
    m = np.asarray(mask)
    if m.ndim != 2:
        raise ValueError("polygon: mask must be 2-d, got shape %r" % (m.shape,))
    h, w = _check_size(*m.shape)
    p = np.zeros((h + 2, w + 2), bool)
    p[1:-1, 1:-1] = m != 0
    a, b, c, d = p[:-1, :-1], p[:-1, 1:], p[1:, :-1], p[1:, 1:]           # [y, x]: north-west, north-east, south-west, south-east
    north, south, west, east = a != b, c != d, a != c, b != d
    saddle = north & south & west & east
    corner = (north ^ south) & (west ^ east)
    visit = np.stack([saddle | (corner & west), saddle | (corner & east)], axis=2)
    y, x, he = np.nonzero(visit)                                           # ascending (y, x, he)
    sad, av, bv, cv = saddle[y, x], a[y, x], b[y, x], c[y, x]
    vs = np.where(sad, np.where(av, he == 1, he == 0), south[y, x])        # the pairing of the turn-right rule
    outv = np.where(vs, cv, bv)
    return x.astype(np.int64), y.astype(np.int64), he.astype(np.int64), vs.astype(np.int64), outv.astype(np.int64)


def encode(mask):
    """mask: 2-d array, foreground where != 0 -> the polygon dict.  Vectorised: corner visits, the successor of each through its
    partner in the row-major or column-major list, ring and rank by pointer jumping - no per-pixel or per-crack Python loop."""
    m = np.asarray(mask)
    x, y, he, vs, outv = corner_visits(m)
    h, w = m.shape
    n = x.size
    if n == 0:
        return {"size": [h, w], "rings": [], "holes": []}
    order = np.argsort((x * (h + 1) + y) * 2 + vs, kind="stable")         # the column-major list
    place = np.empty(n, np.int64)
    place[order] = np.arange(n)
    succ = np.where(outv == 1, order[place ^ 1], np.arange(n) ^ 1)
    label, dist = _jump(succ)
    starts = np.nonzero(label == np.arange(n))[0]
    length = np.zeros(n, np.int64)
    length[starts] = dist[succ[starts]] + 1
    rank = np.where(dist > 0, length[label] - dist, 0)
    by_ring = np.lexsort((rank, label))
    verts = np.stack([x[by_ring], y[by_ring]], axis=1).astype(np.int32)
    rings = np.split(verts, np.cumsum(length[starts])[:-1])
    return {"size": [h, w], "rings": rings, "holes": [twice_area(r) < 0 for r in rings]}


def from_rings(vertices, table, sizes):
    """What the device tracer delivers for a batch -> the polygon dicts: vertices int32 [V, 2]; table int64 [R, 4] of (descriptor,
    offset, length, 2 A) in descriptor order; sizes (h, w) per descriptor."""
    vertices, table = np.asarray(vertices), np.asarray(table, np.int64).reshape(-1, 4)
    out = [{"size": [int(h), int(w)], "rings": [], "holes": []} for h, w in sizes]
    for desc, off, length, area2 in table.tolist():
        if not (0 <= desc < len(out) and 0 <= off and length >= 4 and off + length <= vertices.shape[0] and area2 != 0):
            raise RuntimeError("polygon: ring row %r does not belong to %d vertices of %d masks" % ((desc, off, length, area2), vertices.shape[0], len(out)))
        out[desc]["rings"].append(np.array(vertices[off:off + length], dtype=np.int32))
        out[desc]["holes"].append(area2 < 0)
    return out


def decode(poly):
    """-> uint8 [h, w] of 0 / 255: even-odd filling of all rings, sampled at pixel centres"""
    h, w = validate(poly)
    toggles = np.zeros((h + 1, w + 1), np.int64)
    for r in poly["rings"]:
        n = np.roll(r, -1, axis=0)
        v = r[:, 0] == n[:, 0]                                             # the vertical edges: they toggle the pixels to their right
        xs, y0, y1 = r[v, 0], np.minimum(r[v, 1], n[v, 1]), np.maximum(r[v, 1], n[v, 1])
        np.add.at(toggles, (y0, xs), 1)
        np.add.at(toggles, (y1, xs), -1)
    crossings = np.cumsum(np.cumsum(toggles, axis=0), axis=1)
    return ((crossings[:h, :w] & 1) * 255).astype(np.uint8)


def area(poly):
    """the sum of the signed ring areas = the foreground pixels"""
    validate(poly)
    return sum(twice_area(r) for r in poly["rings"]) // 2


def to_bbox(poly):
    """(x0, y0, x1, y1) half-open from the vertices, None for an empty mask"""
    validate(poly)
    if not poly["rings"]:
        return None
    v = np.concatenate(poly["rings"])
    return int(v[:, 0].min()), int(v[:, 1].min()), int(v[:, 0].max()), int(v[:, 1].max())


def to_coco(poly, holes=False):
    """COCO's polygon segmentation: a list of flat [x0, y0, x1, y1, ...] int lists, one per ring.  COCO polygons CANNOT express
    holes - every listed polygon is filled - so only the outer rings are listed and a mask with holes comes out with them filled;
    fill them in the mask itself first (`Smooth(fill_holes=True)` of predict / evalpost) or exchange RLE (masks="rle") when they
    matter.  holes=True lists every ring in order, for tooling that fills even-odd."""
    validate(poly)
    return [[int(v) for v in r.reshape(-1)] for r, hole in zip(poly["rings"], poly["holes"]) if holes or not hole]
