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

`simplify(p, epsilon)` is the integer-exact Douglas-Peucker simplifier (csrc/simplify_core.h states the predicate): a
result carries "epsilon", its rings are general integer polygons - any k >= 3, any edge direction, 2 A possibly 0 or odd - that
still start at the raster-first vertex, and "holes" keeps the orientation of the TRACED rings.  `validate`, `decode`, `area`,
`to_bbox` and `to_coco` take both forms; a dict without "epsilon" is treated exactly as before.

`encode` is the format's vectorised restatement and the CPU route the device tracer replaces (csrc/polygon.hip behind
evalpost.polygon_count_batch / polygon_collect delivers the packed vertices and the ring table; `from_rings` slices them)."""
import numpy as np

MAX_VERTICES = 2 ** 28      # (h + 1) * (w + 1) must not exceed it (a corner visit is one 32-bit word on the device)
MAX_SIMPLIFY_SIDE = 32767   # h, w of a mask that is simplified: |cross| <= 2 h w < 2^29, so 16 cross^2 < 2^62 fits 64 bits (SP_MAX_SIDE)


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
    horizontal and vertical (hence no collinear vertex), and one bool per ring in "holes".  A dict with "epsilon" (a result of
    `simplify`) needs a valid float epsilon and, per ring, int32 [k, 2] with k >= 3, every vertex inside and no edge of no length."""
    if not isinstance(poly, dict) or "size" not in poly or "rings" not in poly or "holes" not in poly:
        raise ValueError("polygon: expected {'size': [h, w], 'rings': [...], 'holes': [...]}, got %r" % (type(poly).__name__,))
    size = poly["size"]
    if not isinstance(size, (list, tuple)) or len(size) != 2:
        raise ValueError("polygon: size must be [h, w], got %r" % (size,))
    h, w = _check_size(*size)
    rings, holes = poly["rings"], poly["holes"]
    if not isinstance(rings, (list, tuple)) or not isinstance(holes, (list, tuple)) or len(rings) != len(holes):
        raise ValueError("polygon: rings and holes must be lists of one length")
    simplified = "epsilon" in poly
    if simplified:
        if not isinstance(poly["epsilon"], float):
            raise ValueError("polygon: epsilon of a simplified mask must be a float, got %r" % (poly["epsilon"],))
        check_epsilon(poly["epsilon"])
    for k, (r, hole) in enumerate(zip(rings, holes)):
        if not isinstance(hole, (bool, np.bool_)):
            raise ValueError("polygon: holes[%d] must be a bool" % k)
        if not isinstance(r, np.ndarray) or r.dtype != np.int32 or r.ndim != 2 or r.shape[1] != 2:
            raise ValueError("polygon: rings[%d] must be an int32 array [k, 2]" % k)
        if simplified:                                                      # a general integer polygon
            if r.shape[0] < 3:
                raise ValueError("polygon: rings[%d] has %d vertices, a simplified ring has >= 3" % (k, r.shape[0]))
            if int(r.min()) < 0 or int(r[:, 0].max()) > w or int(r[:, 1].max()) > h:
                raise ValueError("polygon: rings[%d] leaves [0, %d] x [0, %d]" % (k, w, h))
            if not (np.roll(r, -1, axis=0) != r).any(axis=1).all():
                raise ValueError("polygon: rings[%d] has an edge of no length" % k)
            continue
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


def simplify_from_rings(vertices, table, sizes, epsilon):
    """What the device simplifier delivers for a batch -> the simplified dicts: vertices int32 [V, 2]; table int64 [R, 5] of
    (descriptor, offset, length, 2 A of the simplified ring, hole flag of the traced ring) in descriptor order; sizes (h, w) per
    descriptor.  The loop over rings is the one `from_rings` has."""
    epsilon = check_epsilon(epsilon) / 4.0
    vertices, table = np.asarray(vertices), np.asarray(table, np.int64).reshape(-1, 5)
    out = [{"size": [int(h), int(w)], "rings": [], "holes": [], "epsilon": epsilon} for h, w in sizes]
    for desc, off, length, _, hole in table.tolist():
        if not (0 <= desc < len(out) and 0 <= off and length >= 3 and off + length <= vertices.shape[0] and hole in (0, 1)):
            raise RuntimeError("polygon: simplified ring row %r does not belong to %d vertices of %d masks" % ((desc, off, length, hole), vertices.shape[0], len(out)))
        out[desc]["rings"].append(np.array(vertices[off:off + length], dtype=np.int32))
        out[desc]["holes"].append(bool(hole))
    return out


def check_epsilon(epsilon):
    """-> q = 4 epsilon as an int in 1 .. 256; raises ValueError unless epsilon is a multiple of 0.25 in [0.25, 64]"""
    ok = not isinstance(epsilon, (bool, np.bool_)) and isinstance(epsilon, (int, float, np.integer, np.floating))
    if ok:
        q = 4.0 * float(epsilon)
        ok = q == q and 1.0 <= q <= 256.0 and q == int(q)
    if not ok:
        raise ValueError("polygon: epsilon must be a multiple of 0.25 in [0.25, 64] (pixels), got %r" % (epsilon,))
    return int(q)


def check_simplify_size(h, w):
    if h > MAX_SIMPLIFY_SIDE or w > MAX_SIMPLIFY_SIDE:
        raise ValueError("polygon: simplify needs h, w <= %d (the 64-bit bound of its split test), got %r" % (MAX_SIMPLIFY_SIDE, (h, w)))


def simplify_kept(rings, q, rounds=None):
    """The Douglas-Peucker selection of DESIGN.md 9b for a list of traced rings at once -> per ring the sorted indices it keeps (the
    ring is removed when fewer than 3).  Round-synchronous like csrc/simplify.hip and vectorised over every segment of every ring:
    positions 0 .. k of each ring lie in one array (position k is v_0 again, the end of the second chain).  Kept so far {0, a, k}
    with a = the smallest index that maximises |v_i - v_0|^2; each round every segment (i, j) of consecutive kept positions takes
    the maximum over its interior of the key (c_m << 32) | (2^32 - 1 - u), c_m = |(v_j - v_i) x (v_m - v_i)| < 2^29,
    u = 2 |t| + (t > 0), t = 2 m - (i + j) - the greatest c_m, then the m nearest the middle, then the smallest m - and keeps it
    iff 16 c_m^2 > q^2 |v_j - v_i|^2 (< 2^62 against < 2^47: int64).  Ends with the first round that keeps nothing.  rounds: a list
    that receives the number of rounds."""
    if not rings:
        return []
    lens = np.array([r.shape[0] for r in rings], np.int64)
    first = np.cumsum(lens + 1) - (lens + 1)                                # position 0 of every ring
    total = int((lens + 1).sum())
    ring_of = np.repeat(np.arange(lens.size), lens + 1)
    local = np.arange(total) - first[ring_of]
    v = np.empty((total, 2), np.int64)
    closing = local == lens[ring_of]
    v[~closing] = np.concatenate(rings)
    v[closing] = v[first]
    d = v - v[first[ring_of]]
    mask32 = np.int64(0xffffffff)
    key = ((d * d).sum(axis=1) << 32) | (mask32 - local)
    key[closing] = -1
    anchor = mask32 - (np.maximum.reduceat(key, first) & mask32)
    kept = closing.copy()
    kept[first] = True
    kept[first + anchor] = True
    index, count = np.arange(total), 0
    while True:
        count += 1
        at = np.nonzero(kept)[0]
        seg = np.cumsum(kept) - 1                                           # the kept position at or before each position
        i, j = at[seg], at[np.minimum(seg + 1, at.size - 1)]
        dij, dim = v[j] - v[i], v - v[i]
        c = np.abs(dij[:, 0] * dim[:, 1] - dij[:, 1] * dim[:, 0])
        t = 2 * index - (i + j)
        key = np.where(kept, np.int64(0), (c << 32) | (mask32 - (2 * np.abs(t) + (t > 0))))
        best = np.maximum.reduceat(key, at)                                 # per segment, from its first kept position on
        i, j = at, np.append(at[1:], at[-1])
        cm, u = best >> 32, mask32 - (best & mask32)
        m = (np.where(u & 1, u >> 1, -(u >> 1)) + i + j) // 2
        dij = v[j] - v[i]
        win = (cm > 0) & (16 * cm * cm > q * q * (dij * dij).sum(axis=1))
        if not win.any():
            break
        kept[m[win]] = True
    if rounds is not None:
        rounds.append(count)
    flags = np.split(kept & ~closing, first[1:])
    return [np.nonzero(f)[0] for f in flags]


def simplify(poly, epsilon):
    """The traced dict `poly` simplified by Douglas-Peucker with tolerance `epsilon` pixels (a multiple of 0.25 in [0.25, 64]) -> a
    new dict {"size", "rings", "holes", "epsilon": float}: per ring the kept vertices in index order (so it still starts at its
    raster-first vertex), rings left with fewer than 3 vertices removed, "holes" the orientation of the traced rings.  Integer
    exact and defined in full in DESIGN.md 9b (`simplify_kept`); the route csrc/simplify.hip replaces.  Raises ValueError before
    any work for a malformed dict, one that is simplified already, a bad epsilon or a side above 32767."""
    q = check_epsilon(epsilon)
    if isinstance(poly, dict) and "epsilon" in poly:
        raise ValueError("polygon: simplify takes a traced dict, this one is simplified already (epsilon %r)" % (poly["epsilon"],))
    h, w = validate(poly)
    check_simplify_size(h, w)
    kept = simplify_kept(poly["rings"], q)
    out = {"size": [h, w], "rings": [], "holes": [], "epsilon": q / 4.0}
    for r, hole, idx in zip(poly["rings"], poly["holes"], kept):
        if idx.size >= 3:
            out["rings"].append(np.ascontiguousarray(r[idx]))
            out["holes"].append(bool(hole))
    return out


def decode(poly):
    """-> uint8 [h, w] of 0 / 255: even-odd filling of all rings, sampled at pixel centres.  The general polygons of a simplified dict
    are filled in exact integers (`_decode_general`)."""
    h, w = validate(poly)
    if "epsilon" in poly:
        return _decode_general(poly["rings"], h, w)
    toggles = np.zeros((h + 1, w + 1), np.int64)
    for r in poly["rings"]:
        n = np.roll(r, -1, axis=0)
        v = r[:, 0] == n[:, 0]                                             # the vertical edges: they toggle the pixels to their right
        xs, y0, y1 = r[v, 0], np.minimum(r[v, 1], n[v, 1]), np.maximum(r[v, 1], n[v, 1])
        np.add.at(toggles, (y0, xs), 1)
        np.add.at(toggles, (y1, xs), -1)
    crossings = np.cumsum(np.cumsum(toggles, axis=0), axis=1)
    return ((crossings[:h, :w] & 1) * 255).astype(np.uint8)


def _decode_general(rings, h, w):
    """even-odd filling of general integer polygons sampled at pixel centres, exactly: in doubled coordinates the centre of pixel
    (px, py) is (2 px + 1, 2 py + 1) and a vertex (2 x, 2 y).  An edge from (x0, y0) to (x1, y1) crosses the centre line Y = 2 py + 1
    iff (2 y0 <= Y) != (2 y1 <= Y) - half-open in y, so a vertex on the line would count once (Y is odd: none is) - and toggles
    the pixels of that row whose centre lies at or right of the crossing: 2 px + 1 >= 2 x0 + (Y - 2 y0) dx / dy, so that a row of
    the filling is half-open too, [left crossing, right crossing).  Vectorised over all (edge, row) pairs."""
    toggles = np.zeros((h, w + 1), np.int64)
    if rings:
        a = np.concatenate(rings).astype(np.int64)
        b = np.concatenate([np.roll(r, -1, axis=0) for r in rings]).astype(np.int64)
        flip = b[:, 1] < a[:, 1]                                           # orient every edge downwards: dy > 0
        a, b = np.where(flip[:, None], b, a), np.where(flip[:, None], a, b)
        keep = b[:, 1] > a[:, 1]                                           # horizontal edges cross no centre line
        a, b = a[keep], b[keep]
        rows = b[:, 1] - a[:, 1]                                           # the centre lines py = y0 .. y1 - 1: 2 y0 <= 2 py + 1 < 2 y1
        edge = np.repeat(np.arange(rows.size), rows)
        py = np.arange(int(rows.sum())) - np.repeat(np.cumsum(rows) - rows, rows) + a[edge, 1]
        dx, dy = (b[:, 0] - a[:, 0])[edge], rows[edge]
        num = (2 * py + 1 - 2 * a[edge, 1]) * dx                            # crossing at 2 x0 + num / dy
        px = a[edge, 0] - (dy - num) // (2 * dy)                            # the smallest px with 2 px + 1 - 2 x0 >= num / dy: a ceiling
        np.add.at(toggles, (py, np.clip(px, 0, w)), 1)
    return ((np.cumsum(toggles, axis=1)[:, :w] & 1) * 255).astype(np.uint8)


def area(poly):
    """the sum of the signed ring areas: the foreground pixels of a traced dict (an int); sum(2 A) / 2 of a simplified one, a float
    when the sum is odd"""
    validate(poly)
    twice = sum(twice_area(r) for r in poly["rings"])
    return twice // 2 if twice % 2 == 0 or "epsilon" not in poly else twice / 2


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
