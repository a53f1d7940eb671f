"""Cases and an independent oracle for the polygon tracer (cris/pytorch_amd/polygon.py on the host, csrc/polygon.hip behind
evalpost.polygon_count_batch / polygon_collect on the device).  The oracle is the plain per-crack follower of the format's
definition - one crack at a time, turn right before straight before left - and a per-pixel even-odd decode, written apart from
polygon.py's vectorised code so that the two check each other.  The cases are the smallest shapes at which the kernels can take
another path: RB vertex rows per band, CG vertex columns per tile, CHUNK visits per block of the ring-base scan."""
import functools

import numpy as np

RB, CG, CHUNK = 32, 64, 1024        # evalpost.POLYGON_RB / POLYGON_CG / POLYGON_CHUNK (csrc/polygon.hip); test_polygon_cpu.py compares them

DX, DY = (1, 0, -1, 0), (0, 1, 0, -1)       # directions 0 east, 1 south, 2 west, 3 north (y grows downwards): turning right is + 1


def pitch_of(w):
    return (w + 3) // 4 * 4


def _padded(mask):
    m = np.asarray(mask) != 0
    p = np.zeros((m.shape[0] + 2, m.shape[1] + 2), bool)
    p[1:-1, 1:-1] = m
    return p.tolist()                                                       # pixel (px, py) is p[py + 1][px + 1]; outside is background


def _crack(p, x, y, d):
    """is there a crack that leaves vertex (x, y) in direction d: foreground on its right, background on its left"""
    if d == 0:
        right, left = p[y + 1][x + 1], p[y][x + 1]                          # heading east: south of it pixel (x, y), north (x, y - 1)
    elif d == 1:
        right, left = p[y + 1][x], p[y + 1][x + 1]                          # heading south: west of it (x - 1, y), east (x, y)
    elif d == 2:
        right, left = p[y][x], p[y + 1][x]                                  # heading west: north of it (x - 1, y - 1), south (x - 1, y)
    else:
        right, left = p[y][x + 1], p[y][x]                                  # heading north: east of it (x, y - 1), west (x - 1, y - 1)
    return right and not left


def oracle_trace(mask):
    """-> (rings, visits): rings = [[(x, y), ...]] each from its raster-first vertex, ordered by those; visits = every corner visit
    as (x, y, direction in, direction out) in no particular order"""
    h, w = np.asarray(mask).shape
    p = _padded(mask)
    seen, rings, visits = set(), [], []
    for y in range(h + 1):
        for x in range(w + 1):
            for d in range(4):
                if (x, y, d) in seen or not _crack(p, x, y, d):
                    continue
                ring, cx, cy, cd = [], x, y, d
                while True:
                    seen.add((cx, cy, cd))
                    cx, cy = cx + DX[cd], cy + DY[cd]
                    for nd in ((cd + 1) % 4, cd, (cd + 3) % 4):             # turn right, straight, turn left
                        if _crack(p, cx, cy, nd):
                            break
                    else:
                        raise AssertionError("a crack ends at (%d, %d)" % (cx, cy))
                    if nd != cd:
                        ring.append((cx, cy))
                        visits.append((cx, cy, cd, nd))
                    cd = nd
                    if (cx, cy, cd) == (x, y, d):
                        break
                first = min(range(len(ring)), key=lambda i: (ring[i][1], ring[i][0]))
                rings.append(ring[first:] + ring[:first])
    rings.sort(key=lambda r: (r[0][1], r[0][0]))
    return rings, visits


def oracle_visit_bits(visit):
    """(x, y, in, out) -> (he, vs, outv): the horizontal crack is the east one, the vertical crack the south one, leaves vertically"""
    _, _, din, dout = visit
    if din in (0, 2):                                                       # arrives horizontally, leaves vertically
        return int(din == 2), int(dout == 1), 1                             # heading west it came along the east crack
    return int(dout == 0), int(din == 3), 0                                 # heading north it came along the south crack


def oracle_twice_area(ring):
    return sum(ring[i][0] * ring[(i + 1) % len(ring)][1] - ring[(i + 1) % len(ring)][0] * ring[i][1] for i in range(len(ring)))


def oracle_decode(rings, h, w):
    """even-odd filling sampled at pixel centres, one pixel at a time: (px + 0.5, py + 0.5) is inside iff an odd number of vertical
    edges lies to its left on its row"""
    edges = [[] for _ in range(h)]
    for r in rings:
        for i, (x0, y0) in enumerate(r):
            x1, y1 = r[(i + 1) % len(r)]
            if x0 == x1:
                for y in range(min(y0, y1), max(y0, y1)):
                    edges[y].append(x0)
    out = np.zeros((h, w), np.uint8)
    for y in range(h):
        if not edges[y]:
            continue
        xs, inside, k = sorted(edges[y]), False, 0
        for px in range(w):
            while k < len(xs) and xs[k] <= px:
                inside, k = not inside, k + 1
            if inside:
                out[y, px] = 255
    return out


def comb(vertices):
    """a 3 x W mask whose single ring has exactly `vertices` corners (vertices >= 8, even): a spine over teeth at the even columns"""
    if vertices % 4 == 0:
        teeth = vertices // 4
        m = np.zeros((3, 2 * teeth - 1), np.uint8)                          # teeth flush with both ends: 4 T
    else:
        teeth = (vertices - 2) // 4
        m = np.zeros((3, 2 * teeth), np.uint8)                              # the spine runs one column past the last tooth: 4 T + 2
    m[0, :] = 255
    m[1:, 0:2 * teeth:2] = 255
    return m


COMB_SIZES = [2 ** k + e for k in (6, 8, 10, 12) for e in (-2, 0, 2)]      # around one wave, one block, one scan chunk and 4096


def serpentine(n=64):
    m = np.zeros((n, n), np.uint8)
    m[0::2, :] = 255
    m[1::4, n - 1] = 255
    m[3::4, 0] = 255
    return m


def _blob(h=480, w=640):
    """the 480 x 640 blob of rle_cases.py, rebuilt here"""
    yy, xx = np.mgrid[0:h, 0:w]
    m = ((xx - 300) / 170.0) ** 2 + ((yy - 250) / 120.0) ** 2 < 1.0
    m &= ~(((xx - 330) / 40.0) ** 2 + ((yy - 230) / 30.0) ** 2 < 1.0)      # a hole
    m |= (np.abs(xx - 60) < 9) & (yy > 400)                                 # a bar that reaches the last row
    m |= np.random.default_rng(5).random((h, w)) < 0.0005                   # specks
    return m.astype(np.uint8) * 255


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, uint8 mask)] - one ragged batch"""
    rng = np.random.default_rng(11)
    rand = lambda h, w, p: (rng.random((h, w)) < p).astype(np.uint8) * 255                       # noqa: E731
    out = [("1x1 background", np.zeros((1, 1), np.uint8)), ("1x1 foreground", np.full((1, 1), 255, np.uint8)),
           ("1x7", np.array([[0, 255, 255, 0, 0, 255, 0]], np.uint8)), ("7x1", np.array([[255, 0, 0, 255, 255, 0, 255]], np.uint8).T)]
    for w in (3, 4, 5):                                                     # pitch padding of 1, 0 and 3 bytes
        out.append(("width %d" % w, rand(9, w, 0.5)))
    out.append(("all background", np.zeros((RB + 5, 10), np.uint8)))
    out.append(("all foreground", np.full((RB + 5, 10), 255, np.uint8)))
    for h in (RB - 2, RB - 1, RB, 2 * RB - 2, 2 * RB - 1, 2 * RB):          # h + 1 vertex rows: one below, at and above one band, then two
        out.append(("height %d" % h, rand(h, 6, 0.4)))
    for w in (CG - 2, CG - 1, CG, 2 * CG - 2, 2 * CG - 1, 2 * CG):          # w + 1 vertex columns around one and two tiles, two bands
        out.append(("width %d" % w, rand(RB + 2, w, 0.3)))
    out.append(("full tile edges", np.full((RB - 1, CG - 1), 255, np.uint8)))      # the last vertex row / column are a tile's last
    yy, xx = np.mgrid[0:35, 0:67]
    out.append(("checkerboard odd", (((yy + xx + 1) & 1) * 255).astype(np.uint8)))  # h odd, (0, 0) foreground: every interior vertex a saddle
    out.append(("checkerboard even", (((yy + xx) & 1) * 255).astype(np.uint8)))
    out.append(("diagonal", (np.eye(13, dtype=np.uint8) * 255)))                    # chains of saddles, either kind
    out.append(("anti-diagonal", (np.eye(13, dtype=np.uint8)[:, ::-1] * 255).copy()))
    frame = np.full((8, 9), 255, np.uint8)
    frame[1:-1, 1:-1] = 0
    out.append(("frame", frame))
    hole = np.full((7, 6), 255, np.uint8)
    hole[2:4, 3:5] = 0
    out.append(("hole", hole))
    island = np.zeros((11, 12), np.uint8)
    island[1:10, 1:11] = 255
    island[3:8, 3:9] = 0
    island[5, 5:7] = 255
    out.append(("island in a hole", island))                               # hole inside outer, outer inside hole
    nested = np.full((13, 13), 255, np.uint8)
    nested[2:11, 2:11] = 0
    nested[4:9, 4:9] = 255
    nested[6, 6] = 0
    out.append(("hole in an island in a hole", nested))
    leak = np.full((4, 5), 255, np.uint8)
    leak[1, 1] = 0
    leak[2, 2] = 0                                                          # (1, 1) meets (2, 2) at a saddle: both visits turn right around
    out.append(("holes that touch across a diagonal", leak))                # their foreground pixel, so ONE hole ring that touches itself
    diag_out = np.array([[255, 255, 255, 0], [255, 0, 255, 0], [255, 255, 0, 0]], np.uint8)
    out.append(("background pixel that meets the outside across a diagonal", diag_out))     # the same rule: one outer ring walks
    ringed = np.array([[0, 255, 0], [255, 0, 255], [0, 255, 0]], np.uint8)                  # round it too, there is no hole ring
    out.append(("pixels that enclose one across diagonals only", ringed))   # four rings of one pixel, the middle is no hole
    out.append(("bytes 1 and 128", np.where(rng.random((12, 13)) < 0.5, np.where(rng.random((12, 13)) < 0.5, 1, 128), 0).astype(np.uint8)))
    dense = rand(45, 77, 0.5)
    out.append(("random 0.5", dense))
    out.append(("random 0.02", rand(150, 131, 0.02)))
    out.append(("random 0.5 again", dense.copy()))                          # equal content at another out_off
    for v in COMB_SIZES:
        out.append(("comb %d" % v, comb(v)))
    out.append(("serpentine", serpentine()))
    out.append(("blob 480x640", _blob()))
    return out


ALIAS = "random 0.02"       # the packed batch ends with one more descriptor that names this case's rectangle
SMALL = 200                 # the cases of at most this many pixels also go through the g++ probe of polygon_core.h


@functools.lru_cache(maxsize=None)
def expected():
    """per case (rings, visits) from the oracle, computed once"""
    return [oracle_trace(m) for _, m in cases()]


def expected_dict(i):
    """case i as the polygon dict the format asks for, from the oracle"""
    m = cases()[i][1]
    rings = expected()[i][0]
    return {"size": [m.shape[0], m.shape[1]], "rings": [np.array(r, np.int32).reshape(-1, 2) for r in rings],
            "holes": [oracle_twice_area(r) < 0 for r in rings]}
