"""Oracle and cases of the connected-component clean-up (evalpost.Components, csrc/evalpost.hip cc_* kernels).

The oracle is plain numpy / Python and shares nothing with the kernels: a two-pass labeller over the horizontal runs of every row
(union-find over runs, the root is the run that starts first in raster order), the filtering rule and the statistics, all per the
definitions of DESIGN.md 9b:

    foreground      byte != 0 (the arrays here have no padding: pitch only enters the label VALUES)
    canonical label y * pitch + x of the component's first pixel in raster order; background -1
    filtering       components of area < min_area go first; keep="largest" then keeps the greatest area, ties to the lowest label
    statistics      (area, score_q16, x_min, y_min, x_end, y_end) over the kept pixels, evalpost.PREDICT_INIT when there are none

Everything is an integer, so every comparison against it is an equality."""
import functools

import numpy as np

PREDICT_INIT = [0, 0, 2 ** 31 - 1, 2 ** 31 - 1, 0, 0]


def pitch_of(w):
    return (int(w) + 3) // 4 * 4


def label(mask, connectivity=8, pitch=None):
    """mask: [h, w], foreground where != 0 -> int32 [h, w] canonical labels (y * pitch + x of the first pixel, -1 background)"""
    if connectivity not in (4, 8):
        raise ValueError("connectivity must be 4 or 8")
    fg = np.asarray(mask) != 0
    h, w = fg.shape
    pitch = pitch_of(w) if pitch is None else int(pitch)
    parent, where = [], []                      # per run: union-find parent; (y, x0, x1) with x1 exclusive

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    reach = 0 if connectivity == 4 else 1       # a run [x0, x1) touches a run [a, b) of the row above iff a < x1 + reach and b > x0 - reach
    prev = []
    for y in range(h):
        edge = np.diff(np.concatenate(([0], fg[y].astype(np.int8), [0])))
        cur, j = [], 0
        for x0, x1 in zip(np.nonzero(edge == 1)[0].tolist(), np.nonzero(edge == -1)[0].tolist()):
            i = len(parent)
            parent.append(i)
            where.append((y, x0, x1))
            while j < len(prev) and prev[j][1] <= x0 - reach:
                j += 1
            k = j
            while k < len(prev) and prev[k][0] < x1 + reach:
                a, b = find(i), find(prev[k][2])
                if a != b:
                    parent[max(a, b)] = min(a, b)           # run ids ascend in raster order: the smaller id starts first
                k += 1
            cur.append((x0, x1, i))
        prev = cur
    out = np.full((h, w), -1, np.int32)
    for i, (y, x0, x1) in enumerate(where):
        ry, rx, _ = where[find(i)]
        out[y, x0:x1] = ry * pitch + rx
    return out


def components(labels):
    """-> (canonical labels ascending, their areas)"""
    roots, areas = np.unique(labels[labels >= 0], return_counts=True)
    return roots.astype(np.int64), areas.astype(np.int64)


def filter_mask(mask, keep="all", min_area=0, connectivity=8, pitch=None):
    """-> (kept: bool [h, w], info: [n_components, kept_components, raw_area, 0], labels)"""
    labels = label(mask, connectivity, pitch)
    roots, areas = components(labels)
    ok = areas >= min_area
    cand, a = roots[ok], areas[ok]
    if keep == "largest" and cand.size:
        cand = cand[np.lexsort((cand, -a))[:1]]             # greatest area, then the lowest label
    elif keep not in ("all", "largest"):
        raise ValueError(keep)
    kept = np.isin(labels, cand) & (labels >= 0)
    return kept, [int(roots.size), int(cand.size), int(areas.sum()), 0], labels


def stats_row(kept, q16=None):
    """the predict_batch statistics row of the pixels `kept`; q16: int64 [h, w] of rint(value * 65536) per pixel (None: 0)"""
    area = int(kept.sum())
    if not area:
        return list(PREDICT_INIT)
    ys, xs = np.nonzero(kept)
    return [area, 0 if q16 is None else int(q16[kept].sum()), int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1]


# ---- cases ----
def _spiral(h, w):
    """a one-pixel-wide rectangular spiral with one-pixel gaps: ONE component at either connectivity, a chain through every tile"""
    m = np.zeros((h, w), np.uint8)
    y = x = turn = 0
    m[0, 0] = 255
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))

    def free(yy, xx):
        return 0 <= yy < h and 0 <= xx < w and not m[yy, xx]

    while True:
        dy, dx = dirs[turn % 4]
        steps = 0
        # walk while the next cell is free and the one behind it is not an arm laid down earlier (stop one short of it)
        while free(y + dy, x + dx) and (free(y + 2 * dy, x + 2 * dx) or not (0 <= y + 2 * dy < h and 0 <= x + 2 * dx < w)):
            y, x = y + dy, x + dx
            m[y, x] = 255
            steps += 1
        if steps < 2 and turn:
            return m
        turn += 1


def _comb(h, w):
    """teeth in every second column, joined only by the LAST row (a U per pair of teeth): every merge is late"""
    m = np.zeros((h, w), np.uint8)
    m[:, ::2] = 200
    m[h - 1, :] = 200
    return m


def _stairs(n):
    """a diagonal and an anti-diagonal staircase that never meet: 2 components at 8, every pixel its own at 4"""
    m = np.zeros((n, 2 * n + 3), np.uint8)
    i = np.arange(n)
    m[i, i] = 255
    m[i, 2 * n + 2 - i] = 1
    return m


def _tie():
    """two components of 12 pixels: the right one starts a row EARLIER, so it has the lower label and wins; a third of 11"""
    m = np.zeros((40, 45), np.uint8)
    m[5:8, 2:6] = 255
    m[4:7, 36:40] = 255
    m[20:31, 33] = 255
    return m


def _specks():
    """components of 1, 2, 3, 4 and 5 pixels, apart at either connectivity"""
    m = np.zeros((12, 39), np.uint8)
    for k in range(1, 6):
        m[3, 7 * k - 5:7 * k - 5 + k] = 255
    return m


def _edge_runs(w):
    """a run that ends in the last column of row y and one that starts in column 0 of row y + 1 (three times): they stay apart,
    across the end of the row and across the pitch padding (pitch != w for 5, 6, 7)"""
    m = np.zeros((7, w), np.uint8)
    m[0, w - 2:] = 255
    m[1, :2] = 255
    m[3, w - 1] = 255
    m[4, 0] = 255
    m[5, w - 1] = 255
    m[6, 0] = 255
    return m


def _random(density, seed):
    return (np.random.default_rng(seed).random((97, 131)) < density).astype(np.uint8) * 255


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, uint8 mask [h, w])]: one ragged batch; "random 0.5 again" repeats the content of "random 0.5" in another descriptor"""
    checker = np.zeros((34, 35), np.uint8)
    checker[::2, ::2] = 255
    checker[1::2, 1::2] = 7
    out = [
        ("empty", np.zeros((9, 13), np.uint8)),
        ("full", np.full((33, 70), 255, np.uint8)),
        ("1x1", np.full((1, 1), 255, np.uint8)),
        ("1x37", np.full((1, 37), 255, np.uint8)),
        ("37x1", np.full((37, 1), 1, np.uint8)),
        ("width 5", _edge_runs(5)),
        ("width 6", _edge_runs(6)),
        ("width 7", _edge_runs(7)),
        ("checkerboard", checker),
        ("spiral", _spiral(150, 200)),
        ("comb", _comb(150, 200)),
        ("stairs", _stairs(70)),
        ("tie", _tie()),
        ("specks", _specks()),
        ("random 0.3", _random(0.3, 3)),
        ("random 0.5", _random(0.5, 5)),
        ("random 0.6", _random(0.6, 6)),
        ("random 0.5 again", _random(0.5, 5)),
    ]
    for _, m in out:
        m.setflags(write=False)
    return out


SPECS = [dict(keep="largest", min_area=0), dict(keep="all", min_area=3), dict(keep="largest", min_area=13), dict(keep="all", min_area=40)]


@functools.lru_cache(maxsize=None)
def expected_labels(connectivity):
    """canonical labels of every case, computed once per connectivity and shared"""
    return [label(m, connectivity) for _, m in cases()]
