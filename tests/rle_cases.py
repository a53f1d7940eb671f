"""Cases and an independent oracle for the COCO run-length encoder (cris/pytorch_amd/rle.py on the host, csrc/rle.hip behind
evalpost.rle_encode_batch on the device).  The oracle is the plain per-pixel loop of pycocotools' rleEncode over the column-major
flattening and a per-character loop of rleToString, written apart from rle.py's vectorised code so that the two check each other.
The cases are the smallest shapes at which the kernels can take another path: RB rows per band, CG columns per block."""
import functools

import numpy as np

RB, CG = 32, 64             # evalpost.RLE_RB / RLE_CG (csrc/rle.hip); tests/test_rle_cpu.py compares them

# the fixtures of the format: (counts, compressed string)
STRINGS = [([0, 5, 3], b"053"), ([2, 3, 40, 1], b"23X1N"), ([16], b"`0"), ([307200], b"PP\\9"), ([0, 307200], b"0PP\\9"),
           ([6, 1, 40, 4, 5, 4, 5, 4, 21], b"61X13mN000`0"), ([1] * 12, b"111000000000")]
MASK_FIXTURE = (np.array([[0, 1, 1], [0, 1, 0], [1, 1, 0]], np.uint8), [2, 7], [2, 5, 2], b"252")


def pitch_of(w):
    return (w + 3) // 4 * 4


def oracle_counts(mask):
    """rleEncode: walk the pixels in column-major order, close a run whenever the value changes; the first run is background"""
    flat = (np.asarray(mask) != 0).flatten(order="F").tolist()
    counts, run, prev = [], 0, False
    for v in flat:
        if v != prev:
            counts.append(run)
            run, prev = 0, v
        run += 1
    counts.append(run)
    return counts


def oracle_positions(mask):
    """the indices at which a run starts, but for the leading background run: the transition positions"""
    out, at = [], 0
    for c in oracle_counts(mask)[:-1]:
        at += c
        out.append(at)
    return out


def oracle_string(counts):
    """rleToString, one value and one character at a time"""
    out = bytearray()
    for j, k in enumerate(counts):
        x = int(k)
        if j > 2:
            x -= int(counts[j - 2])
        more = True
        while more:
            c = x & 0x1f
            x >>= 5
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            out.append(c + 48)
    return bytes(out)


def _blob(h=480, w=640):
    yy, xx = np.mgrid[0:h, 0:w]
    m = ((xx - 300) / 170.0) ** 2 + ((yy - 250) / 120.0) ** 2 < 1.0
    m &= ~(((xx - 330) / 40.0) ** 2 + ((yy - 230) / 30.0) ** 2 < 1.0)      # a hole
    m |= (np.abs(xx - 60) < 9) & (yy > 400)                                 # a bar that reaches the last row
    m |= np.random.default_rng(5).random((h, w)) < 0.0005                   # specks
    return m.astype(np.uint8) * 255


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, uint8 mask)] - one ragged batch"""
    rng = np.random.default_rng(7)
    rand = lambda h, w, p: (rng.random((h, w)) < p).astype(np.uint8) * 255                       # noqa: E731
    out = [("1x1 background", np.zeros((1, 1), np.uint8)), ("1x1 foreground", np.full((1, 1), 255, np.uint8)),
           ("1x7", np.array([[0, 255, 255, 0, 0, 255, 0]], np.uint8)), ("7x1", np.array([[255, 0, 0, 255, 255, 0, 255]], np.uint8).T)]
    for w in (3, 4, 5):                                                     # pitch padding of 1, 0 and 3 bytes
        out.append(("width %d" % w, rand(9, w, 0.5)))
    for h in (RB - 1, RB, RB + 1, 2 * RB + 3):                              # band edges
        out.append(("height %d" % h, rand(h, 6, 0.4)))
    for w in (CG - 1, CG, CG + 1):                                          # column-group edges, two bands
        out.append(("width %d" % w, rand(RB + 2, w, 0.3)))
    out.append(("all background", np.zeros((RB + 5, 10), np.uint8)))
    out.append(("all foreground", np.full((RB + 5, 10), 255, np.uint8)))
    yy, xx = np.mgrid[0:37, 0:70]
    out.append(("checkerboard", (((yy + xx + 1) & 1) * 255).astype(np.uint8)))     # h odd, (0, 0) foreground: every pixel a transition
    first = np.zeros((5, 4), np.uint8)
    first[0, 0] = first[1, 0] = 255
    out.append(("first pixel foreground", first))
    joins = np.zeros((RB + 1, 3), np.uint8)
    joins[-2:, 0] = 255                                                     # column 0 ends in foreground ...
    joins[:3, 1] = 255                                                      # ... and column 1 starts in it: one run, no transition at (1, 0)
    joins[-1, 1] = 255                                                      # column 1 ends in foreground, column 2 starts in background
    out.append(("column joins and breaks", joins))
    out.append(("bytes 1 and 128", np.where(rng.random((12, 13)) < 0.5, np.where(rng.random((12, 13)) < 0.5, 1, 128), 0).astype(np.uint8)))
    dense = rand(45, 77, 0.5)
    out.append(("random 0.5", dense))
    out.append(("random 0.02", rand(150, 131, 0.02)))
    out.append(("random 0.5 again", dense.copy()))                          # equal content at another out_off
    out.append(("blob 480x640", _blob()))
    return out


ALIAS = "random 0.02"       # the packed batch ends with one more descriptor that names this case's rectangle


@functools.lru_cache(maxsize=None)
def expected():
    """per case (positions, counts, string) from the oracle, computed once"""
    out = []
    for _, m in cases():
        counts = oracle_counts(m)
        out.append((oracle_positions(m), counts, oracle_string(counts)))
    return out
