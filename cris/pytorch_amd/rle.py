"""COCO run-length encoding (RLE) of binary masks on the host: numpy only, no device.

    r = rle.encode(mask)             {"size": [h, w], "counts": b"..."}        what RefCOCO / COCO tooling exchanges
    m = rle.decode(r)                uint8 [h, w] of 0 / 255
    json.dump(rle.to_json(r), f)

The format is the one of pycocotools' rleEncode / rleToString / rleFrString, restated here (pycocotools is not a dependency):
pixels in COLUMN-major order, i = x * h + y; v(i) the foreground bit, v(-1) = 0; P = the ascending i with v(i) != v(i - 1);
counts = diff([0] + P + [h * w]) - run lengths that alternate background, foreground, ... and start with background (a mask that
starts with foreground has a leading 0 count; all background is [h * w], all foreground [0, h * w]).  A run continues from the
bottom of a column into the top of the next.  The compressed string stores count j as the difference to count j - 2 (for j > 2) in
5-bit groups, least significant first: bit 0x20 of a character announces another group, bit 0x10 of the last group is the sign;
each group is emitted as chr(group + 48).

This module is also the CPU restatement of the device encoder (csrc/rle.hip, evalpost.rle_encode_batch), which delivers the
positions P; `positions_to_counts` and `counts_to_string` finish the job, and `strings_from_positions` does so for a whole batch."""
import numpy as np

MAX_PIXELS = 2 ** 31        # h * w must stay below it (positions are 32-bit words on the device)
_GROUPS = 7                 # 5-bit groups of one value: 35 bits, enough for any difference of two counts below 2^31
_GROUP_LIMITS = np.array([1 << (5 * g - 1) for g in range(1, _GROUPS)], np.int64)      # g groups hold -2^(5g - 1) <= d < 2^(5g - 1)


def _check_size(h, w):
    if isinstance(h, bool) or isinstance(w, bool) or not isinstance(h, (int, np.integer)) or not isinstance(w, (int, np.integer)):
        raise ValueError("rle: size must be two integers, got %r" % ((h, w),))
    h, w = int(h), int(w)
    if h < 0 or w < 0 or h * w >= MAX_PIXELS:
        raise ValueError("rle: size must be non-negative with h * w < 2^31, got %r" % ((h, w),))
    return h, w


def _check_counts(counts, h, w):
    """-> int64 array; before any work: integers, non-negative, summing to h * w"""
    c = np.asarray(counts)
    if c.ndim != 1 or (c.size and c.dtype.kind not in "iu"):
        raise ValueError("rle: counts must be a flat list of integers")
    c = c.astype(np.int64)
    if c.size and int(c.min()) < 0:
        raise ValueError("rle: negative count")
    if int(c.sum()) != h * w:
        raise ValueError("rle: the counts sum to %d, the mask has %d x %d = %d pixels" % (int(c.sum()), h, w, h * w))
    return c


def positions_to_counts(P, h, w):
    """transition positions (ascending, in [0, h * w)) -> counts = diff([0] + P + [h * w]) as int64"""
    h, w = _check_size(h, w)
    P = np.asarray(P).astype(np.int64).reshape(-1)
    if P.size and (int(P[0]) < 0 or int(P[-1]) >= h * w or (np.diff(P) <= 0).any()):
        raise ValueError("rle: positions must ascend strictly inside [0, h * w)")
    return np.diff(np.concatenate([[0], P, [h * w]]).astype(np.int64))


def _delta_chars(d):
    """d: int64 values (count j minus count j - 2) -> (the characters of all values in order as uint8, characters per value).
    The group rule stops once the rest of the value is its sign alone (x == 0 with bit 0x10 clear, x == -1 with it set), that is
    after the fewest g groups with -2^(5g - 1) <= d < 2^(5g - 1); with that length known per value, group k of a value is
    (d >> 5k) & 0x1f and every group but the last carries 0x20: one pass over the characters, no loop over the groups."""
    d = np.asarray(d, dtype=np.int64)
    magnitude = d ^ (d >> 63)                                               # d for d >= 0, -d - 1 below
    if d.size and int(magnitude.max()) >= 1 << (5 * _GROUPS - 1):
        raise ValueError("rle: a count does not fit %d groups" % _GROUPS)
    length = np.searchsorted(_GROUP_LIMITS, magnitude, side="right") + 1
    start = np.cumsum(length) - length
    k = np.arange(int(length.sum())) - np.repeat(start, length)             # group index of every character within its value
    last = np.repeat(length - 1, length)
    c = ((np.repeat(d, length) >> (5 * k)) & 0x1f) | ((k < last).astype(np.int64) << 5)
    return (c + 48).astype(np.uint8), length


def _deltas(counts, local):
    """counts: int64 (several masks concatenated); local: index of every entry within its own mask -> the stored differences"""
    d = counts.copy()
    far = local > 2
    d[far] -= counts[np.nonzero(far)[0] - 2]
    return d


def counts_to_string(counts):
    """counts (non-negative integers) -> the compressed string as bytes"""
    c = np.asarray(counts)
    if c.ndim != 1 or (c.size and c.dtype.kind not in "iu"):
        raise ValueError("rle: counts must be a flat list of integers")
    c = c.astype(np.int64)
    if c.size and (int(c.min()) < 0 or int(c.max()) >= MAX_PIXELS):
        raise ValueError("rle: counts must lie in [0, 2^31)")
    return _delta_chars(_deltas(c, np.arange(c.size)))[0].tobytes()


def string_to_counts(s):
    """the compressed string (bytes or str) -> counts as int64.  A character outside chr(48) .. chr(111), a last group that
    announces a continuation, a value of more than 7 groups or a negative count is a ValueError"""
    if isinstance(s, str):
        try:
            s = s.encode("ascii")
        except UnicodeEncodeError:
            raise ValueError("rle: the counts string is not ASCII") from None
    if not isinstance(s, (bytes, bytearray, memoryview)):
        raise ValueError("rle: compressed counts must be bytes or str, got %r" % (type(s),))
    b = np.frombuffer(bytes(s), np.uint8).astype(np.int64) - 48
    if b.size == 0:
        return np.zeros(0, np.int64)
    if int(b.min()) < 0 or int(b.max()) > 63:
        raise ValueError("rle: character outside the alphabet of the compressed counts")
    last = (b & 0x20) == 0                                                 # the last group of a value
    if not last[-1]:
        raise ValueError("rle: the string ends inside a count (its last group announces a continuation)")
    ends = np.nonzero(last)[0]
    starts = np.concatenate([[0], ends[:-1] + 1])
    length = ends - starts + 1
    if int(length.max()) > _GROUPS:
        raise ValueError("rle: a count of more than %d groups" % _GROUPS)
    k = np.arange(b.size) - np.repeat(starts, length)                      # group index within its value
    d = np.add.reduceat((b & 0x1f) << (5 * k), starts)
    neg = (b[ends] & 0x10) != 0
    d = np.where(neg, d | (np.int64(-1) << (5 * length)), d)
    c = d.copy()                                                            # undo "minus count j - 2" for j > 2: two running sums
    c[1::2] = np.cumsum(d[1::2])
    c[2::2] = np.cumsum(d[2::2])
    if int(c.min()) < 0:
        raise ValueError("rle: negative count")
    return c


def strings_from_positions(positions, totals, sizes):
    """A whole batch at once: positions = the packed transition positions of every mask (mask 0's, then mask 1's, ...; what
    evalpost.rle_encode_batch delivers), totals[i] = how many belong to mask i, sizes[i] = (h, w) -> list of {"size", "counts"}.
    One np.diff-style pass over the packed array with per-mask boundaries, one pass of the string coder."""
    totals = np.asarray(totals, dtype=np.int64).reshape(-1)
    n = totals.size
    if n != len(sizes):
        raise ValueError("rle: %d totals for %d sizes" % (n, len(sizes)))
    sizes = [_check_size(h, w) for h, w in sizes]
    P = np.asarray(positions).astype(np.int64).reshape(-1)
    if int(totals.sum()) != P.size or (n and int(totals.min()) < 0):
        raise ValueError("rle: the totals do not add up to the number of positions")
    pixels = np.array([h * w for h, w in sizes], np.int64)
    first = np.concatenate([[0], np.cumsum(totals + 1)])                    # mask i has totals[i] + 1 counts
    hi = np.empty(int(first[-1]), np.int64)                                 # [P_i ..., h * w] per mask
    at_end = first[1:] - 1
    body = np.ones(hi.size, bool)
    body[at_end] = False
    hi[body] = P
    hi[at_end] = pixels
    lo = np.empty_like(hi)                                                  # [0, P_i ...] per mask
    lo[1:] = hi[:-1]
    lo[first[:-1]] = 0
    counts = hi - lo
    local = np.arange(hi.size) - np.repeat(first[:-1], totals + 1)
    if (P.size and int(P.min()) < 0) or (counts[local > 0] <= 0).any():     # (only a mask's first count may be 0)
        raise ValueError("rle: positions must ascend strictly inside [0, h * w) of their mask")
    chars, length = _delta_chars(_deltas(counts, local))
    cut = np.concatenate([[0], np.cumsum(length)])[first]                   # characters before each mask
    flat = chars.tobytes()
    return [{"size": [h, w], "counts": flat[int(cut[i]):int(cut[i + 1])]} for i, (h, w) in enumerate(sizes)]


def encode(mask):
    """any 2-D array, non-zero is foreground -> {"size": [h, w], "counts": bytes}"""
    m = np.asarray(mask)
    if m.ndim != 2:
        raise ValueError("rle.encode: the mask must be 2-D, got shape %r" % (m.shape,))
    h, w = _check_size(*m.shape)
    v = (m != 0).T.reshape(-1)                                              # column-major: i = x * h + y
    P = np.nonzero(v != np.concatenate([[False], v[:-1]]))[0]
    return {"size": [h, w], "counts": counts_to_string(positions_to_counts(P, h, w))}


def _parts(rle):
    """-> (h, w, counts int64), validated"""
    try:
        (h, w), counts = rle["size"], rle["counts"]
    except (KeyError, TypeError, ValueError):
        raise ValueError("rle: expected {'size': [h, w], 'counts': ...}, got %r" % (type(rle),)) from None
    h, w = _check_size(h, w)
    if isinstance(counts, (bytes, bytearray, memoryview, str)):
        counts = string_to_counts(counts)
    return h, w, _check_counts(counts, h, w)


def decode(rle):
    """{"size", "counts"} with compressed bytes / str counts or an uncompressed list of integers -> uint8 [h, w] of 0 / 255"""
    h, w, c = _parts(rle)
    v = np.repeat((np.arange(c.size) & 1).astype(np.uint8) * 255, c)
    return np.ascontiguousarray(v.reshape(w, h).T)


def area(rle):
    """foreground pixels: the sum of the odd counts"""
    return int(_parts(rle)[2][1::2].sum())


def to_bbox(rle):
    """(x0, y0, x1, y1) half-open, the form of predict.Prediction.box, or None for an empty mask - from the runs, nothing is decoded"""
    h, _, c = _parts(rle)
    start = (np.cumsum(c) - c)[1::2]
    length = c[1::2]
    start, length = start[length > 0], length[length > 0]
    if start.size == 0:
        return None
    end = start + length - 1
    xs, xe = start // h, end // h
    if (xe > xs).any():                                                     # a run that crosses a column touches its bottom and the next top
        y0, y1 = 0, h
    else:
        y0, y1 = int((start % h).min()), int((end % h).max()) + 1
    return (int(xs.min()), y0, int(xe.max()) + 1, y1)


def to_json(rle):
    """the same RLE with `str` counts: goes straight into json.dump"""
    h, w, _ = _parts(rle)
    counts = rle["counts"]
    if isinstance(counts, (bytes, bytearray, memoryview)):
        counts = bytes(counts).decode("ascii")
    elif not isinstance(counts, str):
        counts = counts_to_string(counts).decode("ascii")
    return {"size": [h, w], "counts": counts}
