"""Cases, references and emulation of the edge audit of the evaluation kernels (csrc/evalpost.hip: sigmoid_bicubic_kernel,
warp_affine_cubic_kernel, eval_iou_batch_kernel, predict_masks_batch_kernel, eval_iou_sweep_batch_kernel and the statistics of
cc_filter_kernel).  tests/test_eval_post_edges_cpu.py settles them without a GPU, tests/test_eval_post_edges.py runs them on one.
Nothing here needs a GPU or the library.

WHAT THE CASES ARE FOR.  Every other evaluation test has square probability maps, border 0 and letter-box matrices.  Here:

    maps         (H, W) = (40, 72) and (72, 40), P = 3 each, built on the host in float32: [0] the oracle's bicubic upsample of
                 sigmoid(randn * 3) from (H / 4, W / 4) logits, [1] a rectangle of 0.9 on 0.05, off-centre, [2] the ties map.
                 They are uploaded as they are: the warp tests do not depend on the upsample kernel.
    descriptors  14 per map shape (`descriptors`): four letter-box inverses to the non-square map, identity, an integer shift, the
                 suite's rotation with shear, a mirror, a transpose, an anisotropic shrink, two singular matrices (the launcher maps
                 them to the zero map: every pixel samples source (0, 0)), an output entirely outside the source at coordinates
                 around -5000 / +7000, and one half outside with negative coordinates (arithmetic shifts and & 31 of negative longs).
    borders      0, 0.5 (above the threshold 0.35: everything outside the source is foreground) and -0.25.
    ties map     every threshold t of every sweep list (`SWEEPS`) as t, nextafter(t, +1) and nextafter(t, -1), and the values
                 (2 k + 1) / 131072 above 0.35, whose product with 65536 is exactly k + 0.5 (rintf must round half to even).
                 Sub-pixel entry 0 of the cubic table is exactly (0, 1, 0, 0): identity and integer shifts copy the values bit for
                 bit, so the comparisons `value > thr` meet exact ties.  `TIE_BORDER` = float32(0.35) is the border of one more
                 shift launch: border pixels equal the threshold and must not count.
    upsample     `UP_SHAPES` (h != w, H = 1, W = 1, h = 1, w = 1, downsampling, the identity size) at logit scales 3 and 30 with
                 B = 3 (B H W is no multiple of 256), one case with +-inf and +-104 logits, one with a single NaN.

REFERENCES.  The warp, the counts, the mask bytes and the statistics are integers or bit-exact floats of oracle/eval_post.py
(`oracle_warp` caches them; the arrays are read-only).  The upsample kernel is compared with `upsample_ref64`: the SAME float32
source coordinates and tap indices torch computes (a float64 coordinate would be another function), the sigmoid, the weight
polynomials and the 16-term sum in float64.

THE UPSAMPLE BOUND.  r0 = max |oracle.eval_post.upsample_bicubic (float32) - upsample_ref64| over every finite output of every
upsample case (`upsample_r0`): the error of a float32 restatement that is NOT the kernel.  Measured: r0 = 1.49e-06 (absolute;
the values lie in about [-0.36, 1.41]).  The GPU test allows 4 r0 = 5.97e-06, recomputed and never typed in: the device expf is
one to two ulps of a value <= 1 off numpy's, and the float32 operations of the weight polynomials may legally be ordered or
contracted differently, an ulp or two per weight over 16 taps - together about one more r0; the rest is reserve.  Every error
switch of the upsample emulation exceeds the bound by at least 10 x in its named case (asserted in the CPU companion).

EMULATION.  `emu_warp`, `emu_counts`, `emu_mask_bytes`, `emu_predict_row`, `emu_sweep_counts` and `emu_upsample` restate the
kernels in numpy, flat addresses included, with one switch per plausible mistake (`WARP_SWITCHES`, `UP_SWITCHES`).  Without a
switch they equal the oracle bit for bit; with any one switch a count, a mask byte, a statistics entry or an upsampled value
changes in the case `SWITCH_CASES` names.  An address a wrong kernel would form outside the buffer wraps around in the emulation."""
import functools
from collections import namedtuple

import numpy as np

from oracle import eval_post as EP

F32 = np.float32
THR = F32(0.35)
MAP_SHAPES = ((40, 72), (72, 40))
P, TIES_MAP = 3, 2
BORDERS = (0.0, 0.5, -0.25)
TIE_BORDER = float(THR)
PREDICT_INIT = [0, 0, 2 ** 31 - 1, 2 ** 31 - 1, 0, 0]
ROT = np.array([[0.9, -0.3, 20.5], [0.25, 1.1, -7.25]], np.float64)      # the rotation + shear of tests/test_predict_gpu.py

# the threshold lists of the sweep: T = 1, 2, 3, the 23 of tests/test_eval_sweep_gpu.py (THRS) and the launcher's limit, 64
SUITE_THRS = np.array([-0.5, 0.0] + [i / 20 for i in range(1, 20)] + [1.0, 1.5], F32)
SWEEPS = {1: np.array([0.35], F32), 2: np.array([0.2, 0.35], F32), 3: np.array([0.2, 0.35, 0.5], F32), 23: SUITE_THRS,
          64: np.linspace(-0.1, 1.1, 64).astype(F32)}
HALF_K = np.arange(30000, 30032)                                         # (2 k + 1) / 131072 = 0.4578 ..: odd and even k alternate


def all_thresholds():
    return np.unique(np.concatenate([THR[None]] + [SWEEPS[T] for T in sorted(SWEEPS)]).astype(F32))


def half_values():
    v = ((2 * HALF_K + 1).astype(np.float64) / 131072.0).astype(F32)
    assert np.array_equal(v.astype(np.float64) * 65536.0, HALF_K + 0.5) and (v > THR).all()
    return v


def tie_values():
    t = all_thresholds()
    return np.concatenate([t, np.nextafter(t, F32(np.inf)), np.nextafter(t, F32(-np.inf)), half_values()]).astype(F32)


def _frozen(a):
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=None)
def maps(H, W):
    """float32 [P, H, W], read-only"""
    rng = np.random.default_rng(100 + H)
    m0 = EP.upsample_bicubic(EP.sigmoid(rng.standard_normal((H // 4, W // 4)).astype(F32) * 3), H, W)
    m1 = np.full((H, W), 0.05, F32)
    m1[H // 8:H // 8 + H // 2, W // 3:W // 3 + W // 2] = 0.9
    m2 = np.resize(tie_values(), H * W).reshape(H, W)
    return _frozen(np.stack([m0, m1, m2]).astype(F32))


Desc = namedtuple("Desc", "name mat h_out w_out")


def letterbox_inverse(oh, ow, S_h, S_w):
    """the matrix the dataset hands to cv2.warpAffine (network input -> original) for an oh x ow original letter-boxed into an
    S_h x S_w input: one scale, the image centred"""
    scale = min(S_h / oh, S_w / ow)
    bx, by = (S_w - ow * scale) / 2.0, (S_h - oh * scale) / 2.0
    return np.array([[1 / scale, 0, -bx / scale], [0, 1 / scale, -by / scale]], np.float64)


@functools.lru_cache(maxsize=None)
def descriptors(H, W):
    def lb(oh, ow):
        return Desc("letterbox %dx%d" % (oh, ow), letterbox_inverse(oh, ow, H, W), oh, ow)

    def d(name, rows, h, w):
        return Desc(name, np.array(rows, np.float64), h, w)

    return (lb(50, 37), lb(30, 90), lb(1, 1), lb(5, 3),
            d("identity", [[1, 0, 0], [0, 1, 0]], H, W),
            d("shift", [[1, 0, 7], [0, 1, -5]], H + 6, W + 9),
            d("rotation", ROT, 43, 61),
            d("mirror", [[-1, 0, W - 1], [0, 1, 0]], H, W),
            d("transpose", [[0, 1, 0], [1, 0, 0]], W, H),
            d("shrink", [[1 / 3, 0, 0.3], [0, 0.4, -0.2]], 17, 29),
            d("singular zero", np.zeros((2, 3)), 7, 13),
            d("singular rank 1", [[1, 2, 3], [2, 4, 1]], 7, 13),
            d("far away", [[1, 0, 5000], [0, 1, -7000]], 10, 21),
            d("half outside", [[1.3, 0.2, 30.4], [-0.1, 0.8, 25.6]], 50, 70))


NAMES = tuple(d.name for d in descriptors(*MAP_SHAPES[0]))
SINGULAR = ("singular zero", "singular rank 1")
# at thr 0.35 against map 0: a foreground count strictly between 0 and all pixels at border 0 and -0.25, another count at 0.5
NONTRIVIAL = ("shift", "rotation", "half outside")
BORDER_SEPARATES = NONTRIVIAL + ("far away",)


def desc_index(name):
    return NAMES.index(name)


@functools.lru_cache(maxsize=None)
def oracle_warp(H, W, k, mp, border):
    """oracle.eval_post.warp_affine_cubic of map `mp` under descriptor k of `descriptors(H, W)`; read-only, computed once"""
    d = descriptors(H, W)[k]
    return _frozen(EP.warp_affine_cubic(maps(H, W)[mp], d.mat, d.w_out, d.h_out, border))


Entry = namedtuple("Entry", "name k mat mask map row")


@functools.lru_cache(maxsize=None)
def batch_layout(H, W):
    """one launch per map shape: every descriptor against map 0 and against a second map (identity and shift: the ties map; the
    others alternate between 1 and 2) - 28 descriptors over 3 maps.  One mask per distinct output size, so the descriptors of a
    size share it; the count / statistics rows are a permutation of the descriptor order.  -> (masks, entries)"""
    descs = descriptors(H, W)
    sizes, masks, pairs = [], [], []
    for k, d in enumerate(descs):
        if (d.h_out, d.w_out) not in sizes:
            sizes.append((d.h_out, d.w_out))
            m = (np.random.default_rng(200 + len(sizes)).random((d.h_out, d.w_out)) > 0.5).astype(np.uint8) * 255
            m[0, 0] = 1                                                    # any non-zero byte counts
            masks.append(_frozen(m))
        second = TIES_MAP if d.name in ("identity", "shift") else 1 + k % 2
        pairs += [(k, 0), (k, second)]
    n = len(pairs)
    entries = tuple(Entry(descs[k].name, k, descs[k].mat, sizes.index((descs[k].h_out, descs[k].w_out)), mp, (5 * j + 3) % n)
                    for j, (k, mp) in enumerate(pairs))
    assert sorted(e.row for e in entries) == list(range(n)) and len(masks) < len(descs)
    return tuple(masks), entries


def pitch_of(w):
    return (int(w) + 3) // 4 * 4


# ---- what the oracle expects of the batch kernels, from a warped map ----
def oracle_mask_bytes(v, thr):
    """[h, pitch] uint8: 255 where v > thr, zero padding bytes"""
    out = np.zeros((v.shape[0], pitch_of(v.shape[1])), np.uint8)
    out[:, :v.shape[1]] = (v > F32(thr)).astype(np.uint8) * 255
    return out


def q16_of(v):
    """rint(v * 65536) per pixel: np.rint (half to even) of the float32 product, which is exact (a power of two)"""
    return np.rint(v.astype(F32) * F32(65536)).astype(np.int64)


def oracle_predict_row(v, thr):
    fg = v > F32(thr)
    if not fg.any():
        return list(PREDICT_INIT)
    ys, xs = np.nonzero(fg)
    return [int(fg.sum()), int(q16_of(v)[fg].sum()), int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1]


def oracle_counts(v, mask, thr):
    _, inter, union = EP.iou(v, mask, F32(thr))
    return [inter, union]


# ---- emulation of the warp kernels, with switchable errors ----
WARP_SWITCHES = ("inside_swap", "stride_swap", "clamp_swap", "map_offset_ww", "border_ignored", "border_clamp", "fxfy_swap", "ge",
                 "bsearch_tie", "round_half_up")
UP_SWITCHES = ("scale_swap", "index_swap", "y_clamp_w", "x_clamp_h", "stride_h")


def emu_invert(mat):
    """ep_warp_setup's matrix part: cv::invertAffineTransform in double, a singular matrix gives the zero map"""
    a = np.asarray(mat, np.float64).reshape(6)
    D = a[0] * a[4] - a[1] * a[3]
    D = 1.0 / D if D != 0.0 else 0.0
    A11, A22, A12, A21 = a[4] * D, a[0] * D, -a[1] * D, -a[3] * D
    return np.array([A11, A12, -A11 * a[2] - A12 * a[5], A21, A22, -A21 * a[2] - A22 * a[5]], np.float64)


def emu_table():
    """ep_warp_setup's table part, one float32 operation per line of the host code"""
    A = F32(-0.75)
    tab = np.zeros((32, 4), F32)
    for i in range(32):
        t = F32(i) / F32(32)
        u = t + F32(1)
        q = A * u; q = q - F32(5) * A; q = q * u; q = q + F32(8) * A; q = q * u; c0 = q - F32(4) * A
        q = (A + F32(2)) * t; q = q - (A + F32(3)); q = q * t; q = q * t; c1 = q + F32(1)
        u = F32(1) - t
        q = (A + F32(2)) * u; q = q - (A + F32(3)); q = q * u; q = q * u; c2 = q + F32(1)
        q = F32(1) - c0; q = q - c1; q = q - c2
        tab[i] = (c0, c1, c2, q)
    return tab


def emu_warp(probs, mp, mat, w_out, h_out, border, err=()):
    """ep_warp_value / warp_affine_cubic_kernel for every pixel of one descriptor: probs float32 [P, H, W] (the whole buffer: the
    kernel forms the address probs + map * H * W + yy * W + xx), mat the matrix the caller passes -> float32 [h_out, w_out]"""
    n_maps, H, W = probs.shape
    flat = np.ascontiguousarray(probs, F32).reshape(-1)
    m, tab = emu_invert(mat), emu_table()
    idx = np.arange(w_out * h_out, dtype=np.int64)
    x, y = (idx % w_out).astype(np.float64), (idx // w_out).astype(np.float64)
    AB = float(1 << 10)
    rnd = lambda v: np.rint(v).astype(np.int64)
    adelta, bdelta = rnd(m[0] * x * AB), rnd(m[3] * x * AB)
    X0, Y0 = rnd((m[1] * y + m[2]) * AB) + 16, rnd((m[4] * y + m[5]) * AB) + 16
    Xq, Yq = (X0 + adelta) >> 5, (Y0 + bdelta) >> 5
    sx, sy, fx, fy = (Xq >> 5) - 1, (Yq >> 5) - 1, Xq & 31, Yq & 31
    if "fxfy_swap" in err:
        fx, fy = fy, fx
    Hi, Wi = (W, H) if "inside_swap" in err else (H, W)
    Hc, Wc = (W, H) if "clamp_swap" in err else (H, W)
    stride = H if "stride_swap" in err else W
    base = mp * (W * W if "map_offset_ww" in err else H * W)
    b = F32(0.0 if "border_ignored" in err else border)
    acc = np.zeros(idx.shape, F32)
    for ky in range(4):
        yy = sy + ky
        for kx in range(4):
            xx = sx + kx
            inside = (yy >= 0) & (yy < Hi) & (xx >= 0) & (xx < Wi)
            val = flat.take(base + np.clip(yy, 0, Hc - 1) * stride + np.clip(xx, 0, Wc - 1), mode="wrap")
            v = val if "border_clamp" in err else np.where(inside, val, b).astype(F32)
            wgt = (tab[fy, ky] * tab[fx, kx]).astype(F32)
            acc = (acc + (v * wgt).astype(F32)).astype(F32)
    return acc.reshape(h_out, w_out)


def _above(v, t, err):
    return v >= F32(t) if "ge" in err else v > F32(t)


def emu_counts(v, mask, thr, err=()):
    p, m = _above(v, thr, err), np.asarray(mask) != 0
    return [int((p & m).sum()), int((p | m).sum())]


def emu_mask_bytes(v, thr, err=()):
    out = np.zeros((v.shape[0], pitch_of(v.shape[1])), np.uint8)
    out[:, :v.shape[1]] = _above(v, thr, err).astype(np.uint8) * 255
    return out


def emu_predict_row(v, thr, err=()):
    fg = _above(v, thr, err)
    if not fg.any():
        return list(PREDICT_INIT)
    prod = (v.astype(F32) * F32(65536)).astype(F32)
    q = np.floor(prod.astype(np.float64) + 0.5).astype(np.int64) if "round_half_up" in err else np.rint(prod).astype(np.int64)
    ys, xs = np.nonzero(fg)
    return [int(fg.sum()), int(q[fg].sum()), int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1]


def emu_sweep_counts(v, mask, thrs, err=()):
    """eval_iou_sweep_batch_kernel after the warp: k per pixel by the bracket test and the binary search, the histogram over
    (mask bit, k) without its k = 0 bins, suffix sums -> int [T, 2]"""
    thrs = np.asarray(thrs, F32)
    T = thrs.shape[0]
    val, m = v.reshape(-1), (np.asarray(mask) != 0).reshape(-1).astype(np.int64)
    above_lo, above_hi = _above(val, thrs[0], err), _above(val, thrs[T - 1], err)
    lo, hi = np.full(val.shape, 1, np.int64), np.full(val.shape, T - 1, np.int64)
    while (lo < hi).any():
        act = lo < hi
        mid = (lo + hi) >> 1
        t = thrs[np.clip(mid, 0, T - 1)]
        up = (val >= t) if ("ge" in err or "bsearch_tie" in err) else (val > t)
        lo = np.where(act & up, mid + 1, lo)
        hi = np.where(act & ~up, mid, hi)
    k = np.where(~above_lo, 0, np.where(above_hi, T, lo))
    hist = np.zeros((2, T + 1), np.int64)
    np.add.at(hist, (m, k), 1)
    gt = int(m.sum())
    hist[:, 0] = 0
    out = np.zeros((T, 2), np.int64)
    for i in range(T):
        inter, pred = int(hist[1, i + 1:].sum()), int(hist[:, i + 1:].sum())
        out[i] = (inter, pred + gt - inter)
    return out


def oracle_sweep_counts(v, mask, thrs):
    return np.array([oracle_counts(v, mask, t) for t in thrs], np.int64)


# ---- the upsample: cases, float64 reference, emulation ----
UP_SHAPES = ((5, 9, 20, 37), (9, 5, 37, 20), (13, 17, 52, 67), (1, 1, 3, 5), (1, 6, 1, 24), (6, 1, 24, 1), (2, 3, 31, 2), (9, 11, 4, 5),
             (4, 7, 4, 7))
UP_B = 3
UP_NAN_AT = (1, 2, 4)                                                    # (b, y, x) of the NaN logit of the 5x9 -> 20x37 case
UP_NAN_FOOTPRINT = 342                                                   # of the 740 outputs of that map
UpCase = namedtuple("UpCase", "name logits H W")


@functools.lru_cache(maxsize=None)
def upsample_cases():
    out = []
    for i, (h, w, H, W) in enumerate(UP_SHAPES):
        for scale in (3, 30):
            x = np.random.default_rng(300 + 2 * i + (scale == 30)).standard_normal((UP_B, h, w)).astype(F32) * F32(scale)
            out.append(UpCase("%dx%d->%dx%d x%d" % (h, w, H, W, scale), _frozen(x), H, W))
    h, w, H, W = UP_SHAPES[0]
    x = np.random.default_rng(340).standard_normal((UP_B, h, w)).astype(F32) * F32(3)
    x[0, 0, 0], x[0, 4, 8], x[0, 2, 3], x[1, 1, 5], x[1, 3, 0], x[2, 4, 4], x[2, 0, 8] = np.inf, -np.inf, 104, -104, np.inf, -np.inf, -104
    x[2, 2, 2] = 104
    out.append(UpCase("special values", _frozen(x), H, W))
    x = np.random.default_rng(341).standard_normal((UP_B, h, w)).astype(F32) * F32(3)
    x[UP_NAN_AT] = np.nan
    out.append(UpCase("one NaN", _frozen(x), H, W))
    assert len({c.name for c in out}) == len(out) and all((UP_B * c.H * c.W) % 256 for c in out)
    return tuple(out)


def up_case(name):
    return next(c for c in upsample_cases() if c.name == name)


def _axis32(n_in, n_out):
    """torch's align_corners source coordinate in float32 -> (tap indices [n_out, 4] clamped to the image, fraction t float32)"""
    scale = F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(0)
    src = np.arange(n_out, dtype=F32) * scale
    i0 = np.floor(src).astype(np.int64)
    t = (src - i0.astype(F32)).astype(F32)
    return np.clip(i0[:, None] + np.arange(-1, 3)[None, :], 0, n_in - 1), t


def _cubic(t):
    """torch's weights of taps -1, 0, +1, +2 (A = -0.75) in the precision of t"""
    A = -0.75
    x0, x1, x2, x3 = t + 1.0, t, 1.0 - t, 2.0 - t
    return np.stack([((A * x0 - 5.0 * A) * x0 + 8.0 * A) * x0 - 4.0 * A, ((A + 2.0) * x1 - (A + 3.0)) * x1 * x1 + 1.0,
                     ((A + 2.0) * x2 - (A + 3.0)) * x2 * x2 + 1.0, ((A * x3 - 5.0 * A) * x3 + 8.0 * A) * x3 - 4.0 * A], -1)


def sigmoid64(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def upsample_ref64(logits, H, W):
    """float64 [B, H, W]: float32 coordinates and tap indices, everything after them in float64"""
    B, h, w = logits.shape
    iy, ty = _axis32(h, H)
    ix, tx = _axis32(w, W)
    cy, cx = _cubic(ty.astype(np.float64)), _cubic(tx.astype(np.float64))
    s = sigmoid64(logits)
    taps = s[:, iy][:, :, :, ix]                                         # [B, H, 4, W, 4]
    return np.einsum("bhiwj,hi,wj->bhw", taps, cy, cx)


def oracle_upsample(logits, H, W):
    """oracle.eval_post.upsample_bicubic(sigmoid(.)) per map -> float32 [B, H, W]"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.stack([EP.upsample_bicubic(EP.sigmoid(x), H, W) for x in logits])


def emu_upsample(logits, H, W, err=()):
    """sigmoid_bicubic_kernel, flat index and flat source address included -> float32 [B, H, W]"""
    B, h, w = logits.shape
    sy = F32(h - 1) / F32(H - 1) if H > 1 else F32(0)
    sx = F32(w - 1) / F32(W - 1) if W > 1 else F32(0)
    if "scale_swap" in err:
        sy, sx = sx, sy
    idx = np.arange(B * H * W, dtype=np.int64)
    if "index_swap" in err:
        X, Y = idx % H, (idx // H) % W
    else:
        X, Y = idx % W, (idx // W) % H
    b = idx // (W * H)
    fy, fx = Y.astype(F32) * sy, X.astype(F32) * sx
    iy, ix = np.floor(fy).astype(np.int64), np.floor(fx).astype(np.int64)
    cy, cx = _cubic((fy - iy.astype(F32)).astype(F32)).astype(F32), _cubic((fx - ix.astype(F32)).astype(F32)).astype(F32)
    with np.errstate(over="ignore", invalid="ignore"):
        sig = np.stack([EP.sigmoid(x) for x in logits]).astype(F32).reshape(-1)
        stride = h if "stride_h" in err else w
        acc = None
        for i in range(4):
            yy = np.clip(iy - 1 + i, 0, (w if "y_clamp_w" in err else h) - 1)
            r = None
            for j in range(4):
                xx = np.clip(ix - 1 + j, 0, (h if "x_clamp_h" in err else w) - 1)
                t = (sig.take(b * h * w + yy * stride + xx, mode="wrap") * cx[:, j]).astype(F32)
                r = t if r is None else (r + t).astype(F32)
            t = (r * cy[:, i]).astype(F32)
            acc = t if acc is None else (acc + t).astype(F32)
    return acc.reshape(B, H, W)


@functools.lru_cache(maxsize=None)
def upsample_r0():
    """max |float32 restatement - float64 reference| over the finite outputs of every upsample case"""
    r0 = 0.0
    for c in upsample_cases():
        with np.errstate(invalid="ignore"):
            d = np.abs(oracle_upsample(c.logits, c.H, c.W).astype(np.float64) - upsample_ref64(c.logits, c.H, c.W))
        r0 = max(r0, float(d[np.isfinite(d)].max()))
    return r0


def upsample_bound():
    return 4.0 * upsample_r0()


def upsample_ratio(got, ref64):
    """worst |got - ref64| / bound over the outputs where the reference is finite"""
    ok = np.isfinite(ref64)
    with np.errstate(invalid="ignore"):
        d = np.abs(np.asarray(got, np.float64) - ref64)[ok]
    return float(np.where(np.isnan(d), np.inf, d).max()) / upsample_bound() if d.size else 0.0


# ---- the case every error switch is caught in ----
# warp switches: (map shape, descriptor, map, border, what changes: "counts" at THR against the layout's mask of that size, the mask
# "bytes" at THR, the predict "row" at THR, or the "sweep" table at T = 23); upsample switches: the upsample case.
SWITCH_CASES = {
    "inside_swap": ((40, 72), "identity", 0, 0.0, "counts"),
    "stride_swap": ((40, 72), "identity", 0, 0.0, "bytes"),
    "clamp_swap": ((72, 40), "identity", 0, 0.0, "bytes"),
    "map_offset_ww": ((40, 72), "identity", 1, 0.0, "bytes"),
    "border_ignored": ((40, 72), "far away", 0, 0.5, "row"),
    "border_clamp": ((72, 40), "far away", 1, 0.5, "counts"),
    "fxfy_swap": ((40, 72), "shrink", 0, 0.0, "bytes"),
    "ge": ((40, 72), "identity", TIES_MAP, 0.0, "bytes"),
    "bsearch_tie": ((40, 72), "shift", TIES_MAP, 0.0, "sweep"),
    "round_half_up": ((72, 40), "identity", TIES_MAP, 0.0, "row"),
    "scale_swap": "5x9->20x37 x3",
    "index_swap": "9x5->37x20 x3",
    "y_clamp_w": "9x5->37x20 x30",
    "x_clamp_h": "5x9->20x37 x30",
    "stride_h": "13x17->52x67 x3",
}


def warp_outputs(shape, name, mp, border, err=()):
    """everything the batch kernels derive from one descriptor, by the emulation: {"value", "counts", "bytes", "row", "sweep"}"""
    H, W = shape
    k = desc_index(name)
    d = descriptors(H, W)[k]
    masks, entries = batch_layout(H, W)
    mask = masks[next(e.mask for e in entries if e.k == k)]
    v = emu_warp(maps(H, W), mp, d.mat, d.w_out, d.h_out, border, err)
    return {"value": v, "counts": emu_counts(v, mask, THR, err), "bytes": emu_mask_bytes(v, THR, err), "row": emu_predict_row(v, THR, err),
            "sweep": emu_sweep_counts(v, mask, SWEEPS[23], err)}


def self_check():
    """the properties the cases were chosen for, on the oracle"""
    tv = tie_values()
    assert len(np.unique(tv)) == len(tv) and len(tv) < 40 * 72 // 4
    assert np.array_equal(EP.cubic_table()[0], np.array([0, 1, 0, 0], F32))
    for T, thrs in SWEEPS.items():
        assert len(thrs) == T and (np.diff(thrs) > 0).all() and thrs.dtype == F32
    for H, W in MAP_SHAPES:
        assert H != W and H % 4 == 0 and W % 4 == 0
        mm, descs = maps(H, W), descriptors(H, W)
        assert mm.shape == (P, H, W) and mm.dtype == F32 and np.isfinite(mm).all()
        assert np.unique(mm[1]).tolist() == [float(F32(0.05)), float(F32(0.9))]
        ys, xs = np.nonzero(mm[1] > 0.5)
        assert (ys.min() + ys.max() + 1) != H and (xs.min() + xs.max() + 1) != W          # the rectangle is off-centre
        for k, d in enumerate(descs):
            assert d.h_out <= 90 and d.w_out <= 90
            counts = {}
            for b in BORDERS:
                v = oracle_warp(H, W, k, 0, b)
                assert v.shape == (d.h_out, d.w_out) and np.isfinite(v).all(), (d.name, b)
                counts[b] = int((v > THR).sum())
            if d.name in NONTRIVIAL:
                assert 0 < counts[0.0] < d.h_out * d.w_out and 0 < counts[-0.25] < d.h_out * d.w_out, (d.name, counts)
            if d.name in BORDER_SEPARATES:
                assert counts[0.5] > counts[0.0] >= counts[-0.25], (d.name, counts)
            if d.name == "far away":
                assert [counts[b] for b in BORDERS] == [0, 210, 0]
            if d.name in SINGULAR:
                assert not emu_invert(d.mat).any()
                for mp in range(P):
                    for b in BORDERS:
                        assert (oracle_warp(H, W, k, mp, b) == mm[mp, 0, 0]).all(), (d.name, mp, b)
        # source coordinates: large and negative ones occur, all below 2^20 pixels
        sx, sy, _, _ = EP.warp_coords(descs[desc_index("far away")].mat, 21, 10)
        assert sx.min() <= -5000 and sy.max() >= 7000 and max(np.abs(sx).max(), np.abs(sy).max()) < 2 ** 20
        sx, sy, _, _ = EP.warp_coords(descs[desc_index("half outside")].mat, 70, 50)
        assert min(sx.min(), sy.min()) <= -30
        # identity and integer shift copy bit for bit: every tie value reaches the output of both
        ident, shift = desc_index("identity"), desc_index("shift")
        assert np.array_equal(oracle_warp(H, W, ident, TIES_MAP, 0.0), mm[TIES_MAP])
        for b in BORDERS + (TIE_BORDER,):
            s = oracle_warp(H, W, shift, TIES_MAP, b)
            assert np.array_equal(s[0:H - 5, 7:W + 7], mm[TIES_MAP, 5:H, 0:W])
            outside = np.ones(s.shape, bool)
            outside[0:H - 5, 7:W + 7] = False
            assert (s[outside] == F32(b)).all() and outside.sum() > 500
            assert np.isin(tv, s).all()
    x = up_case("one NaN")
    nan = np.isnan(oracle_upsample(x.logits, x.H, x.W))
    assert int(nan[UP_NAN_AT[0]].sum()) == UP_NAN_FOOTPRINT and not nan[[b for b in range(UP_B) if b != UP_NAN_AT[0]]].any()
    assert np.array_equal(nan, np.isnan(upsample_ref64(x.logits, x.H, x.W)))
    x = up_case("special values")
    assert np.isinf(x.logits).sum() == 4 and (np.abs(x.logits) == 104).sum() == 4 and np.isfinite(oracle_upsample(x.logits, x.H, x.W)).all()
