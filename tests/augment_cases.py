"""Shared by tests/test_augment_cpu.py and tests/test_augment_gpu.py: small inputs and the numpy restatement of the colour
arithmetic of cris_preprocess_batch_aug (include/cris_hip.h).  The restatement works operation by operation in
np.float32 - numpy rounds every float32 array operation once, which is what the kernel does inside its `fp contract(off)`
region - with the mean luminance in double precision exactly as the header writes it.  The colour transform is this project's
own definition; nothing here is pinned against another library."""
import numpy as np

from oracle import input_pipe as ip

F = np.float32
INPUT_SIZE = (36, 52)                                   # non-square; 1872 pixels is not a multiple of the 256-thread block
SIZES = [(37, 50), (50, 37), (5, 3), (1, 1), (64, 64)]
NO_MASK = 2                                             # the sample that has no mask
TRIPLES = [(0, 1, 1), (2, 1, 1), (1, 0, 1), (1, 2, 1), (1, 1, 0), (1, 1, 2), (0.75, 1.3, 0.6), (1, 1, 1)]


class CountingRng:
    """a np.random.Generator stand-in that records the draws RecordPipeline makes"""

    def __init__(self, seed):
        self.rng, self.calls = np.random.default_rng(seed), []

    def random(self, *a, **k):
        self.calls.append(("random",) + a)
        return self.rng.random(*a, **k)

    def integers(self, *a, **k):
        self.calls.append(("integers",) + a)
        return self.rng.integers(*a, **k)


def image(h, w, seed):
    """smooth structure + noise, so that cubic overshoot and saturation both occur"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = 127 + 120 * np.sin(yy / 7.0)[:, :, None] * np.cos(xx[:, :, None] / 5.0 + np.arange(3)[None, None, :])
    return np.clip(base + rng.integers(-40, 40, (h, w, 3)), 0, 255).astype(np.uint8)


def mask(h, w):
    m = np.zeros((h, w), np.uint8)
    m[h // 4:h // 2 + 1, w // 5:w // 2 + 1] = 255
    return m


def batch():
    imgs = [image(h, w, i) for i, (h, w) in enumerate(SIZES)]
    masks = [None if i == NO_MASK else mask(h, w) for i, (h, w) in enumerate(SIZES)]
    return imgs, masks


def gray_sum(img_u8_hwc):
    """sum of 77 R + 150 G + 29 B over the image, exact"""
    p = img_u8_hwc.astype(np.int64)
    return int((77 * p[..., 0] + 150 * p[..., 1] + 29 * p[..., 2]).sum())


def _clamp01(x):
    return np.where(x < F(0), F(0), np.where(x > F(1), F(1), x)).astype(F)


def colour(v_u8_hwc, gsum, H, W, fb, fc, fs):
    """the colour steps of one sample on its 8-bit warp result [h, w, 3] -> float32 [3, h, w]; (H, W) and gsum describe the SOURCE"""
    fb, fc, fs = F(fb), F(fc), F(fs)
    x = (v_u8_hwc.astype(F) / F(255.)).astype(F)                       # unit[v]
    x = _clamp01((x * fb).astype(F))
    mean = F(np.float64(gsum) / (65280.0 * np.float64(H) * np.float64(W)))
    bm = F(fb * mean)
    pivot = F(1) if bm > F(1) else bm
    k = F(F(F(1) - fc) * pivot)
    t = (x * fc).astype(F)
    x = _clamp01((t + k).astype(F))
    g0, g1, g2 = (F(0.299) * x[..., 0]).astype(F), (F(0.587) * x[..., 1]).astype(F), (F(0.114) * x[..., 2]).astype(F)
    g = ((g0 + g1).astype(F) + g2).astype(F)
    sg = (F(F(1) - fs) * g).astype(F)
    t = (x * fs).astype(F)
    x = _clamp01((t + sg[..., None]).astype(F))
    x = x.transpose(2, 0, 1)
    x = (x - ip.MEAN[:, None, None]).astype(F)
    return (x / ip.STD[:, None, None]).astype(F)


def taps_inside(mat, src_hw, input_size):
    """[S_h, S_w] bool: does any of the 16 cubic taps of the destination pixel lie inside the source"""
    H, W = src_hw
    bx, by, _ = ip.warp_coords_u8(mat, input_size[1], input_size[0])
    return (by + 2 >= 0) & (by - 1 < H) & (bx + 2 >= 0) & (bx - 1 < W)


def reference_image(img_u8_hwc, mat, input_size, fb=1, fc=1, fs=1):
    """what Preprocessor returns for one sample: cubic warp with the CLIP-mean border, then the colour steps - except for an
    all-one sample and on pure letter-box border, which are `convert_image` of the warp"""
    S_h, S_w = input_size
    warped = ip.warp_affine_u8(img_u8_hwc, mat, S_w, S_h, ip.INTER_CUBIC, ip.BORDER_RGB)
    plain = ip.convert_image(warped)
    if F(fb) == 1 and F(fc) == 1 and F(fs) == 1:
        return plain
    H, W = img_u8_hwc.shape[:2]
    col = colour(warped, gray_sum(img_u8_hwc), H, W, fb, fc, fs)
    return np.where(taps_inside(mat, (H, W), input_size)[None], col, plain)


def reference_mask(mask_u8, mat, input_size):
    S_h, S_w = input_size
    return ip.convert_mask(ip.warp_affine_u8(mask_u8, mat, S_w, S_h, ip.INTER_LINEAR, 0.))
