"""Input preprocessing on the GPU - the array part of the reference's `RefDataset.__getitem__`
(reference utils/dataset.py:146-168, `getTransformMat` :190-205, `convert` :207-221) for a whole batch in one launch:

    mat, mat_inv = self.getTransformMat(img_size, True)
    img  = cv2.warpAffine(img, mat, self.input_size, flags=cv2.INTER_CUBIC, borderValue=[0.48145466*255, 0.4578275*255, 0.40821073*255])
    mask = cv2.warpAffine(mask, mat, self.input_size, flags=cv2.INTER_LINEAR, borderValue=0.) / 255.
    img, mask = self.convert(img, mask)          # CHW float, /255, -mean, /std

Inputs are the DECODED uint8 arrays (RGB [h, w, 3], mask [h, w]); record reading, JPEG / PNG decoding and the tokenizer stay
on the CPU side of the loader.  The kernels are in csrc/inputpipe.hip; there is no CPU
fallback.  The 8-bit warp arithmetic is OpenCV's, restated (oracle/input_pipe.py explains what that is anchored on)."""
import ctypes as C
import math
from dataclasses import dataclass, field, replace
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import hip
from .hip import ptr

MEAN = (0.48145466, 0.4578275, 0.40821073)      # utils/dataset.py:106-107
STD = (0.26862954, 0.26130258, 0.27577711)       # utils/dataset.py:108-109


def get_affine_transform(src, dst):
    """cv2.getAffineTransform: 2x3 double matrix mapping three float32 points src -> dst"""
    src = np.asarray(src, np.float32).astype(np.float64)
    dst = np.asarray(dst, np.float32).astype(np.float64)
    return np.linalg.solve(np.concatenate([src, np.ones((3, 1))], 1), dst).T.copy()


def get_transform_mat(img_size, input_size, inverse=False):
    """RefDataset.getTransformMat (utils/dataset.py:190-205): same arguments, same return (mat, mat_inv or None)"""
    ori_h, ori_w = img_size
    inp_h, inp_w = input_size
    scale = min(inp_h / ori_h, inp_w / ori_w)
    new_h, new_w = ori_h * scale, ori_w * scale
    bias_x, bias_y = (inp_w - new_w) / 2., (inp_h - new_h) / 2.
    src = np.array([[0, 0], [ori_w, 0], [0, ori_h]], np.float32)
    dst = np.array([[bias_x, bias_y], [new_w + bias_x, bias_y], [bias_x, new_h + bias_y]], np.float32)
    mat = get_affine_transform(src, dst)
    return (mat, get_affine_transform(dst, src)) if inverse else (mat, None)


@dataclass(frozen=True)
class Augment:
    """Training-time augmentation of the GPU input pipeline, validated here, before a device is touched.
    Geometry, applied to image and mask alike on top of the letter-box: `scale` = (lo, hi) range of an isotropic zoom about the
    centre of the network input, `translate` = largest shift as a fraction of the input width / height, `rotate` = largest
    rotation in degrees, `hflip` = probability of a horizontal mirror.  Colour, image only, in the fixed order brightness,
    contrast, saturation (no hue): each knob j draws a factor from [1 - j, 1 + j].  The colour transform is this project's own
    definition (include/cris_hip.h cris_preprocess_batch_aug) and is not pinned against another library.
    `hflip` defaults to 0 because referring expressions are spatial: "the left zebra" names another animal in the mirrored
    image.  When a sample is mirrored the pipeline exchanges `left` and `right` in its sentence (records.swap_left_right) -
    a heuristic that knows nothing of "clockwise", "3 o'clock" or "west", so leave hflip at 0 unless the data tolerates that.
    The defaults are the identity: no augmentation."""
    scale: Tuple[float, float] = (1.0, 1.0)
    translate: float = 0.0
    rotate: float = 0.0
    hflip: float = 0.0
    brightness: float = 0.0
    contrast: float = 0.0
    saturation: float = 0.0

    def __post_init__(self):
        sc = self.scale
        if isinstance(sc, (str, bytes)) or not hasattr(sc, "__len__") or len(sc) != 2:
            raise ValueError("Augment.scale must be a pair (lo, hi), got %r" % (sc,))
        for v in sc:
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError("Augment.scale must hold two finite numbers, got %r" % (sc,))
        object.__setattr__(self, "scale", (float(sc[0]), float(sc[1])))
        for f in ("translate", "rotate", "hflip", "brightness", "contrast", "saturation"):
            v = getattr(self, f)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError("Augment.%s must be a finite number, got %r" % (f, v))
            object.__setattr__(self, f, float(v))
        if not 0 < self.scale[0] <= self.scale[1]:
            raise ValueError("Augment.scale must satisfy 0 < lo <= hi, got %r" % (self.scale,))
        if not 0 <= self.translate < 1:
            raise ValueError("Augment.translate must be in [0, 1), got %r" % (self.translate,))
        if not 0 <= self.rotate <= 180:
            raise ValueError("Augment.rotate must be in [0, 180] degrees, got %r" % (self.rotate,))
        for f in ("hflip", "brightness", "contrast", "saturation"):
            if not 0 <= getattr(self, f) <= 1:
                raise ValueError("Augment.%s must be in [0, 1], got %r" % (f, getattr(self, f)))

    @staticmethod
    def normalized(spec) -> Optional["Augment"]:
        """None for None and for a spec equal to the defaults (the pipeline as it always was); else the spec"""
        if spec is None:
            return None
        if not isinstance(spec, Augment):
            raise ValueError("augment must be None or an inputpipe.Augment, got %r" % (spec,))
        return None if spec == Augment() else spec


@dataclass(frozen=True)
class AugmentParams:
    """The augmentation of ONE sample: zoom, shift in pixels of the network input, rotation in degrees, mirror, and the three
    colour factors (float32).  `mat` is the 2x3 matrix the Preprocessor used (filled in on its way out; ignored on the way in).
    The defaults are the identity."""
    scale: float = 1.0
    tx: float = 0.0
    ty: float = 0.0
    angle: float = 0.0
    flip: bool = False
    fb: float = 1.0
    fc: float = 1.0
    fs: float = 1.0
    mat: Optional[np.ndarray] = field(default=None, compare=False)

    def __post_init__(self):
        for f in ("scale", "tx", "ty", "angle"):
            v = float(getattr(self, f))
            if not math.isfinite(v):
                raise ValueError("AugmentParams.%s must be finite, got %r" % (f, v))
            object.__setattr__(self, f, v)
        if not self.scale > 0:
            raise ValueError("AugmentParams.scale must be > 0, got %r" % (self.scale,))
        object.__setattr__(self, "flip", bool(self.flip))
        for f in ("fb", "fc", "fs"):
            v = np.float32(getattr(self, f))
            if not np.isfinite(v) or v < 0:
                raise ValueError("AugmentParams.%s must be a finite factor >= 0, got %r" % (f, getattr(self, f)))
            object.__setattr__(self, f, v)

    @property
    def geometric(self):
        return not (self.scale == 1.0 and self.tx == 0.0 and self.ty == 0.0 and self.angle == 0.0 and not self.flip)


def augment_params(aug: Augment, u, input_size) -> List[AugmentParams]:
    """Pure host function: row u[i] of a [B, 8] array of uniforms in [0, 1) -> the parameters of sample i.
    scale = lo + u0 (hi - lo); tx = (2 u1 - 1) translate S_w, ty = (2 u2 - 1) translate S_h; angle = (2 u3 - 1) rotate;
    flip = u4 < hflip; fb, fc, fs = 1 + (2 u - 1) knob from u5, u6, u7, computed in float64 and rounded once to float32 - so a
    knob left at 0 yields a factor of exactly 1.0."""
    u = np.asarray(u, np.float64)
    if u.ndim != 2 or u.shape[1] != 8:
        raise ValueError("augment_params: u must be [B, 8], got %r" % (u.shape,))
    S_h, S_w = input_size
    lo, hi = aug.scale
    out = []
    for r in u:
        out.append(AugmentParams(scale=lo + r[0] * (hi - lo), tx=(2 * r[1] - 1) * aug.translate * S_w, ty=(2 * r[2] - 1) * aug.translate * S_h,
                                 angle=(2 * r[3] - 1) * aug.rotate, flip=bool(r[4] < aug.hflip), fb=np.float32(1 + (2 * r[5] - 1) * aug.brightness),
                                 fc=np.float32(1 + (2 * r[6] - 1) * aug.contrast), fs=np.float32(1 + (2 * r[7] - 1) * aug.saturation)))
    return out


def augment_matrix(img_size, input_size, params: AugmentParams):
    """2x3 float64 source->destination matrix M = (A . L)[:2]: L = get_transform_mat's letter-box as 3x3,
    A = T(c + (tx, ty)) . R(angle) . diag(scale * (-1 if flip else 1), scale) . T(-c) with c = (S_w / 2, S_h / 2) and
    R(a) = [[cos a, -sin a], [sin a, cos a]] (y points down, so a positive angle turns the picture clockwise on screen).
    With identity geometry it is get_transform_mat's matrix itself."""
    mat, _ = get_transform_mat(img_size, input_size, False)
    if not params.geometric:
        return mat
    S_h, S_w = input_size
    cx, cy = S_w / 2., S_h / 2.
    a = math.radians(params.angle)
    ca, sa = math.cos(a), math.sin(a)
    T1 = np.array([[1, 0, cx + params.tx], [0, 1, cy + params.ty], [0, 0, 1]], np.float64)
    R = np.array([[ca, -sa, 0], [sa, ca, 0], [0, 0, 1]], np.float64)
    D = np.diag([params.scale * (-1. if params.flip else 1.), params.scale, 1.])
    T0 = np.array([[1, 0, -cx], [0, 1, -cy], [0, 0, 1]], np.float64)
    L = np.vstack([mat, [0., 0., 1.]])
    return np.ascontiguousarray((T1 @ R @ D @ T0 @ L)[:2])


class Preprocessor:
    """Device-resident tables (remap weights, normalisation look-ups) + `__call__` for one batch."""

    def __init__(self, input_size, device="cuda:0"):
        self.input_size = (int(input_size[0]), int(input_size[1]))
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("the input pipeline runs on the GPU only (no CPU fallback)")
        lin, cub = np.zeros(1024 * 4, np.int16), np.zeros(1024 * 16, np.int16)
        hip.call("cris_remap_tables_u8", lin.ctypes.data_as(C.c_void_p), cub.ctypes.data_as(C.c_void_p))
        self.tab_linear, self.tab_cubic = torch.from_numpy(lin).to(self.dev), torch.from_numpy(cub).to(self.dev)
        v = np.arange(256, dtype=np.float32)
        mean, std = np.array(MEAN, np.float32), np.array(STD, np.float32)
        # img.float().div_(255.).sub_(mean).div_(std): three float32 operations per value, in this order
        lut = (((v[None, :] / np.float32(255.)).astype(np.float32) - mean[:, None]).astype(np.float32) / std[:, None]).astype(np.float32)
        self.lut_img = torch.from_numpy(np.ascontiguousarray(lut)).to(self.dev)
        # mask / 255. is a float64 division in numpy, then .float()
        self.lut_mask = torch.from_numpy((np.arange(256, dtype=np.float64) / 255.).astype(np.float32)).to(self.dev)
        # cv2 turns the Scalar border colour into pixel type: saturate_cast<uchar>(double)
        self.border = np.clip(np.rint(np.array(MEAN, np.float64) * 255), 0, 255).astype(np.uint8)
        # augmented launch only: v / 255 as one float32 division (the first step of lut_img), and mean rgb, std rgb
        self.unit = torch.from_numpy((v / np.float32(255.)).astype(np.float32)).to(self.dev)
        self.norm = np.ascontiguousarray(np.concatenate([mean, std]).astype(np.float32))
        self.last_params = None

    def __call__(self, images, masks=None, params=None):
        """images: list of uint8 RGB arrays / tensors [h, w, 3]; masks: optional list of uint8 [h, w] (None entries allowed).
        Returns (img [B, 3, S, S] float32, mask [B, S, S] float32 or None, mats, mat_invs) - mats as getTransformMat gives them.
        params: optional list of one AugmentParams per sample (training-time augmentation): the warp then uses augment_matrix
        instead of the letter-box - image and mask alike - and mats / mat_invs are that matrix and its cris_invert_affine;
        `last_params` keeps the parameters with the matrix used.  A batch whose colour factors are all 1 is the plain launch
        with other matrices; otherwise cris_preprocess_batch_aug runs instead, after cris_gray_sum_batch when some sample has
        fc != 1 (0, 1 or 2 decisions per batch, all on the current stream, nothing synchronises)."""
        B = len(images)
        if params is not None and len(params) != B:
            raise ValueError("params must hold one AugmentParams per image: %d for %d images" % (len(params), B))
        S_h, S_w = self.input_size
        keep, descs, mats, invs = [], (hip.SampleDesc * B)(), [], []
        for i, im in enumerate(images):
            t = torch.as_tensor(im)
            if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
                raise ValueError("image %d must be uint8 [h, w, 3], got %s %s" % (i, t.dtype, tuple(t.shape)))
            t = t.to(self.dev, non_blocking=True).contiguous()
            if params is not None and t.data_ptr() % 4:
                t = t.clone()                   # (a view at an odd offset: cris_gray_sum_batch reads whole dwords)
            keep.append(t)
            h, w = int(t.shape[0]), int(t.shape[1])
            d = descs[i]
            d.img, d.H, d.W = t.data_ptr(), h, w
            inv_at = C.addressof(d) + hip.SampleDesc.inv.offset
            if params is None:
                mat, mat_inv = get_transform_mat((h, w), self.input_size, True)
            else:
                mat = augment_matrix((h, w), self.input_size, params[i])
            m = np.ascontiguousarray(mat.reshape(6))
            hip.call("cris_invert_affine", m.ctypes.data_as(C.c_void_p), inv_at)
            if params is not None:
                mat_inv = np.array(d.inv, np.float64).reshape(2, 3)
            mats.append(mat)
            invs.append(mat_inv)
            d.mask = None
            if masks is not None and masks[i] is not None:
                mk = torch.as_tensor(masks[i])
                if mk.dtype != torch.uint8 or tuple(mk.shape) != (h, w):
                    raise ValueError("mask %d must be uint8 [%d, %d], got %s %s" % (i, h, w, mk.dtype, tuple(mk.shape)))
                mk = mk.to(self.dev, non_blocking=True).contiguous()
                keep.append(mk)
                d.mask = mk.data_ptr()
        # one upload: the descriptors, then (augmented batches) the [B, 3] colour factors behind them
        factors = sums = None
        if params is not None:
            factors = np.array([[p.fb, p.fc, p.fs] for p in params], np.float32).reshape(B, 3)
            self.last_params = [replace(p, mat=mt) for p, mt in zip(params, mats)]
            if (factors == 1).all():
                factors = None
        table = torch.frombuffer(bytearray(bytes(descs) + (factors.tobytes() if factors is not None else b"")), dtype=torch.uint8).to(self.dev)
        img = torch.empty(B, 3, S_h, S_w, dtype=torch.float32, device=self.dev)
        mask = torch.zeros(B, S_h, S_w, dtype=torch.float32, device=self.dev) if masks is not None else None
        stream = torch.cuda.current_stream().cuda_stream
        if factors is None:
            hip.call("cris_preprocess_batch", ptr(table), B, S_h, S_w, ptr(self.tab_linear), ptr(self.tab_cubic), ptr(self.lut_img),
                     ptr(self.lut_mask), self.border.ctypes.data_as(C.c_void_p), ptr(img), ptr(mask), stream)
        else:
            if (factors[:, 1] != 1).any():     # the contrast pivot needs each source image's mean luminance: one more launch
                sums = torch.zeros(B, dtype=torch.int64, device=self.dev)
                hip.call("cris_gray_sum_batch", C.addressof(descs), ptr(table), B, ptr(sums), stream)
            hip.call("cris_preprocess_batch_aug", ptr(table), B, S_h, S_w, ptr(self.tab_linear), ptr(self.tab_cubic), ptr(self.lut_img),
                     ptr(self.lut_mask), self.border.ctypes.data_as(C.c_void_p), ptr(table) + C.sizeof(descs), ptr(sums), ptr(self.unit),
                     self.norm.ctypes.data_as(C.c_void_p), ptr(img), ptr(mask), stream)
        self._keep = (keep, table, sums)          # until the next call: the launches read them asynchronously
        return img, mask, mats, invs
