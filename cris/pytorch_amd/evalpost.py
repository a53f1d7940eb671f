"""Evaluation post-processing on the GPU - the per-batch body of the reference's `validate` / `inference`
(reference engine/engine.py:100-123, :171-188) behind the same quantities: logits in, per-sample IoU out.

    preds = torch.sigmoid(model(imgs, texts))                                    engine.py:100-101
    preds = F.interpolate(preds, size=imgs.shape[-2:], mode='bicubic', align_corners=True)          :102-106
    pred  = cv2.warpAffine(pred, mat, (w, h), flags=cv2.INTER_CUBIC, borderValue=0.)                :114-116
    pred  = pred > 0.35 ; iou = sum(pred & mask) / (sum(pred | mask) + 1e-6)                        :117-123

The reference copies every prediction to the host and warps it with cv2; here all four steps are kernels of
libcris_hip.so (csrc/evalpost.hip) and only the two integer counts per sample come back.  There is no CPU fallback.

`validate_batch` is the per-sample form (one warp and one count launch per sample, float masks).  `iou_batch` is the batched
form that evaluate.Evaluator drives: steps 3-4 for a whole ragged batch in ONE launch, uint8 masks and the descriptor table
packed into one pinned buffer (`EvalStaging`), the warped map never written, counts accumulated in a table for the whole pass.
`predict_batch` is the same launch without ground truth (predict.Predictor): no mask goes up (`EvalStaging.pack_sizes`), the
binary masks come out at the original sizes and (area, score, bounding box) accumulate in an int64 table (`new_predict_stats`).
`iou_sweep_batch` is `iou_batch` at up to 64 thresholds in one launch (evaluate.Evaluator.sweep): counts [R, T, 2], column i what
`iou_batch` counts at thresholds[i].

`Components` is the optional mask clean-up between the launch that writes the masks and the numbers read from them:
`label_components` (connected-component labels of the packed masks, three launches), `filter_components` (keep the largest
component / drop the small ones in place, statistics over the kept pixels, three launches) and `mask_iou_batch` (intersection /
union counts from mask bytes) - DESIGN.md 9b.

`polygon_count_batch` / `polygon_collect` end the same chain with polygons instead (polygon.py; csrc/polygon.hip): the corner
visits are counted on the device, the host reads the totals, the rings are traced there and only their vertices cross to the host.
`rle_encode_batch` / `rle_collect` are the last stage of that chain: the packed masks, filtered or not, become COCO run-length
encodings (rle.py) - the transition positions are found on the device (csrc/rle.hip, four launches), only they cross to the host,
and the strings of a batch are built there in one vectorised pass.

`Boundary` is the optional second figure of an evaluation pass, Boundary IoU (Cheng et al., CVPR 2021): IoU restricted to the pixels
within `radius` of each mask's contour.  `erode_batch` (erosion of the packed masks by a square, or the boundary it leaves) and
`boundary_iou_batch` (intersection / union counts of the prediction's and the ground truth's boundaries) are three launches each of
csrc/morph.hip over 64-bit bit planes of the masks - DESIGN.md 9b.

`Smooth` is the optional smoothing of a thresholded mask before `Components`: opening (removes specks and thin bridges), closing
(fills pin-holes and narrow gaps) and hole filling, in that order.  `morph_batch` chains erosions and dilations of the packed masks
over the same bit planes (`dilate_batch`, `open_batch`, `close_batch`; csrc/morph.hip cris_morph_masks), `fill_holes_batch` labels
the background with the union-find of `label_components` and fills the components that do not reach the image's frame
(csrc/evalpost.hip cris_fill_holes), `smooth_batch` applies a spec in place - DESIGN.md 9b.

`decode_masks_batch` is the inverse of the encoder and the tracer: RLE and polygon masks (`mask_form`, packed as `MaskSources`)
are decoded on the device straight into either packed layout (csrc/decode.hip), so that encoded ground truth
(`EvalStaging.pack_encoded` / `decode`) and results files (evaluate.score_results) run through the kernels above - DESIGN.md 9b."""
import ctypes as C
import math

import numpy as np
import torch

from . import hip
from .hip import ptr


def _stream():
    return torch.cuda.current_stream().cuda_stream


def sigmoid_upsample(logits, H, W):
    """[B, 1, h, w] (or [B, h, w]) fp32 logits -> [B, H, W] probabilities: sigmoid + bicubic, align_corners=True"""
    if logits.device.type != "cuda":
        raise RuntimeError("evalpost runs on the GPU only (no CPU fallback)")
    x = logits.detach().float().contiguous()
    if x.dim() == 4:
        x = x[:, 0].contiguous()
    B, h, w = x.shape
    out = torch.empty(B, H, W, dtype=torch.float32, device=x.device)
    hip.call("cris_sigmoid_bicubic_up", ptr(x), B, h, w, H, W, ptr(out), _stream())
    return out


def warp_to_original(prob, mat, ori_size, border=0.0):
    """cv2.warpAffine(prob, mat, (w, h), flags=cv2.INTER_CUBIC, borderValue=border): prob [H, W] cuda fp32, mat the 2x3 matrix the
    reference passes (param['inverse'], utils/dataset.py:190-205), ori_size = (h, w) -> [h, w] cuda fp32"""
    H, W = prob.shape
    h, w = int(ori_size[0]), int(ori_size[1])
    m = np.ascontiguousarray(np.asarray(mat, dtype=np.float64).reshape(6))
    out = torch.empty(h, w, dtype=torch.float32, device=prob.device)
    hip.call("cris_warp_affine_cubic", ptr(prob.contiguous()), H, W, m.ctypes.data_as(C.c_void_p), w, h, float(border), ptr(out), _stream())
    return out


def iou_counts(pred, mask, thr=0.35):
    """(intersection, union) of (pred > thr) and (mask != 0) as device int32[2] (+=); pred, mask: same-shape cuda fp32"""
    counts = torch.zeros(2, dtype=torch.int32, device=pred.device)
    hip.call("cris_threshold_iou", ptr(pred.contiguous()), ptr(mask.contiguous()), pred.numel(), float(thr), ptr(counts), _stream())
    return counts


def validate_batch(logits, in_size, mats, ori_sizes, masks, thr=0.35):
    """One batch of engine.validate's loop (engine.py:100-123).  logits: model(imgs, texts) [B, 1, h, w]; in_size:
    imgs.shape[-2:]; mats / ori_sizes: param['inverse'] / param['ori_size'] per sample; masks: per-sample [ori_h, ori_w]
    tensors or arrays holding mask / 255.  Returns the list of per-sample IoUs (python floats, one host read for all)."""
    probs = sigmoid_upsample(logits, int(in_size[0]), int(in_size[1]))
    counts = []
    for b in range(probs.shape[0]):
        p = warp_to_original(probs[b], mats[b], ori_sizes[b])
        m = torch.as_tensor(np.asarray(masks[b], dtype=np.float32) if not torch.is_tensor(masks[b]) else masks[b],
                            dtype=torch.float32, device=p.device)
        counts.append(iou_counts(p, m, thr))
    c = torch.stack(counts).cpu().numpy().astype(np.float64)
    return [float(i / (u + 1e-6)) for i, u in c]


class EvalStaging:
    """One batch of `iou_batch` work on the host and its twin on the device: the descriptor table (hip.EvalDesc) followed by the
    packed uint8 masks, in ONE host buffer (pinned when the device is a GPU) that `upload()` sends with one asynchronous copy.
    Mask rows are padded with zeros to a pitch that is a multiple of 4 (the kernel reads one dword per 4 pixels); every mask
    starts on a 16-byte boundary.  Several descriptors may name one mask (the expressions of one image).  `device=None` keeps
    the host half only (packing is host arithmetic)."""

    ALIGN = 16

    def __init__(self, device=None, max_descs=64, mask_bytes=1 << 20):
        self.device = None if device is None else torch.device(device)
        self.host = self.dev = self.event = None
        self.n = self.mask_bytes = self.out_bytes = 0
        self._reserve(max_descs, mask_bytes)

    @staticmethod
    def _up(v, a):
        return (int(v) + a - 1) // a * a

    def _reserve(self, max_descs, mask_bytes):
        self.wait()
        self.max_descs, self.mask_cap = int(max_descs), self._up(mask_bytes, self.ALIGN)
        self.mask_base = self._up(self.max_descs * C.sizeof(hip.EvalDesc), self.ALIGN)
        pin = self.device is not None and self.device.type == "cuda"
        self.host = torch.zeros(self.mask_base + self.mask_cap, dtype=torch.uint8, pin_memory=pin)
        self.dev = None if self.device is None else torch.empty_like(self.host, device=self.device)
        self.descs = (hip.EvalDesc * self.max_descs).from_address(self.host.data_ptr())
        self._bytes = self.host.numpy()

    def wait(self):
        """until the last upload has left the host buffer (it is about to be overwritten)"""
        if self.event is not None:
            self.event.synchronize()
            self.event = None

    def pack(self, masks, descs):
        """masks: uint8 [h, w] CPU tensors / arrays.  descs: (mat, mask index, map index, count row) per descriptor, `mat` the
        2x3 matrix cv2.warpAffine is given (param['inverse']); the output size of a descriptor is its mask's size."""
        shapes = [(int(m.shape[0]), int(m.shape[1])) for m in masks]
        pitches = [self._up(w, 4) for _, w in shapes]
        need = sum(self._up(p * h, self.ALIGN) for p, (h, _) in zip(pitches, shapes))
        if len(descs) > self.max_descs or need > self.mask_cap:
            self._reserve(max(len(descs), self.max_descs), max(need + need // 4, self.mask_cap))
        self.wait()
        offs, off = [], 0
        for m, p, (h, w) in zip(masks, pitches, shapes):
            rows = self._bytes[self.mask_base + off:self.mask_base + off + p * h].reshape(h, p)
            rows[:, :w] = m.numpy() if torch.is_tensor(m) else np.asarray(m, dtype=np.uint8)
            rows[:, w:] = 0
            offs.append(off)
            off += self._up(p * h, self.ALIGN)
        self.mask_bytes, out_off = off, 0
        for i, (mat, mi, mp, row) in enumerate(descs):
            m = np.ascontiguousarray(np.asarray(mat, dtype=np.float64).reshape(6))
            h, w = shapes[mi]
            hip.call("cris_eval_desc_fill", C.addressof(self.descs[i]), m.ctypes.data_as(C.c_void_p), w, h, int(mp), offs[mi], pitches[mi],
                     out_off, int(row))
            out_off += self._up(pitches[mi] * h, self.ALIGN)
        self.n, self.out_bytes = len(descs), out_off
        return self

    def pack_sizes(self, shapes, descs):
        """`pack` without ground truth (predict_batch): shapes: (h, w) per image; descs: (mat, shape index, map index, stats row)
        per descriptor.  Only the descriptor table is filled and uploaded - no mask bytes (mask_bytes = 0, every mask_off 0 and
        ignored); pitch, out_off and out_bytes are computed as `pack` computes them."""
        shapes = [(int(h), int(w)) for h, w in shapes]
        if len(descs) > self.max_descs:
            self._reserve(len(descs), self.mask_cap)
        self.wait()
        out_off = 0
        for i, (mat, si, mp, row) in enumerate(descs):
            m = np.ascontiguousarray(np.asarray(mat, dtype=np.float64).reshape(6))
            h, w = shapes[si]
            pitch = self._up(w, 4)
            hip.call("cris_eval_desc_fill", C.addressof(self.descs[i]), m.ctypes.data_as(C.c_void_p), w, h, int(mp), 0, pitch, out_off, int(row))
            out_off += self._up(pitch * h, self.ALIGN)
        self.n, self.mask_bytes, self.out_bytes = len(descs), 0, out_off
        return self

    def pack_encoded(self, masks, descs):
        """`pack` for a batch whose masks are, some or all, still encoded.  masks: `mask_form` results - "array" entries (PNG ground
        truth decoded on the host) are packed as `pack` packs them, "rle" / "polygon" entries get a slot of the same shape ON THE DEVICE
        ONLY: their mask-source table (hip.MaskSrc) and payload (`MaskSources`) follow the descriptor table in the part of the buffer
        below mask_base, which grows like the descriptors' own part, and `decode()` fills the slots after `upload()`.  The slots of
        the host-decoded masks come first, so that the one asynchronous copy still covers a prefix: descriptors, sources, payload and
        those masks - without any, the tables and the payload only.  After upload() and decode(), `masks` holds in every slot what
        `pack` of the host-decoded masks in that order (arrays first) would have uploaded.  descs: as for `pack`, the mask index
        names an entry of `masks` in the caller's order."""
        forms = list(masks)
        order = [i for i, f in enumerate(forms) if f[0] == "array"] + [i for i, f in enumerate(forms) if f[0] != "array"]
        shapes = [(f[1], f[2]) for f in forms]
        pitches = [self._up(w, 4) for _, w in shapes]
        offs, off, host_bytes = [0] * len(forms), 0, 0
        for i in order:
            offs[i] = off
            off += self._up(pitches[i] * shapes[i][0], self.ALIGN)
            if forms[i][0] == "array":
                host_bytes = off
        enc = [i for i in order if forms[i][0] != "array"]
        srcs = MaskSources([forms[i] for i in enc], [(offs[i], pitches[i]) for i in enc]) if enc else None
        aux_off = self._up(len(descs) * C.sizeof(hip.EvalDesc), self.ALIGN)
        aux_end = aux_off + (0 if srcs is None else srcs.blob.size)
        if aux_end > self.mask_base or off > self.mask_cap:
            rows = max(-(-(aux_end + aux_end // 4) // C.sizeof(hip.EvalDesc)) if aux_end > self.mask_base else 0, len(descs), self.max_descs)
            self._reserve(rows, max(off + off // 4 if off > self.mask_cap else 0, self.mask_cap))
        self.wait()
        for i in order[:len(forms) - len(enc)]:
            (h, w), p, m = shapes[i], pitches[i], forms[i][3]
            rows = self._bytes[self.mask_base + offs[i]:self.mask_base + offs[i] + p * h].reshape(h, p)
            rows[:, :w] = m.numpy() if torch.is_tensor(m) else m
            rows[:, w:] = 0
        if srcs is not None:
            self._bytes[aux_off:aux_end] = srcs.blob
            srcs.place(self.host.data_ptr() + aux_off, None if self.dev is None else self.dev.data_ptr() + aux_off)
        out_off = 0
        for i, (mat, mi, mp, row) in enumerate(descs):
            m = np.ascontiguousarray(np.asarray(mat, dtype=np.float64).reshape(6))
            h, w = shapes[mi]
            hip.call("cris_eval_desc_fill", C.addressof(self.descs[i]), m.ctypes.data_as(C.c_void_p), w, h, int(mp), offs[mi], pitches[mi],
                     out_off, int(row))
            out_off += self._up(pitches[mi] * h, self.ALIGN)
        self.n, self.mask_bytes, self.out_bytes = len(descs), off, out_off
        self._pending = (srcs, self.mask_base + host_bytes if host_bytes else aux_end)
        return self

    def decode(self, work=None):
        """after `pack_encoded(...).upload()`: decode the encoded masks into their slots of `masks` on the current stream
        (`decode_masks_batch`; nothing to do for a batch that `pack` packed).  work: scratch from `decode_work` to reuse -> the
        scratch used, or `work` itself when there was nothing to decode."""
        srcs = getattr(self, "encoded", None)
        if srcs is None:
            return work
        work = decode_work(srcs, self.device, work)
        decode_masks_batch(srcs, self.masks, work=work)
        return work

    def upload(self):
        """one asynchronous copy of the descriptor table and the masks (the used prefix of the buffer) on the current stream; after
        `pack_encoded` the prefix ends with the last host-decoded mask, or with the payload when there is none"""
        self.encoded, end = self.__dict__.pop("_pending", None) or (None, self.mask_base + self.mask_bytes)
        self.last_upload_bytes = end
        self.dev[:end].copy_(self.host[:end], non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record()
        return self

    @property
    def masks(self):
        """the packed masks on the device (after upload())"""
        return self.dev[self.mask_base:self.mask_base + self.mask_bytes]


def iou_batch(probs, descs, masks_u8, counts, row0, thr=0.35, out_masks=None, border=0.0):
    """ONE launch for a whole batch (cris_eval_iou_batch): for every descriptor of `descs` (an uploaded EvalStaging) the inverse
    warp of probs[map] to the original size, the threshold and counts[row0 + row] += (intersection, union) against its mask in
    `masks_u8` (device uint8, the staging's packed masks).  probs: [P, H, W] cuda fp32 (sigmoid_upsample); counts: [R, 2] cuda
    int32, zeroed by the caller once per pass; out_masks: optional device uint8 buffer of descs.out_bytes that receives
    (warp > thr) * 255 per descriptor (row pitch of its mask, descriptor i at descs.descs[i].out_off)."""
    if probs.device.type != "cuda":
        raise RuntimeError("evalpost runs on the GPU only (no CPU fallback)")
    if probs.dim() != 3 or probs.dtype != torch.float32 or not probs.is_contiguous():
        raise ValueError("iou_batch: probs must be contiguous fp32 [P, H, W]")
    if counts.dtype != torch.int32 or counts.dim() != 2 or counts.shape[1] != 2 or not counts.is_contiguous() or not 0 <= row0 < counts.shape[0]:
        raise ValueError("iou_batch: counts must be contiguous int32 [R, 2] and row0 inside it")
    if masks_u8.dtype != torch.uint8 or not masks_u8.is_contiguous():
        raise ValueError("iou_batch: masks_u8 must be a contiguous uint8 buffer")
    if out_masks is not None and (out_masks.dtype != torch.uint8 or not out_masks.is_contiguous() or out_masks.numel() < descs.out_bytes):
        raise ValueError("iou_batch: out_masks must be a contiguous uint8 buffer of at least descs.out_bytes")
    P, H, W = probs.shape
    hip.call("cris_eval_iou_batch", ptr(probs), P, H, W, C.addressof(descs.descs), descs.dev.data_ptr(), descs.n, ptr(masks_u8),
             masks_u8.numel(), float(thr), float(border), counts.data_ptr() + 8 * int(row0), counts.shape[0] - int(row0),
             ptr(out_masks), 0 if out_masks is None else out_masks.numel(), _stream())


SWEEP_MAX = 64          # thresholds of one sweep launch (EP_SWEEP_MAX of csrc/evalpost.hip)


def iou_sweep_batch(probs, descs, masks_u8, counts, row0, thresholds, border=0.0):
    """`iou_batch` at T thresholds in ONE launch (cris_eval_iou_sweep_batch): the per-pixel value of every descriptor is computed
    once and counts[row0 + row, i] += (intersection, union) of (value > thresholds[i]) against the mask, for every i - column i is
    exactly what `iou_batch(..., thr=float(np.float32(thresholds[i])))` adds.  probs, descs, masks_u8: as for `iou_batch`; counts:
    [R, T, 2] cuda int32, zeroed by the caller once per pass; thresholds: 1 .. 64 finite, strictly increasing values (rounded to
    float32 once, here on the host; the library checks them).  No masks are written."""
    if probs.device.type != "cuda":
        raise RuntimeError("evalpost runs on the GPU only (no CPU fallback)")
    if probs.dim() != 3 or probs.dtype != torch.float32 or not probs.is_contiguous():
        raise ValueError("iou_sweep_batch: probs must be contiguous fp32 [P, H, W]")
    thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64).astype(np.float32))
    if thr.ndim != 1 or not 1 <= thr.shape[0] <= SWEEP_MAX:
        raise ValueError("iou_sweep_batch: thresholds must be a list of 1 .. %d values" % SWEEP_MAX)
    T = int(thr.shape[0])
    if (counts.dtype != torch.int32 or counts.dim() != 3 or counts.shape[1] != T or counts.shape[2] != 2 or not counts.is_contiguous()
            or not 0 <= row0 < counts.shape[0]):
        raise ValueError("iou_sweep_batch: counts must be contiguous int32 [R, T, 2] with T = len(thresholds) and row0 inside it")
    if masks_u8.dtype != torch.uint8 or not masks_u8.is_contiguous():
        raise ValueError("iou_sweep_batch: masks_u8 must be a contiguous uint8 buffer")
    P, H, W = probs.shape
    hip.call("cris_eval_iou_sweep_batch", ptr(probs), P, H, W, C.addressof(descs.descs), descs.dev.data_ptr(), descs.n, ptr(masks_u8),
             masks_u8.numel(), thr.ctypes.data_as(C.c_void_p), T, float(border), counts.data_ptr() + 8 * T * int(row0),
             counts.shape[0] - int(row0), _stream())


PREDICT_FIELDS = ("area", "score_q16", "x_min", "y_min", "x_end", "y_end")
PREDICT_INIT = (0, 0, 2 ** 31 - 1, 2 ** 31 - 1, 0, 0)


def new_predict_stats(rows, device):
    """the initialised statistics table of `predict_batch`: int64 [rows, 6], every row (0, 0, 2^31 - 1, 2^31 - 1, 0, 0) - the
    neutral elements of the kernel's add, add, min, min, max, max (PREDICT_FIELDS)"""
    if int(rows) <= 0:
        raise ValueError("new_predict_stats: rows must be positive")
    return torch.tensor(PREDICT_INIT, dtype=torch.int64).repeat(int(rows), 1).to(device)


def predict_batch(probs, descs, stats, row0, thr=0.35, out_masks=None, border=0.0):
    """ONE launch for a whole batch WITHOUT ground truth (cris_predict_masks_batch): for every descriptor of `descs` (an
    uploaded EvalStaging, `pack_sizes` or `pack`) the inverse warp of probs[map] to the original size - iou_batch's values, bit
    for bit - the threshold, and over the pixels above it stats[row0 + row] (+=, +=, min, min, max, max)= (1, rint(value * 65536),
    x, y, x + 1, y + 1).  probs: [P, H, W] cuda fp32 (sigmoid_upsample); stats: [R, 6] cuda int64 from new_predict_stats;
    out_masks: optional device uint8 buffer of descs.out_bytes that receives (warp > thr) * 255 per descriptor (pitch
    descs.descs[i].pitch, descriptor i at descs.descs[i].out_off); None = statistics only."""
    if probs.device.type != "cuda":
        raise RuntimeError("evalpost runs on the GPU only (no CPU fallback)")
    if probs.dim() != 3 or probs.dtype != torch.float32 or not probs.is_contiguous():
        raise ValueError("predict_batch: probs must be contiguous fp32 [P, H, W]")
    if stats.dtype != torch.int64 or stats.dim() != 2 or stats.shape[1] != 6 or not stats.is_contiguous() or not 0 <= row0 < stats.shape[0]:
        raise ValueError("predict_batch: stats must be contiguous int64 [R, 6] and row0 inside it")
    if out_masks is not None and (out_masks.dtype != torch.uint8 or not out_masks.is_contiguous() or out_masks.numel() < descs.out_bytes):
        raise ValueError("predict_batch: out_masks must be a contiguous uint8 buffer of at least descs.out_bytes")
    P, H, W = probs.shape
    hip.call("cris_predict_masks_batch", ptr(probs), P, H, W, C.addressof(descs.descs), descs.dev.data_ptr(), descs.n, float(thr),
             float(border), stats.data_ptr() + 48 * int(row0), stats.shape[0] - int(row0), ptr(out_masks),
             0 if out_masks is None else out_masks.numel(), _stream())


class Components:
    """Connected-component clean-up of a thresholded mask, as a validated value (the style of ops.SegLoss): components of fewer
    than `min_area` pixels are dropped first; with keep="largest" only the remaining component of greatest area survives (ties:
    the one whose first pixel in raster order comes first).  connectivity: 4 (edges) or 8 (edges and corners).  Host only."""

    KEEP = ("all", "largest")
    __slots__ = ("keep", "min_area", "connectivity")

    def __init__(self, keep="all", min_area=0, connectivity=8):
        if keep not in self.KEEP:
            raise ValueError("Components: keep must be 'all' or 'largest', got %r" % (keep,))
        if isinstance(min_area, bool) or not isinstance(min_area, (int, np.integer)) or min_area < 0:
            raise ValueError("Components: min_area must be an integer >= 0, got %r" % (min_area,))
        if isinstance(connectivity, bool) or connectivity not in (4, 8):
            raise ValueError("Components: connectivity must be 4 or 8, got %r" % (connectivity,))
        object.__setattr__(self, "keep", keep)
        object.__setattr__(self, "min_area", int(min_area))
        object.__setattr__(self, "connectivity", int(connectivity))

    def __setattr__(self, name, value):
        raise AttributeError("Components is immutable")

    @property
    def is_noop(self):
        """keep="all" with min_area <= 1 filters nothing (every component has at least one pixel)"""
        return self.keep == "all" and self.min_area <= 1

    def __eq__(self, other):
        return isinstance(other, Components) and (self.keep, self.min_area, self.connectivity) == (other.keep, other.min_area, other.connectivity)

    def __hash__(self):
        return hash((self.keep, self.min_area, self.connectivity))

    def __repr__(self):
        return "Components(keep=%r, min_area=%d, connectivity=%d)" % (self.keep, self.min_area, self.connectivity)


def components_spec(value, what="components"):
    """None or a Components -> the spec to apply, or None when there is nothing to do (a spec that filters nothing is no spec);
    anything else is a ValueError.  Host only: callers run this before they touch a device."""
    if value is None:
        return None
    if not isinstance(value, Components):
        raise ValueError("%s must be None or an evalpost.Components, got %r" % (what, value))
    return None if value.is_noop else value


INFO_FIELDS = ("n_components", "kept_components", "raw_area", "error")
LABEL_ERROR = -2        # CC_ERR of csrc/evalpost.hip: a union-find walk hit its iteration cap


def _check_packed(name, masks_u8, descs):
    if masks_u8.device.type != "cuda":
        raise RuntimeError("evalpost runs on the GPU only (no CPU fallback)")
    if masks_u8.dtype != torch.uint8 or masks_u8.dim() != 1 or not masks_u8.is_contiguous() or masks_u8.numel() < descs.out_bytes:
        raise ValueError("%s: masks_u8 must be a contiguous uint8 buffer of at least descs.out_bytes" % name)


def label_components(masks_u8, descs, connectivity=8, out=None):
    """Canonical connected-component labels of every descriptor's mask in the packed buffer `masks_u8` (what iou_batch /
    predict_batch wrote into out_masks; `descs`: the uploaded EvalStaging of that launch) -> int32 [descs.out_bytes], one word per
    mask byte at the same offsets: the word of a foreground pixel (byte != 0, x < w_out) is the index y * pitch + x, relative to
    the descriptor's out_off, of the first pixel of its component in raster order; background and pitch padding are -1; words
    between two descriptors' rectangles are not written.  Three launches on the current stream (cris_label_components), none
    depending on the content.  out: an int32 buffer of at least descs.out_bytes words to reuse."""
    _check_packed("label_components", masks_u8, descs)
    if connectivity not in (4, 8):
        raise ValueError("label_components: connectivity must be 4 or 8, got %r" % (connectivity,))
    if out is None:
        out = torch.empty(descs.out_bytes, dtype=torch.int32, device=masks_u8.device)
    elif out.dtype != torch.int32 or out.dim() != 1 or not out.is_contiguous() or out.numel() < descs.out_bytes or out.device != masks_u8.device:
        raise ValueError("label_components: out must be a contiguous int32 buffer of at least descs.out_bytes words on the masks' device")
    hip.call("cris_label_components", ptr(masks_u8), descs.out_bytes, C.addressof(descs.descs), descs.dev.data_ptr(), descs.n,
             int(connectivity), ptr(out), out.numel(), _stream())
    return out[:descs.out_bytes]


def filter_work(descs, device, out=None):
    """the scratch of `filter_components` for this batch (areas per root, one winner word per descriptor): `out` when it is large
    enough, a new int64 buffer otherwise.  The launcher zeroes it itself."""
    words = (hip.load().cris_filter_components_work_bytes(descs.out_bytes, descs.n) + 7) // 8
    if out is not None and out.numel() >= words:
        return out
    return torch.empty(words + words // 4, dtype=torch.int64, device=device)


def filter_components(masks_u8, labels, descs, spec, info, row0, probs=None, stats=None, border=0.0, work=None):
    """Apply `spec` (a Components) to the packed masks IN PLACE, given their `label_components` labels: kept pixels become 255,
    every other byte of a descriptor's rectangle 0.  info: [R, 4] cuda int64 zeroed by the caller once per pass;
    info[row0 + row] += (n_components before filtering, kept_components, raw_area, error) (INFO_FIELDS).  probs / stats (both or
    neither; probs [P, H, W] as for predict_batch, stats from new_predict_stats): stats[row0 + row] receives over the KEPT pixels
    exactly what predict_batch adds over the pixels above its threshold - the value is recomputed by the same device function, so a
    mask of one component gives predict_batch's row bit for bit.  work: scratch from `filter_work` to reuse.  One memset and three
    launches on the current stream (cris_filter_components).  The caller checks the error column when it reads `info`."""
    _check_packed("filter_components", masks_u8, descs)
    if not isinstance(spec, Components):
        raise ValueError("filter_components: spec must be an evalpost.Components, got %r" % (spec,))
    if labels.dtype != torch.int32 or labels.dim() != 1 or not labels.is_contiguous() or labels.numel() < descs.out_bytes:
        raise ValueError("filter_components: labels must be a contiguous int32 buffer of at least descs.out_bytes words")
    if info.dtype != torch.int64 or info.dim() != 2 or info.shape[1] != 4 or not info.is_contiguous() or not 0 <= row0 < info.shape[0]:
        raise ValueError("filter_components: info must be contiguous int64 [R, 4] and row0 inside it")
    if (probs is None) != (stats is None):
        raise ValueError("filter_components: probs and stats go together")
    P = H = W = 0
    if probs is not None:
        if probs.dim() != 3 or probs.dtype != torch.float32 or not probs.is_contiguous():
            raise ValueError("filter_components: probs must be contiguous fp32 [P, H, W]")
        if stats.dtype != torch.int64 or stats.dim() != 2 or stats.shape[1] != 6 or not stats.is_contiguous() or not 0 <= row0 < stats.shape[0]:
            raise ValueError("filter_components: stats must be contiguous int64 [R, 6] and row0 inside it")
        P, H, W = probs.shape
    work = filter_work(descs, masks_u8.device, work)
    hip.call("cris_filter_components", ptr(masks_u8), descs.out_bytes, ptr(labels), labels.numel(), C.addressof(descs.descs),
             descs.dev.data_ptr(), descs.n, 1 if spec.keep == "largest" else 0, min(spec.min_area, 2 ** 31 - 1), ptr(work), 8 * work.numel(),
             info.data_ptr() + 32 * int(row0), info.shape[0] - int(row0), ptr(probs), P, H, W, float(border),
             None if stats is None else stats.data_ptr() + 48 * int(row0), 0 if stats is None else stats.shape[0] - int(row0), _stream())


def check_component_info(info):
    """info: the [R, 4] table of `filter_components` as read by the host -> the same array; raises when an error column is set"""
    info = np.asarray(info)
    bad = np.nonzero(info[:, 3])[0]
    if bad.size:
        raise RuntimeError("connected components: the union-find walk of row(s) %s hit its iteration cap (corrupt label buffer?)" % bad[:8].tolist())
    return info


RLE_RB, RLE_CG = 32, 64  # rows of a band / columns of a block in csrc/rle.hip (the shapes at which its kernels change path)


def rle_work(descs, device, out=None):
    """the scratch of `rle_encode_batch` for this batch (per-segment counts, one base per descriptor): `out` when it is large
    enough, a new int64 buffer otherwise.  Nothing has to be zeroed."""
    words = (hip.load().cris_rle_work_bytes(C.addressof(descs.descs), descs.n) + 7) // 8
    if out is not None and out.numel() >= words:
        return out
    return torch.empty(words + words // 4, dtype=torch.int64, device=device)


def rle_pixels(descs):
    """sum of h * w over the descriptors: the run words that always suffice (a checkerboard has one transition per pixel)"""
    return sum(descs.descs[i].h_out * descs.descs[i].w_out for i in range(descs.n))


def rle_encode_batch(masks_u8, descs, runs=None, work=None):
    """COCO run-length encoding of every descriptor's mask in the packed buffer `masks_u8` (what iou_batch / predict_batch wrote
    into out_masks, filtered or not; `descs`: the uploaded EvalStaging of that launch) -> (runs, totals): runs, uint32 positions
    as an int32 buffer, receives the column-major transition positions (rle.py: P) of descriptor 0, then 1, ..., packed and
    ascending within each; totals, int64 [n + 1]: the number of positions per descriptor and, last, their sum.  runs: a
    contiguous int32 buffer to reuse, of ANY size - the launch never writes past it, positions that do not fit are dropped and
    totals[n] still tells the words needed (`rle_collect` then grows and encodes again); None allocates one word per pixel,
    which always suffices.  work: scratch from `rle_work` to reuse.  Four launches on the current stream (cris_rle_encode), none
    depending on the content; nothing is synchronised or read here."""
    _check_packed("rle_encode_batch", masks_u8, descs)
    if descs.n < 1:
        raise ValueError("rle_encode_batch: no descriptors")
    if runs is None:
        runs = torch.empty(max(rle_pixels(descs), 1), dtype=torch.int32, device=masks_u8.device)
    elif runs.dtype != torch.int32 or runs.dim() != 1 or not runs.is_contiguous() or runs.numel() < 1 or runs.device != masks_u8.device:
        raise ValueError("rle_encode_batch: runs must be a contiguous int32 buffer on the masks' device")
    work = rle_work(descs, masks_u8.device, work)
    totals = torch.empty(descs.n + 1, dtype=torch.int64, device=masks_u8.device)
    hip.call("cris_rle_encode", ptr(masks_u8), descs.out_bytes, C.addressof(descs.descs), descs.dev.data_ptr(), descs.n, ptr(work),
             8 * work.numel(), ptr(runs), runs.numel(), ptr(totals), _stream())
    return runs, totals


def rle_collect(runs, totals, descs, masks_u8=None, work=None):
    """The read of `rle_encode_batch`: totals first, then exactly totals[n] words of `runs` - two device-to-host copies - and the
    strings of the whole batch in one vectorised pass on the host (rle.strings_from_positions) -> list of {"size": [h, w],
    "counts": bytes} per descriptor.  When totals[n] exceeds the capacity of `runs`, a buffer of totals[n] words is allocated and
    the batch is encoded once more from `masks_u8` (the buffer the first call read, still unchanged; without it the overflow is
    a RuntimeError)."""
    from . import rle
    n = descs.n
    t = totals.cpu().numpy()
    need = int(t[n])
    if t.shape != (n + 1,) or need != int(t[:n].sum()) or need < 0:
        raise RuntimeError("rle_collect: totals %r do not belong to these %d descriptors" % (t.tolist()[:8], n))
    if need > runs.numel():
        if masks_u8 is None:
            raise RuntimeError("rle_collect: the batch needs %d run words, the buffer holds %d; pass masks_u8 to encode again" % (need, runs.numel()))
        runs, totals = rle_encode_batch(masks_u8, descs, runs=torch.empty(need, dtype=torch.int32, device=runs.device), work=work)
        t = totals.cpu().numpy()
        if int(t[n]) != need:
            raise RuntimeError("rle_collect: the masks changed between the two encodes (%d positions, then %d)" % (need, int(t[n])))
    words = runs[:need].cpu().numpy().view(np.uint32)
    return rle.strings_from_positions(words, t[:n], [(descs.descs[i].h_out, descs.descs[i].w_out) for i in range(n)])


POLYGON_RB, POLYGON_CG, POLYGON_CHUNK = 32, 64, 1024  # vertex rows of a band / vertex columns of a tile / visits per scan block in csrc/polygon.hip
POLYGON_SIMPLIFY_WAVE, POLYGON_SIMPLIFY_LDS = 256, 4096  # longest ring one wave simplifies / longest ring staged in LDS (SP_WAVE_RING, SP_LDS_RING in csrc/simplify.hip)


def polygon_work(descs, device, out=None):
    """the scratch of `polygon_count_batch` for this batch (per-segment counts of both lists, one base per descriptor): `out` when
    it is large enough, a new int64 buffer otherwise.  Nothing has to be zeroed; `polygon_collect` reads what the count left."""
    words = (hip.load().cris_polygon_work_bytes(C.addressof(descs.descs), descs.n) + 7) // 8
    if out is not None and out.numel() >= words:
        return out
    return torch.empty(words + words // 4, dtype=torch.int64, device=device)


class PolygonBuffers:
    """the grow-only device buffers of `polygon_collect`, reused across batches: trace_work (the tracer's scratch) and out (header,
    ring table and vertices of a batch, one int64 buffer so that one copy reads them).  After a collect: `spans` = the int64 words
    the trace was told it may use (trace_work, out), `table` / `vertices` = what the host read (int64 [rings, 4], int32 [V, 2]).
    A collect with `simplify` also holds simplify_work (the simplifier's scratch) and simplified (its header of 4 words, ring table
    and vertices): `spans` then has four entries (trace_work, out, simplify_work, simplified), `table` is int64 [rings, 5],
    `vertices` the kept ones, and `header` the simplifier's (rings, vertices, traced rings, rounds of the deepest ring) followed by
    the traced vertices."""

    def __init__(self, trace_work=None, out=None, simplify_work=None, simplified=None):
        self.trace_work, self.out = trace_work, out
        self.simplify_work, self.simplified = simplify_work, simplified
        self.spans = self.table = self.vertices = self.header = None

    @staticmethod
    def _grown(buf, words, device):
        if buf is not None and (buf.dtype != torch.int64 or buf.dim() != 1 or not buf.is_contiguous() or buf.device != device):
            raise ValueError("polygon_collect: buffers must hold contiguous int64 buffers on the masks' device")
        return buf if buf is not None and buf.numel() >= words else torch.empty(words + words // 4, dtype=torch.int64, device=device)


def polygon_count_batch(masks_u8, descs, work=None):
    """The vertices of every descriptor's mask in the packed buffer `masks_u8` as polygon rings (polygon.py states the format;
    `descs`: the uploaded EvalStaging of the launch that wrote the masks) -> totals, int64 [n + 1] on the device: vertices per
    descriptor and, last, their sum.  work: scratch from `polygon_work`; hand the same buffer to `polygon_collect`, which reads the
    offsets this call leaves in it.  Three launches on the current stream (cris_polygon_count), none depending on the content;
    nothing is synchronised or read here."""
    _check_packed("polygon_count_batch", masks_u8, descs)
    if descs.n < 1:
        raise ValueError("polygon_count_batch: no descriptors")
    work = polygon_work(descs, masks_u8.device, work)
    totals = torch.empty(descs.n + 1, dtype=torch.int64, device=masks_u8.device)
    hip.call("cris_polygon_count", ptr(masks_u8), descs.out_bytes, C.addressof(descs.descs), descs.dev.data_ptr(), descs.n, ptr(work),
             8 * work.numel(), ptr(totals), _stream())
    return totals


def polygon_collect(masks_u8, descs, totals, work=None, buffers=None, extra_rounds=0, simplify=None):
    """The read of `polygon_count_batch` and the trace between its two copies -> list of polygon dicts per descriptor
    ({"size": [h, w], "rings": [int32 [k, 2]], "holes": [bool]}, polygon.py).  First copy: totals.  Then the buffers are sized from
    them (`buffers`: a PolygonBuffers to reuse, grown only when a batch needs more), cris_polygon_trace runs on the current stream
    with ceil(log2(max vertices of a mask)) + extra_rounds jumping rounds, and the second copy reads the header, the ring table and
    exactly totals[n] vertices.  masks_u8 and work: what the count read and left (work=None counts once more into a new scratch).
    A batch without foreground issues no trace and no second copy.
    simplify: None, or the Douglas-Peucker tolerance in pixels (a multiple of 0.25 in [0.25, 64]; polygon.simplify states the
    definition, every h_out and w_out must be <= 32767).  Then cris_polygon_simplify follows the trace on the stream - the host reads
    nothing in between -, the buffers also hold its scratch and its output, and the dicts are the simplified ones (with "epsilon").
    Instead of the traced header, table and vertices the host reads the simplifier's 4-word header and then exactly the simplified
    table and vertices: one small extra copy, the header, for a second copy that no longer carries every stair-step corner.
    simplify=None issues exactly the calls and allocations it did before there was a simplifier."""
    from . import polygon
    q = None if simplify is None else polygon.check_epsilon(simplify)
    _check_packed("polygon_collect", masks_u8, descs)
    n = descs.n
    if totals.dtype != torch.int64 or totals.shape != (n + 1,) or totals.device != masks_u8.device:
        raise ValueError("polygon_collect: totals must be the int64 [n + 1] tensor of polygon_count_batch for these descriptors")
    if buffers is not None and not isinstance(buffers, PolygonBuffers):
        raise ValueError("polygon_collect: buffers must be an evalpost.PolygonBuffers, got %r" % (buffers,))
    if isinstance(extra_rounds, bool) or not isinstance(extra_rounds, int) or not 0 <= extra_rounds <= 8:
        raise ValueError("polygon_collect: extra_rounds must be an int in 0 .. 8, got %r" % (extra_rounds,))
    sizes = [(descs.descs[i].h_out, descs.descs[i].w_out) for i in range(n)]
    if q is not None:
        for h, w in sizes:
            polygon.check_simplify_size(h, w)
    if work is None:
        work = polygon_work(descs, masks_u8.device)
        totals = polygon_count_batch(masks_u8, descs, work=work)
    elif work.dtype != torch.int64 or not work.is_contiguous() or work.device != masks_u8.device:
        raise ValueError("polygon_collect: work must be the int64 scratch polygon_count_batch used")
    buffers = PolygonBuffers() if buffers is None else buffers
    t = totals.cpu().numpy()                                               # the first copy
    need = int(t[n])
    if need != int(t[:n].sum()) or int(t[:n].min()) < 0 or (t[:n] & 1).any() or need > 2 ** 30:
        raise RuntimeError("polygon_collect: totals %r do not belong to these %d descriptors" % (t.tolist()[:8], n))
    buffers.spans = buffers.table = buffers.vertices = buffers.header = None
    if need == 0:
        if q is not None:
            return polygon.simplify_from_rings(np.zeros((0, 2), np.int32), np.zeros((0, 5), np.int64), sizes, simplify)
        return polygon.from_rings(np.zeros((0, 2), np.int32), np.zeros((0, 4), np.int64), sizes)
    lib = hip.load()
    ring_cap = need // 4
    tw_words = (lib.cris_polygon_trace_work_bytes(need, n) + 7) // 8
    out_words = 2 + 4 * ring_cap + need
    buffers.trace_work = PolygonBuffers._grown(buffers.trace_work, tw_words, masks_u8.device)
    buffers.out = PolygonBuffers._grown(buffers.out, out_words, masks_u8.device)
    buffers.spans = (tw_words, out_words)
    out = buffers.out
    if q is not None:
        sw_words = (lib.cris_polygon_simplify_work_bytes(need, ring_cap) + 7) // 8
        so_words = 4 + 5 * ring_cap + need
        buffers.simplify_work = PolygonBuffers._grown(buffers.simplify_work, sw_words, masks_u8.device)
        buffers.simplified = PolygonBuffers._grown(buffers.simplified, so_words, masks_u8.device)
        buffers.spans = (tw_words, out_words, sw_words, so_words)
    hip.call("cris_polygon_trace", ptr(masks_u8), descs.out_bytes, C.addressof(descs.descs), descs.dev.data_ptr(), n, ptr(work),
             8 * work.numel(), ptr(totals), need, int(t[:n].max()), extra_rounds, ptr(buffers.trace_work), 8 * tw_words,
             out.data_ptr() + 8 * (2 + 4 * ring_cap), need, out.data_ptr() + 16, ring_cap, out.data_ptr(), _stream())
    if q is not None:
        simp = buffers.simplified
        hip.call("cris_polygon_simplify", out.data_ptr() + 8 * (2 + 4 * ring_cap), out.data_ptr() + 16, out.data_ptr(), need, ring_cap, q,
                 C.addressof(descs.descs), n, ptr(buffers.simplify_work), 8 * sw_words, simp.data_ptr() + 8 * (4 + 5 * ring_cap), need,
                 simp.data_ptr() + 32, ring_cap, simp.data_ptr(), _stream())
        head = simp[:4].cpu().numpy()                                      # the small extra copy: the simplifier's header
        rings, kept, traced = int(head[0]), int(head[1]), int(head[2])
        if not (0 < traced <= ring_cap and 0 <= rings <= traced and 3 * rings <= kept <= need):
            raise RuntimeError("polygon_collect: the simplifier left %d rings of %d vertices from %d traced rings of %d vertices: the "
                               "masks or the work buffer changed between the calls" % (rings, kept, traced, need))
        buffers.header = np.append(head, need)                             # ... and, last, the vertices the trace had delivered
        if rings == 0:
            buffers.table, buffers.vertices = np.zeros((0, 5), np.int64), np.zeros((0, 2), np.int32)
        else:                                                              # the second copy: exactly the table and the kept vertices
            words = torch.cat([simp[4:4 + 5 * rings], simp[4 + 5 * ring_cap:4 + 5 * ring_cap + kept]]).cpu().numpy()
            buffers.table = words[:5 * rings].reshape(rings, 5)
            buffers.vertices = words[5 * rings:].view(np.int32).reshape(kept, 2)    # an (x, y) pair is one 64-bit word
        return polygon.simplify_from_rings(buffers.vertices, buffers.table, sizes, simplify)
    words = out[:out_words].cpu().numpy()                                  # the second copy
    rings, written = int(words[0]), int(words[1])
    if not 0 < rings <= ring_cap or written != need:
        raise RuntimeError("polygon_collect: the trace found %d rings of %d vertices, the count %d vertices: the masks or the work "
                           "buffer changed between the two calls" % (rings, written, need))
    buffers.table = words[2:2 + 4 * rings].reshape(rings, 4)
    buffers.vertices = words[2 + 4 * ring_cap:].view(np.int32).reshape(need, 2)
    return polygon.from_rings(buffers.vertices, buffers.table, sizes)


def mask_iou_batch(pred_masks_u8, descs, gt_masks_u8, counts, row0):
    """counts[row0 + row] += (#(pred != 0 and gt != 0), #(pred != 0 or gt != 0)) per descriptor, from mask BYTES
    (cris_mask_iou_batch): pred in the packed output layout (out_off), gt the staging's packed masks (mask_off).  counts: [R, 2] cuda
    int32, iou_batch's table - on iou_batch's own unfiltered out_masks this reproduces its counts."""
    _check_packed("mask_iou_batch", pred_masks_u8, descs)
    if gt_masks_u8.dtype != torch.uint8 or not gt_masks_u8.is_contiguous():
        raise ValueError("mask_iou_batch: gt_masks_u8 must be a contiguous uint8 buffer")
    if counts.dtype != torch.int32 or counts.dim() != 2 or counts.shape[1] != 2 or not counts.is_contiguous() or not 0 <= row0 < counts.shape[0]:
        raise ValueError("mask_iou_batch: counts must be contiguous int32 [R, 2] and row0 inside it")
    hip.call("cris_mask_iou_batch", ptr(pred_masks_u8), descs.out_bytes, C.addressof(descs.descs), descs.dev.data_ptr(), descs.n,
             ptr(gt_masks_u8), gt_masks_u8.numel(), counts.data_ptr() + 8 * int(row0), counts.shape[0] - int(row0), _stream())


class Boundary:
    """Boundary IoU as a validated value (the style of `Components`): the boundary of an h x w mask is what an erosion by a
    (2 d + 1)-square removes from it, d = max(int(round(ratio * sqrt(h^2 + w^2))), min_radius) - Python's round, half to even, in
    float64; ratio=0.02 is the figure LVIS and the COCO panoptic tooling use.  Host only."""

    __slots__ = ("ratio", "min_radius")

    def __init__(self, ratio=0.02, min_radius=1):
        if isinstance(ratio, bool) or not isinstance(ratio, (int, float, np.integer, np.floating)) or not (math.isfinite(ratio) and 0 < ratio <= 1):
            raise ValueError("Boundary: ratio must be a finite number in (0, 1], got %r" % (ratio,))
        if isinstance(min_radius, bool) or not isinstance(min_radius, (int, np.integer)) or min_radius < 1:
            raise ValueError("Boundary: min_radius must be an integer >= 1, got %r" % (min_radius,))
        object.__setattr__(self, "ratio", float(ratio))
        object.__setattr__(self, "min_radius", int(min_radius))

    def __setattr__(self, name, value):
        raise AttributeError("Boundary is immutable")

    def radius(self, h, w):
        """the erosion radius of an h x w mask"""
        h, w = int(h), int(w)
        if h < 1 or w < 1:
            raise ValueError("Boundary.radius: the size must be positive, got %r x %r" % (h, w))
        return max(int(round(self.ratio * math.sqrt(h * h + w * w))), self.min_radius)

    def __eq__(self, other):
        return isinstance(other, Boundary) and (self.ratio, self.min_radius) == (other.ratio, other.min_radius)

    def __hash__(self):
        return hash((self.ratio, self.min_radius))

    def __repr__(self):
        return "Boundary(ratio=%r, min_radius=%d)" % (self.ratio, self.min_radius)


def boundary_spec(value, what="boundary"):
    """None, True or a Boundary -> the spec to apply (True: Boundary()) or None; anything else is a ValueError.  Host only: callers
    run this before they touch a device."""
    if value is None:
        return None
    if value is True:
        return Boundary()
    if not isinstance(value, Boundary):
        raise ValueError("%s must be None, True or an evalpost.Boundary, got %r" % (what, value))
    return value


def boundary_radii(descs, spec):
    """the radius of every descriptor of `descs` (an EvalStaging) under `spec`, from its output size -> host int32 [n]"""
    if not isinstance(spec, Boundary):
        raise ValueError("boundary_radii: spec must be an evalpost.Boundary, got %r" % (spec,))
    return np.array([spec.radius(descs.descs[i].h_out, descs.descs[i].w_out) for i in range(descs.n)], dtype=np.int32)


def boundary_work(descs, device, out=None):
    """the scratch of `erode_batch` / `boundary_iou_batch` for this batch (four bit planes): `out` when it is large enough, a new
    int64 buffer otherwise.  Nothing has to be zeroed."""
    words = (hip.load().cris_boundary_work_bytes(C.addressof(descs.descs), descs.n) + 7) // 8
    if out is not None and out.numel() >= words:
        return out
    return torch.empty(max(words + words // 4, 1), dtype=torch.int64, device=device)


def _radii(name, radii, descs, device):
    """(host int32 [n], device int32 [n]) of `radii`: a host sequence is uploaded with one small asynchronous copy, a CUDA int32
    tensor is read back for the library's host check (callers on the hot path pass the host sequence)"""
    if torch.is_tensor(radii) and radii.device.type == "cuda":
        if radii.dtype != torch.int32 or radii.dim() != 1 or not radii.is_contiguous() or radii.numel() != descs.n:
            raise ValueError("%s: radii must be a contiguous int32 tensor of one radius per descriptor" % name)
        return np.ascontiguousarray(radii.cpu().numpy()), radii
    given = np.asarray(radii.numpy() if torch.is_tensor(radii) else radii)
    if given.ndim != 1 or given.shape[0] != descs.n or given.dtype.kind not in "iu":
        raise ValueError("%s: radii must be one integer radius per descriptor (%d), got %r" % (name, descs.n, radii))
    if (given < 1).any() or (given > 2 ** 31 - 1).any():
        raise ValueError("%s: every radius must be in 1 .. 2^31 - 1" % name)
    host = np.ascontiguousarray(given.astype(np.int32))
    pinned = torch.from_numpy(host.copy()).pin_memory()
    return host, pinned.to(device, non_blocking=True)


def erode_batch(masks_u8, descs, radii, out=None, boundary=False, work=None):
    """Erosion of every descriptor's mask in the packed buffer `masks_u8` by the (2 r + 1)-square, r = radii[i] (`boundary_radii`;
    a host sequence or a CUDA int32 tensor) -> a packed uint8 buffer with the same layout: 255 where the whole window lies inside
    the image and is foreground (byte != 0, x < w_out), else 0; boundary=True: 255 where the mask is foreground and the erosion is
    not.  Only the h_out x w_out pixels of every descriptor are written - pitch padding, gaps and tail of `out` keep their bytes
    (a new buffer is zeroed).  out: a uint8 buffer of at least descs.out_bytes to reuse; `masks_u8` itself erodes in place.  work:
    scratch from `boundary_work`.  Three launches on the current stream (cris_erode_masks), none depending on the content."""
    _check_packed("erode_batch", masks_u8, descs)
    if descs.n < 1:
        raise ValueError("erode_batch: no descriptors")
    if out is None:
        out = torch.zeros(descs.out_bytes, dtype=torch.uint8, device=masks_u8.device)
    elif out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous() or out.numel() < descs.out_bytes or out.device != masks_u8.device:
        raise ValueError("erode_batch: out must be a contiguous uint8 buffer of at least descs.out_bytes on the masks' device")
    host, dev = _radii("erode_batch", radii, descs, masks_u8.device)
    work = boundary_work(descs, masks_u8.device, work)
    hip.call("cris_erode_masks", ptr(masks_u8), descs.out_bytes, C.addressof(descs.descs), descs.dev.data_ptr(), descs.n,
             host.ctypes.data_as(C.c_void_p), ptr(dev), ptr(work), 8 * work.numel(), ptr(out), out.numel(), 1 if boundary else 0, _stream())
    return out


def boundary_iou_batch(pred_masks_u8, descs, gt_masks_u8, radii, counts, row0, work=None):
    """counts[row0 + row] += (#(B(pred) and B(gt)), #(B(pred) or B(gt))) per descriptor, B(M) = M & ~erode(M, radii[i]) the
    boundary of width radii[i] (cris_boundary_iou_batch): pred in the packed output layout (out_off), gt the staging's packed masks
    (mask_off).  counts: [R, 2] cuda int32 like `mask_iou_batch`'s; radii: `boundary_radii` (a host sequence or a CUDA int32
    tensor); work: scratch from `boundary_work`.  Three launches on the current stream, none depending on the content."""
    _check_packed("boundary_iou_batch", pred_masks_u8, descs)
    if descs.n < 1:
        raise ValueError("boundary_iou_batch: no descriptors")
    if gt_masks_u8.dtype != torch.uint8 or not gt_masks_u8.is_contiguous() or gt_masks_u8.device != pred_masks_u8.device:
        raise ValueError("boundary_iou_batch: gt_masks_u8 must be a contiguous uint8 buffer on the masks' device")
    if counts.dtype != torch.int32 or counts.dim() != 2 or counts.shape[1] != 2 or not counts.is_contiguous() or not 0 <= row0 < counts.shape[0]:
        raise ValueError("boundary_iou_batch: counts must be contiguous int32 [R, 2] and row0 inside it")
    host, dev = _radii("boundary_iou_batch", radii, descs, pred_masks_u8.device)
    work = boundary_work(descs, pred_masks_u8.device, work)
    hip.call("cris_boundary_iou_batch", ptr(pred_masks_u8), descs.out_bytes, C.addressof(descs.descs), descs.dev.data_ptr(), descs.n,
             ptr(gt_masks_u8), gt_masks_u8.numel(), host.ctypes.data_as(C.c_void_p), ptr(dev), ptr(work), 8 * work.numel(),
             counts.data_ptr() + 8 * int(row0), counts.shape[0] - int(row0), _stream())


MORPH_OPS = {"erode": 0, "dilate": 1, "erode_clipped": 2}     # CRIS_MORPH_* of include/cris_hip.h
MORPH_MAX_OPS = 8
MORPH_MAX_RADIUS = 65535
FILL_FIELDS = ("holes_filled", "pixels_filled", "holes", "error")


def _morph_ops(name, ops, n):
    """the host form of a chain: (int32 [k] operation codes, int32 [k, n] radii) of `ops`, a sequence of (operation, radius or one
    radius per descriptor).  Host only."""
    if isinstance(ops, (str, bytes)) or not hasattr(ops, "__len__") or not 1 <= len(ops) <= MORPH_MAX_OPS:
        raise ValueError("%s: ops must be a sequence of 1 .. %d (operation, radius) pairs, got %r" % (name, MORPH_MAX_OPS, ops))
    codes = np.zeros(len(ops), np.int32)
    radii = np.zeros((len(ops), n), np.int32)
    for k, item in enumerate(ops):
        if not isinstance(item, (tuple, list)) or len(item) != 2 or item[0] not in MORPH_OPS:
            raise ValueError("%s: ops[%d] must be (%s, radius), got %r" % (name, k, " | ".join(repr(o) for o in MORPH_OPS), item))
        given = np.asarray(item[1].cpu().numpy() if torch.is_tensor(item[1]) else item[1])
        if given.dtype.kind not in "iu" or given.dtype == np.bool_ or given.ndim > 1 or (given.ndim == 1 and given.shape[0] != n):
            raise ValueError("%s: the radius of ops[%d] must be an integer or one integer per descriptor (%d), got %r" % (name, k, n, item[1]))
        if (given < 1).any() or (given > MORPH_MAX_RADIUS).any():
            raise ValueError("%s: every radius must be in 1 .. %d, got %r in ops[%d]" % (name, MORPH_MAX_RADIUS, item[1], k))
        codes[k] = MORPH_OPS[item[0]]
        radii[k, :] = given
    return codes, radii


def morph_work(descs, device, out=None):
    """the scratch of `morph_batch` for this batch (two bit planes, half of `boundary_work`): `out` when it is large enough, a new
    int64 buffer otherwise.  Nothing has to be zeroed."""
    words = (hip.load().cris_boundary_work_bytes(C.addressof(descs.descs), descs.n) // 2 + 7) // 8
    if out is not None and out.numel() >= words:
        return out
    return torch.empty(max(words + words // 4, 1), dtype=torch.int64, device=device)


def morph_batch(masks_u8, descs, ops, out=None, work=None):
    """A chain of window operations on every descriptor's mask in the packed buffer `masks_u8` -> a packed uint8 buffer with the same
    layout, bytes 0 / 255.  ops: a sequence of up to 8 (operation, radius) pairs applied in order, radius an integer >= 1 or one per
    descriptor (a host sequence), operation one of
        "erode"          E_r: 1 iff the whole (2 r + 1)-square lies inside the image and is foreground (`erode_batch`'s result)
        "dilate"         D_r: OR over the square clipped to the image
        "erode_clipped"  E'_r: AND over the square clipped to the image (= not D_r(not M): nothing outside the image exists)
    Only the h_out x w_out pixels of every descriptor are written - pitch padding, gaps and tail of `out` keep their bytes (a new
    buffer is zeroed).  out: a uint8 buffer of at least descs.out_bytes to reuse; `masks_u8` itself works in place.  work: scratch
    from `morph_work`.  2 + 2 len(ops) launches on the current stream (cris_morph_masks), none depending on the content: the masks
    become bit planes once, every operation is a row pass and a column pass between two planes, the bytes are written once."""
    _check_packed("morph_batch", masks_u8, descs)
    if descs.n < 1:
        raise ValueError("morph_batch: no descriptors")
    codes, radii = _morph_ops("morph_batch", ops, descs.n)
    if out is None:
        out = torch.zeros(descs.out_bytes, dtype=torch.uint8, device=masks_u8.device)
    elif out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous() or out.numel() < descs.out_bytes or out.device != masks_u8.device:
        raise ValueError("morph_batch: out must be a contiguous uint8 buffer of at least descs.out_bytes on the masks' device")
    dev = torch.from_numpy(radii.copy()).pin_memory().to(masks_u8.device, non_blocking=True)
    work = morph_work(descs, masks_u8.device, work)
    hip.call("cris_morph_masks", ptr(masks_u8), descs.out_bytes, C.addressof(descs.descs), descs.dev.data_ptr(), descs.n,
             codes.ctypes.data_as(C.c_void_p), len(codes), radii.ctypes.data_as(C.c_void_p), ptr(dev), ptr(work), 8 * work.numel(), ptr(out),
             out.numel(), _stream())
    return out


def dilate_batch(masks_u8, descs, radii, out=None, work=None):
    """D_r of every mask (`morph_batch` with one "dilate"): four launches"""
    return morph_batch(masks_u8, descs, [("dilate", radii)], out=out, work=work)


def open_batch(masks_u8, descs, radii, out=None, work=None):
    """open_r = D_r(E_r(M)) - scipy.ndimage.binary_opening with a full (2 r + 1)-square: removes what the square does not fit into
    (specks, thin bridges); anti-extensive and idempotent.  Six launches."""
    return morph_batch(masks_u8, descs, [("erode", radii), ("dilate", radii)], out=out, work=work)


def close_batch(masks_u8, descs, radii, out=None, work=None):
    """close_r = E'_r(D_r(M)) - binary_erosion(binary_dilation(M, S), S, border_value=1): fills what the square does not fit into
    (pin-holes, narrow gaps); extensive also for objects that touch the image border, and idempotent.  NOT scipy's binary_closing
    default, whose erosion takes the outside for background and eats objects at the border.  Six launches."""
    return morph_batch(masks_u8, descs, [("dilate", radii), ("erode_clipped", radii)], out=out, work=work)


def fill_work(descs, device, out=None):
    """the scratch of `fill_holes_batch` for this batch (one word per mask byte): `out` when it is large enough, a new int64 buffer
    otherwise.  The launcher zeroes it itself."""
    words = (hip.load().cris_fill_holes_work_bytes(descs.out_bytes) + 7) // 8
    if out is not None and out.numel() >= words:
        return out
    return torch.empty(max(words + words // 4, 2), dtype=torch.int64, device=device)


def fill_holes_batch(masks_u8, descs, info, row0, connectivity=4, max_area=None, labels=None, work=None):
    """Fill the holes of every descriptor's mask in the packed buffer IN PLACE: a hole is a connected component of the background
    (connectivity 4, or 8) that holds no pixel of the image's outer frame; every pixel of a hole of at most `max_area` pixels (None:
    of every hole) becomes 255, no other byte changes.  connectivity=4, max_area=None is scipy.ndimage.binary_fill_holes.  info:
    [R, 4] cuda int64 zeroed by the caller once per pass; info[row0 + row] += (holes_filled, pixels_filled, holes, error)
    (FILL_FIELDS; `check_component_info` reads the error column).  labels: an int32 buffer of at least descs.out_bytes words to reuse
    (it receives the labels of the BACKGROUND); work: scratch from `fill_work`.  Five launches and one memset on the current stream
    (cris_fill_holes), none depending on the content.  Descriptors must not alias one rectangle."""
    _check_packed("fill_holes_batch", masks_u8, descs)
    if descs.n < 1:
        raise ValueError("fill_holes_batch: no descriptors")
    if isinstance(connectivity, bool) or connectivity not in (4, 8):
        raise ValueError("fill_holes_batch: connectivity must be 4 or 8, got %r" % (connectivity,))
    if max_area is not None and (isinstance(max_area, bool) or not isinstance(max_area, (int, np.integer)) or max_area < 0):
        raise ValueError("fill_holes_batch: max_area must be None or an integer >= 0, got %r" % (max_area,))
    if info.dtype != torch.int64 or info.dim() != 2 or info.shape[1] != 4 or not info.is_contiguous() or not 0 <= row0 < info.shape[0]:
        raise ValueError("fill_holes_batch: info must be contiguous int64 [R, 4] and row0 inside it")
    if labels is None:
        labels = torch.empty(descs.out_bytes, dtype=torch.int32, device=masks_u8.device)
    elif labels.dtype != torch.int32 or labels.dim() != 1 or not labels.is_contiguous() or labels.numel() < descs.out_bytes or labels.device != masks_u8.device:
        raise ValueError("fill_holes_batch: labels must be a contiguous int32 buffer of at least descs.out_bytes words on the masks' device")
    work = fill_work(descs, masks_u8.device, work)
    hip.call("cris_fill_holes", ptr(masks_u8), descs.out_bytes, C.addressof(descs.descs), descs.dev.data_ptr(), descs.n, int(connectivity),
             -1 if max_area is None else min(int(max_area), 2 ** 31 - 1), ptr(labels), labels.numel(), ptr(work), 8 * work.numel(),
             info.data_ptr() + 32 * int(row0), info.shape[0] - int(row0), _stream())


class Smooth:
    """Mask smoothing after the threshold, as a validated value (the style of `Components`).  The order is fixed: opening by the
    (2 open + 1)-square (removes specks and thin bridges), then closing by the (2 close + 1)-square (fills pin-holes and narrow gaps;
    `close_batch`: objects at the image border are kept), then hole filling (holes of at most `max_hole_area` pixels, None = all;
    background connectivity `hole_connectivity`), then - where the entry point takes one - the `Components` filter.  Radii are
    integers in pixels at the image's own size; 0 means off.  Host only."""

    __slots__ = ("open", "close", "fill_holes", "max_hole_area", "hole_connectivity")

    def __init__(self, open=0, close=0, fill_holes=False, max_hole_area=None, hole_connectivity=4):
        for name, r in (("open", open), ("close", close)):
            if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not 0 <= r <= MORPH_MAX_RADIUS:
                raise ValueError("Smooth: %s must be an integer radius in 0 .. %d, got %r" % (name, MORPH_MAX_RADIUS, r))
        if not isinstance(fill_holes, (bool, np.bool_)):
            raise ValueError("Smooth: fill_holes must be True or False, got %r" % (fill_holes,))
        if max_hole_area is not None and (isinstance(max_hole_area, bool) or not isinstance(max_hole_area, (int, np.integer)) or max_hole_area < 1):
            raise ValueError("Smooth: max_hole_area must be None or an integer >= 1, got %r" % (max_hole_area,))
        if max_hole_area is not None and not fill_holes:
            raise ValueError("Smooth: max_hole_area needs fill_holes=True")
        if isinstance(hole_connectivity, bool) or hole_connectivity not in (4, 8):
            raise ValueError("Smooth: hole_connectivity must be 4 or 8, got %r" % (hole_connectivity,))
        object.__setattr__(self, "open", int(open))
        object.__setattr__(self, "close", int(close))
        object.__setattr__(self, "fill_holes", bool(fill_holes))
        object.__setattr__(self, "max_hole_area", None if max_hole_area is None else int(max_hole_area))
        object.__setattr__(self, "hole_connectivity", int(hole_connectivity))

    def __setattr__(self, name, value):
        raise AttributeError("Smooth is immutable")

    def _key(self):
        return (self.open, self.close, self.fill_holes, self.max_hole_area, self.hole_connectivity)

    @property
    def is_noop(self):
        """both radii 0 and no hole filling: nothing changes"""
        return self.open == 0 and self.close == 0 and not self.fill_holes

    @property
    def ops(self):
        """the window operations of the spec as `morph_batch` takes them: () when both radii are 0"""
        return (((("erode", self.open), ("dilate", self.open)) if self.open else ())
                + ((("dilate", self.close), ("erode_clipped", self.close)) if self.close else ()))

    def __eq__(self, other):
        return isinstance(other, Smooth) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return "Smooth(open=%d, close=%d, fill_holes=%r, max_hole_area=%r, hole_connectivity=%d)" % self._key()


def smooth_spec(value, what="smooth"):
    """None or a Smooth -> the spec to apply, or None when there is nothing to do (a spec that changes nothing is no spec); anything
    else is a ValueError.  Host only: callers run this before they touch a device."""
    if value is None:
        return None
    if not isinstance(value, Smooth):
        raise ValueError("%s must be None or an evalpost.Smooth, got %r" % (what, value))
    return None if value.is_noop else value


def smooth_batch(masks_u8, descs, spec, info, row0, labels=None, work=None, fwork=None):
    """Apply `spec` (a Smooth) to the packed masks IN PLACE on the current stream: `morph_batch` with the spec's operations (open,
    then close - one chain, the masks are packed to bit planes and written back once), then `fill_holes_batch`.  info / row0 /
    labels / fwork: as for `fill_holes_batch` (the table is touched only with fill_holes); work: scratch from `morph_work`."""
    if not isinstance(spec, Smooth):
        raise ValueError("smooth_batch: spec must be an evalpost.Smooth, got %r" % (spec,))
    if spec.ops:
        morph_batch(masks_u8, descs, spec.ops, out=masks_u8, work=work)
    if spec.fill_holes:
        fill_holes_batch(masks_u8, descs, info, row0, spec.hole_connectivity, spec.max_hole_area, labels=labels, work=fwork)


# ---- encoded masks back onto the device: the inverse of rle_encode_batch and of polygon_count_batch / polygon_collect ----

MASK_KINDS = ("array", "rle", "polygon")
DECODE_T = 256          # threads of a block in csrc/decode.hip (the sizes at which its kernels take another chunk)


def mask_form(mask, where="mask"):
    """Any form a mask is exchanged in -> (kind, h, w, payload), validated on the host before anything else happens:
        "array"    uint8 [h, w] array or CPU tensor (non-zero is foreground), or the bytes of an 8-bit gray PNG (decoded here);
                   payload = the uint8 array / tensor
        "rle"      {"size": [h, w], "counts": str | bytes | list of integers} (rle.py; str counts are what a results JSON holds);
                   payload = the counts as int64
        "polygon"  {"size", "rings", "holes"} with or without "epsilon" (polygon.py: traced or simplified); payload = the rings
    An object with a `.mask` attribute (predict.Prediction) stands for that mask.  COCO's flat [x0, y0, x1, y1, ...] polygon lists
    are NOT accepted: polygon.to_coco drops the holes and the "epsilon" marker, and COCO fills such lists as a union, not even-odd,
    so they do not name one mask - exchange RLE (masks="rle") instead.  Raises ValueError (prefixed with `where`)."""
    from . import pngdec, polygon, rle
    if not isinstance(mask, (dict, np.ndarray, bytes, bytearray, memoryview, list)) and not torch.is_tensor(mask) and hasattr(mask, "mask"):
        mask = mask.mask
    try:
        if isinstance(mask, (bytes, bytearray, memoryview)):
            try:
                mask = pngdec.decode_gray(bytes(mask))
            except hip.HipLibraryError as e:
                raise ValueError("bytes that are no 8-bit gray PNG (%s)" % e) from None
        if torch.is_tensor(mask) or isinstance(mask, np.ndarray):
            if mask.ndim != 2 or mask.dtype != (torch.uint8 if torch.is_tensor(mask) else np.uint8) or (torch.is_tensor(mask) and mask.device.type != "cpu"):
                raise ValueError("an array mask must be uint8 [h, w] on the host, got %s %s" % (mask.dtype, tuple(mask.shape)))
            return "array", int(mask.shape[0]), int(mask.shape[1]), mask
        if isinstance(mask, dict) and "counts" in mask:
            h, w, counts = rle._parts(mask)
            return "rle", h, w, counts
        if isinstance(mask, dict) and "rings" in mask:
            h, w = polygon.validate(mask)
            return "polygon", h, w, list(mask["rings"])
        if isinstance(mask, (list, tuple)):
            raise ValueError("COCO's flat polygon lists are not accepted (no holes, no even-odd rule): exchange RLE instead")
        raise ValueError("expected a uint8 array, PNG bytes, an RLE dict or a polygon dict, got %r" % (type(mask).__name__,))
    except ValueError as e:
        raise ValueError("%s: %s" % (where, e)) from None


def mask_to_array(form):
    """the host decode of a `mask_form` result -> uint8 [h, w] numpy array of the mask's own values (array) or 0 / 255"""
    from . import polygon, rle
    kind, h, w, payload = form
    if kind == "array":
        return payload.numpy() if torch.is_tensor(payload) else payload
    if kind == "rle":
        return rle.decode({"size": [h, w], "counts": payload})
    return polygon._decode_general(payload, h, w)


class MaskSources:
    """The tables of one decode call on the host, in ONE contiguous block of bytes (`blob`, uint8) so that one copy uploads them:
    the mask-source table (hip.MaskSrc, one row per mask), the ring table (int64 [R, 3] of (mask, offset, length)), the vertices
    (int32 [V, 2]) and the RLE counts (uint32), each section 8-byte aligned.  `place(host_address, device_address)` tells where the
    block lies when a caller copied it elsewhere (EvalStaging); `upload(device)` makes a pinned copy and sends it with one
    asynchronous copy.  n, n_rle, n_polygon: rows; out_bytes: the end of the farthest slot."""

    def __init__(self, forms, slots):
        """forms: `mask_form` results of kind "rle" / "polygon" with h, w >= 1; slots: (dst_off, pitch) per mask"""
        from . import polygon, rle
        forms, slots = list(forms), list(slots)
        if len(forms) != len(slots) or not 1 <= len(forms) <= 65535:
            raise ValueError("MaskSources: need one slot per mask and 1 .. 65535 masks, got %d masks, %d slots" % (len(forms), len(slots)))
        counts, rings, verts, rows = [], [], [], []
        n_counts = n_rings = n_verts = 0
        self.out_bytes = 0
        for i, ((kind, h, w, payload), (dst_off, pitch)) in enumerate(zip(forms, slots)):
            dst_off, pitch = int(dst_off), int(pitch)
            if kind not in ("rle", "polygon") or h < 1 or w < 1:
                raise ValueError("MaskSources: mask %d must be an RLE or a polygon of positive size, got %r %d x %d" % (i, kind, h, w))
            if h * w >= rle.MAX_PIXELS or (kind == "polygon" and (h + 1) * (w + 1) > polygon.MAX_VERTICES):
                raise ValueError("MaskSources: mask %d is too large (%d x %d)" % (i, h, w))
            if pitch < w or pitch % 4 or pitch * h >= 2 ** 31 or dst_off < 0 or dst_off % 4:
                raise ValueError("MaskSources: slot %d needs a pitch that is a multiple of 4 and >= w and a non-negative offset that is "
                                 "a multiple of 4, got offset %d pitch %d for %d x %d" % (i, dst_off, pitch, h, w))
            self.out_bytes = max(self.out_bytes, dst_off + pitch * h)
            if kind == "rle":
                c = np.asarray(payload, np.int64)
                rows.append((dst_off, n_counts, pitch, h, w, c.size, hip.MASK_RLE))
                counts.append(c.astype(np.uint32))
                n_counts += c.size
            else:
                rows.append((dst_off, n_rings, pitch, h, w, len(payload), hip.MASK_POLYGON))
                for r in payload:
                    rings.append((i, n_verts, r.shape[0]))
                    verts.append(np.asarray(r, np.int32).reshape(-1, 2))
                    n_verts += r.shape[0]
                n_rings += len(payload)
        self.n = len(rows)
        self.n_rle = sum(1 for r in rows if r[6] == hip.MASK_RLE)
        self.n_polygon = self.n - self.n_rle
        self.n_counts, self.n_rings, self.n_vertices = n_counts, n_rings, n_verts
        up = lambda v: (v + 7) // 8 * 8
        self.rings_off = up(self.n * C.sizeof(hip.MaskSrc))
        self.vertices_off = self.rings_off + 24 * max(n_rings, 1)
        self.counts_off = self.vertices_off + 8 * max(n_verts, 1)
        self.blob = np.zeros(up(self.counts_off + 4 * max(n_counts, 1)), np.uint8)
        table = (hip.MaskSrc * self.n).from_buffer(self.blob)
        for t, (dst_off, pay_off, pitch, h, w, pay_len, kind) in zip(table, rows):
            t.dst_off, t.pay_off, t.pitch, t.h, t.w, t.pay_len, t.kind = dst_off, pay_off, pitch, h, w, pay_len, kind
        del table                                                          # (a ctypes view pins the array's buffer)
        if rings:
            self.blob[self.rings_off:self.rings_off + 24 * n_rings] = np.asarray(rings, np.int64).reshape(-1).view(np.uint8)
            self.blob[self.vertices_off:self.vertices_off + 8 * n_verts] = np.concatenate(verts).reshape(-1).view(np.uint8)
        if counts:
            self.blob[self.counts_off:self.counts_off + 4 * n_counts] = np.concatenate(counts).view(np.uint8)
        self.host_addr = self.dev_addr = None
        self._keep = None

    def place(self, host_addr, dev_addr, keep=None):
        """the block's bytes lie at `host_addr` (host) and, once the caller's copy has run, at `dev_addr` (device); both 8-byte aligned"""
        if host_addr % 8 or (dev_addr or 0) % 8:
            raise ValueError("MaskSources.place: both addresses must be 8-byte aligned")
        self.host_addr, self.dev_addr, self._keep = int(host_addr), None if dev_addr is None else int(dev_addr), keep
        return self

    def upload(self, device):
        """a pinned copy of the block and one asynchronous copy to `device` on the current stream"""
        pinned = torch.from_numpy(self.blob).pin_memory()
        dev = pinned.to(device, non_blocking=True)
        return self.place(pinned.data_ptr(), dev.data_ptr(), keep=(pinned, dev))


def desc_slots(descs, layout):
    """(offset, pitch) of every descriptor of `descs` (an EvalStaging): layout "out" = the prediction slots (out_off, what
    iou_batch / predict_batch write), "mask" = the ground-truth slots (mask_off)"""
    if layout not in ("out", "mask"):
        raise ValueError("desc_slots: layout must be 'out' or 'mask', got %r" % (layout,))
    return [(descs.descs[i].out_off if layout == "out" else descs.descs[i].mask_off, descs.descs[i].pitch) for i in range(descs.n)]


def decode_work(srcs, device, out=None):
    """the scratch of `decode_masks_batch` for these sources (per mask the run ends of an RLE or the bit plane of a polygon): `out`
    when it is large enough, a new int64 buffer otherwise.  Nothing has to be zeroed."""
    if not isinstance(srcs, MaskSources):
        raise ValueError("decode_work: srcs must be an evalpost.MaskSources, got %r" % (srcs,))
    words = (hip.load().cris_mask_decode_work_bytes(srcs.blob.ctypes.data_as(C.c_void_p), srcs.n) + 7) // 8
    if out is not None and out.numel() >= words:
        return out
    return torch.empty(words + words // 4, dtype=torch.int64, device=device)


def decode_masks_batch(srcs, out, work=None):
    """Decode every mask of `srcs` (a placed or uploaded MaskSources: RLE and polygon rows mixed) into the packed uint8 buffer `out`
    on the device: mask i becomes h rows of pitch bytes at its dst_off - 0 / 255 at x < w, 0 at w <= x < pitch, byte for byte what
    EvalStaging.pack writes for rle.decode / polygon.decode of it.  Nothing else of `out` is touched (not the gaps between slots, not
    the tail) and the payload is only read.  RLE rows: two launches (cris_rle_decode); polygon rows: one memset of `work` and two
    launches (cris_polygon_fill); none depends on the content, integers only - the same bytes on every run.  work: scratch from
    `decode_work` to reuse.  On the current stream; nothing is synchronised or read.  Returns `out`."""
    if not isinstance(srcs, MaskSources):
        raise ValueError("decode_masks_batch: srcs must be an evalpost.MaskSources, got %r" % (srcs,))
    if not torch.is_tensor(out) or out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous() or out.numel() < srcs.out_bytes:
        raise ValueError("decode_masks_batch: out must be a contiguous uint8 buffer that holds every slot (%d bytes)" % srcs.out_bytes)
    if out.device.type != "cuda":
        raise RuntimeError("evalpost runs on the GPU only (no CPU fallback)")
    if srcs.dev_addr is None:
        raise ValueError("decode_masks_batch: the sources are not on the device (MaskSources.upload, or an EvalStaging's upload)")
    if work is not None and (work.dtype != torch.int64 or not work.is_contiguous() or work.device != out.device):
        raise ValueError("decode_masks_batch: work must be a contiguous int64 buffer on the device of `out`")
    work = decode_work(srcs, out.device, work)
    host, dev = srcs.host_addr, srcs.dev_addr
    if srcs.n_rle:
        hip.call("cris_rle_decode", host, dev, srcs.n, dev + srcs.counts_off, max(srcs.n_counts, 1), ptr(work), 8 * work.numel(), ptr(out),
                 out.numel(), _stream())
    if srcs.n_polygon:
        hip.call("cris_polygon_fill", host, dev, srcs.n, dev + srcs.vertices_off, max(srcs.n_vertices, 1), host + srcs.rings_off,
                 dev + srcs.rings_off, max(srcs.n_rings, 1), 3, ptr(work), 8 * work.numel(), ptr(out), out.numel(), _stream())
    return out


def rle_decode_batch(rles, descs, out, layout="out", work=None):
    """The inverse of `rle_encode_batch` / `rle_collect`: rles[i] (an RLE dict) is decoded into descriptor i's slot of `out` (layout
    "out": out_off, "mask": mask_off; `descs`: an EvalStaging).  One small upload of the counts, then `decode_masks_batch`."""
    return _decode_for_descs("rle_decode_batch", "rle", rles, descs, out, layout, work)


def polygon_fill_batch(polys, descs, out, layout="out", work=None):
    """The inverse of `polygon_count_batch` / `polygon_collect`: polys[i] (a traced or simplified polygon dict) is filled even-odd
    into descriptor i's slot of `out`, as `rle_decode_batch` places an RLE."""
    return _decode_for_descs("polygon_fill_batch", "polygon", polys, descs, out, layout, work)


def _decode_for_descs(name, kind, masks, descs, out, layout, work):
    forms = [mask_form(m, "%s: mask %d" % (name, i)) for i, m in enumerate(masks)]
    if len(forms) != descs.n:
        raise ValueError("%s: %d masks for %d descriptors" % (name, len(forms), descs.n))
    for i, f in enumerate(forms):
        d = descs.descs[i]
        if f[0] != kind or (f[1], f[2]) != (d.h_out, d.w_out):
            raise ValueError("%s: mask %d must be a %s of %d x %d, got %s %d x %d" % (name, i, kind, d.h_out, d.w_out, f[0], f[1], f[2]))
    if not torch.is_tensor(out) or out.device.type != "cuda":
        raise RuntimeError("evalpost runs on the GPU only (no CPU fallback)")
    srcs = MaskSources(forms, desc_slots(descs, layout)).upload(out.device)
    return decode_masks_batch(srcs, out, work=work)
