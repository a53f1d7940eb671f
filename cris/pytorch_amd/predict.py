"""Referring segmentation of UNLABELED images: masks at the original size plus area, bounding box and confidence per expression.

    pred = Predictor(model, RecordPipeline(size, word_len, device, mode="test"), thr=0.35)
    out = pred.predict(images, expressions, images_per_batch=8, masks="host")
    out[i][j] -> Prediction(sentence, mask, area, box, score)

The reference has no such entry point: its `engine.inference` (engine/engine.py:146-215) needs a ground-truth mask per record and
does the last steps per expression on the host (cv2.warpAffine, threshold, numpy).  Here a batch is JPEG decode + letter-box on the
GPU (jpegdec, inputpipe), one visual pass per image (`segment` / `segment_expressions`), `evalpost.sigmoid_upsample` and ONE launch
of `evalpost.predict_batch` (csrc/evalpost.hip cris_predict_masks_batch): inverse warp of every expression to its image's size,
threshold, mask bytes, and integer (area, score, box) statistics in a device table.  Nothing but JPEG bytes and descriptors goes
up; the table of the whole call comes back once at the end, the masks once per batch.  Batching and padding follow
`evaluate.Evaluator.inference` (a short last image batch repeats its last image, the expression count is padded to a multiple of
8 by repeating the last expression), so one graph is captured per shape.

`components=evalpost.Components(keep="largest", min_area=N)` cleans every mask up on the device before its numbers are taken
(connected components: DESIGN.md 9b): the masks of a batch stay in a device buffer, `evalpost.label_components` and
`evalpost.filter_components` run on the stream, and the call returns ComponentPrediction - area, box and score of the KEPT pixels.

`smooth=evalpost.Smooth(open=R, close=R, fill_holes=True)` smooths every mask on the device right after the threshold (opening, closing,
hole filling: DESIGN.md 9b), before the clean-up; area, box and score are then those of the pixels finally set (ComponentPrediction).

`masks="rle"` ends that chain on the device too: the masks of a batch stay in an internal device buffer, `evalpost.rle_encode_batch`
finds their run-length transitions (csrc/rle.hip) and `Prediction.mask` is the COCO RLE dict of rle.py - a few hundred bytes per
mask cross to the host instead of the image-sized mask.  `masks="polygon"` does the same with polygons: `evalpost.polygon_count_batch`
/ `polygon_collect` trace the rings of every mask there (csrc/polygon.hip) and `Prediction.mask` is the polygon dict of polygon.py,
exact stair-step rings of pixel corners.  `coco_results` turns either result into the list a results file holds.

    python -m cris.pytorch_amd.predict --weights CKPT --config YAML --image F --expr "the left one" --out-prefix P [--keep largest]
                                       [--rle-json RESULTS.json] [--polygon-json RESULTS.json [--simplify EPS]] [--open R] [--close R] [--fill-holes] [--max-hole-area N]
"""
from collections import namedtuple

import numpy as np
import torch

from . import evalpost, polygon, rle

Prediction = namedtuple("Prediction", "sentence mask area box score")
Prediction.__doc__ = """sentence: the expression; mask: uint8 [h, w] of 0 / 255 at the image's own size (numpy array, CUDA tensor view, None
with masks="rle" the COCO RLE dict {"size": [h, w], "counts": bytes} of that mask, or with masks="polygon" its polygon dict
{"size", "rings", "holes"} of polygon.py: `masks`); area: pixels above the threshold;
box: (x0, y0, x1, y1) half-open, None when area == 0; score: the mean warped
probability over those pixels, score_q16 / (65536 * area) in float64 (each pixel's value rounded to 1 / 65536), 0.0 when area == 0"""

ComponentPrediction = namedtuple("ComponentPrediction", "sentence mask area box score n_components raw_area")
ComponentPrediction.__doc__ = """what `predict` returns with a `components` spec: sentence, mask, area, box, score as in Prediction but over
the KEPT pixels (mask: the filtered mask); n_components: connected components of the thresholded mask BEFORE filtering; raw_area: its
pixels before filtering (what Prediction.area would have been).  Nothing kept: area 0, box None, score 0.0"""

BatchPlan = namedtuple("BatchPlan", "lo n image_index index descs")
BatchPlan.__doc__ = """images lo .. lo + n of the call; image_index: the batch's images padded to images_per_batch by repeating the last
one; index: image (within the batch) of every expression, padded to a multiple of `multiple` by repeating the last one; descs:
(inverse or None, image within the batch, probability map, statistics row of the WHOLE call) per real expression"""

MASK_MODES = ("host", "device", "rle", None)
POLYGON_MODE = "polygon"    # the mode whose masks come back as polygon dicts (polygon.py); every other mode is in MASK_MODES


def _pad_to(n, multiple):
    return (n + multiple - 1) // multiple * multiple


def plan_predict(sents_per_image, images_per_batch=8, multiple=8, inverses=None):
    """Host arithmetic of a whole predict call: image i has sents_per_image[i] >= 1 expressions; the images are cut into batches
    of `images_per_batch` and each batch is planned as evaluate.plan_inference plans it.  Statistics rows run 0, 1, 2 ... over
    the expressions of the call in order; the padding (images and expressions) gets no descriptor.  `inverses`: optional 2x3
    matrices per image (param['inverse']) placed into the descriptors; None leaves the slot None (the matrices of a batch are
    known once its images are decoded).  Returns the list of BatchPlan."""
    counts = [int(k) for k in sents_per_image]
    if not counts or min(counts) < 1:
        raise ValueError("plan_predict: every image needs at least one expression")
    if images_per_batch < 1 or multiple < 1:
        raise ValueError("plan_predict: images_per_batch and multiple must be positive")
    if inverses is not None and len(inverses) != len(counts):
        raise ValueError("plan_predict: %d inverses for %d images" % (len(inverses), len(counts)))
    plans, row = [], 0
    for lo in range(0, len(counts), images_per_batch):
        part = counts[lo:lo + images_per_batch]
        n = len(part)
        index = [i for i, k in enumerate(part) for _ in range(k)]
        descs = [(None if inverses is None else inverses[lo + i], i, k, row + k) for k, i in enumerate(index)]
        row += len(index)
        plans.append(BatchPlan(lo, n, list(range(n)) + [n - 1] * (images_per_batch - n),
                               index + [index[-1]] * (_pad_to(len(index), multiple) - len(index)), descs))
    return plans


def _check_components(value, default):
    """the spec of one call: "default" -> the constructor's; None / a no-op spec -> None (host only)"""
    if isinstance(value, str) and value == "default":
        return default
    return evalpost.components_spec(value, "predict: components")


def _check_smooth(value, default):
    """the smoothing of one call: "default" -> the constructor's; None / a no-op spec -> None (host only)"""
    if isinstance(value, str) and value == "default":
        return default
    return evalpost.smooth_spec(value, "predict: smooth")


def _check_simplify(value, default, masks, where="predict"):
    """the Douglas-Peucker tolerance of one call: "default" -> the constructor's, which applies to masks="polygon" alone; None ->
    none; a value is checked (polygon.check_epsilon) and is valid only with masks="polygon".  Host only."""
    if isinstance(value, str) and value == "default":
        return default if isinstance(masks, str) and masks == POLYGON_MODE else None
    if value is None:
        return None
    polygon.check_epsilon(value)
    if not (isinstance(masks, str) and masks == POLYGON_MODE):
        raise ValueError("%s: simplify is valid only with masks='polygon', got masks=%r" % (where, masks))
    return float(value)


def _check_inputs(images, expressions, images_per_batch, masks):
    """-> (kind 'bytes' / 'array', expressions as lists); everything here is host-only"""
    if masks not in MASK_MODES and not (isinstance(masks, str) and masks == POLYGON_MODE):
        raise ValueError("predict: masks must be 'host', 'device', 'rle' or None, or 'polygon', got %r" % (masks,))
    if int(images_per_batch) < 1:
        raise ValueError("predict: images_per_batch must be positive")
    images, expressions = list(images), list(expressions)
    if not images:
        raise ValueError("predict: no images")
    if len(images) != len(expressions):
        raise ValueError("predict: %d images but %d expression entries" % (len(images), len(expressions)))
    exprs = []
    for i, e in enumerate(expressions):
        e = [e] if isinstance(e, str) else list(e) if isinstance(e, (list, tuple)) else None
        if not e or not all(isinstance(s, str) and s.strip() for s in e):
            raise ValueError("predict: expressions[%d] must be a non-empty str or a non-empty list of non-empty str" % i)
        exprs.append(e)
    is_bytes = [isinstance(im, (bytes, bytearray, memoryview)) for im in images]
    if all(is_bytes):
        return "bytes", images, exprs
    if any(is_bytes):
        raise ValueError("predict: images must be all JPEG bytes or all decoded arrays (one kind per call)")
    for i, im in enumerate(images):
        shape, dtype = getattr(im, "shape", None), getattr(im, "dtype", None)
        if shape is None or len(shape) != 3 or shape[2] != 3 or shape[0] < 1 or shape[1] < 1 or str(dtype) not in ("uint8", "torch.uint8"):
            raise ValueError("predict: images[%d] must be JPEG bytes or a uint8 RGB array / tensor [h, w, 3]" % i)
    return "array", images, exprs


class Predictor:
    """`Predictor(model, pipeline, thr=0.35, components=None, smooth=None, simplify=None)`: model - an InferenceRunner, the drop-in CRIS module in eval mode, or any callable
    `(img, word) -> logits [B, 1, h, w]`; when it offers `segment(img, word, image_index)` or `segment_expressions`, the visual
    encoder runs once per image, otherwise `model(img[index], word)` is called.  pipeline - a RecordPipeline in mode "test" (its
    preprocessor, tokenizer, word length and decode threads are used; no record is needed).  components - None or an
    evalpost.Components: the mask clean-up `predict` applies unless the call names another.  smooth - None or an evalpost.Smooth:
    the smoothing (open, close, fill holes) `predict` applies before that clean-up unless the call names another.  simplify - None
    or the Douglas-Peucker tolerance in pixels (a multiple of 0.25 in [0.25, 64]) `predict` applies to masks="polygon" results
    unless the call names another."""

    RING = 3            # descriptor staging buffers in flight (evaluate.Evaluator.RING)

    def __init__(self, model, pipeline, thr=0.35, components=None, smooth=None, simplify=None):
        if getattr(pipeline, "mode", None) != "test":
            raise ValueError("Predictor needs a RecordPipeline in mode 'test', got %r" % (getattr(pipeline, "mode", None),))
        thr = float(thr)
        if not 0.0 <= thr < float("inf"):
            raise ValueError("Predictor: thr must be finite and >= 0, got %r" % (thr,))
        self.model, self.pipe, self.thr = model, pipeline, thr
        self.components = evalpost.components_spec(components, "Predictor: components")
        self.smooth = evalpost.smooth_spec(smooth, "Predictor: smooth")
        self.simplify = None if simplify is None else polygon.check_epsilon(simplify) / 4.0
        self.smooth_info = None                                       # after a call with a Smooth spec: [total, 2] holes, pixels filled
        self.simplify_info = None                                     # after a call that simplified: (rings, vertices) traced, before the simplifier
        self.device = pipeline.device
        self._segment = getattr(model, "segment", None) or getattr(model, "segment_expressions", None)
        self._ring, self._turn = None, 0
        self._cc_masks = self._cc_labels = self._cc_work = None       # component clean-up scratch, reused across batches
        self._rle_runs = self._rle_work = None                        # run-length encoder buffers, reused across batches
        self._sm_work = None                                          # smoothing scratch (two bit planes), reused across batches
        self._pg_work = self._pg_buffers = None                       # polygon tracer buffers, reused across batches (masks="polygon" only)

    def _staging(self):
        if self._ring is None:          # (the first device allocation: after every argument check)
            self._ring = [evalpost.EvalStaging(self.device, mask_bytes=16) for _ in range(self.RING)]
        self._turn = (self._turn + 1) % self.RING
        return self._ring[self._turn]

    def _mask_buffer(self, st):
        """the internal mask buffer of a batch whose masks never leave the device as bytes"""
        if self._cc_masks is None or self._cc_masks.numel() < st.out_bytes:
            self._cc_masks = torch.empty(st.out_bytes + st.out_bytes // 4, dtype=torch.uint8, device=self.device)
        return self._cc_masks

    def _encode_rle(self, st, out):
        """the batch's masks in `out` as RLE dicts: the encoder on the stream, then the batch's read (totals, then the positions).
        The run buffer holds one word per mask byte, which no mask can exceed, so nothing is ever encoded twice."""
        if self._rle_runs is None or self._rle_runs.numel() < st.out_bytes:
            self._rle_runs = torch.empty(st.out_bytes + st.out_bytes // 4, dtype=torch.int32, device=self.device)
        self._rle_work = evalpost.rle_work(st, self.device, self._rle_work)
        runs, totals = evalpost.rle_encode_batch(out, st, runs=self._rle_runs, work=self._rle_work)
        return evalpost.rle_collect(runs, totals, st, masks_u8=out, work=self._rle_work)

    def _trace_polygons(self, st, out, simplify=None):
        """the batch's masks in `out` as polygon dicts: the count on the stream, the read of its totals, the trace sized from them
        and the read of the vertices and the ring table (evalpost.polygon_collect); no trace for a batch without foreground.
        simplify: the tolerance of the simplifier that follows the trace on the device, or None"""
        if self._pg_buffers is None:
            self._pg_buffers = evalpost.PolygonBuffers()
        self._pg_work = evalpost.polygon_work(st, self.device, self._pg_work)
        totals = evalpost.polygon_count_batch(out, st, work=self._pg_work)
        if simplify is None:
            return evalpost.polygon_collect(out, st, totals, work=self._pg_work, buffers=self._pg_buffers)
        got = evalpost.polygon_collect(out, st, totals, work=self._pg_work, buffers=self._pg_buffers, simplify=simplify)
        if self._pg_buffers.header is not None:                       # what the trace had found: the simplifier's header and the count's total
            self.simplify_info = (self.simplify_info[0] + int(self._pg_buffers.header[2]), self.simplify_info[1] + int(self._pg_buffers.header[4]))
        return got

    def _component_buffers(self, st, out):
        """the mask buffer of a batch that is cleaned up (out=None: an internal one that never leaves the device) and the label /
        work scratch, grown when a batch needs more and reused otherwise"""
        if out is None:
            out = self._mask_buffer(st)
        if self._cc_labels is None or self._cc_labels.numel() < st.out_bytes:
            self._cc_labels = torch.empty(st.out_bytes + st.out_bytes // 4, dtype=torch.int32, device=self.device)
        self._cc_work = evalpost.filter_work(st, self.device, self._cc_work)
        return out

    @torch.no_grad()
    def predict(self, images, expressions, images_per_batch=8, masks="host", components="default", smooth="default", simplify="default"):
        """images: JPEG bytes per image, or uint8 RGB [h, w, 3] arrays / tensors per image (one kind per call; JPEG files come
        back turned by their EXIF orientation, as cv2.imdecode returns them).  expressions: per image a str or a non-empty list
        of str.  masks: "host" (numpy arrays, one device-to-host copy per batch), "device" (views of one CUDA buffer per batch),
        "rle" (COCO run-length dicts, rle.py: the masks stay in an internal device buffer, are encoded there after any clean-up,
        and only the run positions are copied), "polygon" (polygon dicts, polygon.py: the same internal buffer, traced there after
        any clean-up, and only the ring vertices are copied) or None (statistics only: no mask buffer is allocated).  Returns a list per image
        of Prediction per expression.
        components: an evalpost.Components, None (no clean-up) or "default" (the constructor's).  With a spec every mask is
        labelled and filtered on the device before anything is read, the statistics are those of the kept pixels and the entries
        are ComponentPrediction; with masks=None the masks live in an internal device buffer and never reach the host.
        smooth: an evalpost.Smooth, None (no smoothing) or "default" (the constructor's).  With a spec every mask is opened, closed
        and has its holes filled in place on the device (in that order) right after the threshold, then labelled and filtered
        (`components`, or a filter that keeps everything): the entries are ComponentPrediction whose area, box and score are those
        of the pixels finally set - filled pixels count with their own probability, whatever the threshold - n_components counts the
        components of the smoothed mask and raw_area is the thresholded area before any of it; masks="rle" / "polygon" encode the final mask;
        `smooth_info` holds the [total, 2] holes and pixels filled per expression.
        simplify: a Douglas-Peucker tolerance in pixels (a multiple of 0.25 in [0.25, 64]), None (exact stair-step rings) or
        "default" (the constructor's, which applies to masks="polygon" alone).  Valid only with masks="polygon": the rings are
        simplified on the device right after the trace (csrc/simplify.hip; polygon.simplify states the definition) and
        `Prediction.mask` is the simplified dict {"size", "rings", "holes", "epsilon"}; area, box and score stay those of the mask itself."""
        from . import jpegdec
        spec = _check_components(components, self.components)
        sspec = _check_smooth(smooth, self.smooth)
        if sspec is not None and spec is None:
            spec = evalpost.Components()                               # keeps everything: labels, statistics of the final pixels
        kind, images, exprs = _check_inputs(images, expressions, images_per_batch, masks)
        eps = _check_simplify(simplify, self.simplify, masks)
        images_per_batch = int(images_per_batch)
        plans = plan_predict([len(e) for e in exprs], images_per_batch)
        total = sum(len(e) for e in exprs)
        table = evalpost.new_predict_stats(total, self.device)
        if spec is not None:
            ktable = evalpost.new_predict_stats(total, self.device)    # statistics of the kept pixels
            info = torch.zeros(total, 4, dtype=torch.int64, device=self.device)
        sinfo = None if sspec is None else torch.zeros(total, 4, dtype=torch.int64, device=self.device)
        kept = []                                                      # per expression: its mask (or None)
        self.simplify_info = None if eps is None else (0, 0)
        for b in plans:
            part = images[b.lo:b.lo + b.n]
            if kind == "bytes":
                part = jpegdec.decode_batch([bytes(f) for f in part], self.device, threads=self.pipe.threads)
            img, _, _, invs = self.pipe.pre(part, None)
            shapes = [(int(t.shape[0]), int(t.shape[1])) for t in part]
            if b.n < images_per_batch:                                 # short last batch: repeat its last image, one graph shape
                img = img[torch.tensor(b.image_index, device=self.device)]
            sents = [s for e in exprs[b.lo:b.lo + b.n] for s in e]
            K = len(sents)
            word = self.pipe.tok.tokenize(sents + [sents[-1]] * (len(b.index) - K), self.pipe.word_length, True)
            word = word.to(self.device, non_blocking=True)
            st = self._staging().pack_sizes(shapes, [(invs[i], i, k, row) for _, i, k, row in b.descs]).upload()
            if self._segment is not None:
                logits = self._segment(img, word, b.index)
            else:
                logits = self.model(img[torch.tensor(b.index, device=self.device)], word)
            probs = evalpost.sigmoid_upsample(logits, img.shape[-2], img.shape[-1])
            as_rle, as_polygon = masks == "rle", masks == "polygon"
            out = None if masks is None or as_rle or as_polygon else torch.empty(st.out_bytes, dtype=torch.uint8, device=self.device)
            if (as_rle or as_polygon) and spec is None:
                out = self._mask_buffer(st)
            if spec is not None:
                out = self._component_buffers(st, out)
            evalpost.predict_batch(probs, st, table, 0, self.thr, out_masks=out)
            if sspec is not None:
                if sspec.ops:
                    self._sm_work = evalpost.morph_work(st, self.device, self._sm_work)
                evalpost.smooth_batch(out, st, sspec, sinfo, 0, labels=self._cc_labels, work=self._sm_work, fwork=self._cc_work)
            if spec is not None:
                labels = evalpost.label_components(out, st, spec.connectivity, out=self._cc_labels)
                evalpost.filter_components(out, labels, st, spec, info, 0, probs=probs, stats=ktable, work=self._cc_work)
            if masks is None:
                kept += [None] * K
                continue
            if as_rle:
                kept += self._encode_rle(st, out)
                continue
            if as_polygon:
                kept += self._trace_polygons(st, out, eps)[:K]
                continue
            buf = out.cpu().numpy() if masks == "host" else out        # the batch's masks: one copy
            for k in range(K):
                d = st.descs[k]
                m = buf[d.out_off:d.out_off + d.pitch * d.h_out].reshape(d.h_out, d.pitch)[:, :d.w_out]
                kept.append(np.ascontiguousarray(m) if masks == "host" else m)
        self.smooth_info = None
        if sspec is not None:
            rows = torch.cat([ktable, info, table[:, :1], sinfo], 1).cpu().numpy()     # the call's one read
            self.smooth_info = evalpost.check_component_info(rows[:, 11:15])[:, :2].copy()
            return self._component_result(exprs, kept, rows[:, :11], smoothed=True)
        if spec is not None:
            return self._component_result(exprs, kept, torch.cat([ktable, info, table[:, :1]], 1).cpu().numpy())
        stats = table.cpu().numpy()                                    # the call's one read of the statistics
        result, k = [], 0
        for e in exprs:
            row = []
            for s in e:
                area, q16, x0, y0, x1, y1 = (int(v) for v in stats[k])
                row.append(Prediction(s, kept[k], area, (x0, y0, x1, y1) if area else None, q16 / (65536.0 * area) if area else 0.0))
                k += 1
            result.append(row)
        return result


    @staticmethod
    def _component_result(exprs, kept, rows, smoothed=False):
        """rows: [total, 11] = kept statistics (6), info (4), raw area - the call's one read, the error column checked here.
        smoothed: the labelled mask is the smoothed one, so raw_area is the thresholded area of the plain table and is not compared
        with the labelled foreground"""
        evalpost.check_component_info(rows[:, 6:10])
        result, k = [], 0
        for e in exprs:
            row = []
            for s in e:
                area, q16, x0, y0, x1, y1, n_comp, _, raw, _, raw_stats = (int(v) for v in rows[k])
                if smoothed:
                    raw = raw_stats
                elif raw != raw_stats:
                    raise RuntimeError("predict: the labelled foreground (%d pixels) is not the thresholded mask (%d)" % (raw, raw_stats))
                row.append(ComponentPrediction(s, kept[k], area, (x0, y0, x1, y1) if area else None,
                                               q16 / (65536.0 * area) if area else 0.0, n_comp, raw))
                k += 1
            result.append(row)
        return result


def coco_results(out, image_ids, expressions=True):
    """The entries of a COCO-style results file from what `predict(..., masks="rle")` or `masks="polygon"` returned: out[i][j]
    belongs to image_ids[i].  Per expression {"image_id", "sentence" (left out with expressions=False), "segmentation": the RLE
    with str counts, or for polygon results COCO's list of flat [x0, y0, x1, y1, ...] outer rings (polygon.to_coco: COCO polygons
    cannot express holes; either goes straight into json.dump), "bbox": [x, y, w, h] (COCO's form of Prediction.box; zeros for an empty mask), "area", "score"}.
    Host only."""
    out, image_ids = list(out), list(image_ids)
    if len(out) != len(image_ids):
        raise ValueError("coco_results: %d images but %d image ids" % (len(out), len(image_ids)))
    entries = []
    for image_id, preds in zip(image_ids, out):
        for p in preds:
            if not isinstance(p.mask, dict):
                raise ValueError("coco_results needs a result of predict(..., masks='rle'), got a mask of type %s" % type(p.mask).__name__)
            x0, y0, x1, y1 = p.box if p.box is not None else (0, 0, 0, 0)
            segmentation = polygon.to_coco(p.mask) if "rings" in p.mask else rle.to_json(p.mask)
            entry = {"image_id": image_id, "sentence": p.sentence, "segmentation": segmentation,
                     "bbox": [int(x0), int(y0), int(x1 - x0), int(y1 - y0)], "area": int(p.area), "score": float(p.score)}
            if not expressions:
                del entry["sentence"]
            entries.append(entry)
    return entries


class _WordHashTokenizer:
    """--synthetic only, where the CLIP merge list is not installed: the tokenizer's interface with deterministic word-hash ids
    (random weights attach no meaning to an id anyway)"""

    def tokenize(self, texts, context_length=77, truncate=False):
        texts = [texts] if isinstance(texts, str) else texts
        out = torch.zeros(len(texts), context_length, dtype=torch.long)
        for i, t in enumerate(texts):
            ids = [49406] + [1 + (sum(map(ord, w)) % 40000) for w in t.lower().split()][:context_length - 2] + [49407]
            out[i, :len(ids)] = torch.tensor(ids)
        return out


def _load_config(path):
    """the reference's yaml layout (config/refcoco/cris_r50.yaml: sections of key: value) flattened to one dict"""
    import yaml
    with open(path) as f:
        doc = yaml.safe_load(f)
    flat = {}
    for k, v in doc.items():
        if isinstance(v, dict):
            flat.update(v)
        else:
            flat[k] = v
    return flat


def main(argv=None):
    import argparse
    import os

    from PIL import Image

    from . import arch, records, tokenizer
    from .infer import InferenceRunner
    from .model.segmenter import head_spec_from_cfg
    ap = argparse.ArgumentParser(description="segment referring expressions in one image; writes PREFIX_<j>.png per expression")
    ap.add_argument("--weights", help="checkpoint with a reference-keyed 'state_dict' (not needed with --synthetic)")
    ap.add_argument("--config", help="the yaml the model was trained with (not needed with --synthetic)")
    ap.add_argument("--image", required=True, help="a JPEG file, or any image file Pillow opens")
    ap.add_argument("--expr", action="append", required=True, help="a referring expression; repeat for several")
    ap.add_argument("--out-prefix", help="write PREFIX_<j>.png per expression (required unless --rle-json or --polygon-json is given)")
    ap.add_argument("--rle-json", metavar="PATH", help="write the COCO-style results list (RLE segmentation, bbox, area, score per "
                    "expression) to PATH; the masks are encoded on the GPU")
    ap.add_argument("--polygon-json", metavar="PATH", help="write the COCO-style results list with polygon segmentation (outer rings "
                    "as flat vertex lists, bbox, area, score per expression) to PATH; the masks are traced on the GPU")
    ap.add_argument("--simplify", type=float, default=None, metavar="EPS", help="simplify the polygons of --polygon-json on the GPU (Douglas-Peucker, "
                    "tolerance EPS pixels: a multiple of 0.25 in [0.25, 64])")
    ap.add_argument("--image-id", default=None, help="the image_id of the --rle-json / --polygon-json entries (default: the image's file name)")
    ap.add_argument("--thr", type=float, default=0.35)
    ap.add_argument("--synthetic", nargs="?", const="r50", default=None, metavar="SPEC",
                    help="arch.synthetic_state_dict of r50 (default), r101 or tiny instead of --weights / --config")
    ap.add_argument("--size", type=int, default=None, help="network input size (default: the config's input_size, 416)")
    ap.add_argument("--keep", choices=evalpost.Components.KEEP, default="all",
                    help="connected-component clean-up of every mask: 'largest' keeps the largest component only")
    ap.add_argument("--min-area", type=int, default=0, metavar="N", help="drop components of fewer than N pixels")
    ap.add_argument("--connectivity", type=int, choices=(4, 8), default=8, help="pixels connect through edges (4) or edges and corners (8)")
    ap.add_argument("--open", type=int, default=0, metavar="R", help="open every mask by the (2 R + 1)-square first: removes specks and thin bridges")
    ap.add_argument("--close", type=int, default=0, metavar="R", help="then close it by the (2 R + 1)-square: fills pin-holes and narrow gaps")
    ap.add_argument("--fill-holes", action="store_true", help="then fill the holes: background that does not reach the image's frame")
    ap.add_argument("--max-hole-area", type=int, default=None, metavar="N", help="fill only holes of at most N pixels (with --fill-holes)")
    a = ap.parse_args(argv)
    try:
        spec = evalpost.Components(a.keep, a.min_area, a.connectivity)
        smooth = evalpost.Smooth(a.open, a.close, a.fill_holes, a.max_hole_area)
    except ValueError as e:
        ap.error(str(e))
    if not a.out_prefix and not a.rle_json and not a.polygon_json:
        ap.error("one of --out-prefix, --rle-json and --polygon-json is required")
    if a.simplify is not None:
        if not a.polygon_json:
            ap.error("--simplify is valid only with --polygon-json")
        try:
            polygon.check_epsilon(a.simplify)
        except ValueError as e:
            ap.error(str(e))
    if not torch.cuda.is_available():
        raise SystemExit("predict needs a GPU (there is no CPU fallback)")
    dev = torch.device("cuda:0")
    if a.synthetic:
        clip, head = arch.specs_by_name(a.synthetic)
        sd, size = arch.synthetic_state_dict(clip, head, 0), a.size or (96 if a.synthetic == "tiny" else 416)
    else:
        if not a.weights or not a.config:
            raise SystemExit("--weights and --config are required without --synthetic")
        cfg = _load_config(a.config)
        ck = torch.load(a.weights, map_location="cpu")
        sd = ck.get("state_dict", ck)
        sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
        clip = arch.clip_spec_from_state_dict({k[len("backbone."):]: v for k, v in sd.items() if k.startswith("backbone.")})
        head, size = head_spec_from_cfg(cfg), a.size or int(cfg.get("input_size", 416))
    tok = tokenizer.BPETokenizer() if tokenizer.default_merges_path() else None
    if tok is None:
        if not a.synthetic:
            raise SystemExit("the CLIP merge list (bpe_simple_vocab_16e6.txt.gz) was not found: see tokenizer.default_merges_path")
        tok = _WordHashTokenizer()
    pipe = records.RecordPipeline(size, head.word_len, dev, mode="test", tokenizer=tok)
    runner = InferenceRunner(clip, head, sd, dev, use_graph=False)
    with open(a.image, "rb") as f:
        data = f.read()
    image = data if data[:2] == b"\xff\xd8" else np.array(Image.open(a.image).convert("RGB"))
    predictor = Predictor(runner, pipe, thr=a.thr, components=spec, smooth=smooth)
    if a.rle_json:
        import json
        encoded = predictor.predict([image], [a.expr], images_per_batch=1, masks="rle")
        os.makedirs(os.path.dirname(os.path.abspath(a.rle_json)), exist_ok=True)
        with open(a.rle_json, "w") as f:
            json.dump(coco_results(encoded, [a.image_id if a.image_id is not None else os.path.basename(a.image)]), f)
        print("%s\t%d expressions\t%d bytes of RLE" % (a.rle_json, len(encoded[0]), sum(len(p.mask["counts"]) for p in encoded[0])))
        if not a.out_prefix and not a.polygon_json:
            return encoded[0]
    if a.polygon_json:
        import json
        traced = predictor.predict([image], [a.expr], images_per_batch=1, masks="polygon", simplify=a.simplify)
        os.makedirs(os.path.dirname(os.path.abspath(a.polygon_json)), exist_ok=True)
        with open(a.polygon_json, "w") as f:
            json.dump(coco_results(traced, [a.image_id if a.image_id is not None else os.path.basename(a.image)]), f)
        nrings, nverts = sum(len(p.mask["rings"]) for p in traced[0]), sum(len(r) for p in traced[0] for r in p.mask["rings"])
        if a.simplify is None:
            print("%s\t%d expressions\t%d rings of %d vertices" % (a.polygon_json, len(traced[0]), nrings, nverts))
        else:
            before = predictor.simplify_info
            print("%s\t%d expressions\tepsilon %g\t%d rings of %d vertices before\t%d rings of %d vertices after"
                  % (a.polygon_json, len(traced[0]), a.simplify, before[0], before[1], nrings, nverts))
        if not a.out_prefix:
            return traced[0]
    out = predictor.predict([image], [a.expr], images_per_batch=1, masks="host")[0]
    os.makedirs(os.path.dirname(os.path.abspath(a.out_prefix)), exist_ok=True)
    for j, p in enumerate(out):
        path = "%s_%d.png" % (a.out_prefix, j)
        Image.fromarray(p.mask, "L").save(path)
        extra = "\tcomponents %d\traw area %d" % (p.n_components, p.raw_area) if isinstance(p, ComponentPrediction) else ""
        print("%s\t%r\tbox %s\tarea %d\tscore %.4f%s" % (path, p.sentence, p.box, p.area, p.score, extra))
    return out


if __name__ == "__main__":
    main()
