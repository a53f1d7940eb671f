"""A whole dataset split through the model on the GPU - the bodies of the reference's `validate` and `inference`
(reference engine/engine.py:90-143, :146-215) behind the same results: `(iou, prec)` with `prec` keyed 'Pr@50' ... 'Pr@90'.

    validate:  first sentence of every record, batches of `batch_size`                         engine.py:95-124
    inference: every sentence of every record; the images of a batch share one visual pass      engine.py:152-190
    metrics:   iou_i = inter / (union + 1e-6), IoU = mean, Pr@X = mean(iou_i > X)               engine.py:125-143, :199-215

Per batch: RecordPipeline (JPEG decode + letter-box on the GPU), the model, `evalpost.sigmoid_upsample`, and ONE launch of
`evalpost.iou_batch` that warps every prediction back to its original size, thresholds it and adds (intersection, union) to the
sample's row of a device table.  The masks come from the records' own `mask` bytes (tools/folder2lmdb.py:49-50 stores the file
`mask_dir` names), packed as uint8 next to the descriptors in a pinned buffer: one asynchronous copy per batch.  The table is
read ONCE, after the last batch - no batch waits for the host (a `visualize` callback needs each batch's result and does wait).

`Evaluator.sweep` is either pass at many thresholds at once (`evalpost.iou_sweep_batch`, a [n, T, 2] table): `sweep_metrics` turns
the table into a `SweepResult` - IoU, overall IoU and Pr@X per threshold, the best threshold - whose column t equals the pass at thr=t.

`validate` / `inference` take `components=evalpost.Components(...)`: every predicted mask is cleaned up on the device (connected
components) before it is counted - `iou_batch` writes the masks, `label_components` / `filter_components` rewrite them
in place and `evalpost.mask_iou_batch` adds the counts of the filtered masks to the pass's table.

`validate` / `inference` take `boundary=True` or `evalpost.Boundary(...)`: next to the mask figures the pass counts Boundary IoU
(Cheng et al., CVPR 2021) - the masks the batch wrote (filtered when `components` is given) and the ground truth are eroded on the
device and `evalpost.boundary_iou_batch` adds (intersection, union) of the two boundaries to a second table, read with the first;
`boundary_counts`, `boundary_per_sample`, `boundary_iou` and `boundary_prec` hold the result (`metrics` of that table).

`validate` / `inference` take `smooth=evalpost.Smooth(...)`: every predicted mask is opened, closed and has its holes filled on the
device (in that order, before `components`) and the final masks are counted; the ground truth is never smoothed; `smooth_info`
holds the holes and pixels filled per sample.

A record's `mask` may also be a COCO RLE or a polygon dict (evalpost.mask_form): such ground truth goes up encoded and is decoded
on the device before the first kernel that reads it; records with PNG bytes take the path they always took.  `score_results` scores
two sequences of masks in any of those forms without a model - the same integer tables, read once.
"""
import math

import numpy as np
import torch

from . import evalpost, pngdec

PR_KEYS = tuple("Pr@%d" % (t * 10) for t in range(5, 10))


def pr_thresholds():
    """the reference's `torch.arange(0.5, 1.0, 0.1)`: FLOAT32 values, which its float64-tensor > float32-scalar comparison
    widens to double (0.6f = 0.60000002384..., so an IoU of exactly 0.6 does not count for Pr@60)"""
    return [float(t) for t in torch.arange(0.5, 1.0, 0.1)]


def metrics(counts):
    """counts: [n, 2] integers (intersection, union) per sample -> (iou, prec, per_sample) as the reference computes them on
    the host in float64 (engine.py:123-143): iou_i = inter / (union + 1e-6), iou = mean(iou_i), prec['Pr@X'] =
    mean(iou_i > X) with the float32 thresholds of pr_thresholds() (the reference's `.float().mean()`: a float32 quotient)."""
    c = np.asarray(counts, dtype=np.float64).reshape(-1, 2)
    if c.shape[0] == 0:
        raise ValueError("metrics: no samples")
    per = c[:, 0] / (c[:, 1] + 1e-6)
    n = np.float32(per.shape[0])
    prec = {k: float(np.float32(int((per > t).sum())) / n) for k, t in zip(PR_KEYS, pr_thresholds())}
    return float(per.mean()), prec, per


def overall_iou(counts):
    """counts: [n, 2] integers -> sum(inter) / (sum(union) + 1e-6) in float64: the cumulative ('overall') IoU of the split, the
    second figure RefCOCO papers report next to the mean of the per-sample IoUs"""
    c = np.asarray(counts, dtype=np.float64).reshape(-1, 2)
    if c.shape[0] == 0:
        raise ValueError("overall_iou: no samples")
    return float(c[:, 0].sum() / (c[:, 1].sum() + 1e-6))


def sweep_thresholds():
    """the default grid of a threshold sweep: the 19 float32 values 0.05, 0.10, ... 0.95 (0.35, the reference's cut, is one)"""
    return np.array([i / 20 for i in range(1, 20)], dtype=np.float32)


class SweepResult:
    """What `sweep_metrics` returns: `thresholds` float32 [T]; `iou` [T] (mean of the per-sample IoUs), `overall_iou` [T] and
    `prec[key]` [T] as float64 arrays, `per_sample` [n, T]; entry i of each is the figure at thresholds[i]."""

    def __init__(self, thresholds, iou, overall, prec, per_sample):
        self.thresholds, self.iou, self.overall_iou, self.prec, self.per_sample = thresholds, iou, overall, prec, per_sample

    def _metric(self, metric):
        if metric == "iou":
            return self.iou
        if metric == "overall_iou":
            return self.overall_iou
        if metric in self.prec:
            return self.prec[metric]
        raise ValueError("SweepResult: metric must be 'iou', 'overall_iou' or one of %s" % (PR_KEYS,))

    def best(self, metric="iou"):
        """(threshold, value) of the largest `metric`; the lowest threshold wins a tie"""
        v = self._metric(metric)
        i = int(np.argmax(v))                                      # (the first maximum; thresholds ascend)
        return float(self.thresholds[i]), float(v[i])

    def at(self, thr):
        """(iou, prec) at the threshold whose float32 value is float32(thr) - what `validate` / `inference` return at that thr"""
        hit = np.nonzero(self.thresholds == np.float32(thr))[0]
        if hit.size == 0:
            raise KeyError("SweepResult: %r is not one of the swept thresholds" % (thr,))
        i = int(hit[0])
        return float(self.iou[i]), {k: float(v[i]) for k, v in self.prec.items()}


def sweep_metrics(counts, thresholds):
    """counts: [n, T, 2] integers (intersection, union) per sample and threshold, thresholds: the T ascending values -> SweepResult.
    Column i goes through `metrics` itself, so entry i of iou / prec / per_sample is what `metrics(counts[:, i])` returns."""
    thr = np.asarray(thresholds, dtype=np.float64).astype(np.float32)
    c = np.asarray(counts)
    if thr.ndim != 1 or thr.shape[0] == 0 or not (np.isfinite(thr).all() and (np.diff(thr) > 0).all()):
        raise ValueError("sweep_metrics: thresholds must be a non-empty, finite, strictly increasing list")
    if c.ndim != 3 or c.shape[1] != thr.shape[0] or c.shape[2] != 2:
        raise ValueError("sweep_metrics: counts must be [n, T, 2] with T = len(thresholds)")
    if c.shape[0] == 0:
        raise ValueError("sweep_metrics: no samples")
    cols = [metrics(c[:, i]) for i in range(thr.shape[0])]
    return SweepResult(thr, np.array([m[0] for m in cols], np.float64), np.array([overall_iou(c[:, i]) for i in range(thr.shape[0])], np.float64),
                       {k: np.array([m[1][k] for m in cols], np.float64) for k in PR_KEYS}, np.stack([m[2] for m in cols], 1))


def shard_indices(n, rank, world):
    """the indices `DistributedSampler(range(n), world, rank, shuffle=False)` yields: the list padded by wrapping around to a
    multiple of `world`, then every world-th entry from `rank` on (so the gathered metrics count the wrapped samples twice,
    as the reference's do)"""
    if not 0 <= rank < world or n <= 0:
        raise ValueError("shard_indices: need n > 0 and 0 <= rank < world")
    idx = list(range(n))
    total = math.ceil(n / world) * world
    pad = total - n
    idx += (idx * math.ceil(pad / n))[:pad]
    return idx[rank:total:world]


def gather_counts(counts, group=None):
    """`concat_all_gather` of the per-rank count tables (rank order, duplicates included) when a process group is given or
    torch.distributed is initialised; otherwise `counts` itself.  counts: CPU integer tensor [n, 2], n equal on every rank
    (shard_indices)."""
    import torch.distributed as dist
    if group is None and not (dist.is_available() and dist.is_initialized()):
        return counts
    world = dist.get_world_size(group)
    if world == 1:
        return counts
    dev = "cuda" if "nccl" in str(dist.get_backend(group)).lower() else "cpu"
    mine = counts.to(dev).contiguous()
    parts = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(parts, mine, group=group)
    return torch.cat(parts, 0).cpu()


def _pad_to(n, multiple):
    return (n + multiple - 1) // multiple * multiple


def plan_validate(masks, inverses, row0=0):
    """(masks, descriptors) of one validate batch for EvalStaging.pack: sample b reads probability map b and its own mask and
    counts into row row0 + b.  A padded batch passes its REAL samples only: padding gets no descriptor."""
    return masks, [(inv, b, b, row0 + b) for b, inv in enumerate(inverses)]


def plan_inference(masks, inverses, sents_per_image, multiple=8):
    """One inference batch: image i has sents_per_image[i] expressions.  Returns (image index of every expression padded to a
    multiple of `multiple` by repeating the last one, masks, descriptors): expression k reads map k, the ONE mask of its image
    and counts into row k; the padding gets no descriptor."""
    index = [i for i, k in enumerate(sents_per_image) for _ in range(k)]
    descs = [(inverses[i], i, k, k) for k, i in enumerate(index)]
    return index + [index[-1]] * (_pad_to(len(index), multiple) - len(index)), masks, descs


class ScoreResult:
    """What `score_results` returns: `iou` (mean of the per-sample IoUs), `prec` (Pr@50 ... Pr@90), `overall_iou`, `per_sample` [n]
    and the integer `counts` [n, 2] they come from (`metrics` / `overall_iou` of that table); with `boundary` also `boundary_iou`,
    `boundary_prec`, `boundary_per_sample`, `boundary_counts` (None otherwise)."""

    def __init__(self, counts, boundary_counts=None):
        self.counts = counts
        self.iou, self.prec, self.per_sample = metrics(counts)
        self.overall_iou = overall_iou(counts)
        self.boundary_counts = boundary_counts
        self.boundary_iou = self.boundary_prec = self.boundary_per_sample = None
        if boundary_counts is not None:
            self.boundary_iou, self.boundary_prec, self.boundary_per_sample = metrics(boundary_counts)


_IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def score_results(predictions, ground_truth, device, boundary=None, batch=64):
    """Score masks against masks without a model -> ScoreResult: IoU, Pr@50 ... Pr@90 and overall IoU of predictions[i] against
    ground_truth[i], the figures `Evaluator` reports, from a results file or any other source of masks.
    predictions, ground_truth: two equally long sequences; every entry in any form `evalpost.mask_form` takes - a uint8 [h, w]
    array, PNG bytes, an RLE dict (counts as str, bytes or list: the "segmentation" of a results JSON written from
    predict(..., masks="rle") goes in as it is), a traced or simplified polygon dict, or a predict.Prediction holding one of them.
    COCO's flat [x0, y0, ...] polygon lists are NOT accepted: polygon.to_coco drops holes and the "epsilon" marker and COCO fills such
    lists as a union, not even-odd - exchange RLE.
    Per batch of `batch` pairs both sides are decoded on the device into the two packed layouts (evalpost.decode_masks_batch:
    predictions at out_off, ground truth at mask_off; arrays are packed on the host and uploaded), `evalpost.mask_iou_batch` adds
    (intersection, union) to an integer table and, with boundary (True or an evalpost.Boundary), `boundary_iou_batch` the Boundary
    IoU counts to a second one; the tables are read once, at the end.  A malformed entry or a pair of different sizes raises
    ValueError naming its index before any device work for its batch."""
    bspec = evalpost.boundary_spec(boundary, "score_results: boundary")
    preds, gts = list(predictions), list(ground_truth)
    if len(preds) != len(gts) or not preds:
        raise ValueError("score_results: need two equally long, non-empty sequences, got %d predictions and %d ground-truth masks" % (len(preds), len(gts)))
    if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) or not 1 <= batch <= 65535:
        raise ValueError("score_results: batch must be an integer in 1 .. 65535, got %r" % (batch,))
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("evalpost runs on the GPU only (no CPU fallback)")
    total = len(preds)
    tables = torch.zeros(2 if bspec is not None else 1, total, 2, dtype=torch.int32, device=device)
    ring = [evalpost.EvalStaging(device) for _ in range(2)]
    out = work = bwork = None
    for lo in range(0, total, batch):
        pf = [evalpost.mask_form(m, "score_results: prediction %d" % (lo + i)) for i, m in enumerate(preds[lo:lo + batch])]
        gf = [evalpost.mask_form(m, "score_results: ground truth %d" % (lo + i)) for i, m in enumerate(gts[lo:lo + batch])]
        for i, (p, g) in enumerate(zip(pf, gf)):
            if (p[1], p[2]) != (g[1], g[2]) or p[1] < 1 or p[2] < 1:
                raise ValueError("score_results: pair %d: the prediction is %d x %d, the ground truth %d x %d (both must be one positive size)"
                                 % (lo + i, p[1], p[2], g[1], g[2]))
        st = ring[(lo // batch) % 2].pack_encoded(gf, [(_IDENTITY, i, 0, i) for i in range(len(gf))]).upload()
        work = st.decode(work)
        slots = evalpost.desc_slots(st, "out")
        arrays = [i for i, p in enumerate(pf) if p[0] == "array"]
        if arrays:                                                 # packed on the host in the out_off layout, one copy
            buf = torch.zeros(st.out_bytes, dtype=torch.uint8).pin_memory()
            view = buf.numpy()
            for i in arrays:
                (off, pitch), (_, h, w, m) = slots[i], pf[i]
                view[off:off + pitch * h].reshape(h, pitch)[:, :w] = m.numpy() if torch.is_tensor(m) else m
            out = buf.to(device, non_blocking=True)
        elif out is None or out.numel() < st.out_bytes:
            out = torch.empty(st.out_bytes + st.out_bytes // 4, dtype=torch.uint8, device=device)
        enc = [i for i, p in enumerate(pf) if p[0] != "array"]
        if enc:
            srcs = evalpost.MaskSources([pf[i] for i in enc], [slots[i] for i in enc]).upload(device)
            work = evalpost.decode_work(srcs, device, work)
            evalpost.decode_masks_batch(srcs, out, work=work)
        evalpost.mask_iou_batch(out, st, st.masks, tables[0], lo)
        if bspec is not None:
            bwork = evalpost.boundary_work(st, device, bwork)
            evalpost.boundary_iou_batch(out, st, st.masks, evalpost.boundary_radii(st, bspec), tables[1], lo, work=bwork)
    read = tables.cpu().numpy()                                    # the call's one read
    return ScoreResult(read[0], read[1] if bspec is not None else None)


class Evaluator:
    """`Evaluator(model, pipeline, thr=0.35)`: model - any callable `(img, word) -> logits [B, 1, h, w]` (an InferenceRunner, the
    drop-in CRIS module in eval mode); when it also offers `segment(img, word, image_index)` or `segment_expressions`, `inference`
    runs the visual encoder once per image.  pipeline - a RecordPipeline in mode "val" (validate) or "test" (inference).
    `records` is anything indexable that yields record dicts (records.LmdbRecords, a list).  After a pass `per_sample` holds
    this process's IoUs and `counts` its (intersection, union) table."""

    RING = 3            # staging buffers in flight: a batch's host packing overlaps the copies of the two before it

    def __init__(self, model, pipeline, thr=0.35):
        self.model, self.pipe, self.thr = model, pipeline, float(thr)
        self.device = pipeline.device
        self._segment = getattr(model, "segment", None) or getattr(model, "segment_expressions", None)
        self._ring = [evalpost.EvalStaging(self.device) for _ in range(self.RING)]
        self._turn = 0
        self.per_sample = self.counts = self.sweep_counts = self.component_info = None
        self._cc_masks = self._cc_labels = self._cc_work = self._cc_counts = None      # component clean-up scratch, reused across batches
        self.boundary_counts = self.boundary_per_sample = self.boundary_iou = self.boundary_prec = None
        self._bd_masks = self._bd_work = None                      # boundary scratch (the batch's masks, the bit planes), likewise
        self.smooth_info = None
        self._sm_work = None                                       # smoothing scratch (two bit planes), likewise

    def _staging(self):
        self._turn = (self._turn + 1) % self.RING
        return self._ring[self._turn]

    @staticmethod
    def _masks(recs, params):
        masks = [pngdec.decode_gray(r["mask"]) for r in recs]
        for m, p in zip(masks, params):
            if tuple(m.shape) != tuple(int(v) for v in p["ori_size"]):
                raise ValueError("record %s: mask is %s, image %s" % (p["mask_dir"], tuple(m.shape), tuple(p["ori_size"])))
        return masks

    def _ground_truth(self, recs, params):
        """-> (masks, encoded).  Records whose `mask` is PNG bytes, all of them: (`_masks`, False) - the host decode and the path of
        every pass so far.  Otherwise (`evalpost.mask_form` of every record's mask, True): RLE and polygon ground truth stays encoded
        for the device, a PNG among them is decoded on the host; the size check against `ori_size` is the same."""
        if all(isinstance(r["mask"], (bytes, bytearray, memoryview)) for r in recs):
            return self._masks(recs, params), False
        forms = [evalpost.mask_form(r["mask"], "record %s" % p["mask_dir"]) for r, p in zip(recs, params)]
        for f, p in zip(forms, params):
            if (f[1], f[2]) != tuple(int(v) for v in p["ori_size"]):
                raise ValueError("record %s: mask is %s, image %s" % (p["mask_dir"], (f[1], f[2]), tuple(int(v) for v in p["ori_size"])))
        return forms, True

    def _upload(self, masks, descs, encoded):
        """the batch's staging, packed and uploaded; encoded ground truth is decoded into its slots on the current stream, before
        any kernel that reads `st.masks` is issued"""
        if not encoded:
            return self._staging().pack(masks, descs).upload()
        st = self._staging().pack_encoded(masks, descs).upload()
        self._dec_work = st.decode(getattr(self, "_dec_work", None))
        return st

    def _clean_counts(self, spec, probs, st, table, row0, info, out=None, sspec=None, sinfo=None):
        """one batch with a Components and / or a Smooth spec: iou_batch writes the masks (its own counts go to a scratch table), the
        smoothing (open, close, fill holes) and then the filter rewrite them in place, mask_iou_batch adds the final masks' counts to
        `table`.  The ground truth is never touched.  out=None: an internal, reused mask buffer."""
        if out is None:
            if self._cc_masks is None or self._cc_masks.numel() < st.out_bytes:
                self._cc_masks = torch.empty(st.out_bytes + st.out_bytes // 4, dtype=torch.uint8, device=self.device)
            out = self._cc_masks
        if self._cc_labels is None or self._cc_labels.numel() < st.out_bytes:
            self._cc_labels = torch.empty(st.out_bytes + st.out_bytes // 4, dtype=torch.int32, device=self.device)
        if self._cc_counts is None or self._cc_counts.shape[0] < table.shape[0] - row0:
            self._cc_counts = torch.zeros(table.shape[0] - row0, 2, dtype=torch.int32, device=self.device)
        self._cc_work = evalpost.filter_work(st, self.device, self._cc_work)
        evalpost.iou_batch(probs, st, st.masks, self._cc_counts, 0, self.thr, out_masks=out)
        if sspec is not None:
            if sspec.ops:
                self._sm_work = evalpost.morph_work(st, self.device, self._sm_work)
            evalpost.smooth_batch(out, st, sspec, sinfo, row0, labels=self._cc_labels, work=self._sm_work, fwork=self._cc_work)
        if spec is not None:
            labels = evalpost.label_components(out, st, spec.connectivity, out=self._cc_labels)
            evalpost.filter_components(out, labels, st, spec, info, row0, work=self._cc_work)
        evalpost.mask_iou_batch(out, st, st.masks, table, row0)
        return out

    def _boundary_masks(self, st):
        """the internal, reused buffer a batch's masks are written to when only the boundary counts need them"""
        if self._bd_masks is None or self._bd_masks.numel() < st.out_bytes:
            self._bd_masks = torch.empty(st.out_bytes + st.out_bytes // 4, dtype=torch.uint8, device=self.device)
        return self._bd_masks

    def _boundary_counts(self, bspec, masks, st, btable, row0):
        """one batch with a Boundary spec: `masks` (what the batch wrote, filtered or not) against the staging's ground truth"""
        self._bd_work = evalpost.boundary_work(st, self.device, self._bd_work)
        evalpost.boundary_iou_batch(masks, st, st.masks, evalpost.boundary_radii(st, bspec), btable, row0, work=self._bd_work)

    def _finish_boundary(self, btable, n, group, gather):
        """the pass's read of the boundary table (None: a pass without the spec), after the counts'"""
        self.boundary_counts = self.boundary_per_sample = self.boundary_iou = self.boundary_prec = None
        if btable is None:
            return
        counts = btable[:n].cpu()
        if gather:
            counts = gather_counts(counts, group)
        self.boundary_counts = counts.numpy()
        self.boundary_iou, self.boundary_prec, self.boundary_per_sample = metrics(self.boundary_counts)

    def _finish_components(self, info, n):
        """the pass's read of the component table (after the counts'): raises when an error column is set"""
        self.component_info = evalpost.check_component_info(info[:n].cpu().numpy())

    def _finish_smooth(self, sinfo, n):
        """the pass's read of the hole table (None: a pass without the spec): [n, 2] holes and pixels filled per sample"""
        self.smooth_info = None
        if sinfo is not None:
            self.smooth_info = evalpost.check_component_info(sinfo[:n].cpu().numpy())[:, :2].copy()

    def _finish(self, table, n, group):
        counts = gather_counts(table[:n].cpu(), group)             # the pass's one host read
        iou, prec, per = metrics(counts.numpy())
        self.counts = counts.numpy()
        self.per_sample = per
        return iou, prec

    @torch.no_grad()
    def validate(self, records, indices=None, batch_size=32, group=None, components=None, boundary=None, smooth=None):
        """components: None or an evalpost.Components - clean every predicted mask up before it is counted (`component_info`
        then holds the [n, 4] table of evalpost.INFO_FIELDS per sample).  boundary: None, True or an evalpost.Boundary - also
        count Boundary IoU of the (cleaned) masks: `boundary_iou`, `boundary_prec`, `boundary_per_sample`, `boundary_counts`;
        the return value stays (iou, prec) of the masks.  smooth: None or an evalpost.Smooth - open, close and fill the holes of
        every predicted mask on the device before `components` and before anything is counted (`smooth_info` then holds the
        [n, 2] holes and pixels filled per sample); the ground truth is never smoothed."""
        spec = evalpost.components_spec(components, "validate: components")
        bspec = evalpost.boundary_spec(boundary, "validate: boundary")
        sspec = evalpost.smooth_spec(smooth, "validate: smooth")
        if self.pipe.mode != "val":
            raise ValueError("validate needs a RecordPipeline in mode 'val'")
        indices = list(range(len(records))) if indices is None else [int(i) for i in indices]
        if not indices:
            raise ValueError("validate: no records")
        table = torch.zeros(len(indices), 2, dtype=torch.int32, device=self.device)
        info = None if spec is None else torch.zeros(len(indices), 4, dtype=torch.int64, device=self.device)
        btable = None if bspec is None else torch.zeros(len(indices), 2, dtype=torch.int32, device=self.device)
        sinfo = None if sspec is None else torch.zeros(len(indices), 4, dtype=torch.int64, device=self.device)
        for lo in range(0, len(indices), batch_size):
            recs = [records[i] for i in indices[lo:lo + batch_size]]
            img, word, params = self.pipe(recs)
            n = len(recs)
            if n < batch_size:                                     # short last batch: repeat its last sample, one graph shape
                rep = torch.tensor(list(range(n)) + [n - 1] * (batch_size - n), device=self.device)
                img, word = img[rep], word[rep]
            masks, encoded = self._ground_truth(recs, params)
            st = self._upload(*plan_validate(masks, [p["inverse"] for p in params]), encoded)
            probs = evalpost.sigmoid_upsample(self.model(img, word), img.shape[-2], img.shape[-1])
            if spec is None and sspec is None:
                out = None if bspec is None else self._boundary_masks(st)
                evalpost.iou_batch(probs, st, st.masks, table, lo, self.thr, out_masks=out)
            else:
                out = self._clean_counts(spec, probs, st, table, lo, info, sspec=sspec, sinfo=sinfo)
            if bspec is not None:
                self._boundary_counts(bspec, out, st, btable, lo)
        result = self._finish(table, len(indices), group)
        self._finish_boundary(btable, len(indices), group, True)
        self._finish_smooth(sinfo, len(indices))
        if spec is not None:
            self._finish_components(info, len(indices))
        return result

    @torch.no_grad()
    def inference(self, records, indices=None, images_per_batch=8, visualize=None, components=None, boundary=None, smooth=None):
        """components: as for `validate`; a `visualize` callback then receives the FILTERED masks and their IoUs.  boundary: as for
        `validate` (the expressions of one image share its ground truth).  smooth: as for `validate`; the callback receives the
        smoothed masks."""
        spec = evalpost.components_spec(components, "inference: components")
        bspec = evalpost.boundary_spec(boundary, "inference: boundary")
        sspec = evalpost.smooth_spec(smooth, "inference: smooth")
        if self.pipe.mode != "test":
            raise ValueError("inference needs a RecordPipeline in mode 'test'")
        indices = list(range(len(records))) if indices is None else [int(i) for i in indices]
        if not indices:
            raise ValueError("inference: no records")
        batches = [[records[i] for i in indices[lo:lo + images_per_batch]] for lo in range(0, len(indices), images_per_batch)]
        total = sum(len(r["sents"]) for b in batches for r in b)
        table = torch.zeros(total, 2, dtype=torch.int32, device=self.device)
        info = None if spec is None else torch.zeros(total, 4, dtype=torch.int64, device=self.device)
        btable = None if bspec is None else torch.zeros(total, 2, dtype=torch.int32, device=self.device)
        sinfo = None if sspec is None else torch.zeros(total, 4, dtype=torch.int64, device=self.device)
        row0 = 0
        for recs in batches:
            img, params = self.pipe(recs)
            n = len(recs)
            if n < images_per_batch:
                rep = torch.tensor(list(range(n)) + [n - 1] * (images_per_batch - n), device=self.device)
                img = img[rep]
            sents = [s for p in params for s in p["sents"]]
            masks, encoded = self._ground_truth(recs, params)
            index, masks, descs = plan_inference(masks, [p["inverse"] for p in params],
                                                 [len(p["sents"]) for p in params])
            K = len(sents)
            word = self.pipe.tok.tokenize(sents + [sents[-1]] * (len(index) - K), self.pipe.word_length, True)
            word = word.to(self.device, non_blocking=True)
            st = self._upload(masks, descs, encoded)
            if self._segment is not None:
                logits = self._segment(img, word, index)
            else:
                logits = self.model(img[torch.tensor(index, device=self.device)], word)
            probs = evalpost.sigmoid_upsample(logits, img.shape[-2], img.shape[-1])
            out = None if visualize is None else torch.empty(st.out_bytes, dtype=torch.uint8, device=self.device)
            if spec is None and sspec is None:
                if out is None and bspec is not None:
                    out = self._boundary_masks(st)
                evalpost.iou_batch(probs, st, st.masks, table, row0, self.thr, out_masks=out)
            else:
                out = self._clean_counts(spec, probs, st, table, row0, info, out, sspec=sspec, sinfo=sinfo)
            if bspec is not None:
                self._boundary_counts(bspec, out, st, btable, row0)
            if visualize is not None:
                self._visualize(visualize, recs, sents, index, st, table[row0:row0 + K].cpu().numpy(), out.cpu().numpy())
            row0 += K
        result = self._finish(table, total, None)
        self._finish_boundary(btable, total, None, False)
        self._finish_smooth(sinfo, total)
        if spec is not None:
            self._finish_components(info, total)
        return result

    @torch.no_grad()
    def sweep(self, records, thresholds=None, split="validate", indices=None, batch_size=32, images_per_batch=8, group=None):
        """The split at every threshold of `thresholds` (default sweep_thresholds()) in ONE pass -> SweepResult: the batch loop,
        padding, staging ring and model shapes of `validate` (split="validate": first sentences, batches of `batch_size`) or of
        `inference` (split="inference": every sentence, `images_per_batch` images share a visual pass), with
        `evalpost.iou_sweep_batch` in place of `iou_batch` - one model call and one sweep launch per batch, the [n, T, 2] table
        read once at the end (kept in `sweep_counts`).  Column i equals the `counts` of a pass at thr = thresholds[i]; `self.thr`
        plays no part."""
        if split not in ("validate", "inference"):
            raise ValueError("sweep: split must be 'validate' or 'inference'")
        if self.pipe.mode != ("val" if split == "validate" else "test"):
            raise ValueError("sweep(split=%r) needs a RecordPipeline in mode %r" % (split, "val" if split == "validate" else "test"))
        thr = sweep_thresholds() if thresholds is None else np.asarray(thresholds, dtype=np.float64).astype(np.float32)
        if thr.ndim != 1 or not 1 <= thr.shape[0] <= evalpost.SWEEP_MAX or not (np.isfinite(thr).all() and (np.diff(thr) > 0).all()):
            raise ValueError("sweep: thresholds must be 1 .. %d finite, strictly increasing values" % evalpost.SWEEP_MAX)
        indices = list(range(len(records))) if indices is None else [int(i) for i in indices]
        if not indices:
            raise ValueError("sweep: no records")
        T = int(thr.shape[0])
        if split == "validate":
            total = len(indices)
            table = torch.zeros(total, T, 2, dtype=torch.int32, device=self.device)
            for lo in range(0, total, batch_size):
                recs = [records[i] for i in indices[lo:lo + batch_size]]
                img, word, params = self.pipe(recs)
                n = len(recs)
                if n < batch_size:                                 # short last batch: repeat its last sample, one graph shape
                    rep = torch.tensor(list(range(n)) + [n - 1] * (batch_size - n), device=self.device)
                    img, word = img[rep], word[rep]
                masks, encoded = self._ground_truth(recs, params)
                st = self._upload(*plan_validate(masks, [p["inverse"] for p in params]), encoded)
                probs = evalpost.sigmoid_upsample(self.model(img, word), img.shape[-2], img.shape[-1])
                evalpost.iou_sweep_batch(probs, st, st.masks, table, lo, thr)
        else:
            batches = [[records[i] for i in indices[lo:lo + images_per_batch]] for lo in range(0, len(indices), images_per_batch)]
            total = sum(len(r["sents"]) for b in batches for r in b)
            table = torch.zeros(total, T, 2, dtype=torch.int32, device=self.device)
            row0 = 0
            for recs in batches:
                img, params = self.pipe(recs)
                n = len(recs)
                if n < images_per_batch:
                    rep = torch.tensor(list(range(n)) + [n - 1] * (images_per_batch - n), device=self.device)
                    img = img[rep]
                sents = [s for p in params for s in p["sents"]]
                masks, encoded = self._ground_truth(recs, params)
                index, masks, descs = plan_inference(masks, [p["inverse"] for p in params],
                                                     [len(p["sents"]) for p in params])
                K = len(sents)
                word = self.pipe.tok.tokenize(sents + [sents[-1]] * (len(index) - K), self.pipe.word_length, True)
                word = word.to(self.device, non_blocking=True)
                st = self._upload(masks, descs, encoded)
                if self._segment is not None:
                    logits = self._segment(img, word, index)
                else:
                    logits = self.model(img[torch.tensor(index, device=self.device)], word)
                probs = evalpost.sigmoid_upsample(logits, img.shape[-2], img.shape[-1])
                evalpost.iou_sweep_batch(probs, st, st.masks, table, row0, thr)
                row0 += K
        flat = table.cpu().reshape(total, 2 * T)                   # the pass's one host read
        if split == "validate" or group is not None:               # (as validate gathers and inference does not)
            flat = gather_counts(flat, group)
        self.sweep_counts = flat.numpy().reshape(-1, T, 2)
        return sweep_metrics(self.sweep_counts, thr)

    @staticmethod
    def _visualize(callback, recs, sents, index, st, counts, out):
        """callback(record, sentence, iou, uint8 mask [ori_h, ori_w] with values 0 / 255) per expression (engine.py:192-197)"""
        for k, sent in enumerate(sents):
            d = st.descs[k]
            pred = out[d.out_off:d.out_off + d.pitch * d.h_out].reshape(d.h_out, d.pitch)[:, :d.w_out]
            callback(recs[index[k]], sent, float(counts[k, 0] / (counts[k, 1] + 1e-6)), np.ascontiguousarray(pred))
