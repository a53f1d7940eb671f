"""Evaluation throughput on one GPU: InferenceRunner R50 at 416x416 over synthetic records (originals drawn around 480x640,
1-5 sentences each).  Two measurements, each arm 5 times, interleaved:

  (a) post-processing only, per batch of 32, on fixed logits: the per-sample `evalpost.validate_batch` loop against
      `sigmoid_upsample` + EvalStaging.pack / upload + ONE `iou_batch` launch; both end with the host reading the counts;
  (b) the whole `Evaluator.validate` pass (JPEG decode, letter-box, forward, post-processing; one host read per pass) in samples/s.

The forward alone (graph replay on a resident batch) is timed for scale.  Writes the table as markdown.

    python tools/eval_bench.py [--records 256] [--out profiles/eval_throughput.md]

`--sweep [T]` measures the threshold sweep instead (sweep_main: one `iou_sweep_batch` launch against T `iou_batch` launches, a
whole `Evaluator.sweep` pass against a whole `validate` pass) and writes profiles/eval_sweep.md.

`--boundary` measures Boundary IoU instead (boundary_main: the three launches of `boundary_iou_batch` next to the `iou_batch`
launch that writes the masks, the host route they replace - scipy.ndimage.binary_erosion per mask - and a whole `validate` pass
with and without the spec) and writes profiles/boundary_iou.md.

`--decode` measures the mask decoders instead (decode_main: device time of `cris_rle_decode` and `cris_polygon_fill` on 24 masks of
480 x 640, `evaluate.score_results` on them against the host route it replaces, a whole `validate` pass with RLE ground truth
against the same pass with PNG ground truth, the bytes each uploads per batch) and prints the table; `--png-pass` prints the rounds
of the PNG pass alone, and `--tree DIR` imports the package from another checkout, so that fresh processes can alternate between a
build of the parent commit and this one (profiles/mask_decode.md)."""
import argparse
import io
import os
import pickle
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv[:-1] else ROOT)
from cris.pytorch_amd import arch, evalpost, evaluate, pngdec, records, tokenizer      # noqa: E402
from cris.pytorch_amd.infer import InferenceRunner      # noqa: E402

SIZE, WORD_LEN, BATCH, ROUNDS = 416, 17, 32, 5


class HashTokenizer:
    """stands in where the CLIP merge list is not installed: same interface, deterministic ids (the timing does not read them)"""

    def tokenize(self, texts, context_length=77, truncate=False):
        texts = [texts] if isinstance(texts, str) else texts
        out = torch.zeros(len(texts), context_length, dtype=torch.long)
        for i, t in enumerate(texts):
            ids = [49406] + [1 + (sum(map(ord, w)) % 40000) for w in t.lower().split()][:context_length - 2] + [49407]
            out[i, :len(ids)] = torch.tensor(ids)
        return out


def make_records(n, seed=0):
    from PIL import Image
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        h, w = int(rng.integers(416, 545)), int(rng.integers(576, 705))
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([127 + 100 * np.sin(xx / 7.0 + yy / 13.0 + i), 127 + 100 * np.cos(xx / 5.0 - yy / 9.0), (xx * 3 + yy * 2 + i) % 256], -1)
        img = np.clip(img + rng.normal(0, 8, img.shape), 0, 255).astype(np.uint8)
        m = (((yy - h * rng.uniform(0.3, 0.7)) / (h * 0.25)) ** 2 + ((xx - w * rng.uniform(0.3, 0.7)) / (w * 0.2)) ** 2 < 1).astype(np.uint8) * 255
        jb, pb = io.BytesIO(), io.BytesIO()
        Image.fromarray(img).save(jb, "JPEG", quality=90)
        Image.fromarray(m, "L").save(pb, "PNG")
        k = int(rng.integers(1, 6))
        rec = {"img": jb.getvalue(), "mask": pb.getvalue(), "cat": 1, "seg_id": i, "img_name": "%d.jpg" % i, "num_sents": k,
               "sents": ["the %s one on the left number %d" % ("big" if j % 2 else "small", j) for j in range(k)]}
        out.append(records.load_record(pickle.dumps(rec, protocol=5)))
    return out


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def sweep_main(a, dev, recs, pipe, runner):
    """--sweep T: on the fixed probabilities of one batch of 32 (descriptors and masks uploaded once), launches only:
    (a) one `iou_batch`; (b) T `iou_batch` launches into T tables - the way to these numbers without the sweep kernel; (c) one
    `iou_sweep_batch` at the T thresholds; (c1) the same at ONE threshold (the histogram path without the search).  Then (d) a
    whole `Evaluator.validate` pass against a whole `Evaluator.sweep` pass over the same records."""
    T = int(a.sweep)
    if not 1 <= T <= evalpost.SWEEP_MAX:
        raise SystemExit("--sweep T: 1 <= T <= %d" % evalpost.SWEEP_MAX)
    thrs = evaluate.sweep_thresholds() if T == 19 else np.linspace(0.05, 0.95, T).astype(np.float32)
    img, word, params = pipe(recs[:BATCH])
    for _ in range(3):
        logits = runner(img, word).clone()
    masks_u8 = [pngdec.decode_gray(r["mask"]) for r in recs[:BATCH]]
    st = evalpost.EvalStaging(dev).pack(*evaluate.plan_validate(masks_u8, [p["inverse"] for p in params])).upload()
    probs = evalpost.sigmoid_upsample(logits, SIZE, SIZE)
    one = torch.zeros(BATCH, 2, dtype=torch.int32, device=dev)
    tables = [torch.zeros(BATCH, 2, dtype=torch.int32, device=dev) for _ in range(T)]
    swept = torch.zeros(BATCH, T, 2, dtype=torch.int32, device=dev)
    swept1 = torch.zeros(BATCH, 1, 2, dtype=torch.int32, device=dev)

    def arm_a():
        evalpost.iou_batch(probs, st, st.masks, one, 0, 0.35)

    def arm_b():
        for t, tab in zip(thrs, tables):
            evalpost.iou_batch(probs, st, st.masks, tab, 0, float(t))

    def arm_c():
        evalpost.iou_sweep_batch(probs, st, st.masks, swept, 0, thrs)

    def arm_c1():
        evalpost.iou_sweep_batch(probs, st, st.masks, swept1, 0, [0.35])

    arm_b()
    arm_c()
    torch.cuda.synchronize()
    same = bool(torch.equal(swept, torch.stack(tables, 1)))        # before the timed launches accumulate further
    hist = swept.cpu().numpy().astype(np.int64)
    pixels = sum(int(m.shape[0]) * int(m.shape[1]) for m in masks_u8)
    middle = int(hist[:, 0].sum() - hist[:, -1].sum())             # pred_0 - pred_{T-1}  (pred_i = union_i + inter_i - gt)
    arms = (arm_a, arm_b, arm_c, arm_c1)
    calls = (200 * a.reps, 20 * a.reps, 200 * a.reps, 200 * a.reps)      # a timed window is >= 0.1 s of device work
    for f in arms:
        timed(f, 2)
    t_arm = [[] for _ in arms]
    for _ in range(ROUNDS):
        for f, k, v in zip(arms, calls, t_arm):
            for tab in [one, swept, swept1] + tables:              # (the launches accumulate: keep the int32 counts far from 2^31)
                tab.zero_()
            v.append(timed(f, k) * 1e3)
    t_a, t_b, t_c, t_c1 = t_arm

    ev = evaluate.Evaluator(runner, pipe)
    ev.validate(recs[:2 * BATCH], batch_size=BATCH)                # warm-up: eager call, graph capture
    ev.sweep(recs[:2 * BATCH], thrs, batch_size=BATCH)
    p_val, p_sweep = [], []
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        ev.validate(recs, batch_size=BATCH)
        torch.cuda.synchronize()
        p_val.append(len(recs) / (time.perf_counter() - t0))
        t0 = time.perf_counter()
        res = ev.sweep(recs, thrs, batch_size=BATCH)
        torch.cuda.synchronize()
        p_sweep.append(len(recs) / (time.perf_counter() - t0))

    def row(name, v, unit):
        return "| %s | %s | %.3f | %.3f | %.3f %s |" % (name, " ".join("%.3f" % x for x in v), min(v), max(v), statistics.median(v), unit)

    def ratio(num, den):
        r = [x / y for x, y in zip(num, den)]
        return "%.2f (per round %s)" % (statistics.median(num) / statistics.median(den), " ".join("%.2f" % x for x in r))

    med = statistics.median
    lines = ["# Threshold sweep: T thresholds in one launch against T launches", "",
             "`python tools/eval_bench.py --sweep %d --records %d --reps %d` on %s: R50, %dx%d, %d tokens, synthetic weights, HIP-graph"
             % (T, a.records, a.reps, torch.cuda.get_device_name(0), SIZE, SIZE, WORD_LEN),
             "replay; %d synthetic records (originals 416-544 x 576-704), batch %d, T = %d thresholds %.2f .. %.2f, %d rounds with the arms"
             % (a.records, BATCH, T, thrs[0], thrs[-1], ROUNDS),
             "interleaved.  Arms (a)-(c1) are launches only, on the resident probabilities, descriptors and masks of one batch of 32",
             "(%d original-size pixels); each figure is the mean of %d back-to-back calls (%d for (b)) inside a host clock that ends in a"
             % (pixels, calls[0], calls[1]),
             "device synchronisation.  (d) is a whole pass (JPEG decode, letter-box, forward, post-processing, one host read).", "",
             "| arm | rounds | min | max | median |", "|---|---|---|---|---|",
             row("(a) one `iou_batch` launch, ms", t_a, "ms"),
             row("(b) %d `iou_batch` launches into %d tables, ms" % (T, T), t_b, "ms"),
             row("(c) one `iou_sweep_batch` launch at %d thresholds, ms" % T, t_c, "ms"),
             row("(c1) one `iou_sweep_batch` launch at 1 threshold, ms", t_c1, "ms"),
             row("(d) whole `Evaluator.validate` pass (one threshold), samples/s", p_val, "samples/s"),
             row("(d) whole `Evaluator.sweep` pass (%d thresholds), samples/s" % T, p_sweep, "samples/s"), "",
             "* (c) < (b): %s - median (b) / (c) = %s." % (med(t_c) < med(t_b), ratio(t_b, t_c)),
             "* (c) / (a) = %s; (c1) / (a) = %s." % (ratio(t_c, t_a), ratio(t_c1, t_a)),
             "* sweep pass / validate pass = %s in samples/s." % ratio(p_sweep, p_val),
             "* Every column of the sweep table equals the single-threshold table of its threshold: %s." % same,
             "* %d of the batch's %d pixels (%.2f %%) lie between the lowest and the highest threshold - the ones that take the"
             % (middle, pixels, 100.0 * middle / pixels),
             "  binary search and an LDS add; the others are counted in registers.",
             "* Last sweep: best threshold by mean IoU %.2f (%.4f), by overall IoU %.2f (%.4f)."
             % (res.best("iou") + res.best("overall_iou")), ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


def boundary_main(a, dev, recs, pipe, runner):
    """--boundary: on the fixed probabilities of one batch of 32 (descriptors and masks uploaded once), launches only: (a) one
    `iou_batch` that also writes the masks; (b) `boundary_iou_batch` on those masks (three launches); (c) `erode_batch` (three
    launches, bytes out).  (d) the host route on the same masks: scipy's binary_erosion of prediction and ground truth per sample
    and numpy counts.  Then (e) a whole `Evaluator.validate` pass without and with the spec, interleaved."""
    spec = evalpost.Boundary()
    img, word, params = pipe(recs[:BATCH])
    for _ in range(3):
        logits = runner(img, word).clone()
    masks_u8 = [pngdec.decode_gray(r["mask"]) for r in recs[:BATCH]]
    st = evalpost.EvalStaging(dev).pack(*evaluate.plan_validate(masks_u8, [p["inverse"] for p in params])).upload()
    probs = evalpost.sigmoid_upsample(logits, SIZE, SIZE)
    one = torch.zeros(BATCH, 2, dtype=torch.int32, device=dev)
    btab = torch.zeros(BATCH, 2, dtype=torch.int32, device=dev)
    out = torch.zeros(st.out_bytes, dtype=torch.uint8, device=dev)
    eroded = torch.zeros(st.out_bytes, dtype=torch.uint8, device=dev)
    work = evalpost.boundary_work(st, dev)
    radii_host = evalpost.boundary_radii(st, spec)
    radii = torch.from_numpy(radii_host).to(dev)
    evalpost.iou_batch(probs, st, st.masks, one, 0, 0.35, out_masks=out)
    # the synthetic weights predict little: count the ground truth against a shifted copy of itself as well, so that both
    # boundaries are there (the launches do the same work whatever the masks hold; the host route does not)
    shifted = torch.zeros_like(out)
    for i in range(st.n):
        d = st.descs[i]
        g = st.masks[d.mask_off:d.mask_off + d.pitch * d.h_out].view(d.h_out, d.pitch)
        shifted[d.out_off:d.out_off + d.pitch * d.h_out].view(d.h_out, d.pitch)[7:, 5:d.w_out] = g[:-7, :d.w_out - 5]

    def arm_a():
        evalpost.iou_batch(probs, st, st.masks, one, 0, 0.35, out_masks=out)

    def arm_b():
        evalpost.boundary_iou_batch(shifted, st, st.masks, radii, btab, 0, work=work)

    def arm_c():
        evalpost.erode_batch(shifted, st, radii, out=eroded, work=work)

    def host_counts():
        from scipy import ndimage
        square = np.ones((3, 3), bool)
        res = []
        for i in range(st.n):
            d = st.descs[i]
            p = pred_host[d.out_off:d.out_off + d.pitch * d.h_out].reshape(d.h_out, d.pitch)[:, :d.w_out] != 0
            g = masks_u8[i].numpy() != 0
            r = int(radii_host[i])
            bp = p & ~ndimage.binary_erosion(p, structure=square, iterations=r, border_value=0)
            bg = g & ~ndimage.binary_erosion(g, structure=square, iterations=r, border_value=0)
            res.append([int((bp & bg).sum()), int((bp | bg).sum())])
        return res

    btab.zero_()
    arm_b()
    got = btab.cpu().numpy().tolist()
    pred_host = shifted.cpu().numpy()
    try:
        want = host_counts()
        t_host = []
        for _ in range(ROUNDS):
            t0 = time.perf_counter()
            host_counts()
            t_host.append((time.perf_counter() - t0) * 1e3)
    except ImportError:
        want = t_host = None
    arms = (arm_a, arm_b, arm_c)
    calls = 200 * a.reps                                           # a timed window is >= 0.1 s of device work
    for f in arms:
        timed(f, 2)
    t_arm = [[] for _ in arms]
    for _ in range(ROUNDS):
        for f, v in zip(arms, t_arm):
            one.zero_()
            btab.zero_()                                           # (the launches accumulate: keep the int32 counts far from 2^31)
            v.append(timed(f, calls) * 1e3)
    t_a, t_b, t_c = t_arm

    ev = evaluate.Evaluator(runner, pipe)
    ev.validate(recs[:2 * BATCH], batch_size=BATCH)                # warm-up: eager call, graph capture
    ev.validate(recs[:2 * BATCH], batch_size=BATCH, boundary=spec)
    p_plain, p_bd = [], []
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        ev.validate(recs, batch_size=BATCH)
        torch.cuda.synchronize()
        p_plain.append(len(recs) / (time.perf_counter() - t0))
        t0 = time.perf_counter()
        ev.validate(recs, batch_size=BATCH, boundary=spec)
        torch.cuda.synchronize()
        p_bd.append(len(recs) / (time.perf_counter() - t0))

    def row(name, v, unit):
        if v is None:
            return "| %s | not measured (scipy is not installed) | | | |" % name
        return "| %s | %s | %.3f | %.3f | %.3f %s |" % (name, " ".join("%.3f" % x for x in v), min(v), max(v), statistics.median(v), unit)

    med = statistics.median
    pixels = sum(int(m.shape[0]) * int(m.shape[1]) for m in masks_u8)
    lines = ["# Boundary IoU: three launches on bit planes against per-mask erosion on the host", "",
             "`python tools/eval_bench.py --boundary --records %d --reps %d` on %s: R50, %dx%d, %d tokens, synthetic weights, HIP-graph"
             % (a.records, a.reps, torch.cuda.get_device_name(0), SIZE, SIZE, WORD_LEN),
             "replay; %d synthetic records (originals 416-544 x 576-704), batch %d, radii %d .. %d (2 %% of the diagonal), %d rounds with"
             % (a.records, BATCH, int(radii_host.min()), int(radii_host.max()), ROUNDS),
             "the arms interleaved.  Arms (a)-(c) are launches only, on the resident descriptors and masks of one batch of %d (%d"
             % (BATCH, pixels),
             "original-size pixels; the prediction is the ground truth shifted by (7, 5), so both boundaries exist); each figure is the mean",
             "of %d back-to-back calls inside a host clock that ends in a device synchronisation.  (d) is host work on the same masks,"
             % calls,
             "already in host memory (no copy is counted).  (e) is a whole pass (JPEG decode, letter-box, forward, post-processing, one host",
             "read), the two arms alternating in one process.", "",
             "| arm | rounds | min | max | median |", "|---|---|---|---|---|",
             row("(a) one `iou_batch` launch that writes the masks, ms", t_a, "ms"),
             row("(b) `boundary_iou_batch`, three launches, ms", t_b, "ms"),
             row("(c) `erode_batch`, three launches, ms", t_c, "ms"),
             row("(d) host route: 2 x 32 `scipy.ndimage.binary_erosion` + numpy counts, ms", t_host, "ms"),
             row("(e) whole `Evaluator.validate` pass, samples/s", p_plain, "samples/s"),
             row("(e) whole `Evaluator.validate` pass with `boundary=True`, samples/s", p_bd, "samples/s"), "",
             "* (b) / (a) = %.2f." % (med(t_b) / med(t_a)),
             "* pass with the spec / pass without = %.3f in samples/s (per round %s)."
             % (med(p_bd) / med(p_plain), " ".join("%.3f" % (x / y) for x, y in zip(p_bd, p_plain)))]
    if t_host is not None:
        lines += ["* (d) / (b) = %.0f." % (med(t_host) / med(t_b)),
                  "* The device counts of the batch equal the host route's: %s." % (got == want)]
    lines += ["* Last pass with the spec: mask IoU %.4f, boundary IoU %.4f." % (float(np.mean(ev.per_sample)), ev.boundary_iou), ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


def png_pass(a, recs, pipe, runner):
    """--png-pass: the rounds of a whole `Evaluator.validate` pass over PNG records, samples/s, one line (uses nothing the parent
    commit lacks: run it with --tree on either checkout)"""
    ev = evaluate.Evaluator(runner, pipe)
    ev.validate(recs[:2 * BATCH], batch_size=BATCH)                # warm-up: eager call, graph capture
    rounds = []
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        ev.validate(recs, batch_size=BATCH)
        torch.cuda.synchronize()
        rounds.append(len(recs) / (time.perf_counter() - t0))
    print("png-pass %s | %s | median %.1f samples/s" % (os.path.dirname(os.path.dirname(os.path.abspath(evaluate.__file__))),
                                                         " ".join("%.1f" % v for v in rounds), statistics.median(rounds)))


def decode_masks(n=24, h=480, w=640, seed=0):
    """n masks of h x w as predictions look: a blob with a hole, a bar and specks; and the same shifted, as ground truth"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for i in range(n):
        cx, cy, rx, ry = rng.uniform(0.3, 0.7) * w, rng.uniform(0.3, 0.7) * h, rng.uniform(0.1, 0.3) * w, rng.uniform(0.1, 0.3) * h
        m = ((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 < 1.0
        m &= ~(((xx - cx - 20) / (rx / 4)) ** 2 + ((yy - cy + 10) / (ry / 4)) ** 2 < 1.0)
        m |= (np.abs(xx - 60 - 5 * i) < 9) & (yy > h - 80)
        m |= rng.random((h, w)) < 0.0005
        out.append(m.astype(np.uint8) * 255)
    return out, [np.roll(m, (7, 5), (0, 1)) for m in out]


def decode_main(a, dev, recs, pipe, runner):
    """--decode: (a)-(c) device time of the decoders on 24 masks of 480 x 640 (events around `decode_masks_batch`, sources
    resident); (d) `score_results` on those masks as RLE against (e) the host route it replaces - `rle.decode` per mask, pack,
    upload, `mask_iou_batch`, one read; (f) / (g) a whole `Evaluator.validate` pass with PNG and with RLE ground truth,
    interleaved, and the bytes each uploads per batch."""
    from cris.pytorch_amd import polygon, rle
    preds, gts = decode_masks()
    n = len(preds)
    ident = np.array([[1.0, 0, 0], [0, 1.0, 0]])
    st = evalpost.EvalStaging(dev).pack_sizes([m.shape for m in preds], [(ident, i, 0, i) for i in range(n)]).upload()
    slots = evalpost.desc_slots(st, "out")
    as_rle = [rle.encode(m) for m in preds]
    as_poly = [polygon.encode(m) for m in preds]
    as_simple = [polygon.simplify(p, 1.0) for p in as_poly]
    out = torch.empty(st.out_bytes, dtype=torch.uint8, device=dev)
    t_dev, equal, sizes = [], [], []
    calls = 40 * a.reps
    for items, want in ((as_rle, preds), (as_poly, preds), (as_simple, [polygon.decode(p) for p in as_simple])):
        srcs = evalpost.MaskSources([evalpost.mask_form(x) for x in items], slots).upload(dev)
        work = evalpost.decode_work(srcs, dev)
        out.fill_(0x7F)
        evalpost.decode_masks_batch(srcs, out, work=work)
        got = out.cpu().numpy()
        equal.append(all(np.array_equal(got[o:o + p * m.shape[0]].reshape(m.shape[0], p)[:, :m.shape[1]], m) for (o, p), m in zip(slots, want)))
        sizes.append(srcs.blob.size)
        rounds = []
        for _ in range(ROUNDS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                evalpost.decode_masks_batch(srcs, out, work=work)
            e1.record()
            torch.cuda.synchronize()
            rounds.append(e0.elapsed_time(e1) / calls)
        t_dev.append(rounds)

    gt_rle = [rle.encode(m) for m in gts]
    json_rle = [rle.to_json(r) for r in as_rle]                    # str counts, as a results file holds them

    def scorer():
        return evaluate.score_results(json_rle, gt_rle, dev).counts

    host_st = evalpost.EvalStaging(dev)

    def host_route():
        p_arr, g_arr = [rle.decode(r) for r in json_rle], [rle.decode(r) for r in gt_rle]
        hs = host_st.pack(g_arr, [(ident, i, 0, i) for i in range(n)]).upload()
        buf = torch.zeros(hs.out_bytes, dtype=torch.uint8).pin_memory()
        view = buf.numpy()
        for i, m in enumerate(p_arr):
            d = hs.descs[i]
            view[d.out_off:d.out_off + d.pitch * d.h_out].reshape(d.h_out, d.pitch)[:, :d.w_out] = m
        table = torch.zeros(n, 2, dtype=torch.int32, device=dev)
        evalpost.mask_iou_batch(buf.to(dev, non_blocking=True), hs, hs.masks, table, 0)
        return table.cpu().numpy()

    same_counts = bool(np.array_equal(scorer(), host_route()))
    t_score, t_host = [], []
    for _ in range(ROUNDS):
        t_score.append(timed(scorer, a.reps) * 1e3)
        t_host.append(timed(host_route, a.reps) * 1e3)

    recs_rle = [dict(r, mask=rle.encode(pngdec.decode_gray(r["mask"]).numpy())) for r in recs]
    uploads = []
    real = evalpost.EvalStaging.upload
    evalpost.EvalStaging.upload = lambda self: (real(self), uploads.append(self.last_upload_bytes))[0]
    ev = evaluate.Evaluator(runner, pipe)
    ev.validate(recs[:2 * BATCH], batch_size=BATCH)                # warm-up: eager call, graph capture
    ev.validate(recs_rle[:2 * BATCH], batch_size=BATCH)
    p_png, p_rle, b_png, b_rle, last = [], [], [], [], []
    for _ in range(ROUNDS):
        for rs, rate, nbytes in ((recs, p_png, b_png), (recs_rle, p_rle, b_rle)):
            del uploads[:]
            t0 = time.perf_counter()
            ev.validate(rs, batch_size=BATCH)
            torch.cuda.synchronize()
            rate.append(len(rs) / (time.perf_counter() - t0))
            nbytes += uploads
            last.append(ev.counts.copy())
    same_pass = bool(np.array_equal(last[-2], last[-1]))
    evalpost.EvalStaging.upload = real

    def row(name, v, unit):
        return "| %s | %s | %.3f | %.3f | %.3f %s |" % (name, " ".join("%.3f" % x for x in v), min(v), max(v), statistics.median(v), unit)

    med = statistics.median
    lines = ["`python tools/eval_bench.py --decode --records %d --reps %d` on %s: %d masks of 480 x 640 (a blob with a hole, a bar,"
             % (a.records, a.reps, torch.cuda.get_device_name(0), n),
             "specks; the ground truth is the mask shifted by (7, 5)); R50, %dx%d, synthetic weights, %d synthetic records, batch %d;"
             % (SIZE, SIZE, a.records, BATCH),
             "%d rounds with the arms interleaved.  (a)-(c): events around %d back-to-back `decode_masks_batch` calls, sources resident."
             % (ROUNDS, calls),
             "(d), (e): host clocks around %d calls that end with the counts on the host.  (f), (g): whole passes (JPEG decode, letter-box,"
             % a.reps,
             "forward, post-processing, one host read).", "",
             "| arm | rounds | min | max | median |", "|---|---|---|---|---|",
             row("(a) `cris_rle_decode`, %d masks, device ms" % n, t_dev[0], "ms"),
             row("(b) `cris_polygon_fill`, traced polygons, device ms", t_dev[1], "ms"),
             row("(c) `cris_polygon_fill`, simplified at 1.0, device ms", t_dev[2], "ms"),
             row("(d) `score_results` on %d RLE pairs, ms" % n, t_score, "ms"),
             row("(e) host route: `rle.decode` x %d, pack, upload, `mask_iou_batch`, ms" % (2 * n), t_host, "ms"),
             row("(f) whole `Evaluator.validate` pass, PNG ground truth, samples/s", p_png, "samples/s"),
             row("(g) whole `Evaluator.validate` pass, RLE ground truth, samples/s", p_rle, "samples/s"), "",
             "* Every decoded slot equals the host decode: RLE %s, traced polygons %s, simplified polygons %s." % tuple(equal),
             "* Tables and payload of the %d masks: %d bytes as RLE, %d as traced polygons, %d simplified; the masks themselves %d bytes."
             % (n, sizes[0], sizes[1], sizes[2], n * 480 * 640),
             "* (d) and (e) give equal counts: %s.  (e) / (d) = %.2f; spread of (e) over its rounds %.3f ms."
             % (same_counts, med(t_host) / med(t_score), max(t_host) - min(t_host)),
             "* (g) / (f) = %.3f in samples/s (per round %s); the two passes give equal counts: %s."
             % (med(p_rle) / med(p_png), " ".join("%.3f" % (x / y) for x, y in zip(p_rle, p_png)), same_pass),
             "* Bytes uploaded per full batch of %d by the staging's one copy: PNG %d (median; descriptors and masks), RLE %d (descriptors,"
             % (BATCH, med(b_png), med(b_rle)),
             "  sources and counts; the mask slots exist on the device only).", ""]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", type=int, nargs="?", const=19, default=None, metavar="T",
                    help="measure the threshold sweep at T thresholds (default 19) instead; writes profiles/eval_sweep.md")
    ap.add_argument("--boundary", action="store_true", help="measure Boundary IoU instead; writes profiles/boundary_iou.md")
    ap.add_argument("--decode", action="store_true", help="measure the mask decoders instead; prints the table (profiles/mask_decode.md)")
    ap.add_argument("--png-pass", action="store_true", help="print the rounds of a validate pass over PNG records, nothing else")
    ap.add_argument("--tree", default=None, metavar="DIR", help="import cris.pytorch_amd from this checkout (A/B against another commit)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.boundary + (a.sweep is not None) + a.decode + a.png_pass > 1:
        raise SystemExit("--boundary, --sweep, --decode and --png-pass are separate measurements")
    if not (a.decode or a.png_pass):
        a.out = a.out or os.path.join(ROOT, "profiles", "boundary_iou.md" if a.boundary else "eval_throughput.md" if a.sweep is None else "eval_sweep.md")
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench needs a GPU (nothing here is measured on the CPU)")
    dev = torch.device("cuda:0")
    recs = make_records(a.records)
    tok = tokenizer.BPETokenizer() if tokenizer.default_merges_path() else HashTokenizer()
    pipe = records.RecordPipeline(SIZE, WORD_LEN, dev, mode="val", tokenizer=tok)
    clip, head = arch.specs_by_name("r50")
    runner = InferenceRunner(clip, head, arch.synthetic_state_dict(clip, head, 0), dev)
    if a.sweep is not None:
        return sweep_main(a, dev, recs, pipe, runner)
    if a.boundary:
        return boundary_main(a, dev, recs, pipe, runner)
    if a.decode:
        return decode_main(a, dev, recs, pipe, runner)
    if a.png_pass:
        return png_pass(a, recs, pipe, runner)

    # ---- (a) post-processing of one batch of 32 on fixed logits
    img, word, params = pipe(recs[:BATCH])
    for _ in range(3):
        logits = runner(img, word).clone()
    mats, sizes = [p["inverse"] for p in params], [p["ori_size"] for p in params]
    masks_u8 = [pngdec.decode_gray(r["mask"]) for r in recs[:BATCH]]
    masks_f32 = [m.numpy().astype(np.float32) / 255.0 for m in masks_u8]          # what validate_batch takes (mask / 255.)
    ring, turn = [evalpost.EvalStaging(dev) for _ in range(3)], [0]
    table = torch.zeros(BATCH, 2, dtype=torch.int32, device=dev)

    def old():
        return evalpost.validate_batch(logits, (SIZE, SIZE), mats, sizes, masks_f32)

    def new():
        turn[0] = (turn[0] + 1) % 3
        st = ring[turn[0]].pack(*evaluate.plan_validate(masks_u8, mats)).upload()
        table.zero_()
        evalpost.iou_batch(evalpost.sigmoid_upsample(logits, SIZE, SIZE), st, st.masks, table, 0)
        return evaluate.metrics(table.cpu().numpy())[2].tolist()

    def new_no_read():                                             # as Evaluator.validate runs it: no host read per batch
        turn[0] = (turn[0] + 1) % 3
        st = ring[turn[0]].pack(*evaluate.plan_validate(masks_u8, mats)).upload()
        evalpost.iou_batch(evalpost.sigmoid_upsample(logits, SIZE, SIZE), st, st.masks, table, 0)

    same = old() == new()
    fwd = lambda: runner(img, word)      # noqa: E731
    for f in (old, new, new_no_read, fwd):
        timed(f, 2)
    t_old, t_new, t_nr, t_fwd = [], [], [], []
    for _ in range(ROUNDS):
        t_old.append(timed(old, a.reps) * 1e3)
        t_new.append(timed(new, a.reps) * 1e3)
        t_nr.append(timed(new_no_read, a.reps) * 1e3)
        t_fwd.append(timed(fwd, 4 * a.reps) * 1e3)

    # ---- (b) the whole validate pass
    ev = evaluate.Evaluator(runner, pipe)
    ev.validate(recs[:2 * BATCH], batch_size=BATCH)                # warm-up: eager call, graph capture
    t_pass = []
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        iou, prec = ev.validate(recs, batch_size=BATCH)
        torch.cuda.synchronize()
        t_pass.append(len(recs) / (time.perf_counter() - t0))

    def row(name, v, unit):
        return "| %s | %s | %.3f | %.3f | %.3f %s |" % (name, " ".join("%.3f" % x for x in v), min(v), max(v), statistics.median(v), unit)

    lines = ["# Evaluation throughput: one launch per batch against the per-sample loop", "",
             "`python tools/eval_bench.py --records %d --reps %d` on %s: R50, %dx%d, %d tokens, synthetic weights, folded BatchNorms,"
             % (a.records, a.reps, torch.cuda.get_device_name(0), SIZE, SIZE, WORD_LEN),
             "HIP-graph replay; %d synthetic records (originals 416-544 x 576-704, 1-5 sentences), batch %d, %d rounds with the arms"
             % (a.records, BATCH, ROUNDS),
             "interleaved; every figure is a host clock around work that ends in a device synchronisation.", "",
             "| arm | rounds | min | max | median |", "|---|---|---|---|---|",
             row("(a) `validate_batch` (per-sample loop), ms per batch of 32", t_old, "ms"),
             row("(a) `sigmoid_upsample` + pack + upload + `iou_batch` + host read, ms per batch of 32", t_new, "ms"),
             row("(a) the same without the per-batch host read (as `validate` runs it), ms per batch of 32", t_nr, "ms"),
             row("forward alone, graph replay on a resident batch of 32, ms", t_fwd, "ms"),
             row("(b) whole `Evaluator.validate` pass, samples/s", t_pass, "samples/s"), "",
             "Per-sample IoUs of the two (a) arms equal: %s.  Last pass: IoU %.4f, %s." % (same, iou, prec), ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
