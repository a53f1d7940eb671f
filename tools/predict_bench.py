"""Prediction throughput on one GPU: InferenceRunner R50 at 416x416, 8 synthetic 480x640 JPEGs with 3 expressions each.

  (a) the whole `Predictor.predict` call (JPEG decode, letter-box, one visual pass per image, post-processing, results on the
      host) in images/s and expressions/s, with masks="host" and masks=None;
  (b) post-processing only, on fixed logits of that batch: ONE `evalpost.predict_batch` launch (+ pack / upload, + one copy of the
      masks and one of the statistics table) against the per-expression route it replaces - `evalpost.warp_to_original`, one
      h x w float32 map to the host per expression, threshold and box with numpy.

Each arm 5 rounds, interleaved; every figure is a host clock around work that ends with its results on the host.  Writes the
table as markdown.

    python tools/predict_bench.py [--reps 5] [--out profiles/predict.md]

`--components` measures the connected-component clean-up (evalpost.Components) instead, on the same batch: (c1) the fixed-logits
post-processing with and without the spec, (c2) the whole `predict` call with and without it, (c3) the host route it replaces -
masks="host", then scipy.ndimage.label per mask (tests/components_cases.py's labeller where scipy is missing) and numpy statistics -
and the device time of the label + filter launches alone (events).  The threshold is the median probability of the batch, so the
masks have structure (synthetic weights put every pixel above 0.35).

    python tools/predict_bench.py --components [--keep largest] [--min-area 0] [--out profiles/components_bench.md]

`--rle` measures the COCO run-length output (masks="rle": csrc/rle.hip, rle.py) on the same batch and threshold rule: the whole
`predict` call with masks=None, masks="host", masks="host" followed by `rle.encode` per mask on the host (the route the mode
replaces) and masks="rle"; the encoder and its read alone on resident masks; numpy's encode alone; the device time of the four
launches (events); the bytes each arm copies to the host and the run counts of the batch.

    python tools/predict_bench.py --rle [--out profiles/rle.md]

`--smooth` measures the mask smoothing (evalpost.Smooth: open, close, fill holes; csrc/morph.hip, csrc/evalpost.hip) on the same batch:
the whole `predict` call with and without the spec, masks="host" followed by scipy.ndimage per mask on the host (the route the spec
replaces), and the device time of `smooth_batch` alone on resident masks.

    python tools/predict_bench.py --smooth [--radius 2] [--out profiles/smooth.md]

`--polygon` measures the polygon mask output (masks="polygon": csrc/polygon.hip, polygon.py) on the batch and threshold rule of
`--rle`: the whole `predict` call with masks=None, masks="host", masks="host" followed by `polygon.encode` per mask on the host (the
route the mode replaces) and masks="polygon"; the count and the collect alone on resident masks; numpy's encode alone; the device
time of the count's and of the trace's launches by events; vertices and rings per mask and the bytes copied to the host.

    python tools/predict_bench.py --polygon [--out profiles/polygon.md]

`--simplify EPS` measures the Douglas-Peucker simplifier of those polygons (csrc/simplify.hip, polygon.simplify) on the same batch and
threshold rule: the device time of its launches by events on resident rings, the whole `predict` call with masks="polygon" with and
without simplify=EPS, the route it replaces (masks="polygon", then `polygon.simplify` per mask on the host), the bytes copied,
vertices and rings before and after, the rounds of the deepest ring and the IoU of decode(simplified) against the exact mask.
`--polygon-call` times nothing but the whole masks="polygon" call and prints one JSON line: run from this tree and from a checkout of
the parent commit in alternating processes, it is the comparison of the unsimplified path the profile ends with.

    python tools/predict_bench.py --simplify 1 [--out profiles/polygon_simplify.md]
    python tools/predict_bench.py --polygon-call [--package-root ../parent-checkout]"""
import argparse
import ctypes as C
import io
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# --package-root DIR: import the package from another built checkout (the parent commit's, for --polygon-call)
sys.path.insert(0, next((sys.argv[i + 1] for i, v in enumerate(sys.argv[:-1]) if v == "--package-root"), ROOT))
from cris.pytorch_amd import arch, evalpost, hip, jpegdec, predict, records, tokenizer      # noqa: E402
from cris.pytorch_amd.infer import InferenceRunner      # noqa: E402

SIZE, WORD_LEN, IMAGES, EXPRS, ROUNDS, THR = 416, 17, 8, 3, 5, 0.35


def make_jpegs(n, h=480, w=640, seed=0):
    from PIL import Image
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([127 + 100 * np.sin(xx / 7.0 + yy / 13.0 + i), 127 + 100 * np.cos(xx / 5.0 - yy / 9.0), (xx * 3 + yy * 2 + i) % 256], -1)
        img = np.clip(img + rng.normal(0, 8, img.shape), 0, 255).astype(np.uint8)
        b = io.BytesIO()
        Image.fromarray(img).save(b, "JPEG", quality=90)
        out.append(b.getvalue())
    return out


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def host_route(probs, invs, shapes, index, thr=THR):
    """the per-expression route: one warp launch and one float32 map to the host per expression, numpy for the rest"""
    out = []
    for k, i in enumerate(index):
        v = evalpost.warp_to_original(probs[k], invs[i], shapes[i]).cpu().numpy()
        fg = v > np.float32(thr)
        area = int(fg.sum())
        ys, xs = np.nonzero(fg)
        box = (int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1) if area else None
        q16 = int(np.rint(v[fg] * np.float32(65536)).astype(np.int64).sum())
        out.append((fg.astype(np.uint8) * 255, area, box, q16 / (65536.0 * area) if area else 0.0))
    return out


def host_components(masks, q16, keep, min_area, connectivity):
    """the host route of the clean-up: label every mask, filter, statistics with numpy -> [(kept mask, area, box, q16 sum, n)]"""
    try:
        from scipy import ndimage
        structure = ndimage.generate_binary_structure(2, 1 if connectivity == 4 else 2)
    except ImportError:
        ndimage = None
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import components_cases
    out = []
    for m, q in zip(masks, q16):
        if ndimage is None:
            lab = components_cases.label(m, connectivity)
            ids, lab = np.unique(lab, return_inverse=True)                 # -1 (background) first, then ascending canonical labels
            lab = lab.reshape(m.shape) + (0 if ids[0] == -1 else 1)
            n = int(lab.max())
        else:
            lab, n = ndimage.label(m != 0, structure=structure)            # (labels ascend with the first pixel in raster order)
        areas = np.bincount(lab.ravel(), minlength=n + 1)[1:]
        ok = np.nonzero(areas >= min_area)[0]
        if keep == "largest" and ok.size:
            ok = ok[np.argmax(areas[ok])][None]                            # the first maximum: the lowest label
        kept = np.isin(lab, ok + 1)
        area = int(kept.sum())
        ys, xs = np.nonzero(kept)
        box = (int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1) if area else None
        out.append((kept.astype(np.uint8) * 255, area, box, int(q[kept].sum()) if q is not None else 0, n))
    return out, ndimage is not None


def components_arm(a, dev, files, exprs, pipe, runner, logits, invs, shapes, plan, descs):
    spec = evalpost.Components(a.keep, a.min_area, a.connectivity)
    K = len(descs)
    probs0 = evalpost.sigmoid_upsample(logits, SIZE, SIZE)
    thr = float(probs0.median()) if a.thr is None else a.thr
    ring, turn = [evalpost.EvalStaging(dev, mask_bytes=16) for _ in range(3)], [0]
    scratch = {}

    def post(with_spec, masks):
        turn[0] = (turn[0] + 1) % 3
        st = ring[turn[0]].pack_sizes(shapes, descs).upload()
        table = evalpost.new_predict_stats(K, dev)
        probs = evalpost.sigmoid_upsample(logits, SIZE, SIZE)
        if not with_spec:
            out = torch.empty(st.out_bytes, dtype=torch.uint8, device=dev) if masks else None
            evalpost.predict_batch(probs, st, table, 0, thr, out_masks=out)
            return st, None if out is None else out.cpu().numpy(), table.cpu().numpy(), None
        if masks:
            out = torch.empty(st.out_bytes, dtype=torch.uint8, device=dev)
        else:
            out = scratch["masks"] = scratch["masks"] if scratch.get("masks") is not None else torch.empty(st.out_bytes, dtype=torch.uint8, device=dev)
        ktable, info = evalpost.new_predict_stats(K, dev), torch.zeros(K, 4, dtype=torch.int64, device=dev)
        evalpost.predict_batch(probs, st, table, 0, thr, out_masks=out)
        scratch["labels"] = evalpost.label_components(out, st, spec.connectivity, out=scratch.get("labels"))
        scratch["work"] = evalpost.filter_work(st, dev, scratch.get("work"))
        evalpost.filter_components(out, scratch["labels"], st, spec, info, 0, probs=probs, stats=ktable, work=scratch["work"])
        return st, out.cpu().numpy() if masks else None, torch.cat([ktable, info], 1).cpu().numpy(), out

    def unpack(st, buf):
        return [buf[st.descs[k].out_off:st.descs[k].out_off + st.descs[k].pitch * st.descs[k].h_out].reshape(st.descs[k].h_out, st.descs[k].pitch)
                [:, :st.descs[k].w_out] for k in range(K)]

    q16 = [np.rint(evalpost.warp_to_original(probs0[k], invs[i], shapes[i]).cpu().numpy() * np.float32(65536)).astype(np.int64)
           for k, i in enumerate(plan.index[:K])]

    def host():
        st, buf, stats, _ = post(False, True)
        return host_components(unpack(st, buf), q16, spec.keep, spec.min_area, spec.connectivity)

    (ref, used_scipy), (st, buf, rows, _) = host(), post(True, True)
    same = True
    for k, ((m, area, box, q, n), got) in enumerate(zip(ref, unpack(st, buf))):
        r = [int(v) for v in rows[k]]
        same &= bool(np.array_equal(got, m)) and r[0] == area and r[1] == q and (tuple(r[2:6]) == box if area else True) and r[6] == n and r[9] == 0

    def device_only():
        """label + filter alone on masks already on the device: events around the seven stream operations"""
        st, _, _, out = post(True, False)
        info, ktable = torch.zeros(K, 4, dtype=torch.int64, device=dev), evalpost.new_predict_stats(K, dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fresh = evalpost.new_predict_stats(K, dev)
        evalpost.predict_batch(probs0, st, fresh, 0, thr, out_masks=out)
        e0.record()
        labels = evalpost.label_components(out, st, spec.connectivity, out=scratch["labels"])
        evalpost.filter_components(out, labels, st, spec, info, 0, probs=probs0, stats=ktable, work=scratch["work"])
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    pr = predict.Predictor(runner, pipe, thr=thr)
    arms = [lambda: post(False, False), lambda: post(True, False), lambda: post(False, True), lambda: post(True, True), host,
            lambda: pr.predict(files, exprs, images_per_batch=IMAGES, masks=None), lambda: pr.predict(files, exprs, images_per_batch=IMAGES, masks=None, components=spec),
            lambda: pr.predict(files, exprs, images_per_batch=IMAGES, masks="host"), lambda: pr.predict(files, exprs, images_per_batch=IMAGES, masks="host", components=spec)]
    for f in arms:
        timed(f, 2)
    t = [[] for _ in arms]
    dev_ms = []
    for _ in range(ROUNDS):
        for f, acc in zip(arms, t):
            acc.append(timed(f, a.reps) * 1e3)
        dev_ms.append(statistics.median(device_only() for _ in range(a.reps)))

    def row(name, v):
        return "| %s | %s | %.3f | %.3f | %.3f ms |" % (name, " ".join("%.3f" % x for x in v), min(v), max(v), statistics.median(v))

    ncomp, raw, keptarea = [int(v) for v in rows[:, 6]], [int(v) for v in rows[:, 8]], [int(v) for v in rows[:, 0]]
    lines = ["# Connected-component clean-up of predicted masks: on the device against the host route", "",
             "`python tools/predict_bench.py --components --keep %s --min-area %d --connectivity %d --reps %d` on %s: R50, %dx%d, synthetic"
             % (spec.keep, spec.min_area, spec.connectivity, a.reps, torch.cuda.get_device_name(0), SIZE, SIZE),
             "weights; %d synthetic 480x640 JPEGs x %d expressions = %d masks per call, thr %.4f (the batch's median probability unless --thr);"
             % (IMAGES, EXPRS, K, thr),
             "%d rounds with the arms interleaved, %d calls per round and arm; host clocks around work that ends with its results on the host,"
             % (ROUNDS, a.reps), "except the device-time row (events around the memset and the six launches, masks resident).", "",
             "| arm | rounds | min | max | median |", "|---|---|---|---|---|",
             row("(c1) fixed logits, statistics only, no spec: `sigmoid_upsample` + pack + ONE `predict_batch` + table to the host, ms per %d masks" % K, t[0]),
             row("(c1) the same with the spec: + `label_components` + `filter_components`, two more tables", t[1]),
             row("(c1) fixed logits, masks to the host, no spec", t[2]),
             row("(c1) the same with the spec (the FILTERED masks go to the host)", t[3]),
             row("(c1) device time of label + filter alone (events)", dev_ms),
             row("(c3) host route: masks to the host, %s per mask, numpy filter and statistics" % ("`scipy.ndimage.label`" if used_scipy else "the test oracle's labeller (no scipy here)"), t[4]),
             row("(c2) whole `Predictor.predict`, masks=None, no spec, ms per call", t[5]),
             row("(c2) whole `Predictor.predict`, masks=None, with the spec", t[6]),
             row("(c2) whole `Predictor.predict`, masks=\"host\", no spec", t[7]),
             row("(c2) whole `Predictor.predict`, masks=\"host\", with the spec", t[8]), "",
             "Filtered masks, areas, boxes, score sums and component counts of the device and the host route equal: %s." % same,
             "Components per mask before filtering: min %d, median %d, max %d; raw foreground min %d, max %d; kept min %d, max %d of %d pixels."
             % (min(ncomp), statistics.median(ncomp), max(ncomp), min(raw), max(raw), min(keptarea), max(keptarea), shapes[0][0] * shapes[0][1]), ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


def rle_arm(a, dev, files, exprs, pipe, runner, logits, invs, shapes, plan, descs):
    from cris.pytorch_amd import rle
    K = len(descs)
    probs0 = evalpost.sigmoid_upsample(logits, SIZE, SIZE)
    thr = float(probs0.median()) if a.thr is None else a.thr
    pr = predict.Predictor(runner, pipe, thr=thr)

    def call(masks):
        return [p for x in pr.predict(files, exprs, images_per_batch=IMAGES, masks=masks) for p in x]

    def host_encode():
        return [rle.encode(p.mask) for p in call("host")]

    # the batch's masks resident on the device, for the encoder alone
    st = evalpost.EvalStaging(dev, mask_bytes=16).pack_sizes(shapes, descs).upload()
    out = torch.empty(st.out_bytes, dtype=torch.uint8, device=dev)
    evalpost.predict_batch(probs0, st, evalpost.new_predict_stats(K, dev), 0, thr, out_masks=out)
    runs = torch.empty(st.out_bytes, dtype=torch.int32, device=dev)
    work = evalpost.rle_work(st, dev)
    host_masks = [p.mask for p in call("host")]

    def device_only():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        evalpost.rle_encode_batch(out, st, runs=runs, work=work)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def encode_and_collect():
        return evalpost.rle_collect(*evalpost.rle_encode_batch(out, st, runs=runs, work=work), st)

    def numpy_only():
        return [rle.encode(m) for m in host_masks]

    totals = evalpost.rle_encode_batch(out, st, runs=runs, work=work)[1].cpu().numpy()
    same = [p.mask for p in call("rle")] == host_encode() == encode_and_collect()
    arms = [lambda: call(None), lambda: call("host"), host_encode, lambda: call("rle"), encode_and_collect, numpy_only]
    for f in arms:
        timed(f, 2)
    t = [[] for _ in arms]
    dev_ms = []
    for _ in range(ROUNDS):
        for f, acc in zip(arms, t):
            acc.append(timed(f, a.reps) * 1e3)
        dev_ms.append(statistics.median(device_only() for _ in range(a.reps)))

    def row(name, v, note=""):
        return "| %s | %s | %.3f | %.3f | %.3f ms | %s |" % (name, " ".join("%.3f" % x for x in v), min(v), max(v), statistics.median(v), note)

    table = K * 6 * 8
    rle_bytes = (K + 1) * 8 + 4 * int(totals[K]) + table
    strings = sum(len(r["counts"]) for r in encode_and_collect())
    spread = max(t[2]) - min(t[2])
    slower = statistics.median(t[3]) - statistics.median(t[2])
    lines = ["# COCO run-length masks from predict: encoded on the device against numpy on the host", "",
             "`python tools/predict_bench.py --rle --reps %d` on %s: R50, %dx%d, synthetic weights; %d synthetic 480x640 JPEGs x %d"
             % (a.reps, torch.cuda.get_device_name(0), SIZE, SIZE, IMAGES, EXPRS),
             "expressions = %d masks per call, thr %.4f (the batch's median probability unless --thr); %d rounds with the arms interleaved,"
             % (K, thr, ROUNDS),
             "%d calls per round and arm; host clocks around work that ends with its results on the host, except the device-time row"
             % a.reps, "(events around the four launches of `rle_encode_batch`, masks resident).", "",
             "| arm | rounds | min | max | median | bytes to the host per call |", "|---|---|---|---|---|---|",
             row("whole `Predictor.predict`, masks=None, ms per call", t[0], "%d (the table)" % table),
             row("whole `Predictor.predict`, masks=\"host\"", t[1], "%d (the masks) + %d" % (st.out_bytes, table)),
             row("whole `Predictor.predict`, masks=\"host\", then `rle.encode` per mask on the host (the route replaced)", t[2], "%d + %d" % (st.out_bytes, table)),
             row("whole `Predictor.predict`, masks=\"rle\"", t[3], "%d (totals and positions) + %d" % (rle_bytes - table, table)),
             row("masks resident: `rle_encode_batch` + `rle_collect` (launches, two copies, strings), ms per %d masks" % K, t[4], "%d" % (rle_bytes - table)),
             row("masks on the host: `rle.encode` per mask (numpy), ms per %d masks" % K, t[5], "-"),
             row("device time of `rle_encode_batch` alone (events)", dev_ms, "-"), "",
             "The three routes give equal RLE dicts: %s.  Transition positions per mask: min %d, median %d, max %d; %d in the batch; the"
             % (same, int(totals[:K].min()), int(statistics.median(int(v) for v in totals[:K])), int(totals[:K].max()), int(totals[K])),
             "compressed strings of the batch hold %d bytes against %d bytes of masks." % (strings, st.out_bytes), "",
             "masks=\"rle\" against the host-encode arm: median %+.3f ms; spread of the host-encode arm over its rounds %.3f ms."
             % (slower, spread), ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


def polygon_arm(a, dev, files, exprs, pipe, runner, logits, invs, shapes, plan, descs):
    from cris.pytorch_amd import polygon
    K = len(descs)
    probs0 = evalpost.sigmoid_upsample(logits, SIZE, SIZE)
    thr = float(probs0.median()) if a.thr is None else a.thr
    pr = predict.Predictor(runner, pipe, thr=thr)

    def call(masks):
        return [p for x in pr.predict(files, exprs, images_per_batch=IMAGES, masks=masks) for p in x]

    def host_encode():
        return [polygon.encode(p.mask) for p in call("host")]

    def same_dicts(x, y):
        return len(x) == len(y) and all(p["size"] == q["size"] and p["holes"] == q["holes"] and len(p["rings"]) == len(q["rings"])
                                        and all((u == v).all() for u, v in zip(p["rings"], q["rings"])) for p, q in zip(x, y))

    # the batch's masks resident on the device, for the tracer alone
    st = evalpost.EvalStaging(dev, mask_bytes=16).pack_sizes(shapes, descs).upload()
    out = torch.empty(st.out_bytes, dtype=torch.uint8, device=dev)
    evalpost.predict_batch(probs0, st, evalpost.new_predict_stats(K, dev), 0, thr, out_masks=out)
    work, bufs = evalpost.polygon_work(st, dev), evalpost.PolygonBuffers()
    host_masks = [p.mask for p in call("host")]

    def count_and_collect():
        return evalpost.polygon_collect(out, st, evalpost.polygon_count_batch(out, st, work=work), work=work, buffers=bufs)

    def device_only():
        """events around the launches: the count, then (the totals known from the first collect) the trace into the same buffers"""
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        totals = evalpost.polygon_count_batch(out, st, work=work)
        e[1].record()
        tw_words, out_words = bufs.spans
        rc = need // 4
        hip.call("cris_polygon_trace", out.data_ptr(), st.out_bytes, C.addressof(st.descs), st.dev.data_ptr(), K, work.data_ptr(), 8 * work.numel(),
                 totals.data_ptr(), need, most, 0, bufs.trace_work.data_ptr(), 8 * tw_words, bufs.out.data_ptr() + 8 * (2 + 4 * rc), need,
                 bufs.out.data_ptr() + 16, rc, bufs.out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        e[2].record()
        e[2].synchronize()
        return e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])

    def numpy_only():
        return [polygon.encode(m) for m in host_masks]

    totals = evalpost.polygon_count_batch(out, st, work=work).cpu().numpy()
    need, most = int(totals[K]), int(totals[:K].max())
    traced = count_and_collect()
    same = same_dicts([p.mask for p in call("polygon")], host_encode()) and same_dicts(traced, numpy_only())
    rings = [len(p["rings"]) for p in traced]
    arms = [lambda: call(None), lambda: call("host"), host_encode, lambda: call("polygon"), count_and_collect, numpy_only]
    for f in arms:
        timed(f, 2)
    t = [[] for _ in arms]
    count_ms, trace_ms = [], []
    for _ in range(ROUNDS):
        for f, acc in zip(arms, t):
            acc.append(timed(f, a.reps) * 1e3)
        ev = [device_only() for _ in range(a.reps)]
        count_ms.append(statistics.median(v[0] for v in ev))
        trace_ms.append(statistics.median(v[1] for v in ev))

    def row(name, v, note=""):
        return "| %s | %s | %.3f | %.3f | %.3f ms | %s |" % (name, " ".join("%.3f" % x for x in v), min(v), max(v), statistics.median(v), note)

    table = K * 6 * 8
    poly_bytes = (K + 1) * 8 + 8 * (2 + 4 * (need // 4) + need)
    rounds = max(most - 1, 1).bit_length()
    spread = max(t[2]) - min(t[2])
    slower = statistics.median(t[3]) - statistics.median(t[2])
    verdict = ("beats the host route" if slower < -spread else "is slower than the host route" if slower > spread
               else "is not resolved against the host route (the difference lies inside that arm's spread)")
    lines = ["# Polygon masks from predict: traced on the device against numpy on the host", "",
             "`python tools/predict_bench.py --polygon --reps %d` on %s: R50, %dx%d, synthetic weights; %d synthetic 480x640 JPEGs x %d"
             % (a.reps, torch.cuda.get_device_name(0), SIZE, SIZE, IMAGES, EXPRS),
             "expressions = %d masks per call, thr %.4f (the batch's median probability unless --thr); %d rounds with the arms interleaved,"
             % (K, thr, ROUNDS),
             "%d calls per round and arm; host clocks around work that ends with its results on the host, except the two device-time rows"
             % a.reps, "(events around the 3 launches of `cris_polygon_count` and the 7 + %d of `cris_polygon_trace`, masks resident)." % rounds, "",
             "| arm | rounds | min | max | median | bytes to the host per call |", "|---|---|---|---|---|---|",
             row("whole `Predictor.predict`, masks=None, ms per call", t[0], "%d (the table)" % table),
             row("whole `Predictor.predict`, masks=\"host\"", t[1], "%d (the masks) + %d" % (st.out_bytes, table)),
             row("whole `Predictor.predict`, masks=\"host\", then `polygon.encode` per mask on the host (the route replaced)", t[2], "%d + %d" % (st.out_bytes, table)),
             row("whole `Predictor.predict`, masks=\"polygon\"", t[3], "%d (totals; header, ring table and vertices) + %d" % (poly_bytes, table)),
             row("masks resident: `polygon_count_batch` + `polygon_collect` (launches, two copies, dicts), ms per %d masks" % K, t[4], "%d" % poly_bytes),
             row("masks on the host: `polygon.encode` per mask (numpy), ms per %d masks" % K, t[5], "-"),
             row("device time of `cris_polygon_count` alone (events)", count_ms, "-"),
             row("device time of `cris_polygon_trace` alone (events)", trace_ms, "-"), "",
             "The routes give equal polygon dicts: %s.  Vertices per mask: min %d, median %d, max %d; %d in the batch.  Rings per mask: min %d,"
             % (same, int(totals[:K].min()), int(statistics.median(int(v) for v in totals[:K])), most, need, min(rings)),
             "median %d, max %d; %d in the batch.  %d jumping rounds.  The second copy holds %d bytes against %d bytes of masks."
             % (int(statistics.median(rings)), max(rings), sum(rings), rounds, poly_bytes - (K + 1) * 8, st.out_bytes), "",
             "masks=\"polygon\" against the host-encode arm: median %+.3f ms; spread of the host-encode arm over its rounds %.3f ms:"
             % (slower, spread), "the device route %s on this batch." % verdict, "",
             "The masks=None and masks=\"host\" calls issue the library calls they issued before and allocate nothing new",
             "(tests/test_polygon_gpu.py records the calls); against the parent commit they are measured in alternating processes, below", "when that was run.", ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


def polygon_call_arm(a, dev, files, exprs, pipe, runner, logits):
    """--polygon-call: the whole predict call with masks="polygon" (no simplify) alone, one JSON line - for alternating processes of
    this tree and of the parent commit, whose copy of this file has no such arm: it is run from this copy with --package-root"""
    import json
    probs0 = evalpost.sigmoid_upsample(logits, SIZE, SIZE)
    thr = float(probs0.median()) if a.thr is None else a.thr
    pr = predict.Predictor(runner, pipe, thr=thr)
    call = lambda: pr.predict(files, exprs, images_per_batch=IMAGES, masks="polygon")      # noqa: E731
    timed(call, 3)
    rounds = [round(timed(call, a.reps) * 1e3, 3) for _ in range(ROUNDS)]
    print(json.dumps({"arm": "masks=polygon", "package": os.path.dirname(os.path.abspath(predict.__file__)), "thr": round(thr, 4), "rounds_ms": rounds,
                      "median_ms": statistics.median(rounds), "vertices": sum(len(r) for x in call() for p in x for r in p.mask["rings"])}))


def simplify_arm(a, dev, files, exprs, pipe, runner, logits, invs, shapes, plan, descs):
    """--simplify EPS: see the module docstring"""
    from cris.pytorch_amd import polygon
    eps, q = float(a.simplify), polygon.check_epsilon(a.simplify)
    K = len(descs)
    probs0 = evalpost.sigmoid_upsample(logits, SIZE, SIZE)
    thr = float(probs0.median()) if a.thr is None else a.thr
    pr = predict.Predictor(runner, pipe, thr=thr)

    def call(simplify=None):
        return [p for x in pr.predict(files, exprs, images_per_batch=IMAGES, masks="polygon", simplify=simplify) for p in x]

    def host_simplify():
        return [polygon.simplify(p.mask, eps) for p in call()]

    def same_dicts(x, y):
        return len(x) == len(y) and all(p["size"] == q["size"] and p["holes"] == q["holes"] and len(p["rings"]) == len(q["rings"]) and p["epsilon"] == q["epsilon"]
                                        and all(u.shape == v.shape and (u == v).all() for u, v in zip(p["rings"], q["rings"])) for p, q in zip(x, y))

    # the batch's rings resident on the device, for the simplifier alone
    st = evalpost.EvalStaging(dev, mask_bytes=16).pack_sizes(shapes, descs).upload()
    out = torch.empty(st.out_bytes, dtype=torch.uint8, device=dev)
    evalpost.predict_batch(probs0, st, evalpost.new_predict_stats(K, dev), 0, thr, out_masks=out)
    work, bufs = evalpost.polygon_work(st, dev), evalpost.PolygonBuffers()
    totals = evalpost.polygon_count_batch(out, st, work=work)
    resident = evalpost.polygon_collect(out, st, totals, work=work, buffers=bufs, simplify=eps)
    header = [int(v) for v in bufs.header]
    need, ring_cap = header[4], header[4] // 4
    _, _, sw_words, so_words = bufs.spans

    def device_only():
        """events around the simplifier's launches on the traced rings the collect above left in the buffers"""
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        o, sp = bufs.out, bufs.simplified
        e[0].record()
        hip.call("cris_polygon_simplify", o.data_ptr() + 8 * (2 + 4 * ring_cap), o.data_ptr() + 16, o.data_ptr(), need, ring_cap, q, C.addressof(st.descs), K,
                 bufs.simplify_work.data_ptr(), 8 * sw_words, sp.data_ptr() + 8 * (4 + 5 * ring_cap), need, sp.data_ptr() + 32, ring_cap, sp.data_ptr(),
                 torch.cuda.current_stream().cuda_stream)
        e[1].record()
        e[1].synchronize()
        return e[0].elapsed_time(e[1])

    exact = [p.mask for p in call()]
    host_only = lambda: [polygon.simplify(p, eps) for p in exact]          # noqa: E731
    simplified = [p.mask for p in call(eps)]
    same = same_dicts(simplified, host_simplify()) and same_dicts(resident, host_only())
    ious = []
    for p, s in zip(exact, simplified):
        m, d = polygon.decode(p) != 0, polygon.decode(s) != 0
        ious.append(float((m & d).sum()) / float((m | d).sum()) if (m | d).any() else 1.0)
    arms = [lambda: call(), lambda: call(eps), host_simplify, host_only]
    for f in arms:
        timed(f, 2)
    t = [[] for _ in arms]
    dev_ms = []
    for _ in range(ROUNDS):
        for f, acc in zip(arms, t):
            acc.append(timed(f, a.reps) * 1e3)
        dev_ms.append(statistics.median(device_only() for _ in range(a.reps)))

    def row(name, v, note=""):
        return "| %s | %s | %.3f | %.3f | %.3f ms | %s |" % (name, " ".join("%.3f" % x for x in v), min(v), max(v), statistics.median(v), note)

    def verdict(diff, spread, what):
        return ("is faster than %s" % what if diff < -spread else "is slower than %s" % what if diff > spread
                else "is not resolved against %s (the difference lies inside that arm's spread)" % what)

    table = K * 6 * 8
    before_v, before_r = [sum(len(r) for r in p["rings"]) for p in exact], [len(p["rings"]) for p in exact]
    after_v, after_r = [sum(len(r) for r in p["rings"]) for p in simplified], [len(p["rings"]) for p in simplified]
    poly_bytes = (K + 1) * 8 + 8 * (2 + 4 * ring_cap + need)
    simp_bytes = (K + 1) * 8 + 8 * 4 + 8 * (5 * header[0] + header[1])
    d_plain, s_plain = statistics.median(t[1]) - statistics.median(t[0]), max(t[0]) - min(t[0])
    d_host, s_host = statistics.median(t[1]) - statistics.median(t[2]), max(t[2]) - min(t[2])
    launches = 4 if need > evalpost.POLYGON_SIMPLIFY_WAVE else 3
    lines = ["# Simplified polygons from predict: Douglas-Peucker on the device against numpy on the host", "",
             "`python tools/predict_bench.py --simplify %g --reps %d` on %s: R50, %dx%d, synthetic weights; %d synthetic 480x640 JPEGs x %d"
             % (eps, a.reps, torch.cuda.get_device_name(0), SIZE, SIZE, IMAGES, EXPRS),
             "expressions = %d masks per call, thr %.4f (the batch's median probability unless --thr), epsilon %g pixels; %d rounds with the arms"
             % (K, thr, eps, ROUNDS),
             "interleaved, %d calls per round and arm; host clocks around work that ends with its results on the host, except the device-time row"
             % a.reps, "(events around the %d launches of `cris_polygon_simplify`, the traced rings resident)." % launches, "",
             "| arm | rounds | min | max | median | bytes to the host per call |", "|---|---|---|---|---|---|",
             row("whole `Predictor.predict`, masks=\"polygon\", ms per call", t[0], "%d (totals; header, ring table and vertices) + %d (the table)" % (poly_bytes, table)),
             row("whole `Predictor.predict`, masks=\"polygon\", simplify=%g" % eps, t[1], "%d (totals; header; simplified table and vertices) + %d" % (simp_bytes, table)),
             row("whole `Predictor.predict`, masks=\"polygon\", then `polygon.simplify` per mask on the host (the route replaced)", t[2], "%d + %d" % (poly_bytes, table)),
             row("polygons on the host: `polygon.simplify` per mask (numpy), ms per %d masks" % K, t[3], "-"),
             row("device time of `cris_polygon_simplify` alone (events)", dev_ms, "-"), "",
             "The routes give equal simplified dicts: %s.  Vertices per mask before: min %d, median %d, max %d, %d in the batch; after: min %d,"
             % (same, min(before_v), int(statistics.median(before_v)), max(before_v), sum(before_v), min(after_v)),
             "median %d, max %d, %d in the batch.  Rings per mask before: min %d, median %d, max %d, %d in the batch; after: min %d, median %d,"
             % (int(statistics.median(after_v)), max(after_v), sum(after_v), min(before_r), int(statistics.median(before_r)), max(before_r), sum(before_r),
                min(after_r), int(statistics.median(after_r))),
             "max %d, %d in the batch.  The deepest ring took %d rounds.  IoU of decode(simplified) against the exact mask: min %.4f, median %.4f,"
             % (max(after_r), sum(after_r), header[3], min(ious), statistics.median(ious)),
             "max %.4f." % max(ious), "",
             "simplify=%g against the unsimplified call: median %+.3f ms; spread of the unsimplified arm over its rounds %.3f ms: the simplified call"
             % (eps, d_plain, s_plain), "%s." % verdict(d_plain, s_plain, "the unsimplified one"),
             "simplify=%g against the host route: median %+.3f ms; spread of the host-route arm %.3f ms: the device route %s on this batch."
             % (eps, d_host, s_host, verdict(d_host, s_host, "the host route")), "",
             "masks=\"polygon\" without simplify issues the library calls it issued before and allocates nothing new (tests/test_polygon_simplify_gpu.py",
             "records the calls); against the parent commit it is measured in alternating processes, below when that was run.", ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


def smooth_arm(a, dev, files, exprs, pipe, runner, logits, invs, shapes, plan, descs):
    """--smooth: open + close + fill holes at r = a.radius on the batch's masks: the device time alone on resident masks, the whole
    `predict` call with and without the spec, and the host route the spec replaces (masks="host", then scipy.ndimage per mask)"""
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    K, r = len(descs), a.radius
    probs0 = evalpost.sigmoid_upsample(logits, SIZE, SIZE)
    thr = float(probs0.median()) if a.thr is None else a.thr
    spec = evalpost.Smooth(open=r, close=r, fill_holes=True)
    pr = predict.Predictor(runner, pipe, thr=thr)

    def call(masks, smooth=None):
        return [p for x in pr.predict(files, exprs, images_per_batch=IMAGES, masks=masks, smooth=smooth) for p in x]

    sq = np.ones((2 * r + 1, 2 * r + 1), bool)

    def scipy_masks(masks):
        out = []
        for m in masks:
            m = ndimage.binary_opening(m != 0, structure=sq)
            m = ndimage.binary_erosion(ndimage.binary_dilation(m, structure=sq), structure=sq, border_value=1)
            out.append(ndimage.binary_fill_holes(m))
        return out

    def host_smooth():
        return scipy_masks([p.mask for p in call("host")])

    st = evalpost.EvalStaging(dev, mask_bytes=16).pack_sizes(shapes, descs).upload()
    src = torch.empty(st.out_bytes, dtype=torch.uint8, device=dev)
    evalpost.predict_batch(probs0, st, evalpost.new_predict_stats(K, dev), 0, thr, out_masks=src)
    out = torch.empty_like(src)
    info = torch.zeros(K, 4, dtype=torch.int64, device=dev)
    labels = torch.empty(st.out_bytes, dtype=torch.int32, device=dev)
    work, fwork = evalpost.morph_work(st, dev), evalpost.fill_work(st, dev)

    def device_only():
        out.copy_(src)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        evalpost.smooth_batch(out, st, spec, info, 0, labels=labels, work=work, fwork=fwork)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    host_masks = [p.mask for p in call("host")]
    smoothed = call("host", spec)
    same = "scipy not installed: not compared" if ndimage is None else str(all(
        np.array_equal(p.mask != 0, m) for p, m in zip(smoothed, scipy_masks(host_masks))))
    changed = sum(int(((p.mask != 0) != (m != 0)).sum()) for p, m in zip(smoothed, host_masks))
    arms = [lambda: call(None), lambda: call(None, spec), lambda: call("host"), lambda: call("host", spec)]
    if ndimage is not None:
        arms += [host_smooth, lambda: scipy_masks(host_masks)]
    for f in arms:
        timed(f, 2)
    t = [[] for _ in arms]
    dev_ms = []
    for _ in range(ROUNDS):
        for f, acc in zip(arms, t):
            acc.append(timed(f, a.reps) * 1e3)
        dev_ms.append(statistics.median(device_only() for _ in range(a.reps)))

    def row(name, v):
        return "| %s | %s | %.3f | %.3f | %.3f ms |" % (name, " ".join("%.3f" % x for x in v), min(v), max(v), statistics.median(v))

    missing = "| %s | not measured (scipy is not installed) | | | |"
    lines = ["# Mask smoothing in predict: open, close and fill holes on the device against scipy on the host", "",
             "`python tools/predict_bench.py --smooth --radius %d --reps %d` on %s: R50, %dx%d, synthetic weights; %d synthetic 480x640"
             % (r, a.reps, torch.cuda.get_device_name(0), SIZE, SIZE, IMAGES),
             "JPEGs x %d expressions = %d masks per call, thr %.4f (the batch's median probability unless --thr), %s; %d rounds with the"
             % (EXPRS, K, thr, spec, ROUNDS),
             "arms interleaved, %d calls per round and arm; host clocks around work that ends with its results on the host, except the" % a.reps,
             "device-time row (events around the launches of `smooth_batch`: pack, four row and four column passes, store; label, memset,",
             "count, fill - masks resident).", "",
             "| arm | rounds | min | max | median |", "|---|---|---|---|---|",
             row("whole `Predictor.predict`, masks=None, no spec, ms per call", t[0]),
             row("whole `Predictor.predict`, masks=None, smooth", t[1]),
             row("whole `Predictor.predict`, masks=\"host\", no spec", t[2]),
             row("whole `Predictor.predict`, masks=\"host\", smooth", t[3]),
             row("whole `Predictor.predict`, masks=\"host\", then scipy.ndimage per mask on the host (the route replaced)", t[4])
             if ndimage is not None else missing % "masks=\"host\", then scipy.ndimage per mask on the host (the route replaced)",
             row("masks on the host: scipy.ndimage opening, closing, fill_holes per mask, ms per %d masks" % K, t[5])
             if ndimage is not None else missing % "scipy.ndimage alone",
             row("device time of `smooth_batch` alone (events), ms per %d masks" % K, dev_ms), "",
             "The device's masks equal scipy's (binary_opening; binary_dilation then binary_erosion with border_value=1; binary_fill_holes): %s."
             % same,
             "The smoothing changes %d pixels of the batch's %d masks; the spec also labels and filters (a pass-all `Components`) so that"
             % (changed, K),
             "area, box and score are those of the final pixels - that is part of the smooth arms.", ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="default: profiles/predict.md, with --components profiles/components_bench.md, with --rle profiles/rle.md")
    ap.add_argument("--rle", action="store_true", help="measure the run-length mask output instead")
    ap.add_argument("--polygon", action="store_true", help="measure the polygon mask output instead (writes profiles/polygon.md)")
    ap.add_argument("--simplify", type=float, default=None, metavar="EPS", help="measure the Douglas-Peucker simplifier of the polygon output at this "
                    "tolerance instead (writes profiles/polygon_simplify.md)")
    ap.add_argument("--polygon-call", action="store_true", help="time the whole masks=\"polygon\" call alone and print one JSON line")
    ap.add_argument("--package-root", default=None, metavar="DIR", help="import cris.pytorch_amd from this built checkout instead of this tree")
    ap.add_argument("--components", action="store_true", help="measure the connected-component clean-up instead")
    ap.add_argument("--smooth", action="store_true", help="measure the mask smoothing (open, close, fill holes) instead")
    ap.add_argument("--radius", type=int, default=2, help="--smooth only: the radius of the opening and of the closing")
    ap.add_argument("--keep", choices=evalpost.Components.KEEP, default="largest")
    ap.add_argument("--min-area", type=int, default=0)
    ap.add_argument("--connectivity", type=int, choices=(4, 8), default=8)
    ap.add_argument("--thr", type=float, default=None, help="--components / --rle / --polygon / --smooth only: the threshold (default: the batch's median probability)")
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "components_bench.md" if a.components else "rle.md" if a.rle else "polygon.md" if a.polygon else "polygon_simplify.md" if a.simplify is not None else "smooth.md" if a.smooth else "predict.md")
    if not torch.cuda.is_available():
        raise SystemExit("predict_bench needs a GPU (nothing here is measured on the CPU)")
    dev = torch.device("cuda:0")
    files = make_jpegs(IMAGES)
    exprs = [["the %s one on the left number %d" % ("big" if j % 2 else "small", j + i) for j in range(EXPRS)] for i in range(IMAGES)]
    tok = tokenizer.BPETokenizer() if tokenizer.default_merges_path() else predict._WordHashTokenizer()
    pipe = records.RecordPipeline(SIZE, WORD_LEN, dev, mode="test", tokenizer=tok)
    clip, head = arch.specs_by_name("r50")
    runner = InferenceRunner(clip, head, arch.synthetic_state_dict(clip, head, 0), dev)
    pr = predict.Predictor(runner, pipe, thr=THR)

    # ---- fixed logits of the batch for (b)
    (plan,) = predict.plan_predict([EXPRS] * IMAGES, IMAGES)
    images = jpegdec.decode_batch(files, dev)
    img, _, _, invs = pipe.pre(images, None)
    shapes = [(int(t.shape[0]), int(t.shape[1])) for t in images]
    word = tok.tokenize([s for e in exprs for s in e], WORD_LEN, True).to(dev)
    for _ in range(3):
        logits = runner.segment(img, word, plan.index).clone()
    descs = [(invs[i], i, k, row) for _, i, k, row in plan.descs]
    if a.components:
        return components_arm(a, dev, files, exprs, pipe, runner, logits, invs, shapes, plan, descs)
    if a.rle:
        return rle_arm(a, dev, files, exprs, pipe, runner, logits, invs, shapes, plan, descs)
    if a.polygon_call:
        return polygon_call_arm(a, dev, files, exprs, pipe, runner, logits)
    if a.simplify is not None:
        return simplify_arm(a, dev, files, exprs, pipe, runner, logits, invs, shapes, plan, descs)
    if a.polygon:
        return polygon_arm(a, dev, files, exprs, pipe, runner, logits, invs, shapes, plan, descs)
    if a.smooth:
        return smooth_arm(a, dev, files, exprs, pipe, runner, logits, invs, shapes, plan, descs)
    ring, turn = [evalpost.EvalStaging(dev, mask_bytes=16) for _ in range(3)], [0]
    K = len(descs)

    def old():
        return host_route(evalpost.sigmoid_upsample(logits, SIZE, SIZE), invs, shapes, plan.index)

    def new(masks=True):
        turn[0] = (turn[0] + 1) % 3
        st = ring[turn[0]].pack_sizes(shapes, descs).upload()
        table = evalpost.new_predict_stats(K, dev)
        out = torch.empty(st.out_bytes, dtype=torch.uint8, device=dev) if masks else None
        evalpost.predict_batch(evalpost.sigmoid_upsample(logits, SIZE, SIZE), st, table, 0, THR, out_masks=out)
        return st, None if out is None else out.cpu().numpy(), table.cpu().numpy()

    ref = old()
    st, out_h, stats = new()
    same = True
    for k, (m, area, box, score) in enumerate(ref):
        d = st.descs[k]
        got = out_h[d.out_off:d.out_off + d.pitch * d.h_out].reshape(d.h_out, d.pitch)[:, :d.w_out]
        row = [int(v) for v in stats[k]]
        same &= bool(np.array_equal(got, m)) and row[0] == area and (tuple(row[2:]) == box if area else True)
        same &= (row[1] / (65536.0 * area) if area else 0.0) == score
    whole_host = lambda: pr.predict(files, exprs, images_per_batch=IMAGES, masks="host")      # noqa: E731
    whole_none = lambda: pr.predict(files, exprs, images_per_batch=IMAGES, masks=None)        # noqa: E731
    fwd = lambda: runner.segment(img, word, plan.index)      # noqa: E731
    arms = [old, new, lambda: new(False), whole_host, whole_none, fwd]
    for f in arms:
        timed(f, 2)
    t = [[] for _ in arms]
    for _ in range(ROUNDS):
        for f, acc in zip(arms, t):
            acc.append(timed(f, a.reps) * 1e3)
    areas = [int(v) for v in stats[:, 0]]

    def row(name, v, unit):
        return "| %s | %s | %.3f | %.3f | %.3f %s |" % (name, " ".join("%.3f" % x for x in v), min(v), max(v), statistics.median(v), unit)

    def rate(v, n):
        return [n / (x * 1e-3) for x in v]

    lines = ["# Prediction on unlabeled images: one launch per batch against the per-expression route", "",
             "`python tools/predict_bench.py --reps %d` on %s: R50, %dx%d, %d tokens, synthetic weights, folded BatchNorms, HIP-graph"
             % (a.reps, torch.cuda.get_device_name(0), SIZE, SIZE, WORD_LEN),
             "replay; %d synthetic 480x640 JPEGs x %d expressions = %d masks per call, thr %.2f, %d rounds with the arms interleaved;"
             % (IMAGES, EXPRS, K, THR, ROUNDS),
             "every figure is a host clock around work that ends with its results on the host.", "",
             "| arm | rounds | min | max | median |", "|---|---|---|---|---|",
             row("(b) per-expression route: `warp_to_original` + map to the host + numpy threshold / box / score, ms per %d expressions" % K, t[0], "ms"),
             row("(b) `sigmoid_upsample` + pack_sizes + upload + ONE `predict_batch` + masks and table to the host, ms per %d expressions" % K, t[1], "ms"),
             row("(b) the same with statistics only (no mask buffer), ms per %d expressions" % K, t[2], "ms"),
             row("visual pass + expression stage alone (`segment`, graph replay on a resident batch), ms", t[5], "ms"),
             row("(a) whole `Predictor.predict`, masks=\"host\", ms per call", t[3], "ms"),
             row("(a) whole `Predictor.predict`, masks=None, ms per call", t[4], "ms"),
             row("(a) masks=\"host\", images/s", rate(t[3], IMAGES), "images/s"),
             row("(a) masks=\"host\", expressions/s", rate(t[3], K), "expressions/s"),
             row("(a) masks=None, images/s", rate(t[4], IMAGES), "images/s"),
             row("(a) masks=None, expressions/s", rate(t[4], K), "expressions/s"), "",
             "Masks, areas, boxes and scores of the two (b) arms equal: %s.  Foreground areas of the %d masks (synthetic weights): min %d, max %d of %d pixels."
             % (same, K, min(areas), max(areas), shapes[0][0] * shapes[0][1]), ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
