"""Prediction throughput on one GPU: InferenceRunner R50 at 416x416, 8 synthetic 480x640 JPEGs with 3 expressions each.

  (a) the whole `Predictor.predict` call (JPEG decode, letter-box, one visual pass per image, post-processing, results on the
      host) in images/s and expressions/s, with masks="host" and masks=None;
  (b) post-processing only, on fixed logits of that batch: ONE `evalpost.predict_batch` launch (+ pack / upload, + one copy of the
      masks and one of the statistics table) against the per-expression route it replaces - `evalpost.warp_to_original`, one
      h x w float32 map to the host per expression, threshold and box with numpy.

Each arm 5 rounds, interleaved; every figure is a host clock around work that ends with its results on the host.  Writes the
table as markdown.

    python tools/predict_bench.py [--reps 5] [--out profiles/predict.md]"""
import argparse
import io
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cris.pytorch_amd import arch, evalpost, jpegdec, predict, records, tokenizer      # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict.md"))
    a = ap.parse_args()
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
