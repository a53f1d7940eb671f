"""Evaluation throughput on one GPU: InferenceRunner R50 at 416x416 over synthetic records (originals drawn around 480x640,
1-5 sentences each).  Two measurements, each arm 5 times, interleaved:

  (a) post-processing only, per batch of 32, on fixed logits: the per-sample `evalpost.validate_batch` loop against
      `sigmoid_upsample` + EvalStaging.pack / upload + ONE `iou_batch` launch; both end with the host reading the counts;
  (b) the whole `Evaluator.validate` pass (JPEG decode, letter-box, forward, post-processing; one host read per pass) in samples/s.

The forward alone (graph replay on a resident batch) is timed for scale.  Writes the table as markdown.

    python tools/eval_bench.py [--records 256] [--out profiles/eval_throughput.md]"""
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
sys.path.insert(0, ROOT)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_throughput.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench needs a GPU (nothing here is measured on the CPU)")
    dev = torch.device("cuda:0")
    recs = make_records(a.records)
    tok = tokenizer.BPETokenizer() if tokenizer.default_merges_path() else HashTokenizer()
    pipe = records.RecordPipeline(SIZE, WORD_LEN, dev, mode="val", tokenizer=tok)
    clip, head = arch.specs_by_name("r50")
    runner = InferenceRunner(clip, head, arch.synthetic_state_dict(clip, head, 0), dev)

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
