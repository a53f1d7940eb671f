"""What gradient clipping costs per train step (profiles/grad_clip.md): NativeTrainer at BASELINE.json configs[1] (R50, 416 x 416,
batch 8, one GPU, the step as one captured graph) timed in fresh processes that alternate between
  parent   - a built checkout of the commit to compare against (--parent DIR), max_norm = 0
  off      - this tree, max_norm = 0 (the same launches as the parent)
  on       - this tree, max_norm > 0 (three more launches: two cris_grad_sumsq, one cris_grad_clip_finalize)
so that drift of the machine lands on all of them alike.  Each process warms up, then times `--windows` windows of `--steps`
steps with a host clock around a device synchronise, and reports the median window.
    python tools/grad_clip_bench.py --parent ../parent-checkout --rounds 4 [--out result.json]
    python tools/grad_clip_bench.py --worker --root DIR --max-norm M          (one process of the above)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def worker(args):
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from cris.pytorch_amd import arch, synth
    from cris.pytorch_amd.trainer import NativeTrainer
    dev = torch.device("cuda:0")
    clip, head = arch.specs_by_name("r50")
    kw = {"max_norm": args.max_norm} if args.max_norm > 0 else {}         # (the parent's trainer has no such argument)
    tr = NativeTrainer(clip, head, arch.synthetic_state_dict(clip, head, 0), dev, launch="graph", **kw)
    batches = [tuple(t.to(dev) for t in synth.make_batch(8, 416, head.word_len, 0, s)) for s in range(4)]
    for i in range(args.warmup):
        tr.train_step(*batches[i % 4])
    torch.cuda.synchronize()
    assert tr.launch == "graph" and tr._graph is not None, tr.graph_error
    ms = []
    for _ in range(args.windows):
        t0 = time.perf_counter()
        for i in range(args.steps):
            loss, _ = tr.train_step(*batches[i % 4])
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / args.steps * 1e3)
    res = {"ms_per_step_windows": [round(x, 4) for x in ms], "ms_per_step": round(statistics.median(ms), 4), "loss": float(loss),
           "device": torch.cuda.get_device_name(0)}
    if args.max_norm > 0:
        res["grad_norm"] = float(tr.grad_norm)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--max-norm", type=float, default=0.0)
    ap.add_argument("--parent", default=None, help="built checkout of the commit to compare against")
    ap.add_argument("--on-max-norm", type=float, default=1.0, help="max_norm of the `on` variant")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    variants = [("off", HERE, 0.0), ("on", HERE, args.on_max_norm)]
    if args.parent:
        variants.insert(0, ("parent", args.parent, 0.0))
    runs = {name: [] for name, _, _ in variants}
    for r in range(args.rounds):
        for name, root, mn in (variants if r % 2 == 0 else variants[::-1]):
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--max-norm", str(mn), "--steps", str(args.steps),
                   "--windows", str(args.windows), "--warmup", str(args.warmup)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
            out = p.stdout.decode()
            line = [x for x in out.splitlines() if x.startswith("RESULT ")]
            if p.returncode != 0 or not line:                              # nothing more is started on the GPU after a failure
                sys.exit("round %d %s: rc %d\n%s" % (r, name, p.returncode, out[-3000:]))
            res = json.loads(line[0][7:])
            runs[name].append(res)
            print("round %d %-6s %.3f ms/step  windows %s" % (r, name, res["ms_per_step"], res["ms_per_step_windows"]), flush=True)
    summary = {name: {"ms_per_step_median": round(statistics.median(x["ms_per_step"] for x in rs), 4),
                      "ms_per_step_runs": [x["ms_per_step"] for x in rs]} for name, rs in runs.items()}
    result = {"config": "r50 416x416 batch 8, one GPU, launch=graph", "device": next(iter(runs.values()))[0]["device"],
              "steps_per_window": args.steps, "windows": args.windows, "rounds": args.rounds, "on_max_norm": args.on_max_norm,
              "summary": summary, "runs": runs}
    print(json.dumps(result["summary"]))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
