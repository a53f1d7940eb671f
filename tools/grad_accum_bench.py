"""What gradient accumulation costs (profiles/grad_accum.md): NativeTrainer at R50, 416 x 416, micro-batch 8, one GPU, the whole
optimizer step (all K micro-batches) replayed as one captured graph, for K in {1, 2, 4, 8}, timed in fresh processes that
alternate between
  parent   - a built checkout of the commit to compare against (--parent DIR): its trainer has no accum_steps
  k1       - this tree, accum_steps = 1 (the same launches as the parent)
  k2 k4 k8 - this tree, accum_steps = K, a batch of 8 K samples per step
so that drift of the machine lands on all of them alike.  `parent` and `k1` run in every round (their spread is what a K = 1
difference is judged against), the other arms in the first `--k-rounds` rounds.  Each process warms up, then times `--windows`
windows of about `--micro-batches` micro-batches with a host clock around a device synchronise, and reports the median window
and the peak device memory of the process (torch allocator: allocated and reserved).
    python tools/grad_accum_bench.py --parent ../parent-checkout --rounds 4 [--out result.json] [--md table.md]
    python tools/grad_accum_bench.py --worker --root DIR --accum K          (one process of the above; K = 0: no argument)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MICRO = 8


def worker(args):
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from cris.pytorch_amd import arch, synth
    from cris.pytorch_amd.trainer import NativeTrainer
    dev = torch.device("cuda:0")
    clip, head = arch.specs_by_name("r50")
    K = max(args.accum, 1)
    kw = {"accum_steps": args.accum} if args.accum > 0 else {}            # (the parent's trainer has no such argument)
    tr = NativeTrainer(clip, head, arch.synthetic_state_dict(clip, head, 0), dev, launch="graph", **kw)
    nb = 4 if K == 1 else 2
    batches = [tuple(t.to(dev) for t in synth.make_batch(MICRO * K, 416, head.word_len, 0, s)) for s in range(nb)]
    steps = max(args.micro_batches // K, 4)
    for i in range(max(12 // K, 4)):
        tr.train_step(*batches[i % nb])
    torch.cuda.synchronize()
    assert tr.launch == "graph" and tr._graph is not None, tr.graph_error
    ms = []
    for _ in range(args.windows):
        t0 = time.perf_counter()
        for i in range(steps):
            loss, _ = tr.train_step(*batches[i % nb])
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / steps * 1e3)
    res = {"accum_steps": K, "steps_per_window": steps, "ms_per_step_windows": [round(x, 4) for x in ms],
           "ms_per_step": round(statistics.median(ms), 4), "loss": float(loss),
           "arena_mb": round(tr.engine.grad_arena.numel() * 4 / 2 ** 20, 1),
           "peak_allocated_mb": round(torch.cuda.max_memory_allocated(dev) / 2 ** 20, 1),
           "peak_reserved_mb": round(torch.cuda.max_memory_reserved(dev) / 2 ** 20, 1), "device": torch.cuda.get_device_name(0)}
    print("RESULT " + json.dumps(res), flush=True)


def table(summary):
    lines = ["| arm | K | samples/step | ms/optimizer step (processes) | min | max | median | ms/micro-batch | samples/s | peak allocated MB | peak reserved MB |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, s in summary.items():
        K, med = s["accum_steps"], s["ms_per_step_median"]
        lines.append("| %s | %d | %d | %s | %.3f | %.3f | %.3f | %.3f | %.1f | %.0f | %.0f |"
                     % (name, K, MICRO * K, " ".join("%.3f" % x for x in s["ms_per_step_runs"]), min(s["ms_per_step_runs"]),
                        max(s["ms_per_step_runs"]), med, med / K, MICRO * K / med * 1e3, s["peak_allocated_mb"], s["peak_reserved_mb"]))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--accum", type=int, default=0)
    ap.add_argument("--parent", default=None, help="built checkout of the commit to compare against")
    ap.add_argument("--ks", default="2,4,8")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--k-rounds", type=int, default=2, help="rounds in which the K > 1 arms run as well")
    ap.add_argument("--micro-batches", type=int, default=96, help="micro-batches per timed window")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    base = [("k1", HERE, 1)]
    if args.parent:
        base.insert(0, ("parent", args.parent, 0))
    more = [("k%d" % k, HERE, k) for k in (int(x) for x in args.ks.split(",") if x)]
    runs = {name: [] for name, _, _ in base + more}
    for r in range(args.rounds):
        variants = base + (more if r < args.k_rounds else [])
        for name, root, k in (variants if r % 2 == 0 else variants[::-1]):
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--accum", str(k),
                   "--micro-batches", str(args.micro_batches), "--windows", str(args.windows)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
            out = p.stdout.decode()
            line = [x for x in out.splitlines() if x.startswith("RESULT ")]
            if p.returncode != 0 or not line:                              # nothing more is started on the GPU after a failure
                sys.exit("round %d %s: rc %d\n%s" % (r, name, p.returncode, out[-3000:]))
            res = json.loads(line[0][7:])
            runs[name].append(res)
            print("round %d %-6s %.3f ms/step  windows %s  peak %.0f MB allocated" % (r, name, res["ms_per_step"], res["ms_per_step_windows"],
                                                                                  res["peak_allocated_mb"]), flush=True)
    summary = {name: {"accum_steps": rs[0]["accum_steps"], "ms_per_step_median": round(statistics.median(x["ms_per_step"] for x in rs), 4),
                      "ms_per_step_runs": [x["ms_per_step"] for x in rs], "losses": sorted({x["loss"] for x in rs}),
                      "peak_allocated_mb": max(x["peak_allocated_mb"] for x in rs), "peak_reserved_mb": max(x["peak_reserved_mb"] for x in rs)}
               for name, rs in runs.items() if rs}
    first = next(iter(runs.values()))[0]
    result = {"config": "r50 416x416 micro-batch 8, one GPU, launch=graph", "device": first["device"], "arena_mb": first["arena_mb"],
              "micro_batches_per_window": args.micro_batches, "windows": args.windows, "rounds": args.rounds, "k_rounds": args.k_rounds,
              "summary": summary, "runs": runs}
    print(json.dumps(summary))
    print(table(summary))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    if args.md:
        with open(args.md, "w") as f:
            f.write(table(summary))


if __name__ == "__main__":
    main()
