"""What the weight average costs per train step (profiles/ema.md): NativeTrainer at BASELINE.json configs[1] (R50, 416 x 416,
batch 8, one GPU, the step as one captured graph) timed in fresh processes that alternate between
  parent   - a built checkout of the commit to compare against (--parent DIR): its trainer has no ema_decay
  off      - this tree, ema_decay = None (the same launches as the parent)
  every1   - this tree, ema_decay = 0.999, an update in every step (two more launches: cris_ema_advance, cris_ema_update)
  every4   - this tree, ema_decay = 0.999, ema_every = 4 (the same two launches; three steps in four the update returns at once)
so that drift of the machine lands on all of them alike.  Each process warms up, then times `--windows` windows of `--steps`
steps with a host clock around a device synchronise, and reports the median window, the peak device memory of the torch
allocator and the bytes one update moves (12 per averaged element: read p, read ema, write ema; embedding rows that never had a
gradient are not touched).
    python tools/ema_bench.py --parent ../parent-checkout --rounds 4 [--out result.json] [--md table.md]
    python tools/ema_bench.py --worker --root DIR --every E          (one process of the above; E = 0: no argument at all)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECAY = 0.999


def worker(args):
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from cris.pytorch_amd import arch, synth
    from cris.pytorch_amd.trainer import NativeTrainer
    dev = torch.device("cuda:0")
    clip, head = arch.specs_by_name("r50")
    kw = {"ema_decay": DECAY, "ema_every": args.every} if args.every > 0 else {}      # (the parent's trainer has no such argument)
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
    res = {"every": args.every, "ms_per_step_windows": [round(x, 4) for x in ms], "ms_per_step": round(statistics.median(ms), 4),
           "loss": float(loss), "peak_allocated_mb": round(torch.cuda.max_memory_allocated(dev) / 2 ** 20, 1),
           "peak_reserved_mb": round(torch.cuda.max_memory_reserved(dev) / 2 ** 20, 1), "device": torch.cuda.get_device_name(0)}
    if args.every > 0:
        ema = tr._ema
        n = ema.num_elements
        skipped = sum(int((live == 0).sum()) * ema.views[name].shape[1] for name, live in ema.row_live.items())
        res.update(ema_elements=n, ema_buffer_mb=round(ema.flat.numel() * 4 / 2 ** 20, 1), skipped_elements=skipped,
                   bytes_per_update=12 * (n - skipped), ema_updates=tr.ema_num_updates, steps=tr.step_idx)
    print("RESULT " + json.dumps(res), flush=True)


def table(summary):
    lines = ["| arm | ms/step (processes) | min | max | median | peak allocated MB | peak reserved MB |", "|---|---|---|---|---|---|---|"]
    for name, s in summary.items():
        runs = s["ms_per_step_runs"]
        lines.append("| %s | %s | %.3f | %.3f | %.3f | %.0f | %.0f |" % (name, " ".join("%.3f" % x for x in runs), min(runs), max(runs),
                                                                       s["ms_per_step_median"], s["peak_allocated_mb"], s["peak_reserved_mb"]))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--every", type=int, default=0)
    ap.add_argument("--parent", default=None, help="built checkout of the commit to compare against")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    variants = [("off", HERE, 0), ("every1", HERE, 1), ("every4", HERE, 4)]
    if args.parent:
        variants.insert(0, ("parent", args.parent, 0))
    runs = {name: [] for name, _, _ in variants}
    for r in range(args.rounds):
        for name, root, every in (variants if r % 2 == 0 else variants[::-1]):
            # the worker is THIS file for every arm (the parent checkout has no such tool); --root selects the package it imports
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--every", str(every), "--steps", str(args.steps),
                   "--windows", str(args.windows), "--warmup", str(args.warmup)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
            out = p.stdout.decode()
            line = [x for x in out.splitlines() if x.startswith("RESULT ")]
            if p.returncode != 0 or not line:                              # nothing more is started on the GPU after a failure
                sys.exit("round %d %s: rc %d\n%s" % (r, name, p.returncode, out[-3000:]))
            res = json.loads(line[0][7:])
            runs[name].append(res)
            print("round %d %-7s %.3f ms/step  windows %s  peak %.0f MB allocated" % (r, name, res["ms_per_step"], res["ms_per_step_windows"],
                                                                                   res["peak_allocated_mb"]), flush=True)
    summary = {name: {"ms_per_step_median": round(statistics.median(x["ms_per_step"] for x in rs), 4),
                      "ms_per_step_runs": [x["ms_per_step"] for x in rs], "losses": sorted({x["loss"] for x in rs}),
                      "peak_allocated_mb": max(x["peak_allocated_mb"] for x in rs), "peak_reserved_mb": max(x["peak_reserved_mb"] for x in rs)}
               for name, rs in runs.items()}
    base = summary.get("parent", summary["off"])
    spread = max(base["ms_per_step_runs"]) - min(base["ms_per_step_runs"])
    e1 = runs["every1"][0]
    cost = {name: round(summary[name]["ms_per_step_median"] - base["ms_per_step_median"], 4) for name in summary}
    derived = {"baseline_arm": "parent" if "parent" in summary else "off", "baseline_spread_ms": round(spread, 4), "cost_ms_vs_baseline": cost,
               "bytes_per_update": e1["bytes_per_update"], "ema_elements": e1["ema_elements"], "skipped_elements": e1["skipped_elements"],
               "ema_buffer_mb": e1["ema_buffer_mb"]}
    if cost["every1"] > 0:
        derived["every1_bytes_per_second"] = round(e1["bytes_per_update"] / (cost["every1"] * 1e-3), 0)
    result = {"config": "r50 416x416 batch 8, one GPU, launch=graph, ema_decay=%g" % DECAY, "device": e1["device"],
              "steps_per_window": args.steps, "windows": args.windows, "rounds": args.rounds, "summary": summary, "derived": derived, "runs": runs}
    print(json.dumps(summary))
    print(json.dumps(derived))
    print(table(summary))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    if args.md:
        with open(args.md, "w") as f:
            f.write(table(summary))


if __name__ == "__main__":
    main()
