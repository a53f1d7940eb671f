"""What the per-step learning-rate schedule costs per train step (profiles/lr_schedule.md): NativeTrainer at BASELINE.json
configs[1] (R50, 416 x 416, batch 8, one GPU, the step as one captured graph) timed in fresh processes that alternate between
  parent   - a built checkout of the commit to compare against (--parent DIR): its trainer has no lr_schedule
  off      - this tree, lr_schedule = None (the same launches as the parent)
  on       - this tree, a warm-up + cosine table of one row per timed step (one more launch per Adam table: cris_adam_schedule_lrs)
so that drift of the machine lands on all of them alike.  Each process warms up, then times `--windows` windows of `--steps` steps
with a host clock around a device synchronise, and reports the median window.  The `on` arm also checks that the trainer kept one
captured graph through all of its steps and that the last step used the row it should have.
    python tools/lr_schedule_bench.py --parent ../parent-checkout --rounds 3 [--out result.json] [--md table.md]
    python tools/lr_schedule_bench.py --worker --root DIR --arm off|on|parent          (one process of the above)"""
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
    import numpy as np
    import torch
    from cris.pytorch_amd import arch, synth
    from cris.pytorch_amd.trainer import NativeTrainer
    dev = torch.device("cuda:0")
    clip, head = arch.specs_by_name("r50")
    kw, table = {}, None
    if args.arm == "on":                             # (the parent's trainer has no such argument, and no lr module)
        from cris.pytorch_amd import lr
        n = args.warmup + args.windows * args.steps
        table = lr.with_warmup(lr.cosine([1e-5, 1e-4], n), max(n // 10, 1), 0.01)
        kw["lr_schedule"] = table
    tr = NativeTrainer(clip, head, arch.synthetic_state_dict(clip, head, 0), dev, launch="graph", **kw)
    batches = [tuple(t.to(dev) for t in synth.make_batch(8, 416, head.word_len, 0, s)) for s in range(4)]
    for i in range(args.warmup):
        tr.train_step(*batches[i % 4])
    torch.cuda.synchronize()
    assert tr.launch == "graph" and tr._graph is not None, tr.graph_error
    graph = tr._graph
    ms = []
    for _ in range(args.windows):
        t0 = time.perf_counter()
        for i in range(args.steps):
            loss, _ = tr.train_step(*batches[i % 4])
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / args.steps * 1e3)
    assert tr._graph is graph                        # one capture for the whole run
    res = {"arm": args.arm, "ms_per_step_windows": [round(x, 4) for x in ms], "ms_per_step": round(statistics.median(ms), 4),
           "loss": float(loss), "steps": tr.step_idx, "device": torch.cuda.get_device_name(0)}
    if table is not None:
        last = tr.current_lrs.cpu().numpy()
        assert np.array_equal(last, table[tr.step_idx - 1]), (last, table[tr.step_idx - 1])
        res.update(table_rows=int(table.shape[0]), table_bytes=int(table.nbytes), last_lrs=[float(x) for x in last],
                   launches_added=sum(1 for t in tr.adam.tables.values() if t.n), descriptors=len(tr.names))
    print("RESULT " + json.dumps(res), flush=True)


def table_md(summary):
    lines = ["| arm | ms/step (processes) | min | max | median |", "|---|---|---|---|---|"]
    for name, s in summary.items():
        runs = s["ms_per_step_runs"]
        lines.append("| %s | %s | %.3f | %.3f | %.3f |" % (name, " ".join("%.3f" % x for x in runs), min(runs), max(runs), s["ms_per_step_median"]))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--arm", default="off", choices=["parent", "off", "on"])
    ap.add_argument("--parent", default=None, help="built checkout of the commit to compare against")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    variants = [("off", HERE), ("on", HERE)]
    if args.parent:
        variants.insert(0, ("parent", args.parent))
    runs = {name: [] for name, _ in variants}
    for r in range(args.rounds):
        for name, root in (variants if r % 2 == 0 else variants[::-1]):
            # the worker is THIS file for every arm (the parent checkout has no such tool); --root selects the package it imports
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--arm", name, "--steps", str(args.steps),
                   "--windows", str(args.windows), "--warmup", str(args.warmup)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
            out = p.stdout.decode()
            line = [x for x in out.splitlines() if x.startswith("RESULT ")]
            if p.returncode != 0 or not line:                              # nothing more is started on the GPU after a failure
                sys.exit("round %d %s: rc %d\n%s" % (r, name, p.returncode, out[-3000:]))
            res = json.loads(line[0][7:])
            runs[name].append(res)
            print("round %d %-7s %.3f ms/step  windows %s" % (r, name, res["ms_per_step"], res["ms_per_step_windows"]), flush=True)
    summary = {name: {"ms_per_step_median": round(statistics.median(x["ms_per_step"] for x in rs), 4),
                      "ms_per_step_runs": [x["ms_per_step"] for x in rs], "losses": sorted({x["loss"] for x in rs})}
               for name, rs in runs.items()}
    base = summary.get("parent", summary["off"])
    spread = max(base["ms_per_step_runs"]) - min(base["ms_per_step_runs"])
    on = runs["on"][0]
    derived = {"baseline_arm": "parent" if "parent" in summary else "off", "baseline_spread_ms": round(spread, 4),
               "cost_ms_vs_baseline": {name: round(summary[name]["ms_per_step_median"] - base["ms_per_step_median"], 4) for name in summary},
               "launches_added": on["launches_added"], "descriptors": on["descriptors"], "table_rows": on["table_rows"],
               "table_bytes": on["table_bytes"]}
    result = {"config": "r50 416x416 batch 8, one GPU, launch=graph; on = warm-up + cosine table, one row per step", "device": on["device"],
              "steps_per_window": args.steps, "windows": args.windows, "rounds": args.rounds, "summary": summary, "derived": derived, "runs": runs}
    print(json.dumps(summary))
    print(json.dumps(derived))
    print(table_md(summary))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    if args.md:
        with open(args.md, "w") as f:
            f.write(table_md(summary))


if __name__ == "__main__":
    main()
