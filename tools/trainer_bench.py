"""What the options of NativeTrainer cost per train step, and the proof that a change of the trainer changed nothing.

Timing (profiles/grad_clip.md, grad_accum.md, ema.md, lr_schedule.md, trainer_refactor.md, adamw.md, seg_loss.md): the trainer at BASELINE.json configs[1]
(R50, 416 x 416, micro-batch 8, one GPU, the whole optimizer step as one captured graph), one ARM per row of the table below, each
timed in fresh processes that alternate between the arms - and, with --parent DIR, the same arms run from a built checkout of the
commit to compare against - so that drift of the machine lands on all of them alike.  Each process warms up, then times `--windows`
windows of `--steps` micro-batches with a host clock around a device synchronise and reports the median window and the peak device
memory of the torch allocator.  An arm of this tree is judged against the parent's arm of the same name: its median has to lie
within the parent processes' own spread (max - min) of the parent's median.  An arm whose constructor arguments the parent's
trainer does not know (adamw, adamw_schedule, dice against a commit before them) runs from this tree only.
    python tools/trainer_bench.py [--arms plain,schedule,all] [--parent ../parent-checkout] --rounds 4 [--out result.json] [--md table.md]

--check: every arm in each of the launch modes eager / graph / cmdlist, and `plain` and `all` once more with CRIS_FORCE_DIST=1 (the
exchange branch of the stage hooks, through a one-rank communicator that counts the exchanges), on the tiny spec at 64 x 64: four
steps from synthetic_state_dict(..., 0) on synth.make_batch(..., t).  A process prints the losses and metrics as hex floats, a
sha256 of the state the steps left behind (parameters, BatchNorm buffers, Adam moments, the step / seed / generation counters, the
average and its state record, the rates of the last step, the loss terms of the last step) and, for cmdlist, a sha256 of the recorded list (every entry's name and
its non-pointer arguments; --dump-launches DIR writes the text).  With --parent the run fails unless all of them are equal,
exactly, between the two trees.
    python tools/trainer_bench.py --check --parent ../parent-checkout [--out result.json]

The driver starts one process at a time, each under its own time limit, and nothing more after the first that fails.
    python tools/trainer_bench.py --worker --root DIR --arm NAME [--check --launch MODE]          (one process of the above)"""
import argparse
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEDULE = "warm-up + cosine, one row per step"          # (the table needs the number of steps: the worker builds it)
NO_DECAY = "no_decay_1d_and_positional"                   # (a rule of the package under --root: the worker looks it up)
ARMS = {                                                  # name -> constructor arguments
    "plain": {},
    "clip": {"max_norm": 1.0},                            # three more launches: two cris_grad_sumsq, one cris_grad_clip_finalize
    "track_norm": {"track_grad_norm": True},
    "accum2": {"accum_steps": 2},                         # a batch of 2 x the micro-batch per step
    "ema_every1": {"ema_decay": 0.999, "ema_every": 1},   # two more launches: cris_ema_advance, cris_ema_update
    "ema_every4": {"ema_decay": 0.999, "ema_every": 4},   # the same two; three steps in four the update returns at once
    "schedule": {"lr_schedule": SCHEDULE},                # one more launch per Adam table: cris_adam_schedule_lrs
    "all": {"max_norm": 1.0, "accum_steps": 2, "ema_decay": 0.999, "ema_every": 1, "lr_schedule": SCHEDULE},
    # decoupled decay with the usual exemptions: the Adam launches become cris_adamw_step (not part of `all`, whose recorded list
    # is compared with parents that do not have them)
    "adamw": {"weight_decay": 0.01, "decoupled_weight_decay": True, "no_decay": NO_DECAY},
    "adamw_schedule": {"weight_decay": 0.01, "decoupled_weight_decay": True, "no_decay": NO_DECAY, "lr_schedule": SCHEDULE},
    # BCE + soft Dice: cris_seg_loss_fwd / cris_seg_loss_bwd in the place of cris_bce_fwd / cris_bce_bwd, the same number of launches
    "dice": {"loss": {"dice_weight": 1.0}},               # (the fields of an ops.SegLoss of the package under --root: the worker builds it)
}
CHECK_MAX_NORM = 1e-3                                     # --check: far below the tiny spec's gradient norm, so that it does clip
CHECK_STEPS = 4                                           # eager, capture / recording, two replays
LAUNCHES = ("eager", "graph", "cmdlist")
DIST_ARMS = ("plain", "all")                              # --check: once more with CRIS_FORCE_DIST=1 (K = 1 and K = 2 through the exchange)
MICRO = {"bench": 8, "check": 2}                          # samples per micro-batch


def one_rank_comm(Comm):
    """what CRIS_FORCE_DIST=1 needs on one GPU without a process group: a communicator of one rank whose all-reduces leave the
    data as it is (the sum and the MAX over one rank) and count what they are asked for"""
    class OneRank(Comm):
        supports_max_u8 = True

        def __init__(self):
            super().__init__()
            self.calls = {"sum": 0, "max": 0, "wait_all": 0}

        def allreduce_async(self, t, op="sum"):
            self.calls[op] += 1

        def wait_all(self):
            self.calls["wait_all"] += 1
    return OneRank()


def make_trainer(args, spec, n_steps):
    """(trainer, head, K, the schedule's table or None) of args.arm, from the package under args.root"""
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from cris.pytorch_amd import arch, debug, lr, ops
    from cris.pytorch_amd.engine import Comm
    from cris.pytorch_amd import trainer
    from cris.pytorch_amd.trainer import NativeTrainer
    kw, table = dict(ARMS[args.arm]), None
    if "no_decay" in kw:
        kw["no_decay"] = getattr(trainer, kw["no_decay"])
    if "loss" in kw:
        kw["loss"] = ops.SegLoss(**kw["loss"])
    if "lr_schedule" in kw:
        kw["lr_schedule"] = table = lr.with_warmup(lr.cosine([1e-5, 1e-4], n_steps), max(n_steps // 10, 1), 0.01)
    if args.check and "max_norm" in kw:
        kw["max_norm"] = CHECK_MAX_NORM
    if debug.HOOKS.force_dist:
        kw["comm"] = one_rank_comm(Comm)
    clip, head = arch.specs_by_name(spec)
    tr = NativeTrainer(clip, head, arch.synthetic_state_dict(clip, head, 0), torch.device("cuda:0"), launch=args.launch, **kw)
    return tr, head, kw.get("accum_steps", 1), table


def time_worker(args):
    import numpy as np
    import torch
    K = ARMS[args.arm].get("accum_steps", 1)
    steps, warmup = max(args.steps // K, 4), max(args.warmup // K, 4)
    tr, head, K, table = make_trainer(args, "r50", warmup + args.windows * steps)
    from cris.pytorch_amd import synth
    dev = torch.device("cuda:0")
    batches = [tuple(t.to(dev) for t in synth.make_batch(MICRO["bench"] * K, 416, head.word_len, 0, s)) for s in range(4)]
    for i in range(warmup):
        tr.train_step(*batches[i % 4])
    torch.cuda.synchronize()
    assert tr.launch == "graph" and tr._graph is not None, tr.graph_error
    graph, ms = tr._graph, []
    for _ in range(args.windows):
        t0 = time.perf_counter()
        for i in range(steps):
            loss, _ = tr.train_step(*batches[i % 4])
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / steps * 1e3)
    assert tr._graph is graph                            # one capture for the whole run
    res = {"arm": args.arm, "accum_steps": K, "steps_per_window": steps, "ms_per_step_windows": [round(x, 4) for x in ms],
           "ms_per_step": round(statistics.median(ms), 4), "loss": float(loss), "steps": tr.step_idx,
           "peak_allocated_mb": round(torch.cuda.max_memory_allocated(dev) / 2 ** 20, 1),
           "peak_reserved_mb": round(torch.cuda.max_memory_reserved(dev) / 2 ** 20, 1), "device": torch.cuda.get_device_name(0)}
    if tr.max_norm > 0 or tr.track_grad_norm:
        res["grad_norm"] = float(tr.grad_norm)
    if tr._ema is not None:                              # 12 bytes per averaged element: read p, read ema, write ema; embedding
        ema, n = tr._ema, tr._ema.num_elements           # rows that never had a gradient are not touched
        skipped = sum(int((live == 0).sum()) * ema.views[name].shape[1] for name, live in ema.row_live.items())
        res.update(ema_elements=n, ema_buffer_mb=round(ema.flat.numel() * 4 / 2 ** 20, 1), skipped_elements=skipped,
                   bytes_per_update=12 * (n - skipped), ema_updates=tr.ema_num_updates)
    if getattr(tr, "loss_terms", None) is not None:      # the loss is the weighted sum of the terms the step reports
        res["loss_terms"] = [float(x) for x in tr.loss_terms.cpu()]
        spec = tr.loss_spec
        want = spec.bce_weight * res["loss_terms"][0] + spec.dice_weight * res["loss_terms"][1]
        assert abs(res["loss"] - want) <= 1e-5 * max(1.0, abs(want)), (res["loss"], res["loss_terms"])
    if table is not None:                                # the last step used the row it should have
        last = tr.current_lrs.cpu().numpy()
        assert np.array_equal(last, table[tr.step_idx - 1]), (last, table[tr.step_idx - 1])
        res.update(table_rows=int(table.shape[0]), table_bytes=int(table.nbytes), last_lrs=[float(x) for x in last],
                   launches_added=sum(1 for t in tr.adam.tables.values() if t.n), descriptors=len(tr.names))
    print("RESULT " + json.dumps(res), flush=True)


def launch_text(cmds):
    """one line per entry of a recorded command list: its name, then its ints and floats (pointers differ between processes)"""
    import ctypes as C
    from cris.pytorch_amd import hip
    lines = []
    for _, args, name in cmds:
        types = hip._SIGS[name][1] if args is not None else []
        lines.append(" ".join([name] + [repr(a) for a, t in zip(args or (), types) if t is not C.c_void_p]))
    return "\n".join(lines) + "\n"


def check_worker(args):
    import torch
    tr, head, K, _ = make_trainer(args, "tiny", CHECK_STEPS)
    from cris.pytorch_amd import synth
    losses, metrics = [], []
    for t in range(CHECK_STEPS):
        loss, metric = tr.train_step(*[x.to("cuda:0") for x in synth.make_batch(MICRO["check"] * K, 64, head.word_len, 0, t)])
        losses.append(float(loss).hex())
        metrics.append([float(x).hex() for x in metric.cpu()])
    torch.cuda.synchronize()
    assert tr.launch == args.launch and (args.launch == "eager" or tr._graph is not None or tr._cmds is not None), tr.graph_error
    e = tr.engine
    state = list(e.P.values()) + list(e.Bf.values()) + list(tr.adam.m) + list(tr.adam.v) + [tr.step_dev, tr.seed_dev, tr.xgen_dev]
    if tr._ema is not None:
        state += [tr._ema.flat, tr._ema.state]
    if tr._lr is not None:
        state.append(tr.current_lrs)
    if getattr(tr, "loss_terms", None) is not None:
        state.append(tr.loss_terms)
    h = hashlib.sha256()
    for t in state:
        h.update(t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes())
    res = {"arm": args.arm, "launch": args.launch, "force_dist": os.environ.get("CRIS_FORCE_DIST", "0") == "1", "grad_exchange": tr.grad_exchange,
           "exchanges": getattr(tr.comm, "calls", None), "losses": losses, "metrics": metrics, "state_sha256": h.hexdigest(), "state_tensors": len(state)}
    if tr._cmds is not None:
        text = launch_text(tr._cmds.cmds)
        res.update(launches=text.count("\n"), launches_sha256=hashlib.sha256(text.encode()).hexdigest())
        if args.dump_launches:
            os.makedirs(args.dump_launches, exist_ok=True)
            name = "%s_%s%s.txt" % (args.label, args.arm, "_dist" if res["force_dist"] else "")
            with open(os.path.join(args.dump_launches, name), "w") as f:
                f.write(text)
    print("RESULT " + json.dumps(res), flush=True)


def knows(root, arm):
    """does the trainer of the tree at `root` take every constructor argument of `arm`?  (read from the constructor's parameter
    list in its source: no import)"""
    with open(os.path.join(root, "cris", "pytorch_amd", "trainer.py")) as f:
        src = f.read()
    sig = re.search(r"class NativeTrainer:.*?def __init__\((.*?)\):\n", src, flags=re.S).group(1)
    return all(re.search(r"\b%s\b" % k, sig) for k in ARMS[arm])


def run_worker(label, root, arm, extra=(), env=None):
    """one fresh process, under its own time limit; the driver ends at the first that fails and starts nothing after it.  The
    worker is THIS file for every tree (--root selects the package it imports)"""
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--arm", arm, "--label", label, *extra]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, env=dict(os.environ, **(env or {})))
    out = p.stdout.decode()
    line = [x for x in out.splitlines() if x.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        sys.exit("%s %s %s: rc %d\n%s" % (label, arm, " ".join(extra), p.returncode, out[-3000:]))
    return json.loads(line[0][7:])


def check_driver(args, arms):
    trees = ([("parent", args.parent)] if args.parent else []) + [("this", HERE)]
    cases = [(arm, launch, False) for arm in arms for launch in LAUNCHES] + [(arm, launch, True) for arm in DIST_ARMS for launch in LAUNCHES]
    rows, differing = [], 0
    for arm, launch, dist in cases:
        extra = ["--check", "--launch", launch] + (["--dump-launches", args.dump_launches] if args.dump_launches else [])
        got = {label: run_worker(label, root, arm, extra, {"CRIS_FORCE_DIST": "1" if dist else "0"}) for label, root in trees
               if knows(root, arm)}
        this = got["this"]
        assert this["force_dist"] == dist and (this["grad_exchange"] != "none") == dist and (not dist or this["exchanges"]["sum"] > 0), this
        same = {k: got["parent"].get(k) == this[k] for k in ("losses", "metrics", "state_sha256", "launches_sha256", "exchanges")
                if this.get(k) is not None} if "parent" in got else {}
        differing += int(not all(same.values()))
        rows.append({"arm": arm + (" + CRIS_FORCE_DIST=1" if dist else ""), "launch": launch, "equal": same, **got})
        print("%-30s %-8s %s  state %s  launches %s" % (rows[-1]["arm"], launch, " ".join("%s=%s" % kv for kv in same.items()) or "(no parent with this arm)",
                                                     this["state_sha256"][:12], (this.get("launches_sha256") or "-")[:12]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"steps": CHECK_STEPS, "cases": rows}, f, indent=1)
    if differing:
        sys.exit("CHECK FAILED: %d of %d cases differ from the parent" % (differing, len(cases)))
    print("CHECK %s: %d cases (arm x launch mode)" % ("OK, every case equal to the parent in losses, metrics, state and recorded launches"
                                                     if args.parent else "ran without a parent to compare with", len(cases)))


def table_md(summary):
    lines = ["| arm | K | ms/optimizer step (processes) | min | max | median | samples/s | peak allocated MB | peak reserved MB | against the parent's arm |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for name, s in summary.items():
        runs, K, med = s["ms_per_step_runs"], s["accum_steps"], s["ms_per_step_median"]
        lines.append("| %s | %d | %s | %.3f | %.3f | %.3f | %.1f | %.0f | %.0f | %s |"
                     % (name, K, " ".join("%.3f" % x for x in runs), min(runs), max(runs), med, MICRO["bench"] * K / med * 1e3,
                        s["peak_allocated_mb"], s["peak_reserved_mb"], s.get("verdict", "")))
    return "\n".join(lines) + "\n"


def time_driver(args, arms):
    variants = [("parent:" + a, args.parent, a) for a in arms if args.parent and knows(args.parent, a)] + [(a, HERE, a) for a in arms]
    extra = ["--launch", "graph", "--steps", str(args.steps), "--windows", str(args.windows), "--warmup", str(args.warmup)]
    runs = {label: [] for label, _, _ in variants}
    for r in range(args.rounds):
        for label, root, arm in (variants if r % 2 == 0 else variants[::-1]):
            res = run_worker(label, root, arm, extra)
            runs[label].append(res)
            print("round %d %-18s %.3f ms/step  windows %s  peak %.0f MB allocated" % (r, label, res["ms_per_step"], res["ms_per_step_windows"],
                                                                                    res["peak_allocated_mb"]), flush=True)
    summary = {label: {"accum_steps": rs[0]["accum_steps"], "ms_per_step_median": round(statistics.median(x["ms_per_step"] for x in rs), 4),
                       "ms_per_step_runs": [x["ms_per_step"] for x in rs], "losses": sorted({x["loss"] for x in rs}),
                       "peak_allocated_mb": max(x["peak_allocated_mb"] for x in rs), "peak_reserved_mb": max(x["peak_reserved_mb"] for x in rs)}
               for label, rs in runs.items()}
    for a in arms:
        if "parent:" + a not in summary:
            continue
        p, s = summary["parent:" + a], summary[a]
        spread, diff = max(p["ms_per_step_runs"]) - min(p["ms_per_step_runs"]), s["ms_per_step_median"] - p["ms_per_step_median"]
        s.update(parent_spread_ms=round(spread, 4), diff_ms_vs_parent=round(diff, 4), within_parent_spread=abs(diff) <= spread,
                 verdict="%+.3f ms, parent spread %.3f: %s" % (diff, spread, "within" if abs(diff) <= spread else "OUTSIDE"))
    base = summary.get("parent:plain", summary.get("plain"))
    derived = {}
    if base is not None:                                 # what each arm costs on top of the plain step, and the plain step's own spread
        derived = {"baseline_spread_ms": round(max(base["ms_per_step_runs"]) - min(base["ms_per_step_runs"]), 4),
                   "cost_ms_vs_plain": {label: round(s["ms_per_step_median"] - base["ms_per_step_median"], 4) for label, s in summary.items()}}
        if "plain" in summary and base is not summary["plain"]:          # and on top of THIS tree's plain step
            own = summary["plain"]
            derived.update(own_plain_spread_ms=round(max(own["ms_per_step_runs"]) - min(own["ms_per_step_runs"]), 4),
                           cost_ms_vs_own_plain={label: round(s["ms_per_step_median"] - own["ms_per_step_median"], 4)
                                                 for label, s in summary.items() if not label.startswith("parent:")})
    extras = {label: {k: rs[0][k] for k in ("ema_elements", "ema_buffer_mb", "skipped_elements", "bytes_per_update", "table_rows", "table_bytes",
                                            "launches_added", "descriptors", "grad_norm") if k in rs[0]} for label, rs in runs.items()}
    first = next(iter(runs.values()))[0]
    result = {"config": "r50 416x416 micro-batch %d, one GPU, launch=graph" % MICRO["bench"], "device": first["device"], "arms": {a: ARMS[a] for a in arms},
              "micro_batches_per_window": args.steps, "windows": args.windows, "rounds": args.rounds, "summary": summary, "derived": derived,
              "extras": extras, "runs": runs}
    print(json.dumps(summary))
    print(json.dumps(derived))
    print(table_md(summary))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    if args.md:
        with open(args.md, "w") as f:
            f.write(table_md(summary))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--arm", default="plain", choices=list(ARMS))
    ap.add_argument("--label", default="this")
    ap.add_argument("--launch", default="graph", choices=LAUNCHES)
    ap.add_argument("--check", action="store_true", help="compare losses, state and recorded launches of every arm with --parent, exactly")
    ap.add_argument("--dump-launches", default=None, metavar="DIR", help="--check: write every recorded command list as text")
    ap.add_argument("--arms", default=None, help="comma-separated (default: every arm)")
    ap.add_argument("--parent", default=None, help="built checkout of the commit to compare against")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=100, help="micro-batches per timed window")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    if args.worker:
        return check_worker(args) if args.check else time_worker(args)
    arms = args.arms.split(",") if args.arms else list(ARMS)
    unknown = [a for a in arms if a not in ARMS]
    if unknown:
        ap.error("unknown arms %s (known: %s)" % (unknown, ", ".join(ARMS)))
    return check_driver(args, arms) if args.check else time_driver(args, arms)


if __name__ == "__main__":
    main()
