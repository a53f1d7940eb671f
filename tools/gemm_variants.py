"""Per-shape A/B of the conv_gemm tile variants (cris_conv_gemm_variant): every GEMM shape of the benchmarked training step
(profiles/r02_gemm_shapes.tsv: forward + input-gradient launches) timed with each applicable tile variant - lean epilogue
with BatchNorm statistics, random bf16 operands, `reps` back-to-back launches inside one HIP graph, variants interleaved
round-robin over `rounds` rounds (median reported).  Prints one line per shape and a summary of what the current automatic
choice loses against the best variant.

    python tools/gemm_variants.py [--min-m 5000] [--rounds 5] [--tsv out.tsv]

--fp8: the ModifiedResNet-50 Bottleneck convolutions of the inference forward at --batch (416x416 input) instead, each as the
folded bf16 launch (EPI 2: bias + ReLU, bf16 output, the library's tile) and as the FP8 launch (cris_conv_gemm_fp8: bias + ReLU,
fp8 output, the automatic tile and every named one), interleaved in the same way.

    python tools/gemm_variants.py --fp8 [--batch 32] [--rounds 5] [--tsv out.tsv]
"""
import argparse
import os
import re
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cris.pytorch_amd import ops                 # noqa: E402
from cris.pytorch_amd.ops import Geom            # noqa: E402

dev = torch.device("cuda:0")
bf = torch.bfloat16
HW = {346112: 208, 86528: 104, 21632: 52, 5408: 26, 1352: 13}


def shapes_of_step():
    """[(M, N, K, k, launches per step)] from the committed shape table"""
    out = []
    for line in open(os.path.join(ROOT, "profiles", "r02_gemm_shapes.tsv")):
        m = re.match(r"conv_gemm\tM(\d+) N(\d+) K(\d+) k(\d)\t([\d.]+)", line)
        if m:
            out.append((int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4)), float(m.group(5))))
    return out


def make_runner(M, N, K, k, variant, stats, reps):
    C = K // (k * k)
    hw = HW[M]
    g = Geom(8, hw, hw, C, k, k, 1, k // 2)
    A = torch.randn(M, C, device=dev).to(bf)
    W = (torch.randn(N, K, device=dev) * 0.05).to(bf)
    out = torch.empty(M, N, device=dev, dtype=bf)
    for _ in range(2):
        ops.conv_gemm(A, W, g, N, out=out, stats=stats, variant=variant)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(reps):
            ops.conv_gemm(A, W, g, N, out=out, stats=stats, variant=variant)
    gr.replay()
    torch.cuda.synchronize()

    def run():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        gr.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps
    return run, (A, W, out, gr)


# (H, Cin, N, k, convolutions per R50 forward): layer1 .. layer4 at 104 / 52 / 26 / 13 pixels; a stride-2 block runs its conv1
# and conv2 at the input resolution (the pool follows conv2), its downsample after the pool
R50_BOTTLENECK = [
    (104, 64, 64, 1, 1), (104, 256, 64, 1, 2), (104, 64, 64, 3, 3), (104, 64, 256, 1, 4),
    (104, 256, 128, 1, 1), (104, 128, 128, 3, 1), (52, 512, 128, 1, 3), (52, 128, 128, 3, 3), (52, 128, 512, 1, 4), (52, 256, 512, 1, 1),
    (52, 512, 256, 1, 1), (52, 256, 256, 3, 1), (26, 1024, 256, 1, 5), (26, 256, 256, 3, 5), (26, 256, 1024, 1, 6), (26, 512, 1024, 1, 1),
    (26, 1024, 512, 1, 1), (26, 512, 512, 3, 1), (13, 2048, 512, 1, 2), (13, 512, 512, 3, 2), (13, 512, 2048, 1, 3), (13, 1024, 2048, 1, 1),
]


def make_runner_fp8(B, H, C, N, k, variant, reps):
    """one R50 Bottleneck convolution at batch B: 'bf16' = the folded bf16 launch, else the fp8 launch with tile `variant`"""
    g = Geom(B, H, H, C, k, k, 1, k // 2)
    bias = torch.randn(N, device=dev) * 0.1
    if variant == "bf16":
        A = torch.randn(B * H * H, C, device=dev).to(bf)
        W = (torch.randn(N, g.K, device=dev) * 0.05).to(bf)
        out = torch.empty(g.M, N, device=dev, dtype=bf)

        def launch():
            ops.conv_gemm(A, W, g, N, bias=bias, act=1, out=out)
        keep = (A, W, out)
    else:
        A = (torch.randn(B * H * H, C, device=dev) * 16).to(ops.FP8)
        tab = ops.PackTableFp8()
        W8, e_w = tab.add(torch.randn(N, C, k * k, device=dev), N, C, k * k)
        tab.run()
        out8 = torch.empty(g.M, N, device=dev, dtype=ops.FP8)
        v = -1 if variant == "fp8" else variant

        def launch():
            ops.conv_gemm_fp8(A, W8, e_w, g, N, -4, bias=bias, act=1, out8=out8, e_y=2, variant=v)
        keep = (A, W8, e_w, out8)
    for _ in range(2):
        launch()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(reps):
            launch()
    gr.replay()
    torch.cuda.synchronize()

    def run():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        gr.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps
    return run, (keep, gr)


def main_fp8(args):
    arms = ["bf16", "fp8"] + ["fp8:" + n for n in ops.gemm_fp8_variants()]
    rows = []
    tot = {a: 0.0 for a in arms}
    tot3 = {a: 0.0 for a in arms}
    for (H, C, N, k, cnt) in R50_BOTTLENECK:
        runners = {a: make_runner_fp8(args.batch, H, C, N, k, a.split(":")[1] if ":" in a else a, args.reps) for a in arms}
        ts = {a: [] for a in arms}
        for _ in range(args.rounds):
            for a, (run, _) in runners.items():
                ts[a].append(run())
        med = {a: statistics.median(t) for a, t in ts.items()}
        M, K = args.batch * H * H, k * k * C
        fl = 2.0 * M * N * K
        for a in arms:
            tot[a] += med[a] * cnt
            if k == 3:
                tot3[a] += med[a] * cnt
        print("GEMMFP8 M%d N%d K%d k%d x%d | bf16 %.1fus %.0fTF | fp8 %.1fus %.0fTF | %.2fx | %s" % (
            M, N, K, k, cnt, med["bf16"], fl / med["bf16"] / 1e6, med["fp8"], fl / med["fp8"] / 1e6, med["bf16"] / med["fp8"],
            " ".join("%s=%.1f" % (a, med[a]) for a in arms[2:])), flush=True)
        rows.append((M, N, K, k, cnt, med))
        del runners
        torch.cuda.empty_cache()
    print("GEMMFP8 Bottleneck convolutions per forward, batch %d: bf16 %.3f ms, fp8 %.3f ms (%.2fx); 3x3 only: bf16 %.3f ms, fp8 %.3f ms (%.2fx)" % (
        args.batch, tot["bf16"] / 1e3, tot["fp8"] / 1e3, tot["bf16"] / tot["fp8"], tot3["bf16"] / 1e3, tot3["fp8"] / 1e3,
        tot3["bf16"] / tot3["fp8"]))
    if args.tsv:
        with open(args.tsv, "w") as f:
            f.write("M\tN\tK\tk\tper_forward\t" + "\t".join(arms) + "\n")
            for (M, N, K, k, cnt, med) in rows:
                f.write("%d\t%d\t%d\t%d\t%d\t" % (M, N, K, k, cnt) + "\t".join("%.1f" % med[a] for a in arms) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-m", type=int, default=1000)
    ap.add_argument("--min-k", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--variants", default="")
    ap.add_argument("--tsv", default=None)
    ap.add_argument("--fp8", action="store_true", help="bf16 folded vs FP8 on the R50 Bottleneck convolutions (see the docstring)")
    ap.add_argument("--batch", type=int, default=32)
    args = ap.parse_args()
    if args.fp8:
        return main_fp8(args)
    names = ops.gemm_variants()
    want = [v for v in (args.variants.split(",") if args.variants else names) if not v.startswith("skinny")]
    rows = []
    tot_auto = tot_best = 0.0
    for (M, N, K, k, cnt) in shapes_of_step():
        if M < args.min_m or K < args.min_k or M not in HW:
            continue
        C = K // (k * k)
        runners = {}
        for v in ["auto"] + want:
            if v != "auto" and v.startswith("8w") and C % 64:
                continue
            if v != "auto" and v.startswith("8w") and v != "8w128x128" and (M < 5000 or (v != "8w256x128" and N <= 128) or (v == "8w256x128" and N > 256)):
                continue
            if v == "8w128x128" and (M > 30000 or N <= 64):
                continue
            try:
                runners[v] = make_runner(M, N, K, k, -1 if v == "auto" else v, True, args.reps)
            except Exception as e:      # noqa: BLE001
                print("skip", v, M, N, K, repr(e)[:100])
        ts = {v: [] for v in runners}
        for _ in range(args.rounds):
            for v, (run, _) in runners.items():
                ts[v].append(run())
        med = {v: statistics.median(t) for v, t in ts.items()}
        best = min((v for v in med if v != "auto"), key=lambda v: med[v])
        fl = 2.0 * M * N * K
        tot_auto += med["auto"] * cnt
        tot_best += med[best] * cnt
        line = "M%d N%d K%d k%d x%.0f | auto %.1fus %.0fTF | best %s %.1fus %.0fTF | " % (
            M, N, K, k, cnt, med["auto"], fl / med["auto"] / 1e6, best, med[best], fl / med[best] / 1e6)
        line += " ".join("%s=%.1f" % (v, med[v]) for v in med if v != "auto")
        print("GEMMVAR", line, flush=True)
        rows.append((M, N, K, k, cnt, med))
        del runners
        torch.cuda.empty_cache()
    print("GEMMVAR total per step: auto %.3f ms, best-per-shape %.3f ms" % (tot_auto / 1e3, tot_best / 1e3))
    if args.tsv:
        with open(args.tsv, "w") as f:
            f.write("M\tN\tK\tk\tlaunches\t" + "\t".join(["auto"] + want) + "\n")
            for (M, N, K, k, cnt, med) in rows:
                f.write("%d\t%d\t%d\t%d\t%.0f\t" % (M, N, K, k, cnt) + "\t".join("%.1f" % med[v] if v in med else "-" for v in ["auto"] + want) + "\n")


if __name__ == "__main__":
    main()
