"""throughput of the GPU input preprocessing (cris/pytorch_amd/inputpipe.py): batches of 8 decoded 480x640 RGB images + masks
-> [8, 3, 416, 416] float32 + [8, 416, 416] masks.  Prints samples/s with the uint8 arrays already on the device and with
the host->device copies included (pinned host memory).   python tools/input_pipe_bench.py [iters] [--augment] [--repeats R]

--augment adds the training-time augmentation arm (every knob of inputpipe.Augment on: fresh per-sample parameters each batch,
the luminance pass and the augmented launch) on the same batch.  The two arms alternate inside the one call, R times each
(default 5), and every line carries the median and the spread (min .. max) over the repeats; the last line of each source is
the augmented arm's cost relative to the plain arm."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cris.pytorch_amd.inputpipe import Preprocessor      # noqa: E402

argv = sys.argv[1:]
augment = "--augment" in argv
repeats = int(argv[argv.index("--repeats") + 1]) if "--repeats" in argv else (5 if augment else 1)
pos = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] != "--repeats")]
iters = int(pos[0]) if pos else 200
rng = np.random.default_rng(0)
imgs_h = [torch.from_numpy(rng.integers(0, 255, (480, 640, 3), dtype=np.uint8)).pin_memory() for _ in range(8)]
masks_h = [torch.from_numpy((rng.random((480, 640)) > 0.5).astype(np.uint8) * 255).pin_memory() for _ in range(8)]
imgs_d, masks_d = [t.cuda() for t in imgs_h], [t.cuda() for t in masks_h]
pre = Preprocessor((416, 416))
out_bytes = 8 * (3 * 416 * 416 * 4 + 416 * 416 * 4)
in_bytes = 8 * (480 * 640 * 4)


def plain(a, b):
    pre(a, b)


if augment:
    from cris.pytorch_amd.inputpipe import Augment, augment_params      # noqa: E402
    AUG = Augment(scale=(0.8, 1.25), translate=0.1, rotate=10.0, hflip=0.5, brightness=0.2, contrast=0.2, saturation=0.2)
    arng = np.random.default_rng(1)

    def augmented(a, b):
        pre(a, b, augment_params(AUG, arng.random((8, 8)), (416, 416)))


def timed(fn, a, b):
    for _ in range(5):
        fn(a, b)
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(iters):
        fn(a, b)
    torch.cuda.synchronize()
    return (time.time() - t0) / iters


def line(name, dts, extra_in=0):
    dt = float(np.median(dts))
    spread = "" if len(dts) == 1 else " [%d repeats: %.0f .. %.0f samples/s]" % (len(dts), 8 / max(dts), 8 / min(dts))
    print("%-44s %.3f ms / batch of 8 = %.0f samples/s (%.1f GB/s of input bytes + output bytes)%s" % (
        name, dt * 1e3, 8 / dt, (out_bytes + in_bytes + extra_in) / dt / 1e9, spread))


for name, (a, b) in (("device-resident uint8", (imgs_d, masks_d)), ("pinned host uint8 (incl. H2D)", (imgs_h, masks_h))):
    t_plain, t_aug = [], []
    for _ in range(repeats):
        t_plain.append(timed(plain, a, b))
        if augment:
            t_aug.append(timed(augmented, a, b))
    line(name, t_plain)
    if augment:
        # the luminance pass reads every source image once more: 3 h w bytes per sample
        line(name + " + augment", t_aug, extra_in=8 * 480 * 640 * 3)
        ratios = [x / y for x, y in zip(t_aug, t_plain)]
        print("%-44s augmented / plain time per batch: median %.3f (%.3f .. %.3f)" % (name, float(np.median(ratios)), min(ratios), max(ratios)))
