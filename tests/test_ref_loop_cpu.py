"""The loop restatement of tests/ref_loop.py is pinned to the reference: the reference's OWN `engine.engine.train` drove one small
CPU model over the batches of loop_case() with the Adam / MultiStepLR / GradScaler objects built there, and its parameters and
BatchNorm buffers afterwards are stored in tests/golden/ref_loop_reference.npz (tests/golden/make_golden.py ref_loop).
`ref_loop.train_steps` on the same case must reproduce them bit for bit, and trainMetricGPU's stored answers on random inputs
exactly."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
from torch import nn

from conftest import GOLDEN
import ref_loop

MAX_NORMS = (0.0, 0.5)
# Bit for bit on any x86 host: with torch's default CPU kernels the last bits of these parameters differ between hosts (the
# vector width and oneDNN / MKL code paths follow the CPU model).  Both loops therefore run in a process of their own - torch
# fixes its kernel choice at the first call - with ATen's scalar kernels, oneDNN off, MKL in its conditional numerical
# reproducibility mode and one thread (pinned_states).
PINNED_ENV = {"ATEN_CPU_CAPABILITY": "default", "MKL_CBWR": "COMPATIBLE", "OMP_NUM_THREADS": "1", "MKL_NUM_THREADS": "1"}


class _Toy(nn.Module):
    """the model contract of model/segmenter.py:29-62 in miniature: (img, word, mask) -> (pred.detach(), mask/4, loss)"""

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(3, 4, 3, stride=4, padding=1)
        self.bn = nn.BatchNorm2d(4)
        self.emb = nn.Embedding(50, 4)
        self.head = nn.Conv2d(4, 1, 1)

    def forward(self, img, word, mask=None):
        x = torch.relu(self.bn(self.conv(img))) * self.emb(word).mean(1)[:, :, None, None]
        pred = self.head(x)
        if self.training:
            mask = torch.nn.functional.interpolate(mask, pred.shape[-2:], mode="nearest").detach()
            loss = torch.nn.functional.binary_cross_entropy_with_logits(pred, mask)
            return pred.detach(), mask, loss
        return pred.detach()


def loop_case():
    """(batches, freshly seeded model, (optimizer, scheduler, scaler)) - what both loops are driven with"""
    g = torch.Generator().manual_seed(1)
    batches = [(torch.randn(4, 3, 32, 32, generator=g), torch.randint(0, 50, (4, 5), generator=g),
                (torch.rand(4, 32, 32, generator=g) > 0.5).float()) for _ in range(5)]
    torch.manual_seed(0)
    m = _Toy()
    groups = [{"params": [p for n, p in m.named_parameters() if n.startswith("conv")], "initial_lr": 1e-3},
              {"params": [p for n, p in m.named_parameters() if not n.startswith("conv")], "initial_lr": 1e-2}]
    # (fused: the update's square root in torch's own kernel - the per-tensor Adam hands it to MKL's vector math, whose last bit
    # follows the CPU model whatever MKL_CBWR says)
    opt = torch.optim.Adam(groups, lr=1e-2, weight_decay=0.0, fused=True)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[35], gamma=0.1)
    return batches, m, (opt, sched, torch.amp.GradScaler("cuda", enabled=False))


def metric_cases():
    g = torch.Generator().manual_seed(0)
    out = []
    for _ in range(5):
        x = torch.randn(4, 1, 16, 16, generator=g) * 2
        t = (torch.rand(4, 1, 16, 16, generator=g) > 0.6).float()
        out.append((x, t))
    return out


def pinned_states(train):
    """{"<max_norm>/<state_dict key>": array} after `train(batches, model, optimizer, scheduler, scaler, max_norm)` ran each case
    of loop_case() on one gloo rank; call in a process started with PINNED_ENV"""
    assert all(os.environ.get(k) == v for k, v in PINNED_ENV.items()), "start the process with PINNED_ENV"
    torch.backends.mkldnn.enabled = False
    torch.set_num_threads(1)
    out = {}
    with tempfile.TemporaryDirectory() as td:
        dist.init_process_group("gloo", init_method="file://" + os.path.join(td, "pg"), rank=0, world_size=1)
        try:
            for max_norm in MAX_NORMS:
                batches, model, (opt, sched, scaler) = loop_case()
                train(batches, model, opt, sched, scaler, max_norm)
                out.update({"%g/%s" % (max_norm, k): v.numpy() for k, v in model.state_dict().items()})
        finally:
            dist.destroy_process_group()
    return out


def _restated_train(batches, model, opt, sched, scaler, max_norm):
    res = ref_loop.train_steps(batches, model, opt, scaler, max_norm=max_norm, device_type="cpu")
    assert len(res) == len(batches)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "ref_loop_reference.npz"))


@pytest.fixture(scope="module")
def restated():
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "states.npz")
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), out]
        r = subprocess.run(cmd, env=dict(os.environ, **PINNED_ENV), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stdout[-3000:]
        return dict(np.load(out))


def test_train_metric_matches_reference(golden):
    for (x, t), (iou, pr5) in zip(metric_cases(), golden["metric"]):
        b = ref_loop.train_metric_gpu(x.clone(), t)
        assert float(b[0]) == iou and float(b[1]) == pr5


@pytest.mark.parametrize("max_norm", MAX_NORMS)
def test_restated_loop_equals_reference_engine_train(golden, restated, max_norm):
    keys = sorted(k for k in restated if k.startswith("%g/" % max_norm))
    assert keys and keys == sorted(k for k in golden.files if k.startswith("%g/" % max_norm))
    for k in keys:
        assert torch.equal(torch.from_numpy(restated[k]), torch.from_numpy(golden[k])), k


if __name__ == "__main__":                       # the `restated` fixture's process
    np.savez(sys.argv[1], **pinned_states(_restated_train))
