"""What the NativeTrainer option tests (test_{grad_clip,grad_accum,ema,lr_schedule}_gpu.py) share: the suite's smallest trainer
(tiny spec, 64 x 64, micro-batches of MICRO samples) from synthetic_state_dict(..., 0), its batches, the recorded command list, a
communicator that stands in for a world of two, and the comparisons."""
import torch

from cris.pytorch_amd import arch, synth
from cris.pytorch_amd.engine import Comm
from cris.pytorch_amd.trainer import NativeTrainer

ADAM_TOL = 1e-6          # relative L2 error of the existing Adam comparisons (tests/test_hip_ops.py test_adam_*)
MICRO = 2                # samples per micro-batch


def relerr(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def same_floats(got, want):
    keys = [k for k, v in got.items() if v.is_floating_point()]
    assert keys and set(keys) == {k for k, v in want.items() if v.is_floating_point()}
    bad = [k for k in keys if not torch.equal(got[k], want[k])]
    assert not bad, (len(bad), bad[:5])


def make_trainer(**kw):
    clip, head = arch.specs_by_name("tiny")
    return NativeTrainer(clip, head, arch.synthetic_state_dict(clip, head, 0), torch.device("cuda:0"), **kw), head


def batch(n, head, t):
    return [x.to("cuda:0") for x in synth.make_batch(n, 64, head.word_len, 0, t)]


def recorded(**kw):
    tr, head = make_trainer(launch="cmdlist", **kw)
    for t in range(3):                                                    # eager, recording, replay
        tr.train_step(*batch(MICRO, head, t))
    torch.cuda.synchronize()
    assert tr._cmds is not None and tr.launch == "cmdlist"
    return tr, [(name, None if args is None else len(args)) for _, args, name in tr._cmds.cmds]


class TwoEqualRanks(Comm):
    """what a rank of a world of two sees when both ranks hold the same batch: the all-reduced (summed) gradient is twice its
    own (exact in fp32), the MAX of the embedding-row marks is its own.  Counts the exchanges it is asked for."""
    world = 2
    supports_max_u8 = True

    def __init__(self):
        super().__init__()
        self.calls = {"sum": 0, "max": 0}

    def allreduce_async(self, t, op="sum"):
        self.calls[op] += 1
        if op == "sum":
            t.mul_(2.0)

    def wait_all(self):
        pass
