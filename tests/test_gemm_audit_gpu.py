"""Every GEMM and weight-gradient launch of real training steps, audited element by element (tests/gemm_audit.py).

An Auditor takes the place of ops.KERNEL_TIMER (the hook every conv_gemm / GemmQueue / WgradQueue / conv_wgrad launch goes
through; the trainer runs eagerly while it is set).  For each launch it resolves the tile variant (cris_conv_gemm_plan),
checks that every extent the struct declares lies inside one live block of torch's allocator BEFORE it reads or launches
anything, snapshots inputs and output spans, launches on the current stream and checks every element written against a
float64 restatement, the write footprint and, for group launches, the independence of the problems.

Configurations: BASELINE configs[1] (CRIS-R50, 416x416, batch 8, 17 tokens, decoder dropout 0.1), the reference's other
multi-scale shapes (5 x 320 / 17, 2 x 512 / 22, 3 x 352 / 9) and tiny at 3 x 96 (every tile tail path)."""
import json
import os
import time

import pytest
import torch

from cris.pytorch_amd import arch, hip, ops, synth
from cris.pytorch_amd.trainer import NativeTrainer

import gemm_audit as GA

pytestmark = pytest.mark.gpu

CONFIGS = [("r50", 8, 416, 17), ("r50", 5, 320, 17), ("r50", 2, 512, 22), ("r50", 3, 352, 9), ("tiny", 3, 96, None)]
# every kind of launch the audited steps must contain (gemm_audit.Auditor.launch names them).  "solo skinny" is not required
# as a kind of its own: its only occupant besides the listed split-K kernel is skinny1 (M <= 16 rows), which the tiny and R50
# steps run anyway, while the single-pass skinny9 never runs under the automatic choice (M 17..144 linears take the split-K
# kernel with its workspace for K >= 1024 and a 64x64 tile below).
KINDS = ["solo tile", "4-wave group", "8-wave group", "skinny split-K with workspace", "f32 output", "bf16 residual",
         "f32 residual", "dropout", "outT", "BN partials", "bnr partials", "sliced output", "offset input", "split wgrad",
         "grouped wgrad", "dbias"]
SEEN = {}          # config -> {kinds, variants, launches, seconds, worst per family}


def _execute(fn, args):
    hip.call(fn, *args, torch.cuda.current_stream().cuda_stream)


def _trainer(name, batch, size, word_len):
    import dataclasses
    clip, head = arch.specs_by_name(name)
    if word_len is not None:
        head = dataclasses.replace(head, word_len=word_len)
    sd = arch.synthetic_state_dict(clip, head, 0)
    dev = torch.device("cuda:0")
    tr = NativeTrainer(clip, head, sd, dev, launch="eager")
    img, word, mask = synth.make_batch(batch, size, head.word_len, 0, 0)
    return tr, (img.to(dev), word.to(dev), mask.to(dev))


def _audited_step(tr, batch):
    aud = GA.Auditor(GA.DeviceMemory("cuda:0"), _execute, raise_on_failure=False)
    saved = ops.KERNEL_TIMER
    ops.KERNEL_TIMER = aud
    try:
        loss, _ = tr.train_step(*batch)
        torch.cuda.synchronize()
    finally:
        ops.KERNEL_TIMER = saved
    return aud, loss


@pytest.mark.parametrize("name,batch,size,word_len", CONFIGS)
def test_every_gemm_launch_of_a_train_step(name, batch, size, word_len):
    t0 = time.time()
    tr, b = _trainer(name, batch, size, word_len)
    aud, loss = _audited_step(tr, b)
    secs = time.time() - t0
    assert aud.reports, "no launch went through the hook"
    bad = [r.describe() for r in aud.reports if not r.ok]
    worst = {}
    for r in aud.reports:
        for pr in r.problems:
            worst[pr.family] = max(worst.get(pr.family, 0.0), pr.worst)
    kinds = set().union(*[r.kinds for r in aud.reports])
    key = "%s b%d s%d L%s" % (name, batch, size, word_len)
    SEEN[key] = dict(launches=len(aud.reports), problems=sum(len(r.problems) for r in aud.reports), seconds=round(secs, 1),
                     kinds=sorted(kinds), worst={k: round(v, 4) for k, v in sorted(worst.items())}, loss=float(loss))
    print("\n%s: %s" % (key, json.dumps(SEEN[key])))
    _dump()
    assert not bad, "%d of %d launches failed the audit:\n%s" % (len(bad), len(aud.reports), "\n".join(bad[:10]))
    assert all(v < 1.0 for v in worst.values())


def test_audit_covers_every_kind_of_launch():
    if len(SEEN) < len(CONFIGS):
        pytest.skip("needs the audited steps of this file (run it whole)")
    kinds = set().union(*[set(v["kinds"]) for v in SEEN.values()])
    missing = [k for k in KINDS if k not in kinds]
    assert not missing, missing
    variants = sorted(k for k in kinds if k.startswith("variant "))
    print("\nvariants audited: %s" % variants)


def test_audit_is_not_intrusive():
    """tiny config: loss, gradient arena and parameters after an audited step equal bit for bit those of an unaudited eager
    step from the same state"""
    outs = []
    for audited in (False, True):
        tr, b = _trainer("tiny", 3, 96, None)
        if audited:
            aud, loss = _audited_step(tr, b)
            assert aud.reports and all(r.ok for r in aud.reports)
        else:
            loss, _ = tr.train_step(*b)
            torch.cuda.synchronize()
        outs.append((float(loss), tr.engine.grad_arena.clone(), {k: v.clone() for k, v in tr.engine.P.items()}))
    (l0, g0, p0), (l1, g1, p1) = outs
    assert l0 == l1
    assert torch.equal(g0, g1)
    assert all(torch.equal(p0[k], p1[k]) for k in p0)


def _dump():
    path = os.environ.get("CRIS_GEMM_AUDIT_REPORT")
    if path:
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "w") as f:
            json.dump(SEEN, f, indent=1)
