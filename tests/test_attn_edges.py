"""The six attention kernels (csrc/attention.hip) element by element, each launcher on its own against the float64 statement of
the function it implements (tests/attn_edge_cases.py: references, derived bounds, case tables; tests/test_attn_edges_cpu.py
settles without a GPU that the bounds admit a correct fp32 kernel and refuse seven plausible errors).

As the engine calls them: Q, K, V column slices of wider buffers, O and dQ / dK / dV written into slices, up to 15 (batch, head)
pairs over the remainders of the XCD block remap.  Every output lives in guard bits that must survive the launch, every
token-major input in NaN that poisons a read outside its slice, and the head-split transposed copies are padded once with zeros
and once with +-2^100: the results must be bit-identical, since the kernels give the padding an exact-zero probability.  The
backward launchers get the float64 O, lse and delta (rounded as the kernels store them), not the forward kernel's output, so
an error is seen where it is made.  cris_attn_plan tells that a case ran the kernel (direct or LDS) it is in the table for.

CRIS_ATTN_EDGES_REPORT=<file.json> writes the worst error / bound ratio per output and kernel; they are always printed."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from cris.pytorch_amd import hip  # noqa: E402
import ctypes  # noqa: E402
import attn_edge_cases as A  # noqa: E402
from hip_ops_edge_cases import GUARD_BITS, assert_exact  # noqa: E402

DEV = "cuda"
_IDS = [c.name for c in A.CASES]
WORST = A.Worst()
_SLABS = {"O": "O", "lse": "lse", "delta": "delta", "dQ": "dQ", "dK": "dK", "dV": "dV"}


def launch(name, launcher, fill=0.0):
    """one launch of one launcher on freshly built operands; {output: CPU tensor} after the guards were checked"""
    r = A.reference(name)
    o = A.build_operands(r, DEV, fill)
    A.set_launch(o, launcher)
    w = A.LAUNCHERS.index(launcher)
    assert A.plan(o)[w] == r.case.plan[w], "%s %s: cris_attn_plan %r, the table expects %r" % (name, launcher, A.plan(o), r.case.plan)
    hip.call("cris_attn_" + {"fwd": "fwd", "dq": "bwd_dq", "dkv": "bwd_dkv"}[launcher], ctypes.byref(o.p), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for out in ("O", "lse", "delta", "dQ", "dK", "dV"):          # all of them: a launcher must not touch another one's result either
        getattr(o, _SLABS[out]).assert_guards("%s %s: guards of %s" % (name, launcher, out))
        if out not in A.OUTPUTS[launcher]:
            s = getattr(o, _SLABS[out])
            bits = s.rows.view(torch.int16 if s.dtype == A.BF else torch.int32)
            assert bool((bits == GUARD_BITS[s.dtype]).all()), "%s %s wrote into %s" % (name, launcher, out)
    return {out: getattr(o, _SLABS[out]).get() for out in A.OUTPUTS[launcher]}


def run_and_check(name, launcher):
    r = A.reference(name)
    c = r.case
    kernel = "lds" if c.plan[A.LAUNCHERS.index(launcher)] else "direct"
    got = launch(name, launcher, 0.0)
    huge = launch(name, launcher, A.PAD_HUGE)
    for out in A.OUTPUTS[launcher]:
        dims, names = A.names_of(c, out)
        x = A.ratio(r, out, got[out])
        WORST.add(out, kernel, x, name)
        print("%s %s %s/%s: worst error / bound %.3f" % (name, launcher, out, kernel, x))
        A.check_output(r, out, got[out], "%s %s" % (name, out))
        assert_exact(huge[out], got[out], "%s %s: padding of the transposed copies +-2^100 against 0" % (name, out), dims, names)


@pytest.mark.parametrize("name", _IDS)
def test_fwd(name):
    run_and_check(name, "fwd")


@pytest.mark.parametrize("name", _IDS)
def test_bwd_dq(name):
    run_and_check(name, "dq")


@pytest.mark.parametrize("name", _IDS)
def test_bwd_dkv(name):
    run_and_check(name, "dkv")


@pytest.mark.parametrize("name", [n for n in _IDS if n.startswith("dropsplit-")])
def test_split_seed_is_the_same_dropout(name):
    """the seed split between drop_seed and a device word: bit-identical to the whole seed in drop_seed"""
    whole = name.replace("dropsplit-", "drop-")
    assert A.BY_NAME[name].split_seed and not A.BY_NAME[whole].split_seed
    for launcher in A.LAUNCHERS:
        a, b = launch(name, launcher), launch(whole, launcher)
        for out in A.OUTPUTS[launcher]:
            assert_exact(a[out], b[out], "%s %s" % (name, out), *A.names_of(A.BY_NAME[name], out))


@pytest.mark.parametrize("name,launcher,kernel", A.DETERMINISM, ids=["%s-%s" % (w, "lds" if k else "direct") for _, w, k in A.DETERMINISM])
def test_second_launch_is_bit_identical(name, launcher, kernel):
    assert A.BY_NAME[name].plan[A.LAUNCHERS.index(launcher)] == kernel
    a, b = launch(name, launcher), launch(name, launcher)
    for out in A.OUTPUTS[launcher]:
        assert_exact(a[out], b[out], "%s %s" % (name, out), *A.names_of(A.BY_NAME[name], out))


def test_zz_worst_ratios():
    """(runs last in this file) the worst error / bound ratio per output and kernel of the tests above"""
    print("\nworst error / bound of the HIP kernels, per output and kernel:\n" + WORST.table())
    over = {k: v for k, v in WORST.w.items() if v[0] > 0.9}
    if over:
        print("above 0.9 of the bound: %r" % over)
    path = os.environ.get("CRIS_ATTN_EDGES_REPORT")
    if path:
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "w") as f:
            json.dump(WORST.as_json(), f, indent=1)
