"""Every GEMM tile variant, skinny kernel and weight-gradient tile, forced by name at the edges of its own pipeline and tile
(tests/gemm_edge_cases.py), audited element by element (tests/gemm_audit.py) in guarded slabs.

The audited training steps of tests/test_gemm_audit_gpu.py only reach the variants and shapes the automatic choice takes; four
forward variants (128x64, 8w256x128, 64x64k2, skinny9) and the 256 weight-gradient tile at small shapes never run there.  Here
each table row is one launch through ops.conv_gemm / ops.conv_wgrad or their queues with the Auditor installed as
ops.KERNEL_TIMER: report.ok, worst err/bound < 1 (the auditor's derived bound), every guard element of every output slab intact,
NaN-guarded inputs and NaN-filled workspaces.  The same rows pass a float32 emulation in tests/test_gemm_edges_cpu.py."""
import pytest
import torch

from cris.pytorch_amd import hip, ops

import gemm_audit as GA
import gemm_edge_cases as EC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = EC.all_cases()
WORST = {}          # family -> worst err/bound over the rows that ran
RAN = [0]           # rows that ran and passed
TAIL_VARIANTS = EC.TILE4 + [EC.K2] + EC.TILE8


def _execute(fn, args):
    hip.call(fn, *args, torch.cuda.current_stream().cuda_stream)


@pytest.fixture
def audit(monkeypatch):
    def make():
        aud = EC.make_auditor(GA.DeviceMemory(DEV), _execute, DEV)
        monkeypatch.setattr(ops, "KERNEL_TIMER", aud)
        return aud
    return make


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_edge_case(case, audit):
    EC.check_plan(case)
    aud = audit()
    runs = EC.run_case(case, DEV)
    torch.cuda.synchronize()
    worst = EC.check_reports(aud, case)
    for r in runs:
        r.assert_guards(case.id)
    WORST[case.family] = max(WORST.get(case.family, 0.0), worst)
    RAN[0] += 1


@pytest.mark.parametrize("gc", EC.gemm_group_cases(), ids=lambda c: c.id)
def test_gemm_group_equals_solo_launches(gc, audit):
    aud = audit()
    shared, slices, _ = EC.run_gemm_group(gc, DEV)
    assert len(aud.reports) == 1 and aud.reports[0].fn == "cris_conv_gemm_group_launch" and len(aud.reports[0].problems) == 3
    for p, (M, off, N) in zip(gc.probs, slices):
        solo = EC.run_gemm(p, DEV)
        EC.assert_exact(shared.rows[:M, off:off + N].cpu().contiguous(), solo.get("out"), p.id, names=["row", "col"])
    assert all(r.ok for r in aud.reports), "\n".join(r.describe() for r in aud.reports if not r.ok)


@pytest.mark.parametrize("gc", EC.wgrad_group_cases(), ids=lambda c: c.id)
def test_wgrad_group_equals_solo_launches(gc, audit):
    aud = audit()
    runs = EC.run_wgrad_group(gc, DEV)
    assert len(aud.reports) == 1 and aud.reports[0].fn == "cris_conv_wgrad_group" and len(aud.reports[0].problems) == 3
    for p, grouped in zip(gc.probs, runs):
        solo = EC.run_wgrad(p, DEV)
        for name in ("dW", "dbias"):
            EC.assert_exact(grouped.get(name), solo.get(name), "%s %s" % (p.id, name), names=["row", "col"])
    assert all(r.ok for r in aud.reports), "\n".join(r.describe() for r in aud.reports if not r.ok)


@pytest.mark.parametrize("v", TAIL_VARIANTS + list(EC.SKINNY_M))
def test_second_launch_is_bit_identical(v, audit):
    audit()
    if v in EC.SKINNY_M:
        case = next(c for c in CASES if c.id == "%s-general" % v)
    else:
        case = EC.tail_case(v)
    a, b = EC.run_gemm(case, DEV), EC.run_gemm(case, DEV)
    EC.assert_exact(a.get("out"), b.get("out"), case.id, names=["row", "col"])


@pytest.mark.parametrize("tile", EC.WGRAD_TILES)
def test_second_wgrad_launch_is_bit_identical(tile, audit):
    audit()
    case = next(c for c in CASES if c.id == "wgrad%d-m257-s3" % tile)
    a, b = EC.run_wgrad(case, DEV), EC.run_wgrad(case, DEV)
    for name in ("dW", "dbias"):
        EC.assert_exact(a.get(name), b.get(name), "%s %s" % (case.id, name), names=["row", "col"])


@pytest.mark.parametrize("v", [v for v in EC.TILE4 + EC.TILE8 if v != "128x128"])
def test_tile_equals_128x128_bit_for_bit(v, audit):
    """every tile adds the K-tiles in the same order (test_conv_gemm_8wave_tiles asserts it at interior shapes): at this
    variant's tail shape its result is the 128x128 tile's.  (64x64k2 adds even and odd K-steps apart: not included.)"""
    audit()
    case = EC.tail_case(v)
    a, b = EC.run_gemm(case, DEV), EC.run_gemm(case, DEV, variant="128x128")
    EC.assert_exact(a.get("out"), b.get("out"), case.id, names=["row", "col"])


def test_every_variant_was_audited():
    want = ["gemm " + v for v in GA.VARIANTS] + ["wgrad %d" % t for t in EC.WGRAD_TILES]
    if RAN[0] < len(CASES):
        pytest.skip("needs the audited rows of this file (run it whole)")
    print("\nworst err/bound per family:")
    for fam in sorted(WORST):
        print("  %-16s %.4f" % (fam, WORST[fam]))
    missing = [f for f in want if f not in WORST]
    assert not missing, missing
    assert max(WORST.values()) < 1
