"""The GEMM / weight-gradient edge tables (tests/gemm_edge_cases.py) without a GPU.

For every table row: the launchers' argument checks pass, the plan resolves to the variant the row names, and the float32
emulation (tests/gemm_emulator.py) passes the auditor in both summation orders with intact guards on CPU slabs - so the
bounds, the NaN fills of inputs and workspaces and the +-2^100 fill of dY's readable columns admit a correct kernel.

Then the errors those edges exist to catch, one emulator switch each: every one must be refused in a named case, at the place
the finding names."""
import pytest
import torch

from cris.pytorch_amd import ops

import gemm_audit as GA
import gemm_edge_cases as EC
from gemm_emulator import Emulator

CASES = EC.all_cases()
WORST = {}          # family -> worst err/bound of the emulation


def _audit(monkeypatch, order="blk", mut=None, ring=None):
    aud = EC.make_auditor(GA.CpuMemory(), Emulator(order, mut, ring), "cpu")
    monkeypatch.setattr(ops, "KERNEL_TIMER", aud)
    return aud


def test_tables_are_well_formed():
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids))
    fams = {c.family for c in CASES}
    assert fams == {"gemm " + v for v in GA.VARIANTS} | {"wgrad 128", "wgrad 256"}
    assert set(EC.RING) == set(EC.TILE4 + EC.TILE8 + [EC.K2])


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_emulation_passes(case, monkeypatch):
    EC.check_plan(case)
    for order in ("seq", "blk"):
        aud = _audit(monkeypatch, order)
        runs = EC.run_case(case, "cpu")
        w = EC.check_reports(aud, case)
        for r in runs:
            r.assert_guards(case.id)
        WORST[case.family] = max(WORST.get(case.family, 0.0), w)


def test_group_problems_equal_their_solo_launches(monkeypatch):
    """(the emulation is trivially so; this keeps the comparison code of the GPU file exercised without a GPU)"""
    _audit(monkeypatch)
    gc = EC.gemm_group_cases()[0]
    shared, slices, _ = EC.run_gemm_group(gc, "cpu")
    for p, (M, off, N) in zip(gc.probs, slices):
        solo = EC.run_gemm(p, "cpu")
        EC.assert_exact(shared.rows[:M, off:off + N].clone(), solo.get("out"), p.id)


def test_worst_ratio_per_family():
    if len(WORST) < 14:
        pytest.skip("needs the emulated rows of this file (run it whole)")
    print("\nemulation, worst err/bound per family:")
    for fam in sorted(WORST):
        print("  %-16s %.4f" % (fam, WORST[fam]))
    assert max(WORST.values()) < 1


# ---- the errors the edges exist to catch ------------------------------------------------------------------------------------
def _by_id(cid):
    return next(c for c in CASES if c.id == cid)


def _refused(aud, what):
    bad = [r for r in aud.reports if not r.ok]
    assert bad, "the audit did not notice"
    msg = bad[0].describe()
    assert what in msg, msg
    f = next((f for r in bad[0].problems for f in r.findings), None)
    return f, msg


def test_k_tail_chunk_not_masked(monkeypatch):
    """K = 72: the second K-step holds one live chunk; the next one read lands in Wt's [K, ldb) - NaN"""
    aud = _audit(monkeypatch, mut="ktail_unmasked")
    EC.run_case(_by_id("64x64-lin-k72"), "cpu")
    f, msg = _refused(aud, "out at")
    assert f.got != f.got, msg                                     # the NaN surfaced


def test_stale_ring_buffer(monkeypatch):
    """nk = D + 1: K-step D is the first to land in a refilled buffer"""
    for v in ("128x128", "64x64", "8w128x128"):
        D = EC.RING[v]
        aud = _audit(monkeypatch, mut="stale_ring", ring=D)
        EC.run_case(_by_id("%s-nk%d" % (v, D + 1)), "cpu")
        _refused(aud, "out at")


def test_tap_not_advanced_inside_a_k_step(monkeypatch):
    aud = _audit(monkeypatch, mut="tap_stuck")
    case = _by_id("64x64-3x3-c24")
    EC.run_case(case, "cpu")
    f, msg = _refused(aud, "out at")
    assert 0 <= f.row < case.g.M and 0 <= f.col < case.N, msg


def test_padding_test_off_by_one(monkeypatch):
    """`ih <= H`: the lower border reads the next image's first row - below the last image, the NaN guard rows"""
    aud = _audit(monkeypatch, mut="pad_le")
    case = _by_id("64x64-3x3-c64")
    EC.run_case(case, "cpu")
    f, msg = _refused(aud, "out at")
    g = case.g
    assert (f.row % (g.OH * g.OW)) // g.OW == g.OH - 1, msg         # an output row of the lower border


def test_m_tail_tile_stores_row_M(monkeypatch):
    """the auditor's footprint ends with row M - 1: only the guard row after the slice sees this"""
    aud = _audit(monkeypatch, mut="mtail_row_M")
    case = _by_id("64x64-tail-lean")
    (run,) = EC.run_case(case, "cpu")
    EC.check_reports(aud, case)                                     # the audit alone passes
    with pytest.raises(AssertionError, match="guard elements overwritten"):
        run.assert_guards(case.id)


def test_last_bn_part_divided_by_R(monkeypatch):
    aud = _audit(monkeypatch, mut="bn_last_div_R")
    case = _by_id("64x64-tail-stats")
    EC.run_case(case, "cpu")
    f, msg = _refused(aud, "BN partial M2")
    R = 32
    assert ("part %d " % (case.g.M // R)) in msg, msg               # the incomplete last part, not a full one


def test_k2_second_group_drops_its_last_step(monkeypatch):
    aud = _audit(monkeypatch, mut="k2_drop_last")
    EC.run_case(_by_id("64x64k2-nk3"), "cpu")
    _, msg = _refused(aud, "out at")
    assert "64x64k2" in msg, msg
    aud = _audit(monkeypatch, mut="k2_drop_last")                   # (an even count is not affected)
    EC.run_case(_by_id("64x64k2-nk4"), "cpu")
    EC.check_reports(aud, _by_id("64x64k2-nk4"))


def test_empty_split_k_slice_left_unwritten(monkeypatch):
    aud = _audit(monkeypatch, mut="empty_slice_unwritten")
    EC.run_case(_by_id("skinny9s-empty-slice"), "cpu")
    f, msg = _refused(aud, "out at")
    assert f.got != f.got and "skinny9s" in msg, msg                # the workspace's NaN


def test_wgrad_pixel_step_runs_past_its_split(monkeypatch):
    aud = _audit(monkeypatch, mut="split_overrun")
    case = _by_id("wgrad128-m257-s3")
    assert case.eff == 3
    EC.run_case(case, "cpu")
    _refused(aud, "dW at")


def test_wgrad_dbias_added_once_per_k_tile(monkeypatch):
    aud = _audit(monkeypatch, mut="dbias_per_ktile")
    EC.run_case(_by_id("wgrad128-k136-ldw136"), "cpu")               # two k-tiles of 128
    _refused(aud, "dbias")
