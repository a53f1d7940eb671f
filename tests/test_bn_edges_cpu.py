"""What tests/test_bn_edges.py rests on, without a GPU: (1) on the grid inputs a plain fp32 evaluation of the forward bit-equals
the float64 one after the bf16 rounding - the exactness claim; (2) the fp32 evaluation of every bounded statement meets the
bound the GPU test applies to the kernels, through the same check functions; (3) the Python mirrors of bn_cv_shift,
bn_fast_grid, bn_bwd_geometry and bn_bwd_mask_mode put every case on the kernel (instantiation) it is named for; (4) the checks
refuse the wrong results they exist to catch."""
import pytest
import torch

import hip_ops_edge_cases as E
import bn_edge_cases as N
from hip_ops_edge_cases import BF, F32, F64

CPU_ROWS = 4096          # cases made on the device by the GPU file: the arithmetic is per element, so the CPU evaluates this many rows


def cpu_shape(shape):
    B, H, W, C = shape
    return (B, min(H, CPU_ROWS), W, C) if B * H * W * C > N.ON_DEVICE and W == 1 else shape


_FWD = N.fwd_cases()
_REDUCE = N.reduce_cases()
_APPLY = N.apply_cases()


# ---- (1) exactness of the grid --------------------------------------------------------------------
@pytest.mark.parametrize("variant,relu,shape", [x[1:] for x in _FWD], ids=[x[0] for x in _FWD])
def test_grid_forward_is_exact_in_fp32(variant, relu, shape):
    c = N.make_fwd(variant, relu, *cpu_shape(shape))
    v32, v64 = N.bn_fwd(c, F32), N.bn_fwd(c, F64)
    E.assert_exact(v32.double(), v64, "fp32 evaluation, before rounding")
    N.check_fwd(v32.to(BF), c, "fp32 evaluation")
    for k in ("y", "y2", "ident"):
        if c.get(k) is not None:
            assert bool((c[k].to(BF).float() == c[k]).all()) and float(c[k].abs().max()) <= 8
    pre = c["y"].double() * c["scale"].double() + c["shift"].double()
    assert float(pre.abs().min()) >= 2.0 ** -8, "a single branch's pre-activation is an odd multiple of 2^-8"


@pytest.mark.parametrize("variant", ["m2", "pool_m2", "mul_m2"])
def test_recomputed_mask_is_exact(variant):
    c = N.make_bwd(variant, 2, 4, 6, 40)
    assert N.bwd_mask(c) == 2 and torch.equal(N.relu_mask(c, F32), N.relu_mask(c, F64))


def test_planted_mask_values():
    c = N.make_bwd("m1", 1, 33, 1, 8)
    z = c["z"].view(-1, 8).to(BF)
    assert z[0, :4].view(torch.int16).tolist() == [0, -32768, 0x0080, 0x0080 - 32768]       # +0, -0, 2^-126, -2^-126
    assert N.relu_mask(c, F64).view(-1, 8)[0, :4].tolist() == [False, False, True, False]
    assert N.relu_mask(c, F64).view(-1, 8)[-1, 4:].tolist() == [False, False, True, False]
    assert bool((c["dz"].view(-1, 8)[0, :4] == 4).all())


# ---- (2) the bounds admit a correct fp32 implementation -----------------------------------------------
@pytest.mark.parametrize("variant,shape", [x[1:] for x in _REDUCE], ids=[x[0] for x in _REDUCE])
def test_reduce_bound_admits_fp32(variant, shape):
    c = N.make_bwd(variant, *shape)
    N.check_sums(N.bn_bwd_sums(c, F32), c, "fp32 evaluation")
    if N.wants_dmul(c):
        N.check_dmul(N.bn_bwd_dmul(c, F32), c, "fp32 evaluation")


@pytest.mark.parametrize("C", N.SUM_C)
@pytest.mark.parametrize("nparts", N.SUM_NPARTS)
def test_sum_bound_admits_fp32(nparts, C):
    table, old = N.rand_f32((nparts, 2 * C), 301), N.rand_f32((2 * C,), 302)
    E.assert_bound(N.sum_parts(table, old, F32).double(), N.sum_parts(table, old, F64), N.sum_parts(table, old, F64, absolute=True), 0.0,
                   E.abs_coef(nparts + 1), "fp32 evaluation")


def _apply_fp32(c, sums=None):
    return {k: v.to(BF) for k, v in N.bn_bwd_apply(c, F32, sums=sums).items()}


@pytest.mark.parametrize("variant,dident,dy2,count_factor,shape", [x[1:] for x in _APPLY], ids=[x[0] for x in _APPLY])
def test_apply_bound_admits_fp32(variant, dident, dy2, count_factor, shape):
    c = N.make_bwd(variant, *cpu_shape(shape), dident=dident, dy2=dy2, count_factor=count_factor)
    assert c["count"] == count_factor * c["y"].numel() // c["y"].shape[-1]
    N.check_apply(_apply_fp32(c), c, "fp32 evaluation")


@pytest.mark.parametrize("variant,dident,shape", [x[1:] for x in N.E2E_CASES], ids=[x[0] for x in N.E2E_CASES])
def test_end_to_end_bound_admits_fp32(variant, dident, shape):
    """the fp32 statements, chained as the kernels are (sums of the reduce statement into the apply statement), against autograd"""
    c, ref = N.make_e2e(variant, dident, *shape)
    if N.bwd_mask(c) == 2:
        assert c["margin"] >= N.E2E_MARGIN and torch.equal(N.relu_mask(c, F32), N.relu_mask(c, F64)), "the fp32 coefficients decide every ReLU as float64 does"
    sums = N.bn_bwd_sums(c, F32)
    got = _apply_fp32(c, sums=sums)
    got["sums"] = sums
    if "dmul" in ref:
        got["dmul"] = N.bn_bwd_dmul(c, F32)
    N.check_e2e(got, c, ref, "fp32 evaluation")


@pytest.mark.parametrize("M", N.DIV24_M)
def test_fp32_reference_of_the_div24_cases(M):
    """group C computes its references in fp32: on the grid the forward is exact in it, and the backward's fp32 reference
    meets the bound against float64 with room to spare (a quarter of the absolute term), here on the first rows"""
    c = N.make_bwd("m2", 1, CPU_ROWS, 1, 40)
    ref, S, got = N.bn_bwd_apply(c, F64), N.bn_bwd_apply(c, F64, absolute=True), N.bn_bwd_apply(c, F32)
    E.assert_bound(got["dy"].double(), ref["dy"], S["dy"], 0.0, E.ABS_F32 / 4, "fp32 reference")


# ---- (3) every case reaches the path it is named for -----------------------------------------------
def test_mirrors():
    assert [N.cv_shift(C) for C in (8, 16, 64, 256, 2048)] == [0, 1, 3, 5, 8]
    assert [N.cv_shift(C) for C in (24, 40, 72, 280, 4096, 0)] == [-1] * 6
    assert N.fast_grid(1, 4) == 1 and N.fast_grid(1 << 18, 4) == 1024 and N.fast_grid(1 << 20, 4) == 1024
    assert N.fast_grid((1 << 20) + 1, 4) == 1025 and N.fast_grid(1 << 22, 4) == 2048 and N.fast_grid(1 << 21, 2) == 2048
    g = N.bwd_geometry(130, 280)
    assert (g["chv"], g["chunks"], g["last_cvn"], g["rpb"], g["rbs"]) == (8, 5, 3, 32, 5) and 256 // g["last_cvn"] == 85
    assert N.bwd_geometry(33, 72)["last_cvn"] == 1 and N.bwd_geometry(33, 136)["last_cvn"] == 1 and N.bwd_geometry(33, 136)["chv"] == 4
    assert N.bwd_geometry(33, 64)["rbs"] == 2 and N.row_blocks(33, 64) == [(0, 32), (32, 33)]
    assert N.bwd_geometry(1, 8)["rbs"] == 1 and N.bwd_geometry(2049, 8192) == dict(chv=8, chunks=128, rpb=513, rbs=4, last_cvn=8)


def test_forward_cases_reach_their_kernels():
    seen = set()
    for name, variant, relu, shape in _FWD:
        B, H, W, C = shape
        c = dict(y=torch.empty(0, 0, 0, C), pool=variant == "pool", mul=1 if variant == "mul" else None)
        path = N.fwd_path(c)
        assert path == ("fast" if C in N.FAST_C and variant not in ("pool", "mul") else "generic"), name
        seen.add((path, variant, relu, C))
    for C in N.FAST_C:
        small, big = N.fast_ladder(C)
        rpp = 256 >> N.cv_shift(C)
        assert 1 in small and rpp + 1 in small and (rpp == 1 or rpp - 1 in small)
        assert N.last_pass_partial(big, C, 4) and N.last_pass_partial(big, C, 2)
        assert N.fast_rows(big, C, 4)[1] == 1024 and N.fast_rows(big, C, 2)[1] > 1024
        for variant in ("plain", "ident", "two", "two_ident"):
            assert {("fast", variant, True, C), ("fast", variant, False, C)} <= seen
    for C in N.GENERIC_C:
        for variant in N.FWD_VARIANTS:
            assert {("generic", variant, True, C), ("generic", variant, False, C)} <= seen
    pools = {(H // 2, W // 2) for _, v, _, (B, H, W, C) in _FWD if v == "pool"}
    assert {(1, 1), (2, 3), (1, 3), (2, 5)} <= pools                                  # W = 2; OW = 3; OH * OW = 3; W = 10
    assert {(B, H * W) for _, v, _, (B, H, W, C) in _FWD if v == "mul"} == {(3, 1), (3, 33)}


def test_grid_boundary_cases():
    (_, (_, M1, _, C1)), (_, (_, M2, _, C2)) = N.GRID_BOUNDARY_CASES
    total = M1 * (C1 >> 3)
    assert C1 == 64 and (1 << 20) < total < (1 << 20) + 1024
    assert N.grid_1d(total, 1024, 2048) == 1025 > N.grid_1d(total, 256, 1024) == 1024 and N.fast_grid(total, 4) == 1025
    total = M2 * (C2 >> 3)
    rpp, grid, step = N.fast_rows(M2, C2, 4)
    assert C2 == 512 and (1 << 21) < total and grid == 2048 and N.cdiv(total, 1024) > 2048, "the cap decides the grid"
    assert step * 4 < M2 < step * 4 + step, "a second trip, its first pass partial"


def test_reduce_cases_reach_their_kernels():
    """(MASK, Y2, POOL, MUL) of the one reduce kernel, per variant; every instantiation the launcher admits has a case"""
    want = {"m0": (0, False, False, False), "m1": (1, False, False, False), "m2": (2, False, False, False),
            "pool_m0": (0, False, True, False), "pool_m2": (2, False, True, False), "two_m0": (0, True, False, False),
            "two_m0z": (0, True, False, False), "two_m1": (1, True, False, False), "mul_m0": (0, False, False, True),
            "mul_m1": (1, False, False, True), "mul_m2": (2, False, False, True), "two_mul_m0": (0, True, False, True),
            "two_mul_m1": (1, True, False, True)}
    dmul = {"mul_m1", "mul_m2"}                                      # the multiplier's gradient: plain BatchNorm + ReLU
    seen, reached = set(), set()
    for name, variant, shape in _REDUCE:
        c = N.make_bwd(variant, shape[0], 2, 2, 8)                   # the flags decide, not the shape
        assert N.reduce_instance(c) == want[variant] and N.bwd_mask(c) == want[variant][0], name
        assert N.wants_dmul(c) == (variant in dmul), name
        seen.add(variant)
        reached.add(N.reduce_instance(c))
    assert seen == set(want)
    assert reached == N.REDUCE_INSTANCES and len(N.REDUCE_INSTANCES) == 12
    plain = {(s[3], s[1]) for _, v, s in _REDUCE if v == "m2"}
    assert {(C, M) for C in N.REDUCE_C for M in N.REDUCE_M} <= plain
    assert {N.bwd_geometry(33, C)["last_cvn"] for C in N.REDUCE_C} == {1, 3, 8}
    assert {N.bwd_geometry(33, C)["chv"] for C in N.REDUCE_C} == {1, 2, 4, 8}
    assert N.row_blocks(33, 280)[-1] == (32, 33), "a second row block of one row"
    g = N.bwd_geometry(N.REDUCE_M_RAGGED[8], 8)
    assert g["rpb"] == 1031 and g["rpb"] % (256 * 4) and g["rpb"] % (256 * 2) and g["rpb"] > 256 * 4
    g = N.bwd_geometry(2049, 2048)
    assert g["rpb"] == 129 and g["rpb"] % (32 * 4) == 1
    mul = {(s[0], s[1] * s[2], s[3] >> 3) for _, v, s in _REDUCE if v == "mul_m2"}
    assert mul == {(3, hw, cv) for hw in (1, 33, 100) for cv in (5, 9)} | {(3, 33, cv) for cv in (1, 8, 35)} | {(7, 9419, 1)}
    for C, rs in ((8, {256}), (64, {128}), (280, {32, 85})):                        # row lanes of the full chunks / the last chunk
        g = N.bwd_geometry(99, C)
        assert {256 // g["chv"], 256 // g["last_cvn"]} == rs and g["rpb"] == 32 <= min(rs), "no second in-flight row inside a block"
    B, H, W, C = N.REDUCE_MUL_RAGGED
    g = N.bwd_geometry(B * H * W, C)
    assert B * H * W == 65933 and g["rpb"] == 1031 and (H * W) % 256 and (H * W) % g["rpb"]
    for variant in ("mul_m0", "mul_m1", "two_mul_m0", "two_mul_m1"):
        assert {s for _, v, s in _REDUCE if v == variant} == {(3, 11, 3, 8), (3, 11, 3, 280)}


def test_sentinel_cases():
    inst = set()
    for name, variant, (B, H, W, C) in N.SENTINEL_CASES:
        M = B * H * W
        rows = N.sentinel_rows(M, C)
        blocks = N.row_blocks(M, C)
        assert len(blocks) >= 3 and blocks[-1][1] == M and len(rows) <= 48, name
        assert all(r0 in rows and r1 - 1 in rows for r0, r1 in blocks)
        inst.add(N.reduce_instance(N.make_bwd(variant, B, 2, 2, 8)))
    assert inst == {(2, False, False, False), (1, False, False, False), (0, False, False, False), (2, False, True, False),
                    (1, True, False, False), (2, False, False, True)}
    assert {C for _, _, (_, _, _, C) in N.SENTINEL_CASES} >= {64, 280}
    (B, H, W, C), = [s for _, v, s in N.SENTINEL_CASES if v == "mul_m2"]
    assert any(r0 < H * W < r1 for r0, r1 in N.row_blocks(B * H * W, C)), "a sample boundary inside a row block"


def test_apply_cases_reach_their_kernels():
    fast, generic = set(), set()
    for name, variant, dident, dy2, cf, shape in _APPLY:
        c = N.make_bwd(variant, shape[0], 2, 2, 8, dident=dident, dy2=dy2)
        c["y"] = torch.empty(0, 0, 0, shape[3])
        inst = (c.get("y2") is not None, N.bwd_mask(c), dident, bool(dy2), cf)
        (fast if N.bwd_apply_path(c) == "fast" else generic).add(inst + (shape[3],))
    for C in N.FAST_C:
        here = {i[:5] for i in fast if i[5] == C}
        # [Y2][MASK]: Y2 with MASK 2 does not exist (with y2 the mask comes from z), so five of the table's six entries are reachable
        assert {i[:2] for i in here} == {(False, 0), (False, 1), (False, 2), (True, 0), (True, 1)}
        assert {i[2] for i in here} == {None, "store", "accum"} and {i[4] for i in here} == {1, 2}
        assert any(i[0] and not i[3] for i in here), "dy2 = None"
        small, big = N.fast_ladder(C)
        assert {s[1] for n, v, d, y, f, s in _APPLY if s[3] == C and s[0] == s[2] == 1} == set(small) | {big}
    assert {i[5] for i in generic} == {24, 40, 280, 64}
    assert any(i[0] and i[1] == 0 for i in generic), "y2, no ReLU, no z: the generic apply kernel"


def test_div24_cases():
    lo, hi = N.DIV24_M
    assert lo * 5 == N.DIV24_LIMIT - 1 and hi * 5 == N.DIV24_LIMIT + 4 and N.cv_shift(40) < 0


# ---- (4) the checks refuse what they exist to catch -------------------------------------------------
def test_checks_refuse_wrong_results():
    c = N.make_bwd("two_m1", 1, 33, 1, 8)
    good = N.bn_bwd_sums(c, F32)
    N.check_sums(good, c, "good")
    swapped = torch.cat([good[:16], good[24:], good[16:24]])                         # slots 2 and 3 of the y2 layout exchanged
    with pytest.raises(AssertionError, match="slot=2"):
        N.check_sums(swapped, c, "swapped")
    c = N.make_bwd("m1", 1, 33, 1, 8, dident="store")
    wrong = dict(c, z=torch.where(c["z"] == 0, torch.ones(()), c["z"]))              # `>=` for `>`: the planted zeros pass
    with pytest.raises(AssertionError, match=r"dident.*row=0, c=0"):
        N.check_apply(_apply_fp32(wrong), c, "mask >=")
    with pytest.raises(AssertionError, match="slot=0, c=0"):
        N.check_sums(N.bn_bwd_sums(wrong, F32), c, "mask >=")
    c = N.make_bwd("m2", 1, 33, 1, 8)
    dropped = dict(c, dz=c["dz"].clone())
    dropped["dz"][0, 32] = 0                                                         # the last row (a second row block of one row) lost
    with pytest.raises(AssertionError):
        N.check_sums(N.bn_bwd_sums(dropped, F32), c, "dropped row")
