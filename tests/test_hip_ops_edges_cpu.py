"""The per-element bounds of tests/test_hip_ops_edges.py admit a correct implementation: every linear-op case of groups A and B,
evaluated with plain torch fp32 on the CPU (rounded once to bf16 where the kernel stores bf16), stays inside the bound the GPU
test applies to the HIP kernel, against the same float64 reference.  And the group C shapes land on the intended side of the
grid-stride and division thresholds.  No GPU."""
import pytest
import torch

import hip_ops_edge_cases as E

_CASES = E.linear_cases()


def _leaves(v):
    return list(v) if isinstance(v, (tuple, list)) else [v]


@pytest.mark.parametrize("case", _CASES, ids=[c[0] for c in _CASES])
def test_fp32_evaluation_is_inside_the_bound(case):
    name, bf16_result, terms, ev, ev_abs = case
    ref, S, got = _leaves(ev(E.F64)), _leaves(ev_abs()), _leaves(ev(E.F32))
    assert len(ref) == len(S) == len(got)
    for k, (r, s, g) in enumerate(zip(ref, S, got)):
        assert r.dtype == E.F64 and s.dtype == E.F64 and g.dtype == E.F32
        assert bool((s >= r.abs() * (1 - 1e-12)).all()), "the scale is the reference on absolute values: never below |reference|"
        E.assert_bound(E.to_result(g, bf16_result), r, s, E.REL_BF16 if bf16_result else 0.0, E.abs_coef(terms), "%s[%d]" % (name, k))


def test_bound_rejects_a_one_ulp_error():
    """the bound is tight enough to matter: a bf16 result two ulps off, or an fp32 result 2^-17 off, is refused"""
    name, bf16_result, terms, ev, ev_abs = next(c for c in _CASES if c[0].startswith("upsample2_fwd-4x6x24"))
    ref, S = ev(E.F64), ev_abs()
    good = E.to_result(ev(E.F32), True)
    E.assert_bound(good, ref, S, E.REL_BF16, E.abs_coef(terms), name)
    off = good.clone()
    off.view(-1)[7] *= 1 + 2.0 ** -6
    with pytest.raises(AssertionError, match="flat index 7 "):
        E.assert_bound(off, ref, S, E.REL_BF16, E.abs_coef(terms), name)
    name, bf16_result, terms, ev, ev_abs = next(c for c in _CASES if c[0].startswith("batch_rowsum-3x7x24"))
    off = ev(E.F32).double()
    off.view(-1)[-1] += 2.0 ** -17 * float(ev_abs().view(-1)[-1])
    with pytest.raises(AssertionError):
        E.assert_bound(off, ev(E.F64), ev_abs(), 0.0, E.abs_coef(terms), name)


def test_chunk_and_row_errors_see_one_bad_vector():
    """a dropped last 16-byte vector: invisible to a whole-tensor 4e-3 relative L2, caught by the ragged last chunk"""
    ref = E.randn_bf((2056 * 300,), 1)
    got = ref.clone()
    got[-8:] = 0
    whole = float((got - ref).norm() / ref.norm())
    assert whole < 4e-3
    errs = E.chunk_relerr(got, ref)
    assert len(errs) == 302 and max(errs[:-1]) == 0 and errs[-1] > 0.1
    with pytest.raises(AssertionError):
        E.assert_chunks(got, ref, 4e-3)


@pytest.mark.parametrize("kernel", sorted(E.STRIDE2_CASES))
def test_second_grid_stride_trip_shapes(kernel):
    shape, items = E.STRIDE2_CASES[kernel]
    assert E.GRID_ITEMS < items < 2 * E.GRID_ITEMS and items % E.GRID_ITEMS != 0
    assert items == _work_items(kernel, shape)


@pytest.mark.parametrize("kernel", sorted(E.RCP_TOP_CASES))
def test_reciprocal_division_top_shapes(kernel):
    shape, items = E.RCP_TOP_CASES[kernel]
    assert E.FAST_DIV_LIMIT - 4096 <= items < E.FAST_DIV_LIMIT
    assert items == _work_items(kernel, shape)
    extents = [shape[k] for k in ("H", "W") if k in shape]
    assert all(e & (e - 1) for e in extents), "non-power-of-two extents"


def test_square_stem_shape_is_in_the_reciprocal_range():
    shape, items = E.STEM_SQUARE_CASE
    assert items == _work_items("stem_im2col", shape) == 16760836 and E.GRID_ITEMS < items < E.FAST_DIV_LIMIT


@pytest.mark.parametrize("kernel", sorted(E.DIV64_CASES))
def test_64_bit_division_shapes(kernel):
    shape, items = E.DIV64_CASES[kernel]
    assert items >= E.FAST_DIV_LIMIT
    assert items == _work_items(kernel, shape)


def _work_items(kernel, s):
    """the launchers' own work-item counts (csrc/elementwise.hip), restated"""
    if kernel == "avgpool2_fwd":
        return s["B"] * (s["H"] // 2) * (s["W"] // 2) * (s["C"] // 8)
    if kernel == "avgpool2_bwd":
        return s["B"] * s["H"] * s["W"] * (s["C"] // 8)
    if kernel == "upsample2_fwd":
        return s["B"] * s["H"] * s["W"] * 4 * (s["C"] // 8)
    if kernel == "stem_im2col":
        return s["B"] * ((s["H"] - 1) // 2 + 1) * ((s["W"] - 1) // 2 + 1) * 4
    if kernel == "add_bf16":
        return s["M"] * (s["C"] // 8)
    if kernel == "cast_f32_bf16_drop":
        return s["n"]
    raise KeyError(kernel)


def test_layernorm_case_table():
    lanes = sorted({C // 8 for C, _ in E.LN_CASES})
    assert lanes == [1, 3, 65, 129, 193, 255]
    assert all(C % 8 == 0 and C <= 2048 for C, _ in E.LN_CASES)
    rows = sorted({r for _, r in E.LN_CASES})
    assert rows == [1, 5, 2049, 8193] and 2049 > 512 * 4 and 8193 > 2048 * 4
    assert all(r % E.LN_POS_ROWS for r in rows), "pos_rows divides no row count"
