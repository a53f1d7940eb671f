"""The cases, the bound and the emulation of tests/test_eval_post_edges.py, settled without a GPU (tests/eval_post_edge_cases.py):
the cases have the properties they were chosen for; the numpy restatement of the warp and upsample kernels equals
oracle/eval_post.py bit for bit in every case; with any one of its error switches on it changes a count, a mask byte, a statistics
entry or an upsampled value in a named case; the upsample bound comes from the oracle's own float32 error; and the host half of
the library inverts every matrix exactly as the oracle does and refuses bad launches before it touches a device.

The upsample bound, measured here (test_upsample_bound_comes_from_the_oracle prints it): r0 = max |oracle float32 restatement -
float64 reference| = 1.49e-06 over all upsample cases (absolute, values in [-0.36, 1.41]); the GPU test allows 4 r0 = 5.97e-06.
On the MI355X the kernel's worst error is 0.25 of that bound (5x9->20x37 at logit scale 30), the oracle's own ratio there."""
import ctypes as C

import numpy as np
import pytest

import eval_post_edge_cases as E
from oracle import eval_post as EP


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()


def test_cases_have_the_properties_they_were_chosen_for():
    E.self_check()
    for H, W in E.MAP_SHAPES:
        for name in E.BORDER_SEPARATES:
            k = E.desc_index(name)
            d = E.descriptors(H, W)[k]
            print("%dx%d %-12s foreground at border 0, 0.5, -0.25: %s of %d" % (
                H, W, name, [int((E.oracle_warp(H, W, k, 0, b) > E.THR).sum()) for b in E.BORDERS], d.h_out * d.w_out))


def test_batch_layout_spreads_descriptors_over_maps_and_shares_masks():
    for H, W in E.MAP_SHAPES:
        masks, entries = E.batch_layout(H, W)
        assert len(entries) == 2 * len(E.NAMES) and {e.map for e in entries} == {0, 1, 2}
        assert {e.name for e in entries if e.map == 0} == set(E.NAMES)
        assert {(e.name, e.map) for e in entries} >= {("identity", E.TIES_MAP), ("shift", E.TIES_MAP)}
        shared = [sum(e.mask == i for e in entries) for i in range(len(masks))]
        assert max(shared) >= 4 and min(shared) >= 2                       # several descriptors per mask
        assert [e.row for e in entries] != sorted(e.row for e in entries)  # rows are not the launch order
        for e in entries:
            d = E.descriptors(H, W)[e.k]
            assert masks[e.mask].shape == (d.h_out, d.w_out) and masks[e.mask].dtype == np.uint8


@pytest.mark.parametrize("shape", E.MAP_SHAPES, ids=lambda s: "%dx%d" % s)
def test_error_free_warp_emulation_equals_the_oracle_bit_for_bit(shape):
    H, W = shape
    assert np.array_equal(E.emu_table(), EP.cubic_table())
    masks, entries = E.batch_layout(H, W)
    for k, d in enumerate(E.descriptors(H, W)):
        assert E.emu_invert(d.mat).tobytes() == EP.invert_affine(d.mat).tobytes(), d.name
        mask = masks[next(e.mask for e in entries if e.k == k)]
        for mp in range(E.P):
            for b in E.BORDERS + (E.TIE_BORDER,):
                want = E.oracle_warp(H, W, k, mp, b)
                v = E.emu_warp(E.maps(H, W), mp, d.mat, d.w_out, d.h_out, b)
                assert v.dtype == np.float32 and v.tobytes() == want.tobytes(), (d.name, mp, b)
                assert E.emu_counts(v, mask, E.THR) == E.oracle_counts(want, mask, E.THR)
                assert np.array_equal(E.emu_mask_bytes(v, E.THR), E.oracle_mask_bytes(want, E.THR))
                assert E.emu_predict_row(v, E.THR) == E.oracle_predict_row(want, E.THR)
            for T, thrs in E.SWEEPS.items():                               # bracket test + binary search + histogram algebra
                assert np.array_equal(E.emu_sweep_counts(v, mask, thrs), E.oracle_sweep_counts(want, mask, thrs)), (d.name, mp, T)


def test_error_free_upsample_emulation_equals_the_oracle_bit_for_bit():
    for c in E.upsample_cases():
        got, want = E.emu_upsample(c.logits, c.H, c.W), E.oracle_upsample(c.logits, c.H, c.W)
        assert got.shape == want.shape == (E.UP_B, c.H, c.W) and got.dtype == np.float32
        assert np.array_equal(np.isnan(got), np.isnan(want)) and got[~np.isnan(got)].tobytes() == want[~np.isnan(want)].tobytes(), c.name


def test_upsample_bound_comes_from_the_oracle():
    """r0: the oracle's float32 restatement against the float64 reference - never the kernel; the GPU test allows 4 r0"""
    r0 = E.upsample_r0()
    print("\nupsample: r0 = %.3e (float32 oracle against float64 reference, absolute), bound 4 r0 = %.3e" % (r0, E.upsample_bound()))
    assert E.upsample_bound() == 4.0 * r0
    assert 2.0 ** -21 < r0 < 2.0 ** -18            # a few float32 ulps of values around 1: the reference and the oracle describe one function
    lo = min(float(np.nanmin(E.upsample_ref64(c.logits, c.H, c.W))) for c in E.upsample_cases())
    hi = max(float(np.nanmax(E.upsample_ref64(c.logits, c.H, c.W))) for c in E.upsample_cases())
    print("values in [%.3f, %.3f]" % (lo, hi))
    assert -0.5 < lo < -0.1 and 1.1 < hi < 1.5     # the cubic overshoots on both sides
    # identity size: every weight is exactly (0, 1, 0, 0), the reference is the float64 sigmoid itself
    for c in E.upsample_cases():
        if c.logits.shape[1:] == (c.H, c.W):
            assert np.array_equal(E.upsample_ref64(c.logits, c.H, c.W), E.sigmoid64(c.logits))
    x = E.up_case("special values")
    ref = E.upsample_ref64(x.logits, x.H, x.W)
    assert np.isfinite(ref).all() and E.upsample_ratio(E.oracle_upsample(x.logits, x.H, x.W), ref) <= 0.25
    print("special values: reference in [%.3f, %.3f]" % (ref.min(), ref.max()))


def _changed(good, bad, what):
    return not np.array_equal(np.asarray(good[what]), np.asarray(bad[what]))


@pytest.mark.parametrize("switch", E.WARP_SWITCHES)
def test_each_warp_error_is_caught_in_its_named_case(switch):
    shape, name, mp, border, what = E.SWITCH_CASES[switch]
    good, bad = E.warp_outputs(shape, name, mp, border), E.warp_outputs(shape, name, mp, border, (switch,))
    H, W = shape
    v = E.oracle_warp(H, W, E.desc_index(name), mp, border)
    assert good["value"].tobytes() == v.tobytes() and good["row"] == E.oracle_predict_row(v, E.THR)
    print("%s: %dx%d map %d, %s, border %g: %s %s -> %s" % (switch, H, W, mp, name, border, what,
                                                          np.asarray(good[what]).ravel()[:6].tolist(), np.asarray(bad[what]).ravel()[:6].tolist()))
    assert _changed(good, bad, what), ("the error %r does not change the %s of its named case (%dx%d map %d, %s, border %g): the case "
                                       "list is too weak" % (switch, what, H, W, mp, name, border))


@pytest.mark.parametrize("switch", E.UP_SWITCHES)
def test_each_upsample_error_exceeds_the_bound_tenfold_in_its_named_case(switch):
    c = E.up_case(E.SWITCH_CASES[switch])
    ref = E.upsample_ref64(c.logits, c.H, c.W)
    assert E.upsample_ratio(E.emu_upsample(c.logits, c.H, c.W), ref) <= 0.25
    x = E.upsample_ratio(E.emu_upsample(c.logits, c.H, c.W, (switch,)), ref)
    print("%s: %s, error / bound %.1f" % (switch, c.name, x))
    assert x >= 10.0, "the error %r stays below 10 x the bound in its named case %s: the case list is too weak" % (switch, c.name)


def test_every_switch_has_a_named_case():
    assert set(E.SWITCH_CASES) == set(E.WARP_SWITCHES) | set(E.UP_SWITCHES)
    assert {"inside_swap", "stride_swap", "clamp_swap", "map_offset_ww", "border_ignored", "border_clamp", "fxfy_swap", "ge", "bsearch_tie",
            "round_half_up", "scale_swap", "index_swap", "y_clamp_w"} <= set(E.SWITCH_CASES)


def test_ties_decide_as_strict_comparisons_on_the_oracle():
    """what the GPU test then demands of the kernels: a value equal to a threshold is background, the next float up foreground, the
    k + 0.5 products round to even"""
    H, W = E.MAP_SHAPES[0]
    v = E.oracle_warp(H, W, E.desc_index("identity"), E.TIES_MAP, 0.0)
    for T, thrs in E.SWEEPS.items():
        for i in sorted({0, T - 1, T >> 1}):                               # thr[0], thr[T - 1] and the binary search's first probe
            t = thrs[min(i, T - 1)]
            eq, up = v == t, v == np.nextafter(t, np.float32(np.inf))
            assert eq.any() and up.any(), (T, i)
            assert not (v > t)[eq].any() and (v > t)[up].all()
    half = np.isin(v, E.half_values())
    q = E.q16_of(v)[half]
    assert half.sum() >= len(E.HALF_K) and (q % 2 == 0).all() and set(q.tolist()) == {int(k + (k & 1)) for k in E.HALF_K}
    s = E.oracle_warp(H, W, E.desc_index("shift"), E.TIES_MAP, E.TIE_BORDER)
    inside = np.zeros(s.shape, bool)
    inside[0:H - 5, 7:W + 7] = True
    assert (s[~inside] == E.THR).all() and int((s > E.THR).sum()) == int((s[inside] > E.THR).sum()) > 0


# ---- the host half of the library ----
def test_desc_fill_inverts_every_matrix_as_the_oracle_does(built):
    from cris.pytorch_amd import hip
    l = hip.load()
    d = (hip.EvalDesc * 1)()
    seen = 0
    for H, W in E.MAP_SHAPES:
        for desc in E.descriptors(H, W):
            mat = (C.c_double * 6)(*np.asarray(desc.mat, np.float64).reshape(6).tolist())
            assert l.cris_eval_desc_fill(C.addressof(d), mat, desc.w_out, desc.h_out, 1, 0, E.pitch_of(desc.w_out), 0, 2) == 0
            got = np.array(list(d[0].m), np.float64)
            assert got.tobytes() == EP.invert_affine(desc.mat).reshape(6).tobytes(), (desc.name, got.tolist())
            assert (d[0].w_out, d[0].h_out, d[0].map, d[0].row, d[0].pitch) == (desc.w_out, desc.h_out, 1, 2, E.pitch_of(desc.w_out))
            if desc.name in E.SINGULAR:
                assert (got == 0.0).all(), desc.name                       # six zeros (-m * 0 leaves the sign bit of some set)
                seen += 1
    assert seen == 4


def test_batch_launchers_refuse_before_any_launch(built):
    """a non-finite border, thr < 0 (cris_predict_masks_batch) and a descriptor whose map index is >= P (all three launchers): the
    pointers below are not addresses, so a launcher that got as far as its kernel would not return an argument error"""
    from cris.pytorch_amd import hip
    l = hip.load()
    d = (hip.EvalDesc * 1)()
    mat = (C.c_double * 6)(1, 0, 0, 0, 1, 0)
    Pn, H, W = E.P, 40, 72

    def fill(map=0):
        assert l.cris_eval_desc_fill(C.addressof(d), mat, 5, 4, map, 0, 8, 0, 0) == 0

    def predict(thr=0.35, border=0.0):
        return l.cris_predict_masks_batch(0x1000, Pn, H, W, C.addressof(d), 0x2000, 1, thr, border, 0x4000, 4, None, 0, None)

    def iou(border=0.0):
        return l.cris_eval_iou_batch(0x1000, Pn, H, W, C.addressof(d), 0x2000, 1, 0x3000, 64, 0.35, border, 0x4000, 4, None, 0, None)

    def sweep(border=0.0):
        thr = (C.c_float * 3)(0.2, 0.35, 0.5)
        return l.cris_eval_iou_sweep_batch(0x1000, Pn, H, W, C.addressof(d), 0x2000, 1, 0x3000, 64, thr, 3, border, 0x4000, 4, None)

    def rejected(call, symbol, msg, **kw):
        assert call(**kw) != 0
        err = l.cris_last_error()
        assert symbol in err and msg in err, (kw, err)

    fill()
    for bad in (float("nan"), float("inf"), float("-inf")):
        rejected(predict, b"cris_predict_masks_batch", b"border must be finite", border=bad)
    for bad in (-1e-30, -0.25, float("-inf"), float("nan"), float("inf")):
        rejected(predict, b"cris_predict_masks_batch", b"thr must be finite and >= 0", thr=bad)
    for bad in (Pn, Pn + 1, -1, 2 ** 31 - 1):
        fill(map=bad)
        rejected(predict, b"cris_predict_masks_batch", b"map out of range")
        rejected(iou, b"cris_eval_iou_batch", b"map / row out of range")
        rejected(sweep, b"cris_eval_iou_sweep_batch", b"map / row out of range")
