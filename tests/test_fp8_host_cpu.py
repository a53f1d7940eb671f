"""FP8 inference, host side (no GPU): the power-of-two exponent rule, the reference quantiser the kernels are held to, and the
C ABI of the fp8 kernels (exports, struct mirrors, tile variants)."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from cris.pytorch_amd import hip, ops
    return hip, hip.load(), ops


def test_exponent_rule_hand_cases(lib):
    _, _, ops = lib
    e = ops.fp8_exponent
    # headroom 1 (weights): the smallest e with amax * 2^-e <= 448
    assert e(0.0) == 0
    assert e(448.0) == 0
    assert e(448.0 * 2.0 ** 5) == 5 and e(448.0 * 2.0 ** -7) == -7
    assert e(math.nextafter(448.0, 1e9)) == 1                  # just above the largest e4m3 value
    assert e(math.nextafter(448.0, 0.0)) == 0
    assert e(1.0) == -8 and e(2.0) == -7 and e(0.5) == -9       # powers of two: 2^j * 2^-e = 256
    assert e(1.75) == -8 and e(math.nextafter(1.75, 9.0)) == -7  # 1.75 * 256 = 448 exactly; one ulp more does not fit
    assert e(2.0 ** -30) == -38
    # headroom 4 (activations): limit 112
    assert e(112.0, 4.0) == 0 and e(math.nextafter(112.0, 1e9), 4.0) == 1
    assert e(1.0, 4.0) == -6 and e(3.5, 4.0) == -5
    with pytest.raises(ValueError):
        e(float("inf"))


def test_exponent_rule_is_minimal(lib):
    _, _, ops = lib
    gen = torch.Generator().manual_seed(0)
    xs = (torch.rand(2000, generator=gen, dtype=torch.float64) * torch.exp2(torch.randint(-40, 40, (2000,), generator=gen).double())).tolist()
    for h in (1.0, 4.0, 3.0):
        lim = 448.0 / h
        for a in xs:
            k = ops.fp8_exponent(a, h)
            assert math.ldexp(a, -k) <= lim < math.ldexp(a, -(k - 1)), (a, h, k)


def test_reference_quantiser_saturates(lib):
    _, _, ops = lib
    x = torch.tensor([500.0, -500.0, 448.0, 1e6, 2.0 ** -10, 3 * 2.0 ** -10, 0.0])
    q = ops.quantise_fp8_reference(x, 0).view(torch.uint8).tolist()
    # 500 -> 448 (0x7E), not NaN (0x7F); 2^-10 is the tie between 0 and 2^-9 -> 0 (even); 3 * 2^-10 the tie between
    # 2^-9 and 2 * 2^-9 -> 2 * 2^-9 (0x02, even)
    assert q == [0x7E, 0xFE, 0x7E, 0x7E, 0x00, 0x02, 0x00]
    assert torch.equal(ops.quantise_fp8_reference(x * 8, 3).view(torch.uint8), ops.quantise_fp8_reference(x, 0).view(torch.uint8))


def test_fp8_abi(lib):
    hip, l, ops = lib
    for name in ("cris_conv_gemm_fp8", "cris_conv_gemm_fp8_plan", "cris_pack_weights_fp8", "cris_avgpool2_fwd_fp8", "cris_absmax_bf16"):
        assert name in hip.EXPORTS
    assert l.cris_sizeof(b"cris_conv_gemm_fp8_params") == C.sizeof(hip.ConvGemmFp8Params)
    assert l.cris_sizeof(b"cris_pack_fp8_desc") == C.sizeof(hip.PackFp8Desc)
    assert ops.gemm_fp8_variants() == ["128x128", "64x64"]


def test_fp8_tile_plan(lib):
    hip, l, ops = lib

    def plan(M, N, variant=-1):
        p = hip.ConvGemmFp8Params()
        p.M, p.N = M, N
        return ops.gemm_fp8_variants()[l.cris_conv_gemm_fp8_plan(C.byref(p), variant)] if l.cris_conv_gemm_fp8_plan(C.byref(p), variant) >= 0 else None

    assert plan(346112, 64) == "64x64"           # narrow
    assert plan(5408, 512) == "64x64"            # mid-size: too few 128x128 tiles
    assert plan(346112, 256) == "128x128"
    assert plan(346112, 256, 1) == "64x64"
    assert plan(346112, 256, 7) is None
