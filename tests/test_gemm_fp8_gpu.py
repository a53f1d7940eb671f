"""FP8 inference kernels on the GPU (csrc/gemm_fp8.hip): the quantisers are bit-exact with torch's CPU float8_e4m3fn plus
clamp, the implicit-GEMM convolution stays within an fp32-accumulation bound of a float64 GEMM of the dequantised operands
(exact on small-integer data), writes nothing outside its declared output ranges, and is deterministic and the same for
every tile variant."""
import os
import sys

import pytest
import torch
import torch.nn.functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    g.build()
    from cris.pytorch_amd import ops as o
    return o


def dev():
    return torch.device("cuda:0")


def q_ref(x32, e):
    """torch's CPU reference quantiser: bytes of (x * 2^-e).clamp(+-448).to(e4m3fn)"""
    return (x32.float().cpu() * 2.0 ** -e).clamp(-448, 448).to(FP8).view(torch.uint8)


def wide_values(n, gen, lo=-14, hi=12):
    """values over many binades, with exact e4m3 ties / subnormals / saturation cases mixed in"""
    x = torch.randn(n, generator=gen) * torch.exp2(torch.randint(lo, hi, (n,), generator=gen).float())
    grid = torch.arange(0, 127, dtype=torch.uint8).view(FP8).float().sort().values
    ties = (grid[1:] + grid[:-1]) / 2
    special = torch.cat([grid, ties, -ties, torch.tensor([448., 449., 464., 480., 500., 1e4, -1e4, -448., 0., 2. ** -9, 2. ** -10,
                                                           3 * 2. ** -11, 2. ** -6, -2. ** -10])])
    x[:len(special)] = special[:n]
    return x


# ------------------------------------------------------------------------------------------------------------------------------
# quantisers
# ------------------------------------------------------------------------------------------------------------------------------
def test_weight_pack_bit_exact(ops):
    gen = torch.Generator().manual_seed(1)
    cases = [(48, 64, 9), (64, 24, 1), (40, 16, 9)]          # (N, Cin, taps): Cin 24 -> padded to 32 per tap
    tab = ops.PackTableFp8()
    srcs, outs = [], []
    for (N, Cin, taps) in cases:
        w = torch.randn(N, Cin, taps, generator=gen) * torch.exp2(torch.randint(-10, 8, (N, 1, 1), generator=gen).float())
        w[3] = 0.0                                           # an all-zero row: exponent 0, zero bytes
        w[5, 0, 0] = 448.0 * 2.0 ** 3                        # a row whose max sits exactly on 448 * 2^e
        rs = torch.exp(torch.randn(N, generator=gen) * 0.3)
        rs[7] = -1.5
        wd, rsd = w.to(dev()), rs.to(dev())
        srcs.append((w, rs))
        outs.append(tab.add(wd, N, Cin, taps, row_scale=rsd) + (wd, rsd))
    tab.run()
    torch.cuda.synchronize()
    for (w, rs), (N, Cin, taps), (dst, e_w, _, _) in zip(srcs, cases, outs):
        v = w * rs[:, None, None]                            # fp32, as the kernel computes it
        e_ref = torch.tensor([ops.fp8_exponent(float(v[n].abs().max())) for n in range(N)], dtype=torch.int32)
        assert torch.equal(e_w.cpu(), e_ref)
        Cpad = (Cin + 15) // 16 * 16
        exp = torch.zeros(N, taps, Cpad, dtype=torch.uint8)
        for n in range(N):
            exp[n, :, :Cin] = q_ref(v[n].t(), int(e_ref[n]))
        assert torch.equal(dst.view(torch.uint8).cpu(), exp.reshape(N, taps * Cpad))


def test_avgpool2_fp8_bit_exact(ops):
    gen = torch.Generator().manual_seed(2)
    Bn, H, W, C, ld = 2, 6, 10, 40, 48
    x = wide_values(Bn * H * W * ld, gen, -12, 10).reshape(Bn, H, W, ld).to(torch.bfloat16)
    xd = x.to(dev())
    for e_y in (-3, 0, 2):
        y8 = torch.full((Bn * 3 * 5, 64), 0x55, dtype=torch.uint8, device=dev())
        y = torch.empty(Bn * 3 * 5, C, dtype=torch.bfloat16, device=dev())
        ops.avgpool2_fwd_fp8(xd, Bn, H, W, C, y8.view(FP8), e_y, ldx=ld, xcoff=8, ldq=64, qcoff=16, y=y)
        yb = torch.empty_like(y)
        ops.avgpool2_fwd(xd, Bn, H, W, C, yb, ldx=ld, xcoff=8)
        torch.cuda.synchronize()
        t = x[..., 8:8 + C].float()
        s = (((t[:, 0::2, 0::2] + t[:, 0::2, 1::2]) + t[:, 1::2, 0::2]) + t[:, 1::2, 1::2]) * 0.25
        s = s.reshape(-1, C)
        got = y8.cpu()
        assert torch.equal(got[:, 16:16 + C], q_ref(s, e_y))
        assert (got[:, :16] == 0x55).all() and (got[:, 16 + C:] == 0x55).all()
        assert torch.equal(y.cpu(), yb.cpu()) and torch.equal(y.cpu(), s.to(torch.bfloat16))


def test_absmax(ops):
    gen = torch.Generator().manual_seed(3)
    x = (torch.randn(5000, 72, generator=gen) * 3).to(torch.bfloat16)
    x[1234, 20] = -97.5
    xd = x.to(dev())
    out = torch.empty(1, device=dev())
    ops.absmax_bf16(xd, 5000, 64, out, xcoff=8)
    torch.cuda.synchronize()
    assert float(out) == float(x[:, 8:72].float().abs().max()) == 97.5


# ------------------------------------------------------------------------------------------------------------------------------
# the convolution
# ------------------------------------------------------------------------------------------------------------------------------
MFMA_FP8_REL = 2.0 ** -14
SENT = 0x7BCD            # bf16 guard pattern (a finite value no launch here produces)
SENT8 = 0x5A


def run_conv(ops, A8, lda, W8, e_w, g, N, e_x, *, bias=None, act=0, resid=None, out_mode="both", e_y=0, variant=-1, c_coff=8, q_coff=16):
    M = g.M
    ldc, ldq = c_coff + N + 24, q_coff + N + 32
    out = out8 = None
    if out_mode in ("bf16", "both"):
        out = torch.full((M + 40, ldc), SENT, dtype=torch.int16, device=dev()).view(torch.bfloat16)
    if out_mode in ("fp8", "both"):
        out8 = torch.full((M + 40, ldq), SENT8, dtype=torch.uint8, device=dev())
    ops.conv_gemm_fp8(A8, W8, e_w, g, N, e_x, lda=lda, bias=bias, act=act, resid=resid, out=out, ldc=ldc, c_coff=c_coff,
                      out8=None if out8 is None else out8.view(FP8), ldq=ldq, q_coff=q_coff, e_y=e_y, variant=variant)
    torch.cuda.synchronize()
    res = {}
    if out is not None:
        o = out.view(torch.int16).cpu()
        mask = torch.ones_like(o, dtype=torch.bool)
        mask[:M, c_coff:c_coff + N] = False
        assert (o[mask] == SENT).all(), "bf16 output written outside [0, M) x [c_coff, c_coff + N)"
        res["out"] = o[:M, c_coff:c_coff + N].view(torch.bfloat16).float()
    if out8 is not None:
        o = out8.cpu()
        mask = torch.ones_like(o, dtype=torch.bool)
        mask[:M, q_coff:q_coff + N] = False
        assert (o[mask] == SENT8).all(), "fp8 output written outside [0, M) x [q_coff, q_coff + N)"
        res["out8"] = o[:M, q_coff:q_coff + N].clone()
    return res


def reference(A8, C, W8, e_w, g, N, e_x, bias, act, resid):
    """float64 GEMM of the dequantised operands (+ epilogue), and sum |a*b| per element (for the bound)"""
    a = A8.view(FP8).cpu()[..., :C].double() * 2.0 ** e_x                              # [Bn, H, W, C]
    taps = g.KH * g.KW
    w = W8.view(FP8).cpu()[:, :taps * C].double().reshape(N, g.KH, g.KW, C) * torch.exp2(e_w.cpu().double())[:, None, None, None]
    x = a.permute(0, 3, 1, 2)
    wk = w.permute(0, 3, 1, 2)
    acc = Fn.conv2d(x, wk, stride=g.stride, padding=g.pad).permute(0, 2, 3, 1).reshape(-1, N)
    mag = Fn.conv2d(x.abs(), wk.abs(), stride=g.stride, padding=g.pad).permute(0, 2, 3, 1).reshape(-1, N)
    y = acc + (bias.cpu().double() if bias is not None else 0.0)
    if act == 1:
        y = y.clamp_min(0)
    if resid is not None:
        y = y + resid.cpu()[:, :N].double()
    if act == 3:
        y = y.clamp_min(0)
    return y, mag


def make_operands(ops, gen, Bn, H, Wd, C, N, k, integer=False):
    lda = C + 16
    if integer:
        a = torch.randint(-3, 4, (Bn, H, Wd, lda), generator=gen).float()
        w = torch.randint(-4, 5, (N, C, k * k), generator=gen).float()
        w[:, 0, 0] = 4.0                                                     # every row's max is 4: e_w = -6, W8 = 64 * w exactly
        e_x = 0
    else:
        a = torch.randn(Bn, H, Wd, lda, generator=gen) * 40
        w = torch.randn(N, C, k * k, generator=gen) * torch.exp2(torch.randint(-6, 2, (N, 1, 1), generator=gen).float())
        e_x = -2
    A8 = (a * 2.0 ** -e_x).clamp(-448, 448).to(FP8).to(dev())
    tab = ops.PackTableFp8()
    W8, e_w = tab.add(w.to(dev()), N, C, k * k)
    tab.run()
    return A8, lda, W8, e_w, e_x


GEOMS = [(16, 1), (64, 1), (256, 1), (16, 3), (64, 3), (256, 3)]


@pytest.mark.parametrize("variant", ["128x128", "64x64"])
@pytest.mark.parametrize("C,k", GEOMS)
def test_conv_fp8_audit(ops, variant, C, k):
    from cris.pytorch_amd.ops import Geom
    gen = torch.Generator().manual_seed(10 * C + k)
    Bn, H, Wd, N = 3, 11, 13, 200                    # M = 429 and N = 200: ragged against both tiles
    A8, lda, W8, e_w, e_x = make_operands(ops, gen, Bn, H, Wd, C, N, k)
    g = Geom(Bn, H, Wd, C, k, k, 1, k // 2)
    bias = (torch.randn(N, generator=gen) * 10).to(dev())
    resid = (torch.randn(g.M, N + 8, generator=gen) * 20).to(torch.bfloat16).to(dev())
    for act, rs, mode, e_y in ((0, None, "bf16", 0), (1, None, "fp8", 4), (3, resid, "both", 5), (1, resid, "both", 3)):
        r = run_conv(ops, A8, lda, W8, e_w, g, N, e_x, bias=bias, act=act, resid=rs, out_mode=mode, e_y=e_y, variant=variant)
        ref, mag = reference(A8, C, W8, e_w, g, N, e_x, bias, act, rs)
        # fp32 accumulation: ceil(K/64) dependent MFMA additions + the epilogue adds, plus what one
        # v_mfma_scale_f32_32x32x64_f8f6f4 loses inside its 64-product sum (not a sequential fp32 chain: up to ~2^-17 of
        # sum |a b| measured on MI355X; bounded here by MFMA_FP8_REL)
        acc_bound = 1.1 * ((-(-g.K // 64) + 4) * 2.0 ** -24 + MFMA_FP8_REL) * (mag + bias.abs().cpu().double().max() + 1000.0)
        if "out" in r:
            err = (r["out"].double() - ref).abs()
            bound = acc_bound + 2.0 ** -8 * ref.abs()
            assert (err <= bound).all(), (variant, C, k, act, float((err / bound).max()))
            print("fp8 conv audit %s C%d k%d act%d: max err/bound %.3f" % (variant, C, k, act, float((err / bound).max())))
        if "out8" in r:
            deq = r["out8"].view(FP8).double() * 2.0 ** e_y
            err = (deq - ref.clamp(-448 * 2.0 ** e_y, 448 * 2.0 ** e_y)).abs()
            bound = acc_bound + 2.0 ** -4 * ref.abs() + 2.0 ** (e_y - 10)
            assert (err <= bound).all(), (variant, C, k, act, float((err / bound).max()))


@pytest.mark.parametrize("C,k", [(16, 3), (64, 1), (256, 3)])
def test_conv_fp8_exact_integers(ops, C, k):
    """small integers: every partial sum is exact in fp32, so each output is the rounding of the exact result - bit for bit,
    for both tile variants (this also pins the f8f6f4 operand lane maps: an asymmetric random B)"""
    from cris.pytorch_amd.ops import Geom
    gen = torch.Generator().manual_seed(100 + C + k)
    Bn, H, Wd, N = 2, 9, 15, 136
    A8, lda, W8, e_w, e_x = make_operands(ops, gen, Bn, H, Wd, C, N, k, integer=True)
    assert (e_w.cpu() == -6).all()
    g = Geom(Bn, H, Wd, C, k, k, 1, k // 2)
    bias = torch.randint(-50, 50, (N,), generator=gen).float().to(dev())
    resid = torch.randint(-60, 60, (g.M, N), generator=gen).float().to(torch.bfloat16).to(dev())
    ref, _ = reference(A8, C, W8, e_w, g, N, e_x, bias, 3, resid)
    e_y = 6
    outs = []
    for variant in ("128x128", "64x64"):
        r = run_conv(ops, A8, lda, W8, e_w, g, N, e_x, bias=bias, act=3, resid=resid, out_mode="both", e_y=e_y, variant=variant)
        assert torch.equal(r["out"].to(torch.bfloat16), ref.float().to(torch.bfloat16)), variant
        assert torch.equal(r["out8"], q_ref(ref.float(), e_y)), variant
        outs.append(r)
    assert torch.equal(outs[0]["out"], outs[1]["out"]) and torch.equal(outs[0]["out8"], outs[1]["out8"])


def test_conv_fp8_epilogue_quantiser_bit_exact(ops):
    """A = 0: the fp32 value the epilogue quantises is bias[n] + resid[m, n] (one fp32 add, as torch does it on the CPU)"""
    from cris.pytorch_amd.ops import Geom
    gen = torch.Generator().manual_seed(4)
    Bn, H, Wd, C, N = 1, 16, 16, 32, 256
    g = Geom(Bn, H, Wd, C)
    A8 = torch.zeros(Bn, H, Wd, C, dtype=FP8, device=dev())
    W8 = torch.randn(N, C, generator=gen).clamp(-448, 448).to(FP8).to(dev())
    e_w = torch.zeros(N, dtype=torch.int32, device=dev())
    bias = wide_values(N, gen, -10, 10)
    resid = wide_values(g.M * N, torch.Generator().manual_seed(5), -12, 9).reshape(g.M, N).to(torch.bfloat16)
    resid[:64] = 0
    for e_y in (-4, 0, 3):
        r = run_conv(ops, A8, C, W8, e_w, g, N, 0, bias=bias.to(dev()), act=0, resid=resid.to(dev()), out_mode="both", e_y=e_y, variant=-1)
        x = bias[None, :] + resid.float()
        assert torch.equal(r["out8"], q_ref(x, e_y))
        assert torch.equal(r["out"].to(torch.bfloat16), x.to(torch.bfloat16))


def test_conv_fp8_deterministic_and_variant_independent(ops):
    from cris.pytorch_amd.ops import Geom
    gen = torch.Generator().manual_seed(6)
    Bn, H, Wd, C, N = 2, 26, 26, 128, 256
    A8, lda, W8, e_w, e_x = make_operands(ops, gen, Bn, H, Wd, C, N, 3)
    g = Geom(Bn, H, Wd, C, 3, 3, 1, 1)
    bias = torch.randn(N, generator=gen).to(dev())
    runs = [run_conv(ops, A8, lda, W8, e_w, g, N, e_x, bias=bias, act=1, out_mode="both", e_y=2, variant=v)
            for v in ("128x128", "128x128", "64x64", -1)]
    for r in runs[1:]:
        assert torch.equal(r["out"], runs[0]["out"]) and torch.equal(r["out8"], runs[0]["out8"])


def test_conv_fp8_rejects_bad_channels(ops):
    from cris.pytorch_amd.ops import Geom
    from cris.pytorch_amd.hip import HipLibraryError
    A8 = torch.zeros(1, 4, 4, 24, dtype=FP8, device=dev())
    W8 = torch.zeros(16, 24, dtype=FP8, device=dev())
    e_w = torch.zeros(16, dtype=torch.int32, device=dev())
    out = torch.empty(16, 16, dtype=torch.bfloat16, device=dev())
    with pytest.raises(HipLibraryError, match="multiples of 16"):
        ops.conv_gemm_fp8(A8, W8, e_w, Geom(1, 4, 4, 24), 16, 0, out=out)
