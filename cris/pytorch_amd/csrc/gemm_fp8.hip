// FP8 (OCP e4m3fn) inference kernels for gfx950: the implicit-GEMM convolution on the block-scaled MFMA
// (v_mfma_scale_f32_32x32x64_f8f6f4, unit block scales), the weight quantise + pack, a 2x2 average pool with fp8 output and
// the abs-max reduction that calibrates the activation scales.  Nothing here is used by training or by the bf16 inference path.
//
// Scales are powers of two throughout, so scaling is exact and quantisation is exactly RNE_e4m3(clamp(x * 2^-e, +-448)):
//   weights    per output channel, e_w[n] = the smallest integer with max_k |Wf[n, k]| * 2^-e_w[n] <= 448 (0 for an all-zero row)
//   activations per tensor, e_x from calibration (host)
//   epilogue   out = acc * 2^(e_x + e_w[n]) + bias[n], activation / bf16 residual as the EPI 2 kernels of gemm.hip, then a bf16
//              and / or fp8 store (fp8: its own exponent e_y)
//
// The conv keeps the structure of gemm.hip's 4-wave tiles: LDS-DMA ring with counted vmcnt and one raw barrier per K-step,
// 128-B LDS rows with XOR-swizzled 16-B chunks, XCD-aware tile order, buffer-descriptor zero fill.  A 128-B row holds 128 fp8
// K elements, so one K-step is two 32x32x64 MFMAs per fragment pair and a problem has half the K-steps of its bf16 twin.
// No atomics anywhere; every result is deterministic.
#include "gemm_common.h"

#define BK8 128                 // fp8 K elements per K-step (one 128-B LDS row)
constexpr int ST8_64x64 = 3, ST8_128x128 = 2;      // LDS-DMA ring depth per tile (as the bf16 tiles of gemm.hip)

typedef __attribute__((ext_vector_type(8))) int i32x8;      // 32 fp8 operand bytes of one lane (f8f6f4 MFMA, 32x32x64)

// RNE conversion of a finite float to OCP e4m3fn with saturation to +-448 (the caller has applied the 2^-e scale).
// Equals torch's x.clamp(-448, 448).to(torch.float8_e4m3fn) on every finite input; the sign of a zero result is kept.
__device__ __forceinline__ uint32_t cris_f32_to_e4m3(float x) {
    const uint32_t s = (__float_as_uint(x) >> 24) & 0x80u;
    const float a = fminf(fabsf(x), 448.f);
    if (a < 0.015625f)                                          // below 2^-6: subnormal grid m * 2^-9, m = 0 .. 8 (8 = 2^-6)
        return s | (uint32_t)__builtin_rintf(a * 512.f);
    uint32_t v = __float_as_uint(a);
    v += 0x7FFFFu + ((v >> 20) & 1u);                           // round the mantissa to 3 bits, nearest even
    return s | ((v >> 20) - (120u << 3));                       // exponent bias 127 -> 7
}

// the smallest integer e with amax * 2^-e <= 448 (0 when amax is 0): amax = m * 2^q, m in [0.5, 1); 448 = 0.875 * 2^9
__device__ __forceinline__ int cris_e4m3_exponent(float amax) {
    if (!(amax > 0.f)) return 0;
    int q;
    const float m = frexpf(amax, &q);
    return m <= 0.875f ? q - 9 : q - 8;
}

// 256-thread block maximum through LDS in a fixed tree order (no atomics); every thread returns the result
__device__ __forceinline__ float block_max_256(float* red, float v) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + w]);
        __syncthreads();
    }
    return red[0];
}

// the 32 operand bytes of one lane for K slice ks (0 / 1) of a 128-B LDS row: 16-B chunks ks*4 + fh*2 and the next one
__device__ __forceinline__ i32x8 fp8_fragment(const unsigned char* base, int row, int ks, int fh) {
    const u32x4 lo = *reinterpret_cast<const u32x4*>(base + lds_off(row, ks * 4 + fh * 2));
    const u32x4 hi = *reinterpret_cast<const u32x4*>(base + lds_off(row, ks * 4 + fh * 2 + 1));
    return (i32x8){(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
}

// ------------------------------------------------------------------------------------------------
// the convolution
// ------------------------------------------------------------------------------------------------
template <int BM, int BN, int WAVES_M, int WAVES_N, int STAGES>
__global__ __launch_bounds__(256) void conv_gemm_fp8_kernel(const cris_conv_gemm_fp8_params p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int WTM = BM / WAVES_M, WTN = BN / WAVES_N;
    constexpr int FM = WTM / 32, FN = WTN / 32;
    constexpr int NA = BM / 32, NB = BN / 32;                  // DMA instructions per wave per K-step (8 rows of 128 B each)
    constexpr int A_BYTES = BM * 128;
    constexpr int STAGE_BYTES = (BM + BN) * 128;
    const int bid = cris_xcd_logical_block(blockIdx.x, gridDim.x);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;

    // XCD-aware tile order (as gemm.hip): m fastest once the weight matrix outgrows an XCD's L2 share
    const int tiles_n = (p.N + BN - 1) / BN, tiles_m = (p.M + BM - 1) / BM;
    int tile_m, tile_n;
    if ((long)p.N * p.K > (2L << 20)) {
        tile_n = cris_fast_div(bid, tiles_m, __builtin_amdgcn_rcpf((float)tiles_m));
        tile_m = bid - tile_n * tiles_m;
    } else {
        tile_m = cris_fast_div(bid, tiles_n, __builtin_amdgcn_rcpf((float)tiles_n));
        tile_n = bid - tile_m * tiles_n;
    }
    const int m0 = tile_m * BM, n0 = tile_n * BN;

    // this lane's DMA role: rows (wave + 4i)*8 + (lane>>3), LDS slot lane&7, logical 16-element K-chunk kc
    const int rsub = lane >> 3;
    const int kc = (lane & 7) ^ ((4 * wave + (lane >> 4)) & 7);       // == (lane&7) ^ ((row>>1)&7)
    const int OHW = p.OH * p.OW;
    const bool lin = p.KH == 1 && p.KW == 1 && p.stride == 1 && p.pad == 0 && p.OH == p.H && p.OW == p.W;
    const float r_ohw = __builtin_amdgcn_rcpf((float)OHW), r_ow = __builtin_amdgcn_rcpf((float)p.OW);
    int a_pix[NA], a_ih[NA], a_iw[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int m = m0 + (wave + 4 * i) * 8 + rsub;
        if (m >= p.M) {
            a_pix[i] = 0; a_ih[i] = -(1 << 28); a_iw[i] = 0;
        } else if (lin) {
            a_pix[i] = m; a_ih[i] = 0; a_iw[i] = 0;
        } else {
            const int b = cris_fast_div(m, OHW, r_ohw);
            const int r = m - b * OHW;
            const int oh = cris_fast_div(r, p.OW, r_ow);
            const int ow = r - oh * p.OW;
            a_pix[i] = b * p.H * p.W;
            a_ih[i] = oh * p.stride - p.pad;
            a_iw[i] = ow * p.stride - p.pad;
        }
    }
    unsigned b_off[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) b_off[i] = (unsigned)(n0 + (wave + 4 * i) * 8 + rsub) * (unsigned)p.ldb;
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(p.A), 0, (int)((size_t)p.Bn * p.H * p.W * p.lda),
                                                                        CRIS_BUF_FLAGS);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(p.Wt), 0, (int)((size_t)p.N * p.ldb), CRIS_BUF_FLAGS);

    // general K-step issue (C % 128 != 0): every 16-channel chunk of a lane lies in one tap (C % 16 == 0), the tap is per lane
    int kcur = kc * 16;
    int c_cur = 0, kh = 0, kw = 0;
    const bool fastk = (p.C & (BK8 - 1)) == 0;
    if (!fastk) {
        const int tap = kcur / p.C;
        c_cur = kcur - tap * p.C;
        kh = tap / p.KW;
        kw = tap - kh * p.KW;
    }
    auto issue_gen = [&](int buf) {
        unsigned char* sa = smem + buf * STAGE_BYTES + wave * 1024;
        unsigned char* sb = sa + A_BYTES;
        const bool kvalid = kcur < p.K;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int ih = a_ih[i] + kh, iw = a_iw[i] + kw;
            const bool ok = kvalid && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
            const unsigned off = (unsigned)(a_pix[i] + ih * p.W + iw) * (unsigned)p.lda + (unsigned)(p.a_coff + c_cur);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_void_t*)(sa + i * 4096), 16, ok ? off : CRIS_OOB, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const unsigned off = b_off[i] + (unsigned)kcur;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_void_t*)(sb + i * 4096), 16, kvalid ? off : CRIS_OOB, 0, 0, 0);
        }
        kcur += BK8;
        c_cur += BK8;
        while (c_cur >= p.C) {
            c_cur -= p.C;
            if (++kw == p.KW) { kw = 0; ++kh; }
        }
    };
    // fast K-step issue (C % 128 == 0): a whole K-step lies in one tap (wave-uniform); pixel offsets change once per tap
    int f_kh = 0, f_kw = 0, f_c = 0, f_k = 0;
    bool f_newtap = true;
    unsigned a_base[NA];
    const unsigned lane_k = (unsigned)kc * 16u;
    auto issue_fast = [&](int buf) {
        unsigned char* sa = smem + buf * STAGE_BYTES + wave * 1024;
        unsigned char* sb = sa + A_BYTES;
        if (f_newtap) {
            f_newtap = false;
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const int ih = a_ih[i] + f_kh, iw = a_iw[i] + f_kw;
                const bool ok = (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
                a_base[i] = ok ? (unsigned)(a_pix[i] + ih * p.W + iw) * (unsigned)p.lda + (unsigned)p.a_coff + lane_k : CRIS_OOB;
            }
        }
        const unsigned kvm = f_k < p.K ? 0u : CRIS_OOB;
        const unsigned kb = (unsigned)f_k + lane_k;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const unsigned off = (a_base[i] + (unsigned)f_c) | kvm;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_void_t*)(sa + i * 4096), 16, off, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const unsigned off = (b_off[i] + kb) | kvm;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_void_t*)(sb + i * 4096), 16, off, 0, 0, 0);
        }
        f_k += BK8;
        f_c += BK8;
        if (f_c >= p.C) {
            f_c = 0;
            f_newtap = true;
            if (++f_kw == p.KW) { f_kw = 0; ++f_kh; }
        }
    };
    auto issue_stage = [&](int b_) {
        if (fastk) issue_fast(b_);
        else issue_gen(b_);
    };

    f32x16 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // f8f6f4 32x32x64 operands: lane l holds 32 bytes of row (A) / column (B) l&31; lane half h = l>>5 takes the 32 K elements
    // 32h .. 32h+31 of each 64-deep slice (16-B chunks 2h, 2h+1 of the slice).  A and B use the same map, so the sum over k is
    // the GEMM's whatever order the hardware assigns inside a slice (checked with exact integer data in the tests).
    const int fr = lane & 31, fh = lane >> 5;
    const int nk = (p.K + BK8 - 1) / BK8;
#pragma unroll
    for (int s = 0; s < STAGES - 1; ++s) issue_stage(s);
    int buf = 0;
    for (int kt = 0; kt < nk; ++kt) {
        CRIS_VMCNT((STAGES - 2) * (NA + NB));
        __builtin_amdgcn_s_barrier();
        {
            int nb = buf + STAGES - 1;
            if (nb >= STAGES) nb -= STAGES;
            issue_stage(nb);
        }
        const unsigned char* sa = smem + buf * STAGE_BYTES;
        const unsigned char* sb = sa + A_BYTES;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            i32x8 af[FM], bfr[FN];
#pragma unroll
            for (int i = 0; i < FM; ++i) af[i] = fp8_fragment(sa, wm * WTM + i * 32 + fr, ks, fh);
#pragma unroll
            for (int j = 0; j < FN; ++j) bfr[j] = fp8_fragment(sb, wn * WTN + j * 32 + fr, ks, fh);
#pragma unroll
            for (int i = 0; i < FM; ++i)
#pragma unroll
                for (int j = 0; j < FN; ++j)        // A and B e4m3 (format 0), unit E8M0 block scales (127)
                    acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af[i], bfr[j], acc[i][j], 0, 0, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (++buf == STAGES) buf = 0;
    }
    CRIS_VMCNT(0);

    // epilogue: C/D layout of the 32x32 shapes, col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5).  Elements outside the
    // problem are out-of-range buffer offsets: residual reads return 0, stores are dropped.
    const int row0 = m0 + wm * WTM, col0 = n0 + wn * WTN;
    const bool has_res = p.resid != nullptr, has_out = p.out != nullptr, has_out8 = p.out8 != nullptr;
    const __amdgpu_buffer_rsrc_t rsR = __builtin_amdgcn_make_buffer_rsrc(const_cast<cris_bf16*>(p.resid), 0,
                                                                        has_res ? (int)((size_t)p.M * p.ldr * 2) : 0, CRIS_BUF_FLAGS);
    const __amdgpu_buffer_rsrc_t rsO = __builtin_amdgcn_make_buffer_rsrc(p.out, 0, has_out ? (int)((size_t)p.M * p.ldc * 2) : 0, CRIS_BUF_FLAGS);
    const __amdgpu_buffer_rsrc_t rsQ = __builtin_amdgcn_make_buffer_rsrc(p.out8, 0, has_out8 ? (int)((size_t)p.M * p.ldq) : 0, CRIS_BUF_FLAGS);
    const int act = p.act;
#pragma unroll
    for (int j = 0; j < FN; ++j) {
        const int col = col0 + j * 32 + fr;
        const bool cvalid = col < p.N;
        const int cc = cvalid ? col : 0;
        const int esc = p.e_x + p.e_w[cc];
        const float bias = p.bias ? p.bias[cc] : 0.f;
#pragma unroll
        for (int i = 0; i < FM; ++i) {
            float rres[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = row0 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * fh;
                const unsigned off = (has_res && cvalid && m < p.M) ? ((unsigned)m * (unsigned)p.ldr + (unsigned)(p.r_coff + col)) * 2u : CRIS_OOB;
                rres[e] = bf2f((bf16_t)__builtin_amdgcn_raw_buffer_load_b16(rsR, off, 0, 0));
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = row0 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * fh;
                const bool valid = cvalid && m < p.M;
                float x = __builtin_amdgcn_ldexpf(acc[i][j][e], esc) + bias;
                if (act == 1) x = fmaxf(x, 0.f);
                x += rres[e];
                if (act == 3) x = fmaxf(x, 0.f);
                if (has_out) {
                    const unsigned off = valid ? ((unsigned)m * (unsigned)p.ldc + (unsigned)(p.c_coff + col)) * 2u : CRIS_OOB;
                    __builtin_amdgcn_raw_buffer_store_b16((short)f2bf_hw(x), rsO, off, 0, 0);
                }
                if (has_out8) {
                    const unsigned off = valid ? (unsigned)m * (unsigned)p.ldq + (unsigned)(p.q_coff + col) : CRIS_OOB;
                    __builtin_amdgcn_raw_buffer_store_b8((char)cris_f32_to_e4m3(__builtin_amdgcn_ldexpf(x, -p.e_y)), rsQ, off, 0, 0);
                }
            }
        }
    }
}

enum { V8_128x128 = 0, V8_64x64 = 1, V8_COUNT = 2 };
// the two tile variants, in the order of the enum: 256 threads, a ring of ST stages of (BM + BN) rows of 128 B
struct fp8_variant_desc {
    const char* name;
    int bm, bn, threads, lds_bytes;
    void (*kern)(const cris_conv_gemm_fp8_params);
};
#define CRIS_FP8_ROW(NAME, BM, BN, ST) {NAME, BM, BN, 256, ST * (BM + BN) * 128, conv_gemm_fp8_kernel<BM, BN, 2, 2, ST>}
static const fp8_variant_desc fp8_variants[V8_COUNT] = {CRIS_FP8_ROW("128x128", 128, 128, ST8_128x128), CRIS_FP8_ROW("64x64", 64, 64, ST8_64x64)};

static int fp8_pick_variant(const cris_conv_gemm_fp8_params& p) {
    // as the bf16 plan: narrow problems and grids of too few 128x128 tiles to fill the chip take the 64x64 tile
    if (p.N <= 64) return V8_64x64;
    if (p.M <= 8192 || (long)cris_cdiv(p.M, 128) * cris_cdiv(p.N, 128) < 448) return V8_64x64;
    return V8_128x128;
}

static int conv_gemm_fp8_check(const cris_conv_gemm_fp8_params& p) {
    CRIS_CHECK_ARG(p.A && p.Wt && p.e_w, "null operand");
    CRIS_CHECK_ARG(p.out || p.out8, "no output");
    CRIS_CHECK_ARG(p.M > 0 && p.N > 0 && p.K > 0, "empty problem");
    CRIS_CHECK_ARG((p.C & 15) == 0 && (p.lda & 15) == 0 && (p.a_coff & 15) == 0, "fp8: A channels / ld / offset must be multiples of 16");
    CRIS_CHECK_ARG((p.ldb & 15) == 0 && p.ldb >= p.K, "fp8: W ld must be a multiple of 16 and >= K");
    CRIS_CHECK_ARG(p.K == p.KH * p.KW * p.C, "K != KH*KW*C");
    CRIS_CHECK_ARG(p.M == p.Bn * p.OH * p.OW, "M != Bn*OH*OW");
    CRIS_CHECK_ARG(p.act == 0 || p.act == 1 || p.act == 3, "fp8: act 0, 1 or 3");
    CRIS_CHECK_ARG(p.M < (1 << 24) && (long)cris_cdiv(p.M, 64) * cris_cdiv(p.N, 64) < (1L << 22), "more than 2^24 rows / 2^22 tiles");
    CRIS_CHECK_ARG((uintptr_t)p.A % 16 == 0 && (uintptr_t)p.Wt % 16 == 0, "operands must be 16-byte aligned");
    CRIS_CHECK_ARG(!p.resid || (p.ldr >= p.r_coff + p.N), "residual ld");
    CRIS_CHECK_ARG(!p.out || (p.ldc >= p.c_coff + p.N), "output ld");
    CRIS_CHECK_ARG(!p.out8 || (p.ldq >= p.q_coff + p.N), "fp8 output ld");
    CRIS_CHECK_ARG((size_t)p.Bn * p.H * p.W * p.lda < (1UL << 31) && ((size_t)p.N + 256) * p.ldb < (1UL << 31) &&
                       (!p.out || (size_t)p.M * p.ldc * 2 < (1UL << 31)) && (!p.resid || (size_t)p.M * p.ldr * 2 < (1UL << 31)) &&
                       (!p.out8 || (size_t)p.M * p.ldq < (1UL << 31)),
                   "operand extent must stay below 2 GiB (32-bit buffer offsets)");
    return 0;
}

extern "C" int cris_conv_gemm_fp8_plan(const cris_conv_gemm_fp8_params* p, int variant) {
    if (variant < 0) return fp8_pick_variant(*p);
    return variant < V8_COUNT ? variant : -1;
}
extern "C" int cris_conv_gemm_fp8_num_variants(void) { return V8_COUNT; }
extern "C" const char* cris_conv_gemm_fp8_variant_name(int v) { return (v >= 0 && v < V8_COUNT) ? fp8_variants[v].name : "?"; }

extern "C" int cris_conv_gemm_fp8(const cris_conv_gemm_fp8_params* pp, int variant, void* stream) {
    const cris_conv_gemm_fp8_params& p = *pp;
    if (conv_gemm_fp8_check(p) != 0) return -1;
    const int v = cris_conv_gemm_fp8_plan(pp, variant);
    CRIS_CHECK_ARG(v >= 0, "fp8 tile variant out of range");
    static const int lds_ready = [] {
        int rc = 0;
        for (const fp8_variant_desc& r : fp8_variants) rc |= cris_set_lds((const void*)r.kern, r.lds_bytes);
        return rc;
    }();
    if (lds_ready != 0) {
        cris_set_error("%s: hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed (%d)", __func__, lds_ready);
        return lds_ready;
    }
    const fp8_variant_desc& r = fp8_variants[v];
    return cris_launch_tile(r.kern, cris_tile_blocks(r.bm, r.bn, p.M, p.N), r.threads, r.lds_bytes, (hipStream_t)stream, p);
}

// ------------------------------------------------------------------------------------------------
// weight quantise + pack: one block per output channel of a table of tensors
// ------------------------------------------------------------------------------------------------
// v = src * row_scale[n] (fp32, the folded weight of the bf16 pack), e_w[n] from the row's abs-max (fixed-order LDS tree: no
// atomics), dst[n][tap * Cpad + c] = e4m3(v * 2^-e_w[n]); channels Cin .. Cpad-1 and columns up to ld are written as zeros.
__global__ __launch_bounds__(256) void pack_weights_fp8_kernel(const cris_pack_fp8_desc* __restrict__ tab, int n_desc) {
    __shared__ float red[256];
    int lo = 0, hi = n_desc - 1;
    const int bid = blockIdx.x;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].block_start <= bid) lo = mid; else hi = mid - 1;
    }
    const cris_pack_fp8_desc d = tab[lo];
    const int n = bid - d.block_start;
    const float rs = d.row_scale ? d.row_scale[n] : 1.f;
    const int len = d.taps * d.Cpad;
    const float* src = d.src + (size_t)n * d.Cin * d.taps;          // parameter layout [N][Cin][taps]
    float amax = 0.f;
    for (int i = threadIdx.x; i < d.Cin * d.taps; i += 256) amax = fmaxf(amax, fabsf(src[i] * rs));
    const int e = cris_e4m3_exponent(block_max_256(red, amax));
    if (threadIdx.x == 0) d.e_w[n] = e;
    uint8_t* dst = d.dst + (size_t)n * d.ld;
    for (int i = threadIdx.x; i < d.ld; i += 256) {
        uint32_t q = 0;
        if (i < len) {
            const int tap = i / d.Cpad, c = i - tap * d.Cpad;
            if (c < d.Cin) q = cris_f32_to_e4m3(__builtin_amdgcn_ldexpf(src[(size_t)c * d.taps + tap] * rs, -e));
        }
        dst[i] = (uint8_t)q;
    }
}

extern "C" int cris_pack_weights_fp8(const cris_pack_fp8_desc* dev_table, int n_desc, int total_blocks, void* stream) {
    CRIS_CHECK_ARG(dev_table && n_desc > 0 && total_blocks > 0, "empty table");
    hipLaunchKernelGGL(pack_weights_fp8_kernel, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, dev_table, n_desc);
    CRIS_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// 2x2 / stride 2 average pool of an NHWC bf16 map, fp8 output (and optionally the bf16 one)
// ------------------------------------------------------------------------------------------------
// same arithmetic as avgpool2_fwd_kernel (elementwise.hip): four taps added in (dy, dx) order, * 0.25
__global__ void avgpool2_fp8_kernel(const bf16_t* __restrict__ x, int ldx, int xcoff, int Bn, int H, int W, int C, bf16_t* __restrict__ y,
                                    int ldy, int ycoff, uint8_t* __restrict__ y8, int ldq, int qcoff, int e_y) {
    const int CV = C >> 3, OH = H >> 1, OW = W >> 1;
    const long total = (long)Bn * OH * OW * CV;
    const bool small = total < (1L << 24);
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const cris_idx4 q = cris_split4(idx, CV, OW, OH, small);
        const int cv = q.cv, ow = q.x, oh = q.y, b = q.b;
        const long mo = ((long)b * OH + oh) * OW + ow;
        float o[8] = {0, 0, 0, 0, 0, 0, 0, 0}, t[8];
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                unpack8(*reinterpret_cast<const uint4*>(x + (((size_t)b * H + oh * 2 + dy) * W + ow * 2 + dx) * ldx + xcoff + cv * 8), t);
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] += t[j];
            }
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] *= 0.25f;
        if (y) *reinterpret_cast<uint4*>(y + (size_t)mo * ldy + ycoff + cv * 8) = pack8(o);
        uint2 w;
        w.x = cris_f32_to_e4m3(__builtin_amdgcn_ldexpf(o[0], -e_y)) | (cris_f32_to_e4m3(__builtin_amdgcn_ldexpf(o[1], -e_y)) << 8) |
              (cris_f32_to_e4m3(__builtin_amdgcn_ldexpf(o[2], -e_y)) << 16) | (cris_f32_to_e4m3(__builtin_amdgcn_ldexpf(o[3], -e_y)) << 24);
        w.y = cris_f32_to_e4m3(__builtin_amdgcn_ldexpf(o[4], -e_y)) | (cris_f32_to_e4m3(__builtin_amdgcn_ldexpf(o[5], -e_y)) << 8) |
              (cris_f32_to_e4m3(__builtin_amdgcn_ldexpf(o[6], -e_y)) << 16) | (cris_f32_to_e4m3(__builtin_amdgcn_ldexpf(o[7], -e_y)) << 24);
        *reinterpret_cast<uint2*>(y8 + (size_t)mo * ldq + qcoff + cv * 8) = w;
    }
}

extern "C" int cris_avgpool2_fwd_fp8(const cris_bf16* x, int ldx, int xcoff, int Bn, int H, int W, int C, cris_bf16* y, int ldy, int ycoff,
                                     uint8_t* y8, int ldq, int qcoff, int e_y, void* stream) {
    CRIS_CHECK_ARG(x && y8 && !(H & 1) && !(W & 1) && !(C & 7) && !(ldx & 7) && !(xcoff & 7) && !(ldq & 7) && !(qcoff & 7) &&
                       (!y || (!(ldy & 7) && !(ycoff & 7))),
                   "bad args");
    const long total = (long)Bn * (H / 2) * (W / 2) * (C / 8);
    hipLaunchKernelGGL(avgpool2_fp8_kernel, dim3(cris_grid_1d(total, 256)), dim3(256), 0, (hipStream_t)stream, x, ldx, xcoff, Bn, H, W, C, y,
                       ldy, ycoff, y8, ldq, qcoff, e_y);
    CRIS_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// abs-max of an NHWC bf16 tensor (calibration): per-block maxima, then one block over them; no atomics
// ------------------------------------------------------------------------------------------------
#define ABSMAX_BLOCKS 1024

__global__ __launch_bounds__(256) void absmax_partial_kernel(const bf16_t* __restrict__ x, int ldx, int xcoff, long rows, int C,
                                                             float* __restrict__ part) {
    __shared__ float red[256];
    const int CV = C >> 3;
    const long total = rows * CV;
    float m = 0.f;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long r = idx / CV;
        const int cv = (int)(idx - r * CV);
        float t[8];
        unpack8(*reinterpret_cast<const uint4*>(x + (size_t)r * ldx + xcoff + cv * 8), t);
#pragma unroll
        for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf(t[j]));
    }
    m = block_max_256(red, m);
    if (threadIdx.x == 0) part[blockIdx.x] = m;
}

__global__ __launch_bounds__(256) void absmax_final_kernel(const float* __restrict__ part, int n, float* __restrict__ out) {
    __shared__ float red[256];
    float m = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) m = fmaxf(m, part[i]);
    m = block_max_256(red, m);
    if (threadIdx.x == 0) out[0] = m;
}

extern "C" int cris_absmax_ws_floats(void) { return ABSMAX_BLOCKS; }

extern "C" int cris_absmax_bf16(const cris_bf16* x, int ldx, int xcoff, long rows, int C, float* ws, float* out, void* stream) {
    CRIS_CHECK_ARG(x && ws && out && rows > 0 && C > 0 && !(C & 7) && !(ldx & 7) && !(xcoff & 7), "bad args");
    const int nb = (int)std::min<long>(ABSMAX_BLOCKS, (rows * (C / 8) + 255) / 256);
    hipLaunchKernelGGL(absmax_partial_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, x, ldx, xcoff, rows, C, ws);
    hipLaunchKernelGGL(absmax_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, ws, nb, out);
    CRIS_LAUNCH_CHECK();
    return 0;
}
