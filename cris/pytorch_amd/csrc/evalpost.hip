// Evaluation post-processing on the GPU (reference engine/engine.py:100-123 `validate`, :171-188 `inference`): sigmoid +
// bicubic (align_corners) upsample of the logits to the network input size, inverse affine warp to the original image size
// with OpenCV's INTER_CUBIC arithmetic, threshold and intersection / union counts.  The reference does steps 3-4 per sample
// on the CPU (cv2 + numpy after a device-to-host copy); here the prediction never leaves HBM.  HBM-bound elementwise kernels;
// the arithmetic order follows torch's upsample_bicubic2d and cv::warpAffine so that results can be compared value by value
// (oracle/eval_post.py; the cv2 step is restated from the published algorithm - cv2 is not available here).
#include "common.h"
#include "../../../include/cris_hip.h"

// No fused multiply-adds in this file: the kernels restate torch / OpenCV float arithmetic operation by operation, and hipcc
// contracts a*b+c by default (HIP's __fmul_rn / __fadd_rn are plain operators defined in a header OUTSIDE this pragma: their
// results still get fused; the ep_* helpers below are inside it).
#pragma clang fp contract(off)
__device__ __forceinline__ float ep_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float ep_add(float a, float b) { return a + b; }
__device__ __forceinline__ double ep_dmul(double a, double b) { return a * b; }
__device__ __forceinline__ double ep_dadd(double a, double b) { return a + b; }

__device__ __forceinline__ float ep_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// torch upsample_bicubic2d (A = -0.75): weights of taps -1, 0, +1, +2 for the fractional offset t
__device__ __forceinline__ void ep_cubic_torch(float t, float* c) {
    const float A = -0.75f;
    const float x0 = t + 1.0f, x1 = t, x2 = 1.0f - t, x3 = 2.0f - t;
    c[0] = ((A * x0 - 5.0f * A) * x0 + 8.0f * A) * x0 - 4.0f * A;
    c[1] = ((A + 2.0f) * x1 - (A + 3.0f)) * x1 * x1 + 1.0f;
    c[2] = ((A + 2.0f) * x2 - (A + 3.0f)) * x2 * x2 + 1.0f;
    c[3] = ((A * x3 - 5.0f * A) * x3 + 8.0f * A) * x3 - 4.0f * A;
}

// out[b][Y][X] = bicubic(sigmoid(logits[b]))(Y, X), align_corners = True, border indices clamped
__global__ __launch_bounds__(256) void sigmoid_bicubic_kernel(const float* __restrict__ logits, int Bn, int h, int w, int H, int W,
                                                              float sy_scale, float sx_scale, float* __restrict__ out) {
    const long total = (long)Bn * H * W;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int X = (int)(idx % W);
        const int Y = (int)((idx / W) % H);
        const int b = (int)(idx / ((long)W * H));
        const float fy = (float)Y * sy_scale, fx = (float)X * sx_scale;
        const int iy = (int)floorf(fy), ix = (int)floorf(fx);
        float cy[4], cx[4];
        ep_cubic_torch(fy - (float)iy, cy);
        ep_cubic_torch(fx - (float)ix, cx);
        const float* src = logits + (size_t)b * h * w;
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int yy = min(max(iy - 1 + i, 0), h - 1);
            float r = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int xx = min(max(ix - 1 + j, 0), w - 1);
                const float t = ep_mul(ep_sigmoid(src[yy * w + xx]), cx[j]);
                r = j == 0 ? t : ep_add(r, t);
            }
            const float t = ep_mul(r, cy[i]);
            acc = i == 0 ? t : ep_add(acc, t);
        }
        out[idx] = acc;
    }
}

extern "C" int cris_sigmoid_bicubic_up(const float* logits, int Bn, int h, int w, int H, int W, float* out, void* stream) {
    CRIS_CHECK_ARG(logits && out && Bn > 0 && h > 0 && w > 0 && H > 0 && W > 0, "bad args");
    const float sy = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f, sx = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f;
    hipLaunchKernelGGL(sigmoid_bicubic_kernel, dim3(cris_grid_1d((long)Bn * H * W, 256)), dim3(256), 0, (hipStream_t)stream, logits, Bn,
                       h, w, H, W, sy, sx, out);
    CRIS_LAUNCH_CHECK();
    return 0;
}

// ---- cv::warpAffine, INTER_CUBIC, BORDER_CONSTANT (imgwarp.cpp): fixed-point source coordinates (AB_BITS = 10) quantised to
// 1/32 pixel (INTER_BITS = 5), 4 x 4 weights = products of two entries of a 32 x 4 float table (A = -0.75) ----
#define EP_AB_BITS 10
#define EP_INTER_BITS 5
struct ep_warp_args {
    double m[6];                  // destination -> source map (the inverse of the matrix the caller passes, in double)
    float tab[32][4];             // cv::interpolateCubic coefficients of the 32 sub-pixel positions, built on the host
};

__global__ __launch_bounds__(256) void warp_affine_cubic_kernel(const float* __restrict__ src, int H, int W, const ep_warp_args a,
                                                                int w_out, int h_out, float border, float* __restrict__ dst) {
    const long total = (long)w_out * h_out;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int x = (int)(idx % w_out), y = (int)(idx / w_out);
        const double AB = (double)(1 << EP_AB_BITS);
        const int round_delta = (1 << EP_AB_BITS) / (1 << EP_INTER_BITS) / 2;
        // (explicit _rn operations: no fused multiply-add, so that the fixed-point coordinates equal a host evaluation bit for bit)
        const long adelta = (long)rint(ep_dmul(ep_dmul(a.m[0], (double)x), AB)), bdelta = (long)rint(ep_dmul(ep_dmul(a.m[3], (double)x), AB));
        const long X0 = (long)rint(ep_dmul(ep_dadd(ep_dmul(a.m[1], (double)y), a.m[2]), AB)) + round_delta;
        const long Y0 = (long)rint(ep_dmul(ep_dadd(ep_dmul(a.m[4], (double)y), a.m[5]), AB)) + round_delta;
        const long Xq = (X0 + adelta) >> (EP_AB_BITS - EP_INTER_BITS), Yq = (Y0 + bdelta) >> (EP_AB_BITS - EP_INTER_BITS);
        const int sx = (int)(Xq >> EP_INTER_BITS) - 1, sy = (int)(Yq >> EP_INTER_BITS) - 1;
        const int fx = (int)(Xq & 31), fy = (int)(Yq & 31);
        float acc = 0.f;
#pragma unroll
        for (int ky = 0; ky < 4; ++ky) {
            const int yy = sy + ky;
#pragma unroll
            for (int kx = 0; kx < 4; ++kx) {
                const int xx = sx + kx;
                const bool inside = yy >= 0 && yy < H && xx >= 0 && xx < W;
                const float v = inside ? src[(size_t)min(max(yy, 0), H - 1) * W + min(max(xx, 0), W - 1)] : border;
                const float wgt = ep_mul(a.tab[fy][ky], a.tab[fx][kx]);
                acc = ep_add(acc, ep_mul(v, wgt));
            }
        }
        dst[idx] = acc;
    }
}

// Host side of both warp launchers: cv::invertAffineTransform in double (the caller passes the matrix cv2.warpAffine is given,
// without WARP_INVERSE_MAP) into m (skipped when mat is NULL: the batched launcher's descriptors hold inverted matrices already,
// made by cris_eval_desc_fill through this same function), and the 32 x 4 table of cv::interpolateCubic.
static void ep_warp_setup(const double* mat, double* m, float (*tab)[4]) {
    if (mat) {
        double D = mat[0] * mat[4] - mat[1] * mat[3];
        D = D != 0.0 ? 1.0 / D : 0.0;
        const double A11 = mat[4] * D, A22 = mat[0] * D, A12 = -mat[1] * D, A21 = -mat[3] * D;
        m[0] = A11; m[1] = A12; m[2] = -A11 * mat[2] - A12 * mat[5];
        m[3] = A21; m[4] = A22; m[5] = -A21 * mat[2] - A22 * mat[5];
    }
    if (!tab) return;
    const volatile float A = -0.75f;                            // (volatile: keep the float operations separate, no contraction)
    for (int i = 0; i < 32; ++i) {
        const volatile float t = (float)i / 32.0f;
        volatile float u = t + 1.0f, c0, c1, c2, q;
        q = A * u; q = q - 5.0f * A; q = q * u; q = q + 8.0f * A; q = q * u; c0 = q - 4.0f * A;
        q = (A + 2.0f) * t; q = q - (A + 3.0f); q = q * t; q = q * t; c1 = q + 1.0f;
        u = 1.0f - t;
        q = (A + 2.0f) * u; q = q - (A + 3.0f); q = q * u; q = q * u; c2 = q + 1.0f;
        q = 1.0f - c0; q = q - c1; q = q - c2;
        tab[i][0] = c0; tab[i][1] = c1; tab[i][2] = c2; tab[i][3] = q;
    }
}

extern "C" int cris_warp_affine_cubic(const float* src, int H, int W, const double* mat, int w_out, int h_out, float border, float* dst,
                                      void* stream) {
    CRIS_CHECK_ARG(src && mat && dst && H > 0 && W > 0 && w_out > 0 && h_out > 0, "bad args");
    ep_warp_args a;
    ep_warp_setup(mat, a.m, a.tab);
    hipLaunchKernelGGL(warp_affine_cubic_kernel, dim3(cris_grid_1d((long)w_out * h_out, 256)), dim3(256), 0, (hipStream_t)stream, src, H, W,
                       a, w_out, h_out, border, dst);
    CRIS_LAUNCH_CHECK();
    return 0;
}

// counts[0] += #(pred > thr and mask != 0), counts[1] += #(pred > thr or mask != 0): integer atomics (exact, order-free)
__global__ __launch_bounds__(256) void threshold_iou_kernel(const float* __restrict__ pred, const float* __restrict__ mask, long n, float thr,
                                                            int* __restrict__ counts) {
    int inter = 0, uni = 0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const bool p = pred[i] > thr, m = mask[i] != 0.f;
        inter += (p && m) ? 1 : 0;
        uni += (p || m) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        inter += __shfl_xor(inter, o, 64);
        uni += __shfl_xor(uni, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(counts, inter);
        atomicAdd(counts + 1, uni);
    }
}

extern "C" int cris_threshold_iou(const float* pred, const float* mask, long n, float thr, int* counts, void* stream) {
    CRIS_CHECK_ARG(pred && mask && counts && n > 0, "bad args");
    hipLaunchKernelGGL(threshold_iou_kernel, dim3(cris_grid_1d(n, 256, 512)), dim3(256), 0, (hipStream_t)stream, pred, mask, n, thr, counts);
    CRIS_LAUNCH_CHECK();
    return 0;
}

// ---- one launch per batch: warp + threshold + counts for n ragged samples (engine.py:108-124 / :166-190 as one kernel) ----
// blockIdx.y = descriptor, blockIdx.x strides over that sample's groups of 4 consecutive x positions (one mask dword each).
// The per-pixel value is warp_affine_cubic_kernel's, operation for operation (same fixed-point coordinates, same 16-tap
// accumulation order); it is compared with thr in a register and never stored.  Integer sums: wave shuffle, then the 4 waves of
// the block through LDS, then one atomicAdd pair per block (exact, order-free).
struct ep_cubic_tab {
    float tab[32][4];
};

// The arithmetic both batch kernels share, written once.  ep_warp_row: the fixed-point source coordinates of destination row y
// (cv::warpAffine's X0 / Y0); ep_warp_value: the value of destination pixel x of that row - warp_affine_cubic_kernel's, operation
// for operation.  `tab` is the block's LDS copy of the 32 x 4 coefficient table.  Both live inside this file's no-contraction
// region and are inlined: eval_iou_batch_kernel compiles to the instructions it had with the code written out in place (only the
// operand order of some commutative multiplies differs: DESIGN.md 9b).
__device__ __forceinline__ void ep_warp_row(const double* m, int y, long& X0, long& Y0) {
    const double AB = (double)(1 << EP_AB_BITS);
    const int round_delta = (1 << EP_AB_BITS) / (1 << EP_INTER_BITS) / 2;
    X0 = (long)rint(ep_dmul(ep_dadd(ep_dmul(m[1], (double)y), m[2]), AB)) + round_delta;
    Y0 = (long)rint(ep_dmul(ep_dadd(ep_dmul(m[4], (double)y), m[5]), AB)) + round_delta;
}

__device__ __forceinline__ float ep_warp_value(const float* __restrict__ src, int H, int W, const float (*tab)[4], const double* m, long X0,
                                               long Y0, int x, float border) {
    const double AB = (double)(1 << EP_AB_BITS);
    const long adelta = (long)rint(ep_dmul(ep_dmul(m[0], (double)x), AB)), bdelta = (long)rint(ep_dmul(ep_dmul(m[3], (double)x), AB));
    const long Xq = (X0 + adelta) >> (EP_AB_BITS - EP_INTER_BITS), Yq = (Y0 + bdelta) >> (EP_AB_BITS - EP_INTER_BITS);
    const int sx = (int)(Xq >> EP_INTER_BITS) - 1, sy = (int)(Yq >> EP_INTER_BITS) - 1;
    const int fx = (int)(Xq & 31), fy = (int)(Yq & 31);
    float acc = 0.f;
#pragma unroll
    for (int ky = 0; ky < 4; ++ky) {
        const int yy = sy + ky;
#pragma unroll
        for (int kx = 0; kx < 4; ++kx) {
            const int xx = sx + kx;
            const bool inside = yy >= 0 && yy < H && xx >= 0 && xx < W;
            const float v = inside ? src[(size_t)min(max(yy, 0), H - 1) * W + min(max(xx, 0), W - 1)] : border;
            const float wgt = ep_mul(tab[fy][ky], tab[fx][kx]);
            acc = ep_add(acc, ep_mul(v, wgt));
        }
    }
    return acc;
}

__global__ __launch_bounds__(256) void eval_iou_batch_kernel(const float* __restrict__ probs, int H, int W,
                                                             const cris_eval_desc* __restrict__ descs,
                                                             const unsigned char* __restrict__ masks, const ep_cubic_tab t, float thr,
                                                             float border, int* __restrict__ counts, unsigned char* __restrict__ out) {
    __shared__ float tab[32][4];
    __shared__ int red[2][4];
    if (threadIdx.x < 128) tab[threadIdx.x >> 2][threadIdx.x & 3] = t.tab[threadIdx.x >> 2][threadIdx.x & 3];
    __syncthreads();
    const cris_eval_desc d = descs[blockIdx.y];
    const float* __restrict__ src = probs + (size_t)d.map * H * W;
    const unsigned char* __restrict__ mrow = masks + d.mask_off;
    const int gpr = d.pitch >> 2;                                  // groups per row (the pitch is a multiple of 4)
    const long total = (long)gpr * d.h_out;
    int inter = 0, uni = 0;
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long)gridDim.x * blockDim.x) {
        const int y = (int)(g / gpr), x0 = (int)(g % gpr) * 4;
        const size_t boff = (size_t)y * d.pitch + x0;
        const unsigned int mword = *reinterpret_cast<const unsigned int*>(mrow + boff);
        long X0, Y0;
        ep_warp_row(d.m, y, X0, Y0);
        unsigned int oword = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = x0 + j;
            if (x < d.w_out) {                                     // (lanes past w_out: padding bytes, not counted)
                const float acc = ep_warp_value(src, H, W, tab, d.m, X0, Y0, x, border);
                const bool p = acc > thr, m = ((mword >> (8 * j)) & 0xffu) != 0u;
                inter += (p && m) ? 1 : 0;
                uni += (p || m) ? 1 : 0;
                oword |= p ? (0xffu << (8 * j)) : 0u;
            }
        }
        if (out) *reinterpret_cast<unsigned int*>(out + d.out_off + boff) = oword;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        inter += __shfl_xor(inter, o, 64);
        uni += __shfl_xor(uni, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = inter;
        red[1][threadIdx.x >> 6] = uni;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(counts + 2 * (size_t)d.row, red[0][0] + red[0][1] + red[0][2] + red[0][3]);
        atomicAdd(counts + 2 * (size_t)d.row + 1, red[1][0] + red[1][1] + red[1][2] + red[1][3]);
    }
}

// ---- prediction without ground truth: warp + threshold + (area, score, bounding box) for n ragged descriptors in one launch ----
// The grid, the 4-pixel groups, the per-pixel value and the mask bytes are eval_iou_batch_kernel's; no mask is read.  Over the
// pixels with value > thr, row d.row of the table stats [rows][6] of unsigned 64-bit words receives
//     [0] += 1    [1] += (long long)rintf(value * 65536.f)    [2] min= x    [3] min= y    [4] max= x + 1    [5] max= y + 1
// (65536 is a power of two: the product is exact, rintf rounds half to even; value > thr >= 0, so every term is positive and the
// unsigned atomics are the signed ones).  Integer add / min / max are exact and order-free: wave shuffle, the block's 4 waves
// through LDS, then one set of six 64-bit atomics per block that found a pixel - every run gives the same table.
__global__ __launch_bounds__(256) void predict_masks_batch_kernel(const float* __restrict__ probs, int H, int W,
                                                                  const cris_eval_desc* __restrict__ descs, const ep_cubic_tab t, float thr,
                                                                  float border, unsigned long long* __restrict__ stats,
                                                                  unsigned char* __restrict__ out) {
    __shared__ float tab[32][4];
    __shared__ unsigned long long red_score[4];
    __shared__ int red[5][4];
    if (threadIdx.x < 128) tab[threadIdx.x >> 2][threadIdx.x & 3] = t.tab[threadIdx.x >> 2][threadIdx.x & 3];
    __syncthreads();
    const cris_eval_desc d = descs[blockIdx.y];
    const float* __restrict__ src = probs + (size_t)d.map * H * W;
    const int gpr = d.pitch >> 2;                                  // groups per row (the pitch is a multiple of 4)
    const long total = (long)gpr * d.h_out;
    int area = 0, x_min = 0x7fffffff, y_min = 0x7fffffff, x_end = 0, y_end = 0;     // (w_out * h_out < 2^31: a launch's area fits)
    unsigned long long score = 0;
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long)gridDim.x * blockDim.x) {
        const int y = (int)(g / gpr), x0 = (int)(g % gpr) * 4;
        long X0, Y0;
        ep_warp_row(d.m, y, X0, Y0);
        unsigned int oword = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = x0 + j;
            if (x < d.w_out) {                                     // (lanes past w_out: padding bytes, not counted)
                const float acc = ep_warp_value(src, H, W, tab, d.m, X0, Y0, x, border);
                if (acc > thr) {
                    area += 1;
                    score += (unsigned long long)(long long)rintf(ep_mul(acc, 65536.f));
                    x_min = min(x_min, x); x_end = max(x_end, x + 1);
                    y_min = min(y_min, y); y_end = max(y_end, y + 1);
                    oword |= 0xffu << (8 * j);
                }
            }
        }
        if (out) *reinterpret_cast<unsigned int*>(out + d.out_off + (size_t)y * d.pitch + x0) = oword;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        area += __shfl_xor(area, o, 64);
        score += __shfl_xor(score, o, 64);
        x_min = min(x_min, __shfl_xor(x_min, o, 64)); y_min = min(y_min, __shfl_xor(y_min, o, 64));
        x_end = max(x_end, __shfl_xor(x_end, o, 64)); y_end = max(y_end, __shfl_xor(y_end, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        red_score[w] = score;
        red[0][w] = area; red[1][w] = x_min; red[2][w] = y_min; red[3][w] = x_end; red[4][w] = y_end;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int a = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        if (a > 0) {                                               // (a block without a pixel would add 0 and min / max nothing)
            unsigned long long* row = stats + 6 * (size_t)d.row;
            atomicAdd(row, (unsigned long long)a);
            atomicAdd(row + 1, red_score[0] + red_score[1] + red_score[2] + red_score[3]);
            atomicMin(row + 2, (unsigned long long)min(min(red[1][0], red[1][1]), min(red[1][2], red[1][3])));
            atomicMin(row + 3, (unsigned long long)min(min(red[2][0], red[2][1]), min(red[2][2], red[2][3])));
            atomicMax(row + 4, (unsigned long long)max(max(red[3][0], red[3][1]), max(red[3][2], red[3][3])));
            atomicMax(row + 5, (unsigned long long)max(max(red[4][0], red[4][1]), max(red[4][2], red[4][3])));
        }
    }
}

// ---- threshold sweep: warp + classification against T ascending thresholds + counts for n ragged descriptors in one launch ----
// The grid, the 4-pixel groups, the mask dword and the per-pixel value are eval_iou_batch_kernel's.  Per pixel
// k = #{i : value > thr[i]} (comparisons of exactly that form: a bracket test against thr[0] and thr[T-1], a binary search
// between them; a NaN gives 0) and m = (mask byte != 0).  Column i of the table needs  pred_i = #(k > i),  inter_i = #(k > i, m)
// and gt = #(m):  union_i = pred_i + gt - inter_i.  The bins with k = 0 enter no pred_i or inter_i, so they are never counted;
// gt and the two k = T bins (confident foreground - with k = 0 the bulk of a bimodal map) stay in registers and go through the
// wave shuffle; only 0 < k < T (pixels between the lowest and the highest threshold: the rim of a segment) go to the wave's LDS
// histogram hist[wave][m][k - 1], equal keys of a thread's four pixels merged into one ds_add.  Block end: the four waves'
// histograms are summed, thread i < T takes the suffix sums over k, one integer atomicAdd pair per (block, i) with a non-zero
// term (exact, order-free: every run gives the same table).
#define EP_SWEEP_MAX 64
struct ep_thr_tab {
    float v[EP_SWEEP_MAX];
};

__global__ __launch_bounds__(256) void eval_iou_sweep_batch_kernel(const float* __restrict__ probs, int H, int W,
                                                                   const cris_eval_desc* __restrict__ descs,
                                                                   const unsigned char* __restrict__ masks, const ep_cubic_tab t,
                                                                   const ep_thr_tab th, int T, float border, int* __restrict__ counts) {
    __shared__ float tab[32][4];
    __shared__ float thr[EP_SWEEP_MAX];
    __shared__ int hist[4][2][EP_SWEEP_MAX];                        // [wave][mask bit][k - 1], 0 < k < T
    __shared__ int red[3][4];
    if (threadIdx.x < 128) tab[threadIdx.x >> 2][threadIdx.x & 3] = t.tab[threadIdx.x >> 2][threadIdx.x & 3];
    if (threadIdx.x < EP_SWEEP_MAX) thr[threadIdx.x] = th.v[threadIdx.x];
    for (int i = threadIdx.x; i < 4 * 2 * EP_SWEEP_MAX; i += blockDim.x) (&hist[0][0][0])[i] = 0;
    __syncthreads();
    const cris_eval_desc d = descs[blockIdx.y];
    const float* __restrict__ src = probs + (size_t)d.map * H * W;
    const unsigned char* __restrict__ mrow = masks + d.mask_off;
    const int gpr = d.pitch >> 2;                                  // groups per row (the pitch is a multiple of 4)
    const long total = (long)gpr * d.h_out;
    const float thr_lo = thr[0], thr_hi = thr[T - 1];
    int (*const my)[EP_SWEEP_MAX] = hist[threadIdx.x >> 6];
    int gt = 0, top = 0, top_m = 0;                                // #(m), #(k == T), #(k == T, m)
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long)gridDim.x * blockDim.x) {
        const int y = (int)(g / gpr), x0 = (int)(g % gpr) * 4;
        const size_t boff = (size_t)y * d.pitch + x0;
        const unsigned int mword = *reinterpret_cast<const unsigned int*>(mrow + boff);
        long X0, Y0;
        ep_warp_row(d.m, y, X0, Y0);
        int run_key = -1, run = 0;                                 // the pending LDS add: key = m * EP_SWEEP_MAX + k - 1
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = x0 + j;
            if (x < d.w_out) {                                     // (lanes past w_out: padding bytes, not counted)
                const float acc = ep_warp_value(src, H, W, tab, d.m, X0, Y0, x, border);
                const int m = ((mword >> (8 * j)) & 0xffu) != 0u ? 1 : 0;
                gt += m;
                if (acc > thr_lo) {                                // (false for a NaN: k = 0)
                    if (acc > thr_hi) {
                        top += 1;
                        top_m += m;
                    } else {                                       // 1 <= k <= T - 1: the first i with !(acc > thr[i])
                        int lo = 1, hi = T - 1;
                        while (lo < hi) {
                            const int mid = (lo + hi) >> 1;
                            if (acc > thr[mid]) lo = mid + 1; else hi = mid;
                        }
                        const int key = m * EP_SWEEP_MAX + lo - 1;
                        if (key == run_key) {
                            run += 1;
                        } else {
                            if (run) atomicAdd(&my[0][0] + run_key, run);
                            run_key = key;
                            run = 1;
                        }
                    }
                }
            }
        }
        if (run) atomicAdd(&my[0][0] + run_key, run);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        gt += __shfl_xor(gt, o, 64);
        top += __shfl_xor(top, o, 64);
        top_m += __shfl_xor(top_m, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = gt;
        red[1][threadIdx.x >> 6] = top;
        red[2][threadIdx.x >> 6] = top_m;
    }
    __syncthreads();
    if (threadIdx.x < 2 * EP_SWEEP_MAX) {                          // the four waves' histograms into wave 0's
        const int b = threadIdx.x >> 6, k = threadIdx.x & 63;
        hist[0][b][k] = hist[0][b][k] + hist[1][b][k] + hist[2][b][k] + hist[3][b][k];
    }
    __syncthreads();
    if (threadIdx.x < T) {
        const int i = threadIdx.x;
        const int gts = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        int pred = red[1][0] + red[1][1] + red[1][2] + red[1][3];  // k == T
        int inter = red[2][0] + red[2][1] + red[2][2] + red[2][3];
        for (int k = i + 1; k < T; ++k) {                          // k > i, k < T
            inter += hist[0][1][k - 1];
            pred += hist[0][0][k - 1] + hist[0][1][k - 1];
        }
        int* row = counts + ((size_t)d.row * T + i) * 2;
        const int uni = pred + gts - inter;
        if (inter) atomicAdd(row, inter);
        if (uni) atomicAdd(row + 1, uni);
    }
}

extern "C" int cris_eval_desc_fill(cris_eval_desc* desc, const double* mat, int w_out, int h_out, int map, long mask_off, int pitch,
                                   long out_off, int row) {
    CRIS_CHECK_ARG(desc && mat, "bad args");
    ep_warp_setup(mat, desc->m, nullptr);
    desc->w_out = w_out; desc->h_out = h_out; desc->map = map; desc->row = row;
    desc->mask_off = mask_off; desc->out_off = out_off; desc->pitch = pitch; desc->pad_ = 0;
    return 0;
}

extern "C" int cris_eval_iou_batch(const float* probs, int P, int H, int W, const cris_eval_desc* descs_host,
                                   const cris_eval_desc* descs_dev, int n, const unsigned char* masks, size_t mask_bytes, float thr,
                                   float border, int* counts, int count_rows, unsigned char* out_masks, size_t out_bytes, void* stream) {
    CRIS_CHECK_ARG(probs && descs_host && descs_dev && masks && counts, "null operand");
    CRIS_CHECK_ARG(P > 0 && H > 0 && W > 0 && n > 0 && n <= 65535 && count_rows > 0, "bad sizes");
    CRIS_CHECK_ARG(((uintptr_t)masks & 3) == 0 && ((uintptr_t)out_masks & 3) == 0, "mask buffers must be 4-byte aligned");
    long most = 0;
    for (int i = 0; i < n; ++i) {                                  // every address the kernel forms is checked here, on the host copy
        const cris_eval_desc& d = descs_host[i];
        CRIS_CHECK_ARG(d.w_out > 0 && d.h_out > 0 && (long)d.w_out * d.h_out < (1L << 31), "descriptor: bad output size");
        CRIS_CHECK_ARG(d.map >= 0 && d.map < P && d.row >= 0 && d.row < count_rows, "descriptor: map / row out of range");
        CRIS_CHECK_ARG(d.pitch >= d.w_out && (d.pitch & 3) == 0 && d.pitch - d.w_out < (1 << 20), "descriptor: the pitch must be a multiple of 4, >= w_out");
        const size_t bytes = (size_t)d.pitch * d.h_out;
        CRIS_CHECK_ARG(d.mask_off >= 0 && (d.mask_off & 3) == 0 && (size_t)d.mask_off + bytes <= mask_bytes, "descriptor: mask outside the buffer");
        if (out_masks)
            CRIS_CHECK_ARG(d.out_off >= 0 && (d.out_off & 3) == 0 && (size_t)d.out_off + bytes <= out_bytes, "descriptor: output outside the buffer");
        const long groups = (long)(d.pitch >> 2) * d.h_out;
        if (groups > most) most = groups;
    }
    ep_cubic_tab t;
    ep_warp_setup(nullptr, nullptr, t.tab);
    const int cap = 2048 / n > 8 ? 2048 / n : 8;                   // ~2048 blocks in all, grid-stride for the rest
    hipLaunchKernelGGL(eval_iou_batch_kernel, dim3(cris_grid_1d(most, 256, cap), n), dim3(256), 0, (hipStream_t)stream, probs, H, W,
                       descs_dev, masks, t, thr, border, counts, out_masks);
    CRIS_LAUNCH_CHECK();
    return 0;
}

extern "C" int cris_eval_iou_sweep_batch(const float* probs, int P, int H, int W, const cris_eval_desc* descs_host,
                                         const cris_eval_desc* descs_dev, int n, const unsigned char* masks, size_t mask_bytes,
                                         const float* thresholds, int T, float border, int* counts, int count_rows, void* stream) {
    CRIS_CHECK_ARG(probs && descs_host && descs_dev && masks && thresholds && counts, "null operand");
    CRIS_CHECK_ARG(P > 0 && H > 0 && W > 0 && count_rows > 0, "bad sizes");
    CRIS_CHECK_ARG(n > 0 && n <= 65535, "n must be in 1 .. 65535");
    CRIS_CHECK_ARG(T >= 1 && T <= EP_SWEEP_MAX, "T must be in 1 .. 64");
    ep_thr_tab th;
    for (int i = 0; i < EP_SWEEP_MAX; ++i) {
        th.v[i] = i < T ? thresholds[i] : thresholds[T - 1];       // (the kernel reads the first T)
        if (i >= T) continue;
        CRIS_CHECK_ARG(th.v[i] >= -3.0e38f && th.v[i] <= 3.0e38f, "thresholds must be finite");       // (false for a NaN)
        CRIS_CHECK_ARG(i == 0 || th.v[i] > th.v[i - 1], "thresholds must be strictly increasing");
    }
    CRIS_CHECK_ARG(((uintptr_t)masks & 3) == 0 && ((uintptr_t)counts & 3) == 0, "masks and counts must be 4-byte aligned");
    long most = 0;
    for (int i = 0; i < n; ++i) {                                  // every address the kernel forms is checked here, on the host copy
        const cris_eval_desc& d = descs_host[i];
        CRIS_CHECK_ARG(d.w_out > 0 && d.h_out > 0 && (long)d.w_out * d.h_out < (1L << 31), "descriptor: bad output size");
        CRIS_CHECK_ARG(d.map >= 0 && d.map < P && d.row >= 0 && d.row < count_rows, "descriptor: map / row out of range");
        CRIS_CHECK_ARG(d.pitch >= d.w_out && (d.pitch & 3) == 0 && d.pitch - d.w_out < (1 << 20), "descriptor: the pitch must be a multiple of 4, >= w_out");
        CRIS_CHECK_ARG(d.mask_off >= 0 && (d.mask_off & 3) == 0 && (size_t)d.mask_off + (size_t)d.pitch * d.h_out <= mask_bytes,
                       "descriptor: mask outside the buffer");
        const long groups = (long)(d.pitch >> 2) * d.h_out;
        if (groups > most) most = groups;
    }
    ep_cubic_tab t;
    ep_warp_setup(nullptr, nullptr, t.tab);
    const int cap = 2048 / n > 8 ? 2048 / n : 8;                   // the grid of cris_eval_iou_batch
    hipLaunchKernelGGL(eval_iou_sweep_batch_kernel, dim3(cris_grid_1d(most, 256, cap), n), dim3(256), 0, (hipStream_t)stream, probs, H, W,
                       descs_dev, masks, t, th, T, border, counts);
    CRIS_LAUNCH_CHECK();
    return 0;
}

extern "C" int cris_predict_masks_batch(const float* probs, int P, int H, int W, const cris_eval_desc* descs_host,
                                        const cris_eval_desc* descs_dev, int n, float thr, float border, long long* stats, int stat_rows,
                                        unsigned char* out_masks, size_t out_bytes, void* stream) {
    CRIS_CHECK_ARG(probs && descs_host && descs_dev && stats, "null operand");
    CRIS_CHECK_ARG(P > 0 && H > 0 && W > 0 && stat_rows > 0, "bad sizes");
    CRIS_CHECK_ARG(n > 0 && n <= 65535, "n must be in 1 .. 65535");
    CRIS_CHECK_ARG(thr >= 0.f && thr <= 3.0e38f, "thr must be finite and >= 0 (counted values are positive)");      // (false for a NaN)
    CRIS_CHECK_ARG(border >= -3.0e38f && border <= 3.0e38f, "border must be finite");
    CRIS_CHECK_ARG(((uintptr_t)stats & 7) == 0 && ((uintptr_t)out_masks & 3) == 0, "stats must be 8-byte, out_masks 4-byte aligned");
    long most = 0;
    for (int i = 0; i < n; ++i) {                                  // every address the kernel forms is checked here, on the host copy
        const cris_eval_desc& d = descs_host[i];
        CRIS_CHECK_ARG(d.w_out > 0 && d.h_out > 0 && (long)d.w_out * d.h_out < (1L << 31), "descriptor: bad output size");
        CRIS_CHECK_ARG(d.map >= 0 && d.map < P, "descriptor: map out of range");
        CRIS_CHECK_ARG(d.row >= 0 && d.row < stat_rows, "descriptor: row out of range");
        CRIS_CHECK_ARG(d.pitch >= d.w_out && (d.pitch & 3) == 0 && d.pitch - d.w_out < (1 << 20), "descriptor: the pitch must be a multiple of 4, >= w_out");
        if (out_masks)
            CRIS_CHECK_ARG(d.out_off >= 0 && (d.out_off & 3) == 0 && (size_t)d.out_off + (size_t)d.pitch * d.h_out <= out_bytes,
                           "descriptor: output outside the buffer");
        const long groups = (long)(d.pitch >> 2) * d.h_out;
        if (groups > most) most = groups;
    }
    ep_cubic_tab t;
    ep_warp_setup(nullptr, nullptr, t.tab);
    const int cap = 2048 / n > 8 ? 2048 / n : 8;                   // the grid of cris_eval_iou_batch
    hipLaunchKernelGGL(predict_masks_batch_kernel, dim3(cris_grid_1d(most, 256, cap), n), dim3(256), 0, (hipStream_t)stream, probs, H, W,
                       descs_dev, t, thr, border, reinterpret_cast<unsigned long long*>(stats), out_masks);
    CRIS_LAUNCH_CHECK();
    return 0;
}

// ---- connected components of the packed masks: keep the largest / drop the small ones ----
// The masks are the bytes cris_predict_masks_batch / cris_eval_iou_batch write (descriptor i at out_off, rows of `pitch` bytes).  A
// pixel is foreground iff its byte is != 0 and x < w_out; the pitch padding is background and never a neighbour.  The canonical label
// of a component is the index y * pitch + x (relative to out_off) of its first pixel in raster order; background and padding are -1.
// Union-find with min-index roots over the label words: label[i] <= i always, a root has label[i] == i.  A fixed sequence of launches,
// nothing iterates through the host and no block waits for another:
//   cris_label_components   1 cc_tile_label      32 x 32 tiles, union-find in LDS, one global word per pixel (tile-local roots)
//                           2 cc_merge_borders   unions across tile borders (atomicMin on roots)
//                           3 cc_flatten         every pixel's word becomes its root
//   cris_filter_components  (the work buffer is zeroed by a memset node on the stream)
//                           4 cc_count           area per root, raw area and the error column
//                           5 cc_pick            roots per descriptor, the winner by one 64-bit atomicMax
//                           6 cc_filter          mask bytes rewritten, statistics over the kept pixels
// Chains pass through tile roots only (launch 1 leaves every pixel pointing at its tile's root, launch 2 links roots to roots), and
// strictly decrease, so a find visits at most one word per tile of the image: fewer than 2^21 for w_out * h_out < 2^31.  CC_FIND_CAP
// is a hard cap above that; a walk that hits it (or meets CC_ERR) marks its pixel CC_ERR, which launch 4 turns into the error column.
#define CC_TILE 32
#define CC_FIND_CAP (1 << 22)
#define CC_ERR (-2)

// find: label[i] <= i is the invariant, so the chain x -> label[x] strictly decreases and ends at a root; capped anyway.
template <int SCOPE>
__device__ __forceinline__ int cc_find(int* L, int x, int cap, bool& err) {
    for (int it = 0; it < cap; ++it) {
        const int nx = __hip_atomic_load(L + x, __ATOMIC_RELAXED, SCOPE);
        if (nx == x) return x;
        if (nx < 0) break;
        x = nx;
    }
    err = true;
    return x;
}

// union of the sets of a and b: the larger root is linked below the smaller one with atomicMin.  When another thread linked that root
// first (old != a), its link may have been replaced by ours, so the walk goes on with (old, b): a strictly decreases, the loop ends.
template <int SCOPE>
__device__ __forceinline__ bool cc_union(int* L, int a, int b, int cap) {
    bool err = false;
    for (int it = 0; it < cap; ++it) {
        a = cc_find<SCOPE>(L, a, cap, err);
        b = cc_find<SCOPE>(L, b, cap, err);
        if (err) return true;
        if (a == b) return false;
        if (a < b) { const int s = a; a = b; b = s; }
        const int old = __hip_atomic_fetch_min(L + a, b, __ATOMIC_RELAXED, SCOPE);
        if (old == a) return false;
        if (old < 0) return true;
        a = old;
    }
    return true;
}

// Launch 1.  Visibility: the kernel boundary - a block reads mask bytes the previous launch wrote and writes label words no other
// block of this launch touches; the union-find runs in LDS (workgroup-scope atomics between the barriers).
// blockIdx.y = descriptor, blockIdx.x strides over its 32 x 32 tiles (tiles cover the pitch: padding words are written -1).
// bg = 1 labels the BACKGROUND instead (cris_fill_holes): the pixels whose byte is 0, x < w_out; everything after this line of the
// three launches sees label words only.
__global__ __launch_bounds__(256) void cc_tile_label_kernel(const unsigned char* __restrict__ masks, const cris_eval_desc* __restrict__ descs,
                                                            int conn8, int bg, int* __restrict__ labels) {
    __shared__ int lab[CC_TILE * CC_TILE];
    const cris_eval_desc d = descs[blockIdx.y];
    const int tiles_x = (d.pitch + CC_TILE - 1) / CC_TILE, tiles_y = (d.h_out + CC_TILE - 1) / CC_TILE;
    const long tiles = (long)tiles_x * tiles_y;
    const int ly = threadIdx.x >> 3, lx0 = (threadIdx.x & 7) * 4, l0 = ly * CC_TILE + lx0;
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int ty = (int)(tile / tiles_x), tx = (int)(tile % tiles_x);
        const int y = ty * CC_TILE + ly, x0 = tx * CC_TILE + lx0;
        const bool in = y < d.h_out && x0 < d.pitch;              // (the pitch is a multiple of 4: a group is inside or outside)
        const size_t boff = (size_t)d.out_off + (size_t)y * d.pitch + x0;
        const unsigned int mword = in ? *reinterpret_cast<const unsigned int*>(masks + boff) : 0u;
        bool fg[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            fg[j] = in && x0 + j < d.w_out && (((mword >> (8 * j)) & 0xffu) != 0u) != (bg != 0);
            lab[l0 + j] = fg[j] ? l0 + j : -1;
        }
        __syncthreads();
        bool err = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!fg[j]) continue;
            const int l = l0 + j, lx = lx0 + j;                    // neighbours inside the tile only: its borders are launch 2's
            if (lx > 0 && lab[l - 1] >= 0) err |= cc_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, l, l - 1, 2 * CC_TILE * CC_TILE);
            if (ly > 0) {
                if (lab[l - CC_TILE] >= 0) err |= cc_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, l, l - CC_TILE, 2 * CC_TILE * CC_TILE);
                if (conn8 && lx > 0 && lab[l - CC_TILE - 1] >= 0)
                    err |= cc_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, l, l - CC_TILE - 1, 2 * CC_TILE * CC_TILE);
                if (conn8 && lx < CC_TILE - 1 && lab[l - CC_TILE + 1] >= 0)
                    err |= cc_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, l, l - CC_TILE + 1, 2 * CC_TILE * CC_TILE);
            }
        }
        __syncthreads();
        int4 o;
        int* ov = reinterpret_cast<int*>(&o);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ov[j] = -1;
            if (fg[j]) {
                const int r = cc_find<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, l0 + j, 2 * CC_TILE * CC_TILE, err);
                ov[j] = err ? CC_ERR : (ty * CC_TILE + (r >> 5)) * d.pitch + tx * CC_TILE + (r & (CC_TILE - 1));
            }
        }
        if (in) *reinterpret_cast<int4*>(labels + boff) = o;
        __syncthreads();                                           // (lab is rewritten by the next tile)
    }
}

// Launch 2.  Visibility: blocks read and write each other's label words within this launch, so EVERY access to a label word here is
// an agent-scope atomic (__hip_atomic_load / __hip_atomic_fetch_min, relaxed): no L1 copy is ever used, and any value a load
// returns is an ancestor of its pixel - the result does not depend on which.  64 threads per tile: lane t < 32 owns pixel (t, 0) of
// the tile's left column, lane 32 + t pixel (0, t) of its top row.  A neighbour is tested inside 0 <= x < w_out, 0 <= y < h_out
// only: never across the end of a row, never outside the descriptor's rectangle.
__global__ __launch_bounds__(64) void cc_merge_borders_kernel(const cris_eval_desc* __restrict__ descs, int conn8, int* labels) {
    const cris_eval_desc d = descs[blockIdx.y];
    const int tiles_x = (d.w_out + CC_TILE - 1) / CC_TILE, tiles_y = (d.h_out + CC_TILE - 1) / CC_TILE;
    const long tiles = (long)tiles_x * tiles_y;
    int* L = labels + d.out_off;
    const bool left = threadIdx.x < CC_TILE;
    const int t = threadIdx.x & (CC_TILE - 1);
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int ty = (int)(tile / tiles_x), tx = (int)(tile % tiles_x);
        const int y = ty * CC_TILE + (left ? t : 0), x = tx * CC_TILE + (left ? 0 : t);
        if (y >= d.h_out || x >= d.w_out || (left ? tx == 0 : ty == 0)) continue;
        const int p = y * d.pitch + x;
        if (__hip_atomic_load(L + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0) continue;
        bool err = false;
        // across a vertical border: (y, x - 1) and at 8 (y - 1, x - 1), (y + 1, x - 1); across a horizontal one: (y - 1, x) and at 8
        // (y - 1, x - 1), (y - 1, x + 1)
        const int dy0 = left ? 0 : -1, dx0 = left ? -1 : 0, dy1 = -1, dx1 = -1, dy2 = left ? 1 : -1, dx2 = left ? -1 : 1;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (k > 0 && !conn8) break;
            const int yy = y + (k == 0 ? dy0 : k == 1 ? dy1 : dy2), xx = x + (k == 0 ? dx0 : k == 1 ? dx1 : dx2);
            if (yy < 0 || yy >= d.h_out || xx < 0 || xx >= d.w_out) continue;
            const int q = yy * d.pitch + xx;
            if (__hip_atomic_load(L + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0) continue;
            err |= cc_union<__HIP_MEMORY_SCOPE_AGENT>(L, p, q, CC_FIND_CAP);
        }
        if (err) __hip_atomic_fetch_min(L + p, CC_ERR, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Launch 3.  Visibility: a block's chains run through words (tile roots) that other blocks rewrite in this launch, so EVERY access
// to a label word here is an agent-scope atomic load or store (relaxed).  A word only ever holds an ancestor of its pixel, so each
// walk ends at the same root whichever value it meets: the labels after this launch are the canonical ones on every run.
__global__ __launch_bounds__(256) void cc_flatten_kernel(const cris_eval_desc* __restrict__ descs, int* labels) {
    const cris_eval_desc d = descs[blockIdx.y];
    int* L = labels + d.out_off;
    const int gpr = d.pitch >> 2;
    const long total = (long)gpr * d.h_out;
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long)gridDim.x * blockDim.x) {
        const int y = (int)(g / gpr), x0 = (int)(g % gpr) * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (x0 + j >= d.w_out) continue;
            const int i = y * d.pitch + x0 + j;
            const int v = __hip_atomic_load(L + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (v < 0 || v == i) continue;
            bool err = false;
            const int r = cc_find<__HIP_MEMORY_SCOPE_AGENT>(L, v, CC_FIND_CAP, err);
            __hip_atomic_store(L + i, err ? CC_ERR : r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// sum over the block of one int per thread (4 waves): wave shuffle, LDS, valid in thread 0
__device__ __forceinline__ int cc_block_sum(int v, int* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// A[lab] += cnt for every lane with lab >= 0, pre-summed over the wave: the lanes that hold one label add once.  Called by all 64
// lanes (wave-uniform control flow around it); each pass retires its leader's label: at most 64 passes.
__device__ __forceinline__ void cc_wave_add(int* A, int lab, int cnt, int lane) {
    unsigned long long todo = __ballot(lab >= 0);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int lv = __shfl(lab, leader, 64);
        const bool m = lab == lv;
        int s = m ? cnt : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == leader) atomicAdd(A + lv, s);
        todo &= ~__ballot(m);
    }
}

// Launch 4.  Visibility: the kernel boundary (labels are final; areas / info only receive integer atomicAdd / atomicOr, exact and
// order-free).  areas[out_off + root] += 1 per pixel, pre-summed per wave: the lanes that hold one label add once (a wave's 256
// consecutive pixels mostly share it).  info[row] = (n_components, kept_components, raw_area, error): [2] += foreground pixels,
// [3] |= 1 when a pixel carries CC_ERR or a label outside the rectangle (such a word indexes nothing, here or in launch 6).
__global__ __launch_bounds__(256) void cc_count_kernel(const cris_eval_desc* __restrict__ descs, const int* __restrict__ labels,
                                                       int* __restrict__ areas, unsigned long long* __restrict__ info) {
    __shared__ int red[2][4];
    const cris_eval_desc d = descs[blockIdx.y];
    const int* __restrict__ L = labels + d.out_off;
    int* A = areas + d.out_off;
    const int gpr = d.pitch >> 2, lane = threadIdx.x & 63, limit = d.pitch * d.h_out;
    const long total = (long)gpr * d.h_out;
    int raw = 0, bad = 0;
    for (long base = (long)blockIdx.x * blockDim.x; base < total; base += (long)gridDim.x * blockDim.x) {      // (uniform trip count)
        const long g = base + threadIdx.x;
        int lab[4] = {-1, -1, -1, -1}, cnt[4] = {1, 1, 1, 1};
        if (g < total) {
            const int y = (int)(g / gpr), x0 = (int)(g % gpr) * 4;
            const int4 v = *reinterpret_cast<const int4*>(L + (size_t)y * d.pitch + x0);
            const int* vv = reinterpret_cast<const int*>(&v);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (x0 + j >= d.w_out) continue;
                const bool wild = vv[j] < -1 || vv[j] >= limit;      // CC_ERR, or a word no labelling of this rectangle wrote
                lab[j] = wild ? -1 : vv[j];
                raw += lab[j] >= 0 ? 1 : 0;
                bad |= wild ? 1 : 0;
            }
        }
#pragma unroll
        for (int j = 1; j < 4; ++j)                                // equal neighbours of a thread's four pixels: one count
            if (lab[j] >= 0 && lab[j] == lab[j - 1]) { cnt[j] += cnt[j - 1]; lab[j - 1] = -1; }
#pragma unroll
        for (int j = 0; j < 4; ++j) cc_wave_add(A, lab[j], cnt[j], lane);
    }
    const int raws = cc_block_sum(raw, red[0]), bads = cc_block_sum(bad, red[1]);
    if (threadIdx.x == 0) {
        if (raws) atomicAdd(info + 4 * (size_t)d.row + 2, (unsigned long long)raws);
        if (bads) atomicOr(info + 4 * (size_t)d.row + 3, 1ull);
    }
}

// Launch 5.  Visibility: the kernel boundary (areas are complete).  A root is a pixel whose label is its own index: info[row][0] +=
// roots; with `largest`, every root of area >= min_area bids (area << 32) | (0xffffffff - label) in ONE 64-bit atomicMax on the
// descriptor's winner word: the greatest area wins, among equals the lowest label.  0 = nothing survived.
__global__ __launch_bounds__(256) void cc_pick_kernel(const cris_eval_desc* __restrict__ descs, const int* __restrict__ labels,
                                                      const int* __restrict__ areas, int min_area, int largest,
                                                      unsigned long long* __restrict__ winner, unsigned long long* __restrict__ info) {
    __shared__ int red[4];
    const cris_eval_desc d = descs[blockIdx.y];
    const int* __restrict__ L = labels + d.out_off;
    const int* __restrict__ A = areas + d.out_off;
    const int gpr = d.pitch >> 2;
    const long total = (long)gpr * d.h_out;
    int roots = 0;
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long)gridDim.x * blockDim.x) {
        const int y = (int)(g / gpr), x0 = (int)(g % gpr) * 4;
        const int i0 = y * d.pitch + x0;
        const int4 v = *reinterpret_cast<const int4*>(L + i0);
        const int* vv = reinterpret_cast<const int*>(&v);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (x0 + j >= d.w_out || vv[j] != i0 + j) continue;
            roots += 1;
            const int a = A[i0 + j];
            if (largest && a >= min_area)
                atomicMax(winner + blockIdx.y, ((unsigned long long)(unsigned int)a << 32) | (unsigned long long)(0xffffffffu - (unsigned int)(i0 + j)));
        }
    }
    const int n = cc_block_sum(roots, red);
    if (threadIdx.x == 0 && n) atomicAdd(info + 4 * (size_t)d.row, (unsigned long long)n);
}

// Launch 6.  Visibility: the kernel boundary (areas and winners are complete; a block rewrites mask words no other block touches).
// A pixel is kept iff its component has area >= min_area and, with `largest`, is the winner.  Kept bytes become 255, all others 0;
// info[row][1] += kept roots.  With probs / stats the kept pixels add to stats[row] what predict_masks_batch_kernel adds per pixel
// above the threshold - the value recomputed by ep_warp_value, the same rintf(ep_mul(value, 65536)) - through the same reduction,
// so a mask of one component gives that kernel's row bit for bit.
__global__ __launch_bounds__(256) void cc_filter_kernel(const float* __restrict__ probs, int H, int W, const cris_eval_desc* __restrict__ descs,
                                                        const ep_cubic_tab t, float border, const int* __restrict__ labels,
                                                        const int* __restrict__ areas, const unsigned long long* __restrict__ winner,
                                                        int min_area, int largest, unsigned char* __restrict__ masks,
                                                        unsigned long long* __restrict__ info, unsigned long long* __restrict__ stats) {
    __shared__ float tab[32][4];
    __shared__ unsigned long long red_score[4];
    __shared__ int red[5][4];
    __shared__ int red_kept[4];
    if (threadIdx.x < 128) tab[threadIdx.x >> 2][threadIdx.x & 3] = t.tab[threadIdx.x >> 2][threadIdx.x & 3];
    __syncthreads();
    const cris_eval_desc d = descs[blockIdx.y];
    const float* __restrict__ src = probs + (size_t)d.map * H * W;
    const int* __restrict__ L = labels + d.out_off;
    const int* __restrict__ A = areas + d.out_off;
    const unsigned long long wv = largest ? winner[blockIdx.y] : 0ull;
    const int wlab = wv ? (int)(0xffffffffu - (unsigned int)wv) : -1;
    const int gpr = d.pitch >> 2, limit = d.pitch * d.h_out;
    const long total = (long)gpr * d.h_out;
    int area = 0, x_min = 0x7fffffff, y_min = 0x7fffffff, x_end = 0, y_end = 0, kept = 0;
    unsigned long long score = 0;
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long)gridDim.x * blockDim.x) {
        const int y = (int)(g / gpr), x0 = (int)(g % gpr) * 4;
        const int i0 = y * d.pitch + x0;
        const int4 v = *reinterpret_cast<const int4*>(L + i0);
        const int* vv = reinterpret_cast<const int*>(&v);
        long X0, Y0;
        ep_warp_row(d.m, y, X0, Y0);
        unsigned int oword = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = x0 + j, lab = vv[j];
            if (x >= d.w_out || lab < 0 || lab >= limit) continue;
            if (largest ? lab != wlab : A[lab] < min_area) continue;     // (the winner bid with area >= min_area)
            oword |= 0xffu << (8 * j);
            kept += lab == i0 + j ? 1 : 0;
            if (stats) {
                const float acc = ep_warp_value(src, H, W, tab, d.m, X0, Y0, x, border);
                area += 1;
                score += (unsigned long long)(long long)rintf(ep_mul(acc, 65536.f));
                x_min = min(x_min, x); x_end = max(x_end, x + 1);
                y_min = min(y_min, y); y_end = max(y_end, y + 1);
            }
        }
        *reinterpret_cast<unsigned int*>(masks + d.out_off + (size_t)y * d.pitch + x0) = oword;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        area += __shfl_xor(area, o, 64);
        score += __shfl_xor(score, o, 64);
        kept += __shfl_xor(kept, o, 64);
        x_min = min(x_min, __shfl_xor(x_min, o, 64)); y_min = min(y_min, __shfl_xor(y_min, o, 64));
        x_end = max(x_end, __shfl_xor(x_end, o, 64)); y_end = max(y_end, __shfl_xor(y_end, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        red_score[w] = score;
        red_kept[w] = kept;
        red[0][w] = area; red[1][w] = x_min; red[2][w] = y_min; red[3][w] = x_end; red[4][w] = y_end;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int k = red_kept[0] + red_kept[1] + red_kept[2] + red_kept[3];
        if (k) atomicAdd(info + 4 * (size_t)d.row + 1, (unsigned long long)k);
        const int a = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        if (a > 0) {                                               // (only with stats: area stays 0 without)
            unsigned long long* row = stats + 6 * (size_t)d.row;
            atomicAdd(row, (unsigned long long)a);
            atomicAdd(row + 1, red_score[0] + red_score[1] + red_score[2] + red_score[3]);
            atomicMin(row + 2, (unsigned long long)min(min(red[1][0], red[1][1]), min(red[1][2], red[1][3])));
            atomicMin(row + 3, (unsigned long long)min(min(red[2][0], red[2][1]), min(red[2][2], red[2][3])));
            atomicMax(row + 4, (unsigned long long)max(max(red[3][0], red[3][1]), max(red[3][2], red[3][3])));
            atomicMax(row + 5, (unsigned long long)max(max(red[4][0], red[4][1]), max(red[4][2], red[4][3])));
        }
    }
}

// counts[row] += (#(pred != 0 and gt != 0), #(pred != 0 or gt != 0)) over x < w_out: eval_iou_batch_kernel's counts from mask bytes
// (pred at out_off, gt at mask_off, one pitch), its reduction and its integer atomics.  Visibility: the kernel boundary.
__global__ __launch_bounds__(256) void mask_iou_batch_kernel(const unsigned char* __restrict__ pred, const cris_eval_desc* __restrict__ descs,
                                                             const unsigned char* __restrict__ gt, int* __restrict__ counts) {
    __shared__ int red[2][4];
    const cris_eval_desc d = descs[blockIdx.y];
    const int gpr = d.pitch >> 2;
    const long total = (long)gpr * d.h_out;
    int inter = 0, uni = 0;
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long)gridDim.x * blockDim.x) {
        const int y = (int)(g / gpr), x0 = (int)(g % gpr) * 4;
        const size_t boff = (size_t)y * d.pitch + x0;
        const unsigned int pword = *reinterpret_cast<const unsigned int*>(pred + d.out_off + boff);
        const unsigned int mword = *reinterpret_cast<const unsigned int*>(gt + d.mask_off + boff);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (x0 + j >= d.w_out) continue;
            const bool p = ((pword >> (8 * j)) & 0xffu) != 0u, m = ((mword >> (8 * j)) & 0xffu) != 0u;
            inter += (p && m) ? 1 : 0;
            uni += (p || m) ? 1 : 0;
        }
    }
    const int is = cc_block_sum(inter, red[0]), us = cc_block_sum(uni, red[1]);
    if (threadIdx.x == 0) {
        atomicAdd(counts + 2 * (size_t)d.row, is);
        atomicAdd(counts + 2 * (size_t)d.row + 1, us);
    }
}

// what the three launchers below check per descriptor on the host copy, before any launch: every address the kernels form
static const char* cc_check_descs(const cris_eval_desc* descs_host, int n, size_t out_bytes, int rows, bool gt, size_t gt_bytes, long* most) {
    *most = 0;
    for (int i = 0; i < n; ++i) {
        const cris_eval_desc& d = descs_host[i];
        if (!(d.w_out > 0 && d.h_out > 0 && (long)d.w_out * d.h_out < (1L << 31))) return "descriptor: bad output size";
        if (!(d.pitch >= d.w_out && (d.pitch & 3) == 0 && d.pitch - d.w_out < (1 << 20) && (long)d.pitch * d.h_out < (1L << 31)))
            return "descriptor: the pitch must be a multiple of 4, >= w_out, pitch * h_out < 2^31";
        const size_t bytes = (size_t)d.pitch * d.h_out;
        if (!(d.out_off >= 0 && (d.out_off & 3) == 0 && (size_t)d.out_off + bytes <= out_bytes)) return "descriptor: output outside the buffer";
        if (rows >= 0 && !(d.row >= 0 && d.row < rows)) return "descriptor: row out of range";
        if (gt && !(d.mask_off >= 0 && (d.mask_off & 3) == 0 && (size_t)d.mask_off + bytes <= gt_bytes)) return "descriptor: mask outside the buffer";
        const long groups = (long)(d.pitch >> 2) * d.h_out;
        if (groups > *most) *most = groups;
    }
    return nullptr;
}

// launches 1 - 3 for checked operands: the components of the foreground (bg = 0) or of the background (bg = 1)
static int cc_label_launches(const unsigned char* masks, const cris_eval_desc* descs_dev, int n, int conn8, int bg, long most,
                             int* labels, void* stream) {
    const int cap = 2048 / n > 8 ? 2048 / n : 8;                   // the grid of cris_eval_iou_batch
    const long tiles = (most * 4 + CC_TILE * CC_TILE - 1) / (CC_TILE * CC_TILE) + 1;      // (a bound: the blocks stride over their own count)
    hipLaunchKernelGGL(cc_tile_label_kernel, dim3(cris_grid_1d(tiles, 1, 4 * cap), n), dim3(256), 0, (hipStream_t)stream, masks, descs_dev,
                       conn8, bg, labels);
    CRIS_LAUNCH_CHECK();
    hipLaunchKernelGGL(cc_merge_borders_kernel, dim3(cris_grid_1d(tiles, 1, 4 * cap), n), dim3(64), 0, (hipStream_t)stream, descs_dev, conn8,
                       labels);
    CRIS_LAUNCH_CHECK();
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(cris_grid_1d(most, 256, cap), n), dim3(256), 0, (hipStream_t)stream, descs_dev, labels);
    CRIS_LAUNCH_CHECK();
    return 0;
}

extern "C" int cris_label_components(const unsigned char* masks, size_t mask_bytes, const cris_eval_desc* descs_host,
                                     const cris_eval_desc* descs_dev, int n, int connectivity, int* labels, size_t label_words,
                                     void* stream) {
    CRIS_CHECK_ARG(masks && descs_host && descs_dev && labels, "null operand");
    CRIS_CHECK_ARG(n > 0 && n <= 65535, "n must be in 1 .. 65535");
    CRIS_CHECK_ARG(connectivity == 4 || connectivity == 8, "connectivity must be 4 or 8");
    CRIS_CHECK_ARG(((uintptr_t)masks & 3) == 0 && ((uintptr_t)labels & 15) == 0, "masks must be 4-byte, labels 16-byte aligned");
    CRIS_CHECK_ARG(label_words >= mask_bytes, "the label buffer must hold one word per mask byte");
    long most = 0;
    const char* bad = cc_check_descs(descs_host, n, mask_bytes, -1, false, 0, &most);
    CRIS_CHECK_ARG(!bad, bad);
    return cc_label_launches(masks, descs_dev, n, connectivity == 8, 0, most, labels, stream);
}

extern "C" size_t cris_filter_components_work_bytes(size_t mask_bytes, int n) {
    return ((mask_bytes * 4 + 7) & ~(size_t)7) + 8 * (size_t)(n > 0 ? n : 0);
}

extern "C" int cris_filter_components(unsigned char* masks, size_t mask_bytes, const int* labels, size_t label_words,
                                      const cris_eval_desc* descs_host, const cris_eval_desc* descs_dev, int n, int keep_largest,
                                      int min_area, void* work, size_t work_bytes, long long* info, int info_rows, const float* probs, int P,
                                      int H, int W, float border, long long* stats, int stat_rows, void* stream) {
    CRIS_CHECK_ARG(masks && labels && descs_host && descs_dev && work && info, "null operand");
    CRIS_CHECK_ARG(n > 0 && n <= 65535, "n must be in 1 .. 65535");
    CRIS_CHECK_ARG((keep_largest == 0 || keep_largest == 1) && min_area >= 0, "keep_largest must be 0 or 1 and min_area >= 0");
    CRIS_CHECK_ARG(info_rows > 0, "bad sizes");
    CRIS_CHECK_ARG(((uintptr_t)masks & 3) == 0 && ((uintptr_t)labels & 15) == 0 && ((uintptr_t)work & 15) == 0 && ((uintptr_t)info & 7) == 0,
                   "masks must be 4-byte, labels and work 16-byte, info 8-byte aligned");
    CRIS_CHECK_ARG(label_words >= mask_bytes, "the label buffer must hold one word per mask byte");
    CRIS_CHECK_ARG(work_bytes >= cris_filter_components_work_bytes(mask_bytes, n), "the work buffer is too small");
    CRIS_CHECK_ARG((probs != nullptr) == (stats != nullptr), "probs and stats go together");
    if (probs) {
        CRIS_CHECK_ARG(P > 0 && H > 0 && W > 0 && stat_rows > 0, "bad sizes");
        CRIS_CHECK_ARG(border >= -3.0e38f && border <= 3.0e38f, "border must be finite");
        CRIS_CHECK_ARG(((uintptr_t)stats & 7) == 0, "stats must be 8-byte aligned");
    }
    long most = 0;
    const char* bad = cc_check_descs(descs_host, n, mask_bytes, probs && stat_rows < info_rows ? stat_rows : info_rows, false, 0, &most);
    CRIS_CHECK_ARG(!bad, bad);
    if (probs)
        for (int i = 0; i < n; ++i) CRIS_CHECK_ARG(descs_host[i].map >= 0 && descs_host[i].map < P, "descriptor: map out of range");
    int* areas = reinterpret_cast<int*>(work);
    unsigned long long* winner = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(work) + ((mask_bytes * 4 + 7) & ~(size_t)7));
    unsigned long long* inf = reinterpret_cast<unsigned long long*>(info);
    const hipError_t e = hipMemsetAsync(work, 0, cris_filter_components_work_bytes(mask_bytes, n), (hipStream_t)stream);
    if (e != hipSuccess) {
        cris_set_error("%s: memset failed: %s", __func__, hipGetErrorString(e));
        return (int)e;
    }
    ep_cubic_tab t;
    ep_warp_setup(nullptr, nullptr, t.tab);
    const int cap = 2048 / n > 8 ? 2048 / n : 8;                   // the grid of cris_eval_iou_batch
    const dim3 grid(cris_grid_1d(most, 256, cap), n);
    hipLaunchKernelGGL(cc_count_kernel, grid, dim3(256), 0, (hipStream_t)stream, descs_dev, labels, areas, inf);
    CRIS_LAUNCH_CHECK();
    hipLaunchKernelGGL(cc_pick_kernel, grid, dim3(256), 0, (hipStream_t)stream, descs_dev, labels, (const int*)areas, min_area, keep_largest,
                       winner, inf);
    CRIS_LAUNCH_CHECK();
    hipLaunchKernelGGL(cc_filter_kernel, grid, dim3(256), 0, (hipStream_t)stream, probs, H, W, descs_dev, t, border, labels, (const int*)areas,
                       (const unsigned long long*)winner, min_area, keep_largest, masks, inf, reinterpret_cast<unsigned long long*>(stats));
    CRIS_LAUNCH_CHECK();
    return 0;
}

extern "C" int cris_mask_iou_batch(const unsigned char* pred, size_t pred_bytes, const cris_eval_desc* descs_host,
                                   const cris_eval_desc* descs_dev, int n, const unsigned char* gt, size_t gt_bytes, int* counts,
                                   int count_rows, void* stream) {
    CRIS_CHECK_ARG(pred && descs_host && descs_dev && gt && counts, "null operand");
    CRIS_CHECK_ARG(n > 0 && n <= 65535, "n must be in 1 .. 65535");
    CRIS_CHECK_ARG(count_rows > 0, "bad sizes");
    CRIS_CHECK_ARG(((uintptr_t)pred & 3) == 0 && ((uintptr_t)gt & 3) == 0 && ((uintptr_t)counts & 3) == 0, "pred, gt and counts must be 4-byte aligned");
    long most = 0;
    const char* bad = cc_check_descs(descs_host, n, pred_bytes, count_rows, true, gt_bytes, &most);
    CRIS_CHECK_ARG(!bad, bad);
    const int cap = 2048 / n > 8 ? 2048 / n : 8;                   // the grid of cris_eval_iou_batch
    hipLaunchKernelGGL(mask_iou_batch_kernel, dim3(cris_grid_1d(most, 256, cap), n), dim3(256), 0, (hipStream_t)stream, pred, descs_dev, gt,
                       counts);
    CRIS_LAUNCH_CHECK();
    return 0;
}

// ---- hole filling: the components of the BACKGROUND that own no pixel of the image's outer frame ----
//   cris_fill_holes   1 - 3  the labeller's launches with bg = 1: the label word of a background pixel is its component's root
//                     (the work buffer is zeroed by a memset node on the stream)
//                     4 cc_hole_count   area per root (bits 0 .. 30 of its word) and CC_FRAME when the component owns a frame pixel
//                     5 cc_hole_fill    the pixels of unmarked roots of area <= max_area become 255
#define CC_FRAME 0x80000000u

// Launch 4.  Visibility: the kernel boundary (labels are final).  areas[out_off + root] receives integer atomicAdd (the wave's
// pre-summed count, as in cc_count_kernel) and atomicOr of bit 31, which no area reaches (pitch * h_out < 2^31): exact, order-free.
// info[row][3] |= 1 when a pixel carries CC_ERR or a label outside the rectangle (such a word indexes nothing, here or in launch 5).
__global__ __launch_bounds__(256) void cc_hole_count_kernel(const cris_eval_desc* __restrict__ descs, const int* __restrict__ labels,
                                                            int* __restrict__ areas, unsigned long long* __restrict__ info) {
    __shared__ int red[4];
    const cris_eval_desc d = descs[blockIdx.y];
    const int* __restrict__ L = labels + d.out_off;
    int* A = areas + d.out_off;
    const int gpr = d.pitch >> 2, lane = threadIdx.x & 63, limit = d.pitch * d.h_out;
    const long total = (long)gpr * d.h_out;
    int bad = 0;
    for (long base = (long)blockIdx.x * blockDim.x; base < total; base += (long)gridDim.x * blockDim.x) {      // (uniform trip count)
        const long g = base + threadIdx.x;
        int lab[4] = {-1, -1, -1, -1}, cnt[4] = {1, 1, 1, 1};
        if (g < total) {
            const int y = (int)(g / gpr), x0 = (int)(g % gpr) * 4;
            const int4 v = *reinterpret_cast<const int4*>(L + (size_t)y * d.pitch + x0);
            const int* vv = reinterpret_cast<const int*>(&v);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int x = x0 + j;
                if (x >= d.w_out) continue;
                const bool wild = vv[j] < -1 || vv[j] >= limit;
                lab[j] = wild ? -1 : vv[j];
                bad |= wild ? 1 : 0;
                if (lab[j] >= 0 && (y == 0 || y == d.h_out - 1 || x == 0 || x == d.w_out - 1))
                    atomicOr(reinterpret_cast<unsigned int*>(A) + lab[j], CC_FRAME);
            }
        }
#pragma unroll
        for (int j = 1; j < 4; ++j)                                // equal neighbours of a thread's four pixels: one count
            if (lab[j] >= 0 && lab[j] == lab[j - 1]) { cnt[j] += cnt[j - 1]; lab[j - 1] = -1; }
#pragma unroll
        for (int j = 0; j < 4; ++j) cc_wave_add(A, lab[j], cnt[j], lane);
    }
    const int bads = cc_block_sum(bad, red);
    if (threadIdx.x == 0 && bads) atomicOr(info + 4 * (size_t)d.row + 3, 1ull);
}

// Launch 5.  Visibility: the kernel boundary (areas and marks are complete; a block rewrites mask words no other block touches, and
// only the bytes of filled pixels change: a byte that was 0 becomes 255, the other bytes of its word are stored as they were read).
// info[row] += (holes filled, pixels filled, holes of any area, 0): a hole is counted at its root, the pixel whose label is its own index.
__global__ __launch_bounds__(256) void cc_hole_fill_kernel(const cris_eval_desc* __restrict__ descs, const int* __restrict__ labels,
                                                           const int* __restrict__ areas, int max_area, unsigned char* __restrict__ masks,
                                                           unsigned long long* __restrict__ info) {
    __shared__ int red[3][4];
    const cris_eval_desc d = descs[blockIdx.y];
    const int* __restrict__ L = labels + d.out_off;
    const int* __restrict__ A = areas + d.out_off;
    const int gpr = d.pitch >> 2, limit = d.pitch * d.h_out;
    const long total = (long)gpr * d.h_out;
    int holes = 0, filled = 0, pixels = 0;
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long)gridDim.x * blockDim.x) {
        const int y = (int)(g / gpr), x0 = (int)(g % gpr) * 4;
        const int i0 = y * d.pitch + x0;
        const int4 v = *reinterpret_cast<const int4*>(L + i0);
        const int* vv = reinterpret_cast<const int*>(&v);
        unsigned int oword = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int lab = vv[j];
            if (x0 + j >= d.w_out || lab < 0 || lab >= limit) continue;
            const unsigned int a = (unsigned int)A[lab];
            if (a & CC_FRAME) continue;                            // joined to the outside: no hole
            const int root = lab == i0 + j ? 1 : 0;
            holes += root;
            if (max_area >= 0 && a > (unsigned int)max_area) continue;
            oword |= 0xffu << (8 * j);
            pixels += 1;
            filled += root;
        }
        if (oword) {
            unsigned int* p = reinterpret_cast<unsigned int*>(masks + d.out_off + (size_t)y * d.pitch + x0);
            *p |= oword;
        }
    }
    const int fs = cc_block_sum(filled, red[0]), ps = cc_block_sum(pixels, red[1]), hs = cc_block_sum(holes, red[2]);
    if (threadIdx.x == 0) {
        if (fs) atomicAdd(info + 4 * (size_t)d.row, (unsigned long long)fs);
        if (ps) atomicAdd(info + 4 * (size_t)d.row + 1, (unsigned long long)ps);
        if (hs) atomicAdd(info + 4 * (size_t)d.row + 2, (unsigned long long)hs);
    }
}

extern "C" size_t cris_fill_holes_work_bytes(size_t mask_bytes) { return (mask_bytes * 4 + 7) & ~(size_t)7; }

extern "C" int cris_fill_holes(unsigned char* masks, size_t mask_bytes, const cris_eval_desc* descs_host, const cris_eval_desc* descs_dev, int n,
                               int connectivity, int max_area, int* labels, size_t label_words, void* work, size_t work_bytes,
                               long long* info, int info_rows, void* stream) {
    CRIS_CHECK_ARG(masks && descs_host && descs_dev && labels && work && info, "null operand");
    CRIS_CHECK_ARG(n > 0 && n <= 65535, "n must be in 1 .. 65535");
    CRIS_CHECK_ARG(connectivity == 4 || connectivity == 8, "connectivity must be 4 or 8");
    CRIS_CHECK_ARG(max_area >= -1, "max_area must be >= 0, or -1 for no cap");
    CRIS_CHECK_ARG(info_rows > 0, "bad sizes");
    CRIS_CHECK_ARG(((uintptr_t)masks & 3) == 0 && ((uintptr_t)labels & 15) == 0 && ((uintptr_t)work & 15) == 0 && ((uintptr_t)info & 7) == 0,
                   "masks must be 4-byte, labels and work 16-byte, info 8-byte aligned");
    CRIS_CHECK_ARG(label_words >= mask_bytes, "the label buffer must hold one word per mask byte");
    CRIS_CHECK_ARG(work_bytes >= cris_fill_holes_work_bytes(mask_bytes), "the work buffer is too small");
    long most = 0;
    const char* bad = cc_check_descs(descs_host, n, mask_bytes, info_rows, false, 0, &most);
    CRIS_CHECK_ARG(!bad, bad);
    const int rc = cc_label_launches(masks, descs_dev, n, connectivity == 8, 1, most, labels, stream);
    if (rc) return rc;
    const hipError_t e = hipMemsetAsync(work, 0, cris_fill_holes_work_bytes(mask_bytes), (hipStream_t)stream);
    if (e != hipSuccess) {
        cris_set_error("%s: memset failed: %s", __func__, hipGetErrorString(e));
        return (int)e;
    }
    int* areas = reinterpret_cast<int*>(work);
    unsigned long long* inf = reinterpret_cast<unsigned long long*>(info);
    const int cap = 2048 / n > 8 ? 2048 / n : 8;                   // the grid of cris_eval_iou_batch
    const dim3 grid(cris_grid_1d(most, 256, cap), n);
    hipLaunchKernelGGL(cc_hole_count_kernel, grid, dim3(256), 0, (hipStream_t)stream, descs_dev, (const int*)labels, areas, inf);
    CRIS_LAUNCH_CHECK();
    hipLaunchKernelGGL(cc_hole_fill_kernel, grid, dim3(256), 0, (hipStream_t)stream, descs_dev, (const int*)labels, (const int*)areas, max_area,
                       masks, inf);
    CRIS_LAUNCH_CHECK();
    return 0;
}
