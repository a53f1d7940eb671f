// Input preprocessing on the GPU (reference utils/dataset.py:146-168 `RefDataset.__getitem__`, :207-221 `convert`): per
// sample  img = cv2.warpAffine(rgb_u8, mat, (S, S), INTER_CUBIC, borderValue = CLIP mean * 255),
//         mask = cv2.warpAffine(mask_u8, mat, (S, S), INTER_LINEAR, borderValue = 0) / 255,
//         img = (img.float() / 255 - mean) / std  as [3, S, S].
// The reference does this in 32 DataLoader worker processes per node; at > 500 samples/s per GPU that is ~4 k letterbox warps
// per second and node, so the decoded uint8 images are uploaded as they are (a 640x480 RGB image is 0.9 MB, a third of
// its float tensor) and one launch per BATCH produces the network input directly in HBM.  HBM-bound integer kernel: one
// thread per destination pixel, 16 + 4 byte taps, the three channels and the mask of a pixel share the coordinates.
//
// Arithmetic = OpenCV's 8-bit path, restated in oracle/input_pipe.py (cv2 itself is not available offline - unpinned):
// fixed-point destination->source coordinates (AB_BITS 10, 1/32 pixel), 16-bit weight tables x 2^15 whose rows sum to 2^15
// (cris_remap_tables_u8 builds them like cv::initInterTab2D), border taps read the border colour, (sum + 2^14) >> 15
// saturated to 8 bits.  All integer except the coordinate set-up (double, explicitly unfused), so results are bit exact
// against the oracle.  The normalisation is a 256-entry lookup per channel built on the host with the reference's float ops.
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include "common.h"
#include "../../../include/cris_hip.h"

#pragma clang fp contract(off)
__device__ __forceinline__ double ip_dmul(double a, double b) { return a * b; }
__device__ __forceinline__ double ip_dadd(double a, double b) { return a + b; }

#define IP_AB_BITS 10
#define IP_INTER_BITS 5
#define IP_COEF_BITS 15

// Photometric jitter of the augmented launch (this project's own definition, fixed order brightness, contrast,
// saturation, no hue - not pinned against another library).  factors [n][3] = (fb, fc, fs) per sample, sums [n] = what
// gray_sum_batch_kernel left (NULL when no sample has fc != 1: the pivot is then multiplied by an exact 0), unit[v] = v / 255,
// norm = mean rgb, std rgb.  Every float operation below is one separately rounded IEEE operation (contract off).
struct ip_aug_args {
    const float* factors;
    const unsigned long long* sums;
    const float* unit;
    float norm[6];
};
__device__ __forceinline__ float ip_clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }

struct ip_no_args {};
template <bool AUG> struct ip_extra { typedef ip_no_args type; };
template <> struct ip_extra<true> { typedef ip_aug_args type; };

// block = 256 destination pixels of sample blockIdx.y.  One warp code, two instantiations: AUG = false is cris_preprocess_batch,
// with the instructions and registers it had before the flag existed.  (The kernel itself is the template, its last argument an
// empty struct without the flag: a shared __device__ body behind two kernels lost the __restrict__ of the pointers when it was
// inlined and cost the plain kernel 14 more VGPRs.)
template <bool AUG>
__global__ __launch_bounds__(256) void preprocess_batch_kernel(const cris_sample_desc* __restrict__ samples, int S_h, int S_w,
                                                               const short* __restrict__ tab_linear, const short* __restrict__ tab_cubic,
                                                               const float* __restrict__ lut_img, const float* __restrict__ lut_mask,
                                                               cris_u8x4 border, float* __restrict__ img_out, float* __restrict__ mask_out,
                                                               typename ip_extra<AUG>::type extra) {
    [[maybe_unused]] const typename ip_extra<AUG>::type* aug = &extra;
    const int b = blockIdx.y;
    const cris_sample_desc s = samples[b];
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= S_h * S_w) return;
    const int x = idx % S_w, y = idx / S_w;
    const double AB = (double)(1 << IP_AB_BITS);
    const int round_delta = (1 << IP_AB_BITS) / (1 << IP_INTER_BITS) / 2;
    const long adelta = (long)rint(ip_dmul(ip_dmul(s.inv[0], (double)x), AB)), bdelta = (long)rint(ip_dmul(ip_dmul(s.inv[3], (double)x), AB));
    const long X0 = (long)rint(ip_dmul(ip_dadd(ip_dmul(s.inv[1], (double)y), s.inv[2]), AB)) + round_delta;
    const long Y0 = (long)rint(ip_dmul(ip_dadd(ip_dmul(s.inv[4], (double)y), s.inv[5]), AB)) + round_delta;
    const long Xq = (X0 + adelta) >> (IP_AB_BITS - IP_INTER_BITS), Yq = (Y0 + bdelta) >> (IP_AB_BITS - IP_INTER_BITS);
    const int bx = (int)(Xq >> IP_INTER_BITS), by = (int)(Yq >> IP_INTER_BITS);
    const int ent = (int)(Yq & 31) * 32 + (int)(Xq & 31);
    const int H = s.H, W = s.W;
    if (s.img != nullptr) {                                  // INTER_CUBIC, 3 interleaved channels
        const short* w = tab_cubic + ent * 16;
        int acc[3] = {0, 0, 0};
        const int cv[3] = {border.v[0], border.v[1], border.v[2]};
#pragma unroll
        for (int ky = 0; ky < 4; ++ky) {
            const int yy = by - 1 + ky;
#pragma unroll
            for (int kx = 0; kx < 4; ++kx) {
                const int xx = bx - 1 + kx;
                const int wt = w[ky * 4 + kx];
                if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
                    const unsigned char* p = s.img + ((size_t)yy * W + xx) * 3;
                    acc[0] += (int)p[0] * wt; acc[1] += (int)p[1] * wt; acc[2] += (int)p[2] * wt;
                } else {
                    acc[0] += cv[0] * wt; acc[1] += cv[1] * wt; acc[2] += cv[2] * wt;
                }
            }
        }
        if constexpr (!AUG) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int v = min(max((acc[c] + (1 << (IP_COEF_BITS - 1))) >> IP_COEF_BITS, 0), 255);
                img_out[(((size_t)b * 3 + c) * S_h + y) * S_w + x] = lut_img[c * 256 + v];
            }
        } else {
            int v[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = min(max((acc[c] + (1 << (IP_COEF_BITS - 1))) >> IP_COEF_BITS, 0), 255);
            // the 4x4 taps are rows by-1 .. by+2, columns bx-1 .. bx+2: none inside the source = pure letter-box border, which
            // stays the normalised border colour; a sample whose factors are all exactly 1 takes the lookup as well (both
            // are then cris_preprocess_batch's bits by construction)
            const float fb = aug->factors[b * 3], fc = aug->factors[b * 3 + 1], fs = aug->factors[b * 3 + 2];
            const bool taps_inside = by + 2 >= 0 && by - 1 < H && bx + 2 >= 0 && bx - 1 < W;
            if (taps_inside && !(fb == 1.0f && fc == 1.0f && fs == 1.0f)) {
                float xc[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) xc[c] = ip_clamp01(aug->unit[v[c]] * fb);
                const float mean = aug->sums != nullptr ? (float)((double)aug->sums[b] / ip_dmul(ip_dmul(65280.0, (double)H), (double)W)) : 0.0f;
                const float bm = fb * mean;
                const float pivot = bm > 1.0f ? 1.0f : bm;
                const float k = (1.0f - fc) * pivot;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float t = xc[c] * fc;
                    xc[c] = ip_clamp01(t + k);
                }
                const float g0 = 0.299f * xc[0], g1 = 0.587f * xc[1], g2 = 0.114f * xc[2];
                const float g = (g0 + g1) + g2;
                const float sg = (1.0f - fs) * g;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float t = xc[c] * fs;
                    const float o = ip_clamp01(t + sg);
                    img_out[(((size_t)b * 3 + c) * S_h + y) * S_w + x] = (o - aug->norm[c]) / aug->norm[3 + c];
                }
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) img_out[(((size_t)b * 3 + c) * S_h + y) * S_w + x] = lut_img[c * 256 + v[c]];
            }
        }
    }
    if (s.mask != nullptr && mask_out != nullptr) {          // INTER_LINEAR, 1 channel, border 0
        const short* w = tab_linear + ent * 4;
        int acc = 0;
#pragma unroll
        for (int ky = 0; ky < 2; ++ky)
#pragma unroll
            for (int kx = 0; kx < 2; ++kx) {
                const int yy = by + ky, xx = bx + kx;
                if (yy >= 0 && yy < H && xx >= 0 && xx < W) acc += (int)s.mask[(size_t)yy * W + xx] * (int)w[ky * 2 + kx];
            }
        const int v = min(max((acc + (1 << (IP_COEF_BITS - 1))) >> IP_COEF_BITS, 0), 255);
        mask_out[((size_t)b * S_h + y) * S_w + x] = lut_mask[v];
    }
}

// sums[b] += sum over the source pixels of sample b of 77 R + 150 G + 29 B (exact integers; 77 + 150 + 29 = 256, so a pixel adds
// at most 65280 and a 32-bit total would wrap after 65 793 white pixels: every accumulator here is 64 bits wide).  Block
// (blockIdx.x, b) strides over the image in groups of 4 pixels = 3 dwords (the interleaved bytes of a contiguous [H][W][3] image
// whose base is 4-byte aligned - the launcher checks it); block 0 adds the last H*W % 4 pixels byte by byte.  Wave shuffle, LDS,
// then one 64-bit atomic add per block: integer addition is exact and order-free (the argument evalpost.hip makes for its counts).
#define IP_GRAY_GROUP(w0, w1, w2)                                                                                              \
    (77u * (((w0) & 0xffu) + ((w0) >> 24) + (((w1) >> 16) & 0xffu) + (((w2) >> 8) & 0xffu)) +                                    \
     150u * ((((w0) >> 8) & 0xffu) + ((w1) & 0xffu) + ((w1) >> 24) + (((w2) >> 16) & 0xffu)) +                                  \
     29u * ((((w0) >> 16) & 0xffu) + (((w1) >> 8) & 0xffu) + ((w2) & 0xffu) + ((w2) >> 24)))
__global__ __launch_bounds__(256) void gray_sum_batch_kernel(const cris_sample_desc* __restrict__ samples, unsigned long long* __restrict__ sums) {
    __shared__ unsigned long long red[4];
    const int b = blockIdx.y;
    const unsigned char* img = samples[b].img;
    const long npix = (long)samples[b].H * samples[b].W;
    const long groups = npix >> 2;
    if ((long)blockIdx.x * 256 >= groups && blockIdx.x != 0) return;          // (block-uniform) nothing of this sample left for this block
    const unsigned int* words = reinterpret_cast<const unsigned int*>(img);
    unsigned long long acc = 0;
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long)gridDim.x * 256) {
        const unsigned int w0 = words[3 * g], w1 = words[3 * g + 1], w2 = words[3 * g + 2];      // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
        acc += IP_GRAY_GROUP(w0, w1, w2);                                                          // <= 4 * 65280: fits 32 bits
    }
    if (blockIdx.x == 0) {
        const long p = groups * 4 + threadIdx.x;
        if (threadIdx.x < 3 && p < npix) acc += 77u * img[3 * p] + 150u * img[3 * p + 1] + 29u * img[3 * p + 2];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(sums + b, red[0] + red[1] + red[2] + red[3]);
}

extern "C" int cris_gray_sum_batch(const cris_sample_desc* samples_host, const cris_sample_desc* samples_dev, int n, unsigned long long* sums_dev,
                                   void* stream) {
    CRIS_CHECK_ARG(samples_host && samples_dev && sums_dev, "null pointer");
    CRIS_CHECK_ARG(n > 0 && n <= 65535, "n must be in 1 .. 65535");
    CRIS_CHECK_ARG(((uintptr_t)sums_dev & 7) == 0, "sums must be 8-byte aligned");
    long max_groups = 0;
    for (int i = 0; i < n; ++i) {
        const cris_sample_desc& s = samples_host[i];
        CRIS_CHECK_ARG(s.img != nullptr, "null image");
        CRIS_CHECK_ARG(s.H > 0 && s.W > 0, "image sizes must be positive");
        CRIS_CHECK_ARG(((uintptr_t)s.img & 3) == 0, "image base must be 4-byte aligned (the rows are read as dwords)");
        const long g = ((long)s.H * s.W) >> 2;
        max_groups = g > max_groups ? g : max_groups;
    }
    // 4 groups (16 pixels) per thread and pass at the largest image, at most 128 blocks per sample
    hipLaunchKernelGGL(gray_sum_batch_kernel, dim3(cris_grid_1d(max_groups, 256 * 4, 128), n), dim3(256), 0, (hipStream_t)stream, samples_dev,
                       sums_dev);
    CRIS_LAUNCH_CHECK();
    return 0;
}

extern "C" int cris_preprocess_batch_aug(const cris_sample_desc* samples_dev, int n, int S_h, int S_w, const short* tab_linear,
                                         const short* tab_cubic, const float* lut_img, const float* lut_mask, const unsigned char* border_rgb,
                                         const float* factors_dev, const unsigned long long* sums_dev, const float* unit_dev,
                                         const float* norm, float* img_out, float* mask_out, void* stream) {
    CRIS_CHECK_ARG(samples_dev && tab_linear && tab_cubic && lut_img && lut_mask && border_rgb && factors_dev && unit_dev && norm && img_out,
                   "null pointer");
    CRIS_CHECK_ARG(n > 0 && n <= 65535, "n must be in 1 .. 65535");
    CRIS_CHECK_ARG(S_h > 0 && S_w > 0 && (long)S_h * S_w < (1L << 31), "bad output size");
    CRIS_CHECK_ARG(((uintptr_t)factors_dev & 3) == 0 && ((uintptr_t)unit_dev & 3) == 0 && ((uintptr_t)sums_dev & 7) == 0,
                   "factors / unit must be 4-byte and sums 8-byte aligned");
    for (int c = 0; c < 3; ++c) CRIS_CHECK_ARG(norm[c] == norm[c] && norm[3 + c] > 0.0f, "norm = mean rgb, std rgb with std > 0");
    cris_u8x4 bd;
    bd.v[0] = border_rgb[0]; bd.v[1] = border_rgb[1]; bd.v[2] = border_rgb[2]; bd.v[3] = 0;
    ip_aug_args aug;
    aug.factors = factors_dev; aug.sums = sums_dev; aug.unit = unit_dev;
    for (int c = 0; c < 6; ++c) aug.norm[c] = norm[c];
    hipLaunchKernelGGL(preprocess_batch_kernel<true>, dim3(cris_cdiv(S_h * S_w, 256), n), dim3(256), 0, (hipStream_t)stream, samples_dev, S_h,
                       S_w, tab_linear, tab_cubic, lut_img, lut_mask, bd, img_out, mask_out, aug);
    CRIS_LAUNCH_CHECK();
    return 0;
}

extern "C" int cris_preprocess_batch(const cris_sample_desc* samples_dev, int n, int S_h, int S_w, const short* tab_linear,
                                     const short* tab_cubic, const float* lut_img, const float* lut_mask, const unsigned char* border_rgb,
                                     float* img_out, float* mask_out, void* stream) {
    CRIS_CHECK_ARG(samples_dev && n > 0 && S_h > 0 && S_w > 0 && tab_linear && tab_cubic && lut_img && lut_mask && border_rgb && img_out,
                   "bad args");
    cris_u8x4 bd;
    bd.v[0] = border_rgb[0]; bd.v[1] = border_rgb[1]; bd.v[2] = border_rgb[2]; bd.v[3] = 0;
    hipLaunchKernelGGL(preprocess_batch_kernel<false>, dim3(cris_cdiv(S_h * S_w, 256), n), dim3(256), 0, (hipStream_t)stream, samples_dev, S_h, S_w,
                       tab_linear, tab_cubic, lut_img, lut_mask, bd, img_out, mask_out, ip_no_args());
    CRIS_LAUNCH_CHECK();
    return 0;
}

// ---- host helpers -------------------------------------------------------------------------------------------------

// cv::invertAffineTransform in double: the destination->source map cv2.warpAffine applies when it is given `mat`
extern "C" int cris_invert_affine(const double* mat, double* inv) {
    CRIS_CHECK_ARG(mat && inv, "bad args");
    double D = mat[0] * mat[4] - mat[1] * mat[3];
    D = D != 0.0 ? 1.0 / D : 0.0;
    const double A11 = mat[4] * D, A22 = mat[0] * D, A12 = -mat[1] * D, A21 = -mat[3] * D;
    inv[0] = A11; inv[1] = A12; inv[2] = -A11 * mat[2] - A12 * mat[5];
    inv[3] = A21; inv[4] = A22; inv[5] = -A21 * mat[2] - A22 * mat[5];
    return 0;
}

static short ip_sat_short(float v) {                         // saturate_cast<short>(float): cvRound (ties to even), saturated
    const long r = lrintf(v);
    return (short)(r < -32768 ? -32768 : r > 32767 ? 32767 : r);
}

// cv::initInterTab2D(method, fixpt = true) for INTER_LINEAR ([1024][4]) and INTER_CUBIC ([1024][16]): entry fy*32 + fx, tap
// ky*ksize + kx.  The sum correction looks at the 2x2 window that starts at tap (ksize/2, ksize/2), like the original - for
// the bilinear table that window lies in the entries that follow (not yet filled: zero).
static void ip_table(int ksize, const float (*c1d)[4], short* out) {
    const int n = 32 * 32, kk = ksize * ksize;
    short* buf = (short*)calloc((size_t)n * kk + 4 * ksize + 4, sizeof(short));
    for (int i = 0; i < 32; ++i)
        for (int j = 0; j < 32; ++j) {
            short* it = buf + (size_t)(i * 32 + j) * kk;
            int isum = 0;
            for (int k1 = 0; k1 < ksize; ++k1)
                for (int k2 = 0; k2 < ksize; ++k2) {
                    const volatile float v = c1d[i][k1] * c1d[j][k2];
                    const volatile float vs = v * 32768.0f;
                    it[k1 * ksize + k2] = ip_sat_short(vs);
                    isum += it[k1 * ksize + k2];
                }
            if (isum != 32768) {
                const int diff = isum - 32768, k0 = ksize / 2;
                int Mk1 = k0, Mk2 = k0, mk1 = k0, mk2 = k0;
                for (int k1 = k0; k1 < k0 + 2; ++k1)
                    for (int k2 = k0; k2 < k0 + 2; ++k2) {
                        if (it[k1 * ksize + k2] < it[mk1 * ksize + mk2]) { mk1 = k1; mk2 = k2; }
                        else if (it[k1 * ksize + k2] > it[Mk1 * ksize + Mk2]) { Mk1 = k1; Mk2 = k2; }
                    }
                if (diff < 0) it[Mk1 * ksize + Mk2] = (short)(it[Mk1 * ksize + Mk2] - diff);
                else it[mk1 * ksize + mk2] = (short)(it[mk1 * ksize + mk2] - diff);
            }
        }
    memcpy(out, buf, (size_t)n * kk * sizeof(short));
    free(buf);
}

extern "C" int cris_remap_tables_u8(short* tab_linear, short* tab_cubic) {
    CRIS_CHECK_ARG(tab_linear && tab_cubic, "bad args");
    static float lin[32][4], cub[32][4];
    const volatile float A = -0.75f;                         // (volatile: every float operation separately rounded)
    for (int i = 0; i < 32; ++i) {
        const volatile float t = (float)i * (1.0f / 32.0f);
        lin[i][0] = 1.0f - t; lin[i][1] = t; lin[i][2] = lin[i][3] = 0.f;
        volatile float u = t + 1.0f, c0, c1, c2, q;
        q = A * u; q = q - 5.0f * A; q = q * u; q = q + 8.0f * A; q = q * u; c0 = q - 4.0f * A;
        q = (A + 2.0f) * t; q = q - (A + 3.0f); q = q * t; q = q * t; c1 = q + 1.0f;
        u = 1.0f - t;
        q = (A + 2.0f) * u; q = q - (A + 3.0f); q = q * u; q = q * u; c2 = q + 1.0f;
        q = 1.0f - c0; q = q - c1; q = q - c2;
        cub[i][0] = c0; cub[i][1] = c1; cub[i][2] = c2; cub[i][3] = q;
    }
    ip_table(2, lin, tab_linear);
    ip_table(4, cub, tab_cubic);
    return 0;
}
