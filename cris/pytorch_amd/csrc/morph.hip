// Square-structuring-element erosion of the packed masks and the boundary counts built on it: Boundary IoU
// (Cheng et al., CVPR 2021) for the evaluator, and the morphology of the mask tool set: cris_morph_masks, further down, chains
// erosions and dilations over the same planes (opening, closing).
//
// The masks are the bytes cris_eval_iou_batch / cris_predict_masks_batch / cris_filter_components leave (descriptor i at d.out_off,
// d.h_out rows of d.pitch bytes) and, for the ground truth, the staging's packed masks (d.mask_off, the same pitch).  A pixel is
// foreground iff its byte is != 0 and x < w_out: no lane ever owns a column >= w_out, so the pitch padding is never read as a pixel.
// With the radius r of descriptor i (radii[i], computed on the host; the device reads integers)
//     E_r(M)[y, x] = 1 iff every pixel of [y - r, y + r] x [x - r, x + r] lies inside the image and is foreground
//     B_r(M) = M & ~E_r(M)                      counts[d.row] += (|B_r(P) & B_r(G)|, |B_r(P) | B_r(G)|)
//
// A mask becomes a bit plane in `work`: h rows of wpr = ceil(w / 64) words, bit i of word c = pixel 64 c + i, the bits at x >= w
// zero.  Every descriptor gets `stride` = max over the batch of h * wpr words per plane, so a block finds its slot from blockIdx.y
// alone (descriptors may alias one rectangle: their slots do not).  Three launches, none depending on the content, no block waits
// for another, integers only:
//   1 morph_pack    one wave per plane word: lane = pixel, a wave64 __ballot turns 64 bytes into the word (prediction and ground
//                   truth in one launch)
//   2 morph_row     one thread per word: the window AND of 2 r + 1 bits along x (morph_core.h: shift-and-AND doubling inside the
//                   word, the nearest 0 within ceil(r / 64) words on either side beyond it)
//   3 morph_count   one thread per (row pair, word column): the AND of the row-eroded words of rows y - r .. y + r for both masks,
//                   m & ~e, __popcll of the AND and of the OR, a wave + LDS reduction and ONE integer atomic pair per block
//     morph_unpack  (cris_erode_masks instead of 3) one wave per (row pair, word column): the same words, lane = pixel, bytes 0 / 255
// Every cross-block dependency is a kernel boundary: launch 1 has read every source byte before launch 3 writes one, which is why
// cris_erode_masks may run in place.  Every plane word a launch reads was written by the launch before it: `work` need not be zeroed.
#include "common.h"
#include "../../../include/cris_hip.h"
#include "morph_core.h"

typedef unsigned long long morph_word;      // (uint64_t of morph_core.h; what __ballot returns)

__device__ __forceinline__ int morph_wpr(const cris_eval_desc& d) { return (d.w_out + 63) >> 6; }

// Launch 1.  Visibility: the kernel boundary - the mask bytes are earlier launches' (or an upload's); every plane word has one writer.
// blockIdx.y = descriptor; the waves of blockIdx.x stride over its h * wpr words.  b == nullptr: one plane.
__global__ __launch_bounds__(256) void morph_pack_kernel(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b,
                                                         const cris_eval_desc* __restrict__ descs, size_t stride, morph_word* __restrict__ pa,
                                                         morph_word* __restrict__ pb) {
    const cris_eval_desc d = descs[blockIdx.y];
    const int wpr = morph_wpr(d), lane = threadIdx.x & 63;
    const long words = (long)d.h_out * wpr;
    const unsigned char* __restrict__ A = a + d.out_off;
    const unsigned char* __restrict__ B = b ? b + d.mask_off : nullptr;
    const size_t slot = (size_t)blockIdx.y * stride;
    for (long t = (long)blockIdx.x * 4 + (threadIdx.x >> 6); t < words; t += (long)gridDim.x * 4) {          // (wave-uniform)
        const int y = (int)(t / wpr), x = (int)(t % wpr) * 64 + lane;
        const size_t at = (size_t)y * d.pitch + x;
        const bool in = x < d.w_out;
        const morph_word wa = __ballot(in && A[at] != 0);
        if (lane == 0) pa[slot + t] = wa;
        if (B) {
            const morph_word wb = __ballot(in && B[at] != 0);
            if (lane == 0) pb[slot + t] = wb;
        }
    }
}

// Launch 2.  Visibility: the kernel boundary (launch 1 wrote the raw planes).  blockIdx.y = descriptor, blockIdx.z = plane; a thread
// reads words of its own row of its own slot only and writes one word of the row-eroded plane.
__global__ __launch_bounds__(256) void morph_row_kernel(const cris_eval_desc* __restrict__ descs, const int* __restrict__ radii, size_t stride,
                                                        size_t plane_words, const morph_word* __restrict__ raw, morph_word* __restrict__ rowp) {
    const cris_eval_desc d = descs[blockIdx.y];
    const int r = radii[blockIdx.y], wpr = morph_wpr(d);
    const bool empty = morph_empty(d.h_out, d.w_out, r);
    const long words = (long)d.h_out * wpr;
    const size_t slot = (size_t)blockIdx.z * plane_words + (size_t)blockIdx.y * stride;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < words; t += (long)gridDim.x * blockDim.x) {
        const long y = t / wpr;
        const int c = (int)(t % wpr);
        rowp[slot + t] = empty ? 0ull : morph_row_word(reinterpret_cast<const uint64_t*>(raw + slot + (size_t)y * wpr), wpr, c, r);
    }
}

// sum over the 256 threads of a block, valid in thread 0.  lds: 4 words
__device__ __forceinline__ int morph_block_sum(int v, int* lds) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return lds[0] + lds[1] + lds[2] + lds[3];
}

// Launch 3 of cris_boundary_iou_batch.  Visibility: the kernel boundary (launches 1 and 2 wrote all four planes).  The bits at
// x >= w are 0 in the raw planes, hence in both boundaries.  Integer atomics after the block's reduction: exact and order-free.
__global__ __launch_bounds__(256) void morph_count_kernel(const cris_eval_desc* __restrict__ descs, const int* __restrict__ radii, size_t stride,
                                                          size_t plane_words, const morph_word* __restrict__ raw,
                                                          const morph_word* __restrict__ rowp, int* __restrict__ counts) {
    __shared__ int red[2][4];
    const cris_eval_desc d = descs[blockIdx.y];
    const int r = radii[blockIdx.y], wpr = morph_wpr(d), h = d.h_out;
    const bool empty = morph_empty(h, d.w_out, r);
    const long items = (long)((h + 1) >> 1) * wpr;
    const size_t slot = (size_t)blockIdx.y * stride;
    const morph_word* __restrict__ mp = raw + slot;
    const morph_word* __restrict__ mg = raw + plane_words + slot;
    const uint64_t* __restrict__ rp = reinterpret_cast<const uint64_t*>(rowp + slot);
    const uint64_t* __restrict__ rg = reinterpret_cast<const uint64_t*>(rowp + plane_words + slot);
    int inter = 0, uni = 0;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < items; t += (long)gridDim.x * blockDim.x) {
        const int y0 = (int)(t / wpr) * 2, c = (int)(t % wpr);
        uint64_t ep0 = 0, ep1 = 0, eg0 = 0, eg1 = 0;
        if (!empty) {
            morph_col_pair(rp, wpr, h, y0, c, r, &ep0, &ep1);
            morph_col_pair(rg, wpr, h, y0, c, r, &eg0, &eg1);
        }
        const size_t at = (size_t)y0 * wpr + c;
        const morph_word bp0 = mp[at] & ~ep0, bg0 = mg[at] & ~eg0;
        inter += __popcll(bp0 & bg0);
        uni += __popcll(bp0 | bg0);
        if (y0 + 1 < h) {
            const morph_word bp1 = mp[at + wpr] & ~ep1, bg1 = mg[at + wpr] & ~eg1;
            inter += __popcll(bp1 & bg1);
            uni += __popcll(bp1 | bg1);
        }
    }
    const int is = morph_block_sum(inter, red[0]), us = morph_block_sum(uni, red[1]);
    if (threadIdx.x == 0 && us) {
        atomicAdd(counts + 2 * (size_t)d.row, is);
        atomicAdd(counts + 2 * (size_t)d.row + 1, us);
    }
}

// Launch 3 of cris_erode_masks.  Visibility: the kernel boundary.  One wave per (row pair, word column): its lanes form the same
// two words (wave-uniform loads) and lane i stores the byte of pixel 64 c + i when that is < w_out - nothing else of `out` is written.
__global__ __launch_bounds__(256) void morph_unpack_kernel(const cris_eval_desc* __restrict__ descs, const int* __restrict__ radii, size_t stride,
                                                           const morph_word* __restrict__ raw, const morph_word* __restrict__ rowp, int boundary,
                                                           unsigned char* __restrict__ out) {
    const cris_eval_desc d = descs[blockIdx.y];
    const int r = radii[blockIdx.y], wpr = morph_wpr(d), h = d.h_out, lane = threadIdx.x & 63;
    const bool empty = morph_empty(h, d.w_out, r);
    const long items = (long)((h + 1) >> 1) * wpr;
    const size_t slot = (size_t)blockIdx.y * stride;
    const uint64_t* __restrict__ rp = reinterpret_cast<const uint64_t*>(rowp + slot);
    unsigned char* __restrict__ O = out + d.out_off;
    for (long t = (long)blockIdx.x * 4 + (threadIdx.x >> 6); t < items; t += (long)gridDim.x * 4) {           // (wave-uniform)
        const int y0 = (int)(t / wpr) * 2, c = (int)(t % wpr), x = c * 64 + lane;
        uint64_t e0 = 0, e1 = 0;
        if (!empty) morph_col_pair(rp, wpr, h, y0, c, r, &e0, &e1);
        if (x >= d.w_out) continue;
        const size_t at = (size_t)y0 * wpr + c;
        const morph_word v0 = boundary ? raw[slot + at] & ~e0 : e0;
        O[(size_t)y0 * d.pitch + x] = (v0 >> lane) & 1ull ? 255 : 0;
        if (y0 + 1 < h) {
            const morph_word v1 = boundary ? raw[slot + at + wpr] & ~e1 : e1;
            O[(size_t)(y0 + 1) * d.pitch + x] = (v1 >> lane) & 1ull ? 255 : 0;
        }
    }
}

// what both entry points read from the host copies, before any launch: every address the kernels form.  *stride = max h * wpr
static const char* morph_check(const cris_eval_desc* descs_host, const int* radii_host, int n, size_t out_bytes, int rows, bool gt, size_t gt_bytes,
                               size_t* stride) {
    *stride = 0;
    for (int i = 0; i < n; ++i) {
        const cris_eval_desc& d = descs_host[i];
        if (!(d.w_out > 0 && d.h_out > 0 && (long)d.w_out * d.h_out < (1L << 31))) return "descriptor: bad output size";
        if (!(d.pitch >= d.w_out && (d.pitch & 3) == 0 && (long)d.pitch * d.h_out < (1L << 31)))
            return "descriptor: the pitch must be a multiple of 4, >= w_out, pitch * h_out < 2^31";
        const size_t bytes = (size_t)d.pitch * d.h_out;
        if (!(d.out_off >= 0 && (size_t)d.out_off + bytes <= out_bytes)) return "descriptor: output outside the buffer";
        if (rows >= 0 && !(d.row >= 0 && d.row < rows)) return "descriptor: row out of range";
        if (gt && !(d.mask_off >= 0 && (size_t)d.mask_off + bytes <= gt_bytes)) return "descriptor: mask outside the buffer";
        if (radii_host[i] < 1) return "every radius must be >= 1";
        const size_t words = (size_t)d.h_out * (size_t)((d.w_out + 63) >> 6);
        if (words > *stride) *stride = words;
    }
    return nullptr;
}

extern "C" size_t cris_boundary_work_bytes(const cris_eval_desc* descs_host, int n) {
    if (!descs_host || n <= 0 || n > 65535) return 0;
    size_t stride = 0;
    for (int i = 0; i < n; ++i) {                                           // (bad descriptors count nothing: the launchers name them)
        const cris_eval_desc& d = descs_host[i];
        if (!(d.w_out > 0 && d.h_out > 0 && (long)d.w_out * d.h_out < (1L << 31))) continue;
        const size_t words = (size_t)d.h_out * (size_t)((d.w_out + 63) >> 6);
        if (words > stride) stride = words;
    }
    return 4 * 8 * (size_t)n * stride;
}

static dim3 morph_grid(size_t stride, int per_block, int n, int z = 1) {
    const int cap = 2048 / n > 8 ? 2048 / n : 8;                            // the grid of cris_eval_iou_batch
    return dim3(cris_grid_1d((long)stride, per_block, cap), n, z);
}

extern "C" int cris_erode_masks(const unsigned char* masks, size_t mask_bytes, const cris_eval_desc* descs_host, const cris_eval_desc* descs_dev,
                                int n, const int* radii_host, const int* radii_dev, void* work, size_t work_bytes, unsigned char* out,
                                size_t out_bytes, int boundary, void* stream) {
    CRIS_CHECK_ARG(masks && descs_host && descs_dev && radii_host && radii_dev && work && out, "null operand");
    CRIS_CHECK_ARG(n > 0 && n <= 65535, "n must be in 1 .. 65535");
    CRIS_CHECK_ARG(boundary == 0 || boundary == 1, "boundary must be 0 or 1");
    CRIS_CHECK_ARG(((uintptr_t)work & 7) == 0 && ((uintptr_t)radii_dev & 3) == 0, "work must be 8-byte, radii 4-byte aligned");
    size_t stride = 0;
    const char* bad = morph_check(descs_host, radii_host, n, mask_bytes < out_bytes ? mask_bytes : out_bytes, -1, false, 0, &stride);
    CRIS_CHECK_ARG(!bad, bad);
    const size_t plane = (size_t)n * stride;                               // words of one plane of the batch
    CRIS_CHECK_ARG(work_bytes >= 2 * 8 * plane, "the work buffer is too small");
    morph_word* raw = reinterpret_cast<morph_word*>(work);
    morph_word* rowp = raw + plane;
    hipLaunchKernelGGL(morph_pack_kernel, morph_grid(stride, 4, n), dim3(256), 0, (hipStream_t)stream, masks, (const unsigned char*)nullptr,
                       descs_dev, stride, raw, (morph_word*)nullptr);
    CRIS_LAUNCH_CHECK();
    hipLaunchKernelGGL(morph_row_kernel, morph_grid(stride, 256, n), dim3(256), 0, (hipStream_t)stream, descs_dev, radii_dev, stride, plane,
                       (const morph_word*)raw, rowp);
    CRIS_LAUNCH_CHECK();
    hipLaunchKernelGGL(morph_unpack_kernel, morph_grid((stride + 1) / 2, 4, n), dim3(256), 0, (hipStream_t)stream, descs_dev, radii_dev, stride,
                       (const morph_word*)raw, (const morph_word*)rowp, boundary, out);
    CRIS_LAUNCH_CHECK();
    return 0;
}

// ---- chained operations on the planes: dilation, clipped erosion, and with them opening and closing ----
// cris_morph_masks packs once (launch 1 above), runs per operation one row pass A -> B and one column pass B -> A over the two planes
// of `work`, and stores the bytes once.  Every launch reads only what the launch before it wrote, in its own descriptor's slot.

// Row pass of operation `op` (CRIS_MORPH_ERODE / DILATE / ERODE_CLIPPED; uniform over the launch).  Visibility: the kernel boundary.
// One thread per word: it reads words of its own row of `src` and writes one word of `dst`.
__global__ __launch_bounds__(256) void morph_row_op_kernel(const cris_eval_desc* __restrict__ descs, const int* __restrict__ radii, int op,
                                                           size_t stride, const morph_word* __restrict__ src, morph_word* __restrict__ dst) {
    const cris_eval_desc d = descs[blockIdx.y];
    const int r = radii[blockIdx.y], wpr = morph_wpr(d);
    const bool empty = morph_empty(d.h_out, d.w_out, r);
    const long words = (long)d.h_out * wpr;
    const size_t slot = (size_t)blockIdx.y * stride;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < words; t += (long)gridDim.x * blockDim.x) {
        const long y = t / wpr;
        const int c = (int)(t % wpr);
        const uint64_t* row = reinterpret_cast<const uint64_t*>(src + slot + (size_t)y * wpr);
        dst[slot + t] = op == CRIS_MORPH_ERODE ? (empty ? 0ull : morph_row_word(row, wpr, c, r))
                                               : morph_row_or_word(row, wpr, d.w_out, c, r, op == CRIS_MORPH_ERODE_CLIPPED);
    }
}

// Column pass of operation `op`.  Visibility: the kernel boundary (the row pass wrote every word of `rowp` this launch reads).  One
// thread per (row pair, word column): it reads words of its column of `rowp` and writes the two words of `dst` - another plane, so no
// thread reads what a thread of this launch writes.
__global__ __launch_bounds__(256) void morph_col_op_kernel(const cris_eval_desc* __restrict__ descs, const int* __restrict__ radii, int op,
                                                           size_t stride, const morph_word* __restrict__ rowp, morph_word* __restrict__ dst) {
    const cris_eval_desc d = descs[blockIdx.y];
    const int r = radii[blockIdx.y], wpr = morph_wpr(d), h = d.h_out;
    const bool empty = morph_empty(h, d.w_out, r);
    const long items = (long)((h + 1) >> 1) * wpr;
    const size_t slot = (size_t)blockIdx.y * stride;
    const uint64_t* __restrict__ rp = reinterpret_cast<const uint64_t*>(rowp + slot);
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < items; t += (long)gridDim.x * blockDim.x) {
        const int y0 = (int)(t / wpr) * 2, c = (int)(t % wpr);
        uint64_t e0 = 0, e1 = 0;
        if (op == CRIS_MORPH_DILATE) morph_col_pair_or(rp, wpr, h, y0, c, r, &e0, &e1);
        else if (op == CRIS_MORPH_ERODE_CLIPPED) morph_col_pair_and_clipped(rp, wpr, h, y0, c, r, &e0, &e1);
        else if (!empty) morph_col_pair(rp, wpr, h, y0, c, r, &e0, &e1);
        const size_t at = slot + (size_t)y0 * wpr + c;
        dst[at] = e0;
        if (y0 + 1 < h) dst[at + wpr] = e1;
    }
}

// The last launch of cris_morph_masks.  Visibility: the kernel boundary.  One wave per plane word (the walk of launch 1): lane i
// stores the byte of pixel 64 c + i when that is < w_out - nothing else of `out` is written.
__global__ __launch_bounds__(256) void morph_store_kernel(const cris_eval_desc* __restrict__ descs, size_t stride, const morph_word* __restrict__ plane,
                                                          unsigned char* __restrict__ out) {
    const cris_eval_desc d = descs[blockIdx.y];
    const int wpr = morph_wpr(d), lane = threadIdx.x & 63;
    const long words = (long)d.h_out * wpr;
    const size_t slot = (size_t)blockIdx.y * stride;
    unsigned char* __restrict__ O = out + d.out_off;
    for (long t = (long)blockIdx.x * 4 + (threadIdx.x >> 6); t < words; t += (long)gridDim.x * 4) {           // (wave-uniform)
        const int y = (int)(t / wpr), x = (int)(t % wpr) * 64 + lane;
        if (x >= d.w_out) continue;
        O[(size_t)y * d.pitch + x] = (plane[slot + t] >> lane) & 1ull ? 255 : 0;
    }
}

extern "C" int cris_morph_masks(const unsigned char* masks, size_t mask_bytes, const cris_eval_desc* descs_host, const cris_eval_desc* descs_dev,
                                int n, const int* ops_host, int n_ops, const int* radii_host, const int* radii_dev, void* work, size_t work_bytes,
                                unsigned char* out, size_t out_bytes, void* stream) {
    CRIS_CHECK_ARG(masks && descs_host && descs_dev && ops_host && radii_host && radii_dev && work && out, "null operand");
    CRIS_CHECK_ARG(n > 0 && n <= 65535, "n must be in 1 .. 65535");
    CRIS_CHECK_ARG(n_ops >= 1 && n_ops <= CRIS_MORPH_MAX_OPS, "n_ops must be in 1 .. 8");
    CRIS_CHECK_ARG(((uintptr_t)work & 7) == 0 && ((uintptr_t)radii_dev & 3) == 0, "work must be 8-byte, radii 4-byte aligned");
    for (int k = 0; k < n_ops; ++k) {
        CRIS_CHECK_ARG(ops_host[k] == CRIS_MORPH_ERODE || ops_host[k] == CRIS_MORPH_DILATE || ops_host[k] == CRIS_MORPH_ERODE_CLIPPED,
                       "every operation must be 0 (erode), 1 (dilate) or 2 (clipped erode)");
        for (int i = 0; i < n; ++i)
            CRIS_CHECK_ARG(radii_host[(size_t)k * n + i] >= 1 && radii_host[(size_t)k * n + i] <= 65535, "every radius must be in 1 .. 65535");
    }
    size_t stride = 0;
    const char* bad = morph_check(descs_host, radii_host, n, mask_bytes < out_bytes ? mask_bytes : out_bytes, -1, false, 0, &stride);
    CRIS_CHECK_ARG(!bad, bad);
    const size_t plane = (size_t)n * stride;                               // words of one plane of the batch
    CRIS_CHECK_ARG(work_bytes >= 2 * 8 * plane, "the work buffer is too small");
    morph_word* pa = reinterpret_cast<morph_word*>(work);                   // the masks, and the result of every operation
    morph_word* pb = pa + plane;                                            // the row pass of the operation under way
    hipLaunchKernelGGL(morph_pack_kernel, morph_grid(stride, 4, n), dim3(256), 0, (hipStream_t)stream, masks, (const unsigned char*)nullptr,
                       descs_dev, stride, pa, (morph_word*)nullptr);
    CRIS_LAUNCH_CHECK();
    for (int k = 0; k < n_ops; ++k) {
        hipLaunchKernelGGL(morph_row_op_kernel, morph_grid(stride, 256, n), dim3(256), 0, (hipStream_t)stream, descs_dev,
                           radii_dev + (size_t)k * n, ops_host[k], stride, (const morph_word*)pa, pb);
        CRIS_LAUNCH_CHECK();
        hipLaunchKernelGGL(morph_col_op_kernel, morph_grid((stride + 1) / 2, 256, n), dim3(256), 0, (hipStream_t)stream, descs_dev,
                           radii_dev + (size_t)k * n, ops_host[k], stride, (const morph_word*)pb, pa);
        CRIS_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(morph_store_kernel, morph_grid(stride, 4, n), dim3(256), 0, (hipStream_t)stream, descs_dev, stride, (const morph_word*)pa,
                       out);
    CRIS_LAUNCH_CHECK();
    return 0;
}

extern "C" int cris_boundary_iou_batch(const unsigned char* pred, size_t pred_bytes, const cris_eval_desc* descs_host,
                                       const cris_eval_desc* descs_dev, int n, const unsigned char* gt, size_t gt_bytes, const int* radii_host,
                                       const int* radii_dev, void* work, size_t work_bytes, int* counts, int count_rows, void* stream) {
    CRIS_CHECK_ARG(pred && descs_host && descs_dev && gt && radii_host && radii_dev && work && counts, "null operand");
    CRIS_CHECK_ARG(n > 0 && n <= 65535, "n must be in 1 .. 65535");
    CRIS_CHECK_ARG(count_rows > 0, "bad sizes");
    CRIS_CHECK_ARG(((uintptr_t)work & 7) == 0 && ((uintptr_t)radii_dev & 3) == 0 && ((uintptr_t)counts & 3) == 0,
                   "work must be 8-byte, radii and counts 4-byte aligned");
    size_t stride = 0;
    const char* bad = morph_check(descs_host, radii_host, n, pred_bytes, count_rows, true, gt_bytes, &stride);
    CRIS_CHECK_ARG(!bad, bad);
    const size_t plane = (size_t)n * stride;
    CRIS_CHECK_ARG(work_bytes >= 4 * 8 * plane, "the work buffer is too small");
    morph_word* raw = reinterpret_cast<morph_word*>(work);                  // [prediction | ground truth]
    morph_word* rowp = raw + 2 * plane;                                     // the same two, eroded along x
    hipLaunchKernelGGL(morph_pack_kernel, morph_grid(stride, 4, n), dim3(256), 0, (hipStream_t)stream, pred, gt, descs_dev, stride, raw,
                       raw + plane);
    CRIS_LAUNCH_CHECK();
    hipLaunchKernelGGL(morph_row_kernel, morph_grid(stride, 256, n, 2), dim3(256), 0, (hipStream_t)stream, descs_dev, radii_dev, stride, plane,
                       (const morph_word*)raw, rowp);
    CRIS_LAUNCH_CHECK();
    hipLaunchKernelGGL(morph_count_kernel, morph_grid((stride + 1) / 2, 256, n), dim3(256), 0, (hipStream_t)stream, descs_dev, radii_dev, stride,
                       plane, (const morph_word*)raw, (const morph_word*)rowp, counts);
    CRIS_LAUNCH_CHECK();
    return 0;
}
