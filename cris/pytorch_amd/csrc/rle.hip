// COCO run-length encoding of the packed masks on the device: the transition positions of every descriptor's mask
// in column-major order, packed contiguously; the host turns them into counts and the compressed string (cris/pytorch_amd/rle.py).
//
// The masks are the bytes cris_predict_masks_batch / cris_eval_iou_batch / cris_filter_components leave (descriptor d at d.out_off,
// d.h_out rows of d.pitch bytes).  A pixel is foreground iff its byte is != 0 and x < w_out: no lane ever owns a column >= w_out, so
// the pitch padding is never read as a pixel.  With i = x * h + y, v(i) the foreground bit and v(-1) = 0, the positions P are the
// ascending i with v(i) != v(i - 1): the predecessor of (x, y > 0) is the pixel above, of (x > 0, 0) it is (x - 1, h - 1), of (0, 0)
// the constant 0.  counts = diff([0] + P + [h * w]) on the host.
//
// A mask is cut into segments (column x, band k of RLE_RB rows), numbered in column-major order s = x * nb + k, which is the order of
// the positions themselves.  Four launches, none depending on the content, no block waits for another, integers only, no atomics:
//   1 rle_count    one wave per (RLE_CG adjacent columns, band): lane = column, the lanes walk down the band's rows together (every
//                  row read is contiguous across the wave); work[d * stride + s] = transitions of the segment
//   2 rle_scan     one block per descriptor: exclusive scan of its w * nb counts in place, the sum to totals[d]
//   3 rle_totals   one block: exclusive scan of totals[0 .. n) to the packed bases, the sum to totals[n]
//   4 rle_write    the geometry of launch 1: each lane walks its segment again and stores x * h + y at base + offset + rank when that
//                  index is < run_words
// Every cross-block dependency is a kernel boundary.  The work buffer gives every descriptor `stride` = max over the batch of
// w * nb words, so a block finds its slot from blockIdx.y alone (descriptors may alias one rectangle: their slots do not).
#include "common.h"
#include "../../../include/cris_hip.h"

#define RLE_RB 32          // rows of a band
#define RLE_CG 64          // columns of a block: one wave, one column per lane

// the transitions of segment (x, band k) in order: f(y) is called for every y of the band with v(x, y) != v(predecessor)
template <typename F>
__device__ __forceinline__ void rle_walk(const unsigned char* __restrict__ M, const cris_eval_desc& d, int x, int k, F f) {
    const int y0 = k * RLE_RB, y1 = min(d.h_out, y0 + RLE_RB);
    bool prev = false;
    if (y0 > 0) prev = M[(size_t)(y0 - 1) * d.pitch + x] != 0;
    else if (x > 0) prev = M[(size_t)(d.h_out - 1) * d.pitch + (x - 1)] != 0;
    for (int y = y0; y < y1; ++y) {
        const bool cur = M[(size_t)y * d.pitch + x] != 0;
        if (cur != prev) f(y);
        prev = cur;
    }
}

// Launch 1.  Visibility: the kernel boundary - the mask bytes are the previous launch's; every work word has one writer.
// blockIdx.y = descriptor, blockIdx.x strides over its (column group, band) tiles.
__global__ __launch_bounds__(RLE_CG) void rle_count_kernel(const unsigned char* __restrict__ masks, const cris_eval_desc* __restrict__ descs,
                                                           size_t stride, int* __restrict__ work) {
    const cris_eval_desc d = descs[blockIdx.y];
    const unsigned char* __restrict__ M = masks + d.out_off;
    const int nb = (d.h_out + RLE_RB - 1) / RLE_RB, ncg = (d.w_out + RLE_CG - 1) / RLE_CG;
    int* __restrict__ seg = work + (size_t)blockIdx.y * stride;
    for (long t = blockIdx.x; t < (long)ncg * nb; t += gridDim.x) {
        const int x = (int)(t / nb) * RLE_CG + (int)threadIdx.x, k = (int)(t % nb);
        if (x >= d.w_out) continue;
        int cnt = 0;
        rle_walk(M, d, x, k, [&](int) { ++cnt; });
        seg[(size_t)x * nb + k] = cnt;
    }
}

// inclusive scan over the 256 threads of a block; *total = the block's sum.  lds: 4 words, free again on return
template <typename T>
__device__ __forceinline__ T rle_block_scan(T v, T* lds, T* total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    if (lane == 63) lds[wv] = v;
    __syncthreads();
    T add = 0, tot = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const T s = lds[j];
        if (j < wv) add += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return v + add;
}

// Launch 2.  Visibility: the kernel boundary (launch 1 wrote the counts); block d alone reads and writes descriptor d's slot and
// totals[d].  A segment's count is at most RLE_RB and a descriptor's sum at most h * w < 2^31: int.
__global__ __launch_bounds__(256) void rle_scan_kernel(const cris_eval_desc* __restrict__ descs, size_t stride, int* __restrict__ work,
                                                       long long* __restrict__ totals) {
    __shared__ int lds[4];
    const cris_eval_desc d = descs[blockIdx.x];
    const long segs = (long)d.w_out * ((d.h_out + RLE_RB - 1) / RLE_RB);
    int* __restrict__ seg = work + (size_t)blockIdx.x * stride;
    int carry = 0;
    for (long base = 0; base < segs; base += 256) {
        const long s = base + threadIdx.x;
        const int v = s < segs ? seg[s] : 0;
        int tot;
        const int incl = rle_block_scan(v, lds, &tot);
        if (s < segs) seg[s] = carry + incl - v;
        carry += tot;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

// Launch 3.  Visibility: the kernel boundary (launch 2 wrote totals[0 .. n)); one block.  bases[d] = sum of totals[< d], totals[n] = all.
__global__ __launch_bounds__(256) void rle_totals_kernel(int n, long long* __restrict__ totals, long long* __restrict__ bases) {
    __shared__ long long lds[4];
    long long carry = 0;
    for (int base = 0; base < n; base += 256) {
        const int i = base + (int)threadIdx.x;
        const long long v = i < n ? totals[i] : 0;
        long long tot;
        const long long incl = rle_block_scan(v, lds, &tot);
        if (i < n) bases[i] = carry + incl - v;
        carry += tot;
    }
    if (threadIdx.x == 0) totals[n] = carry;
}

// Launch 4.  Visibility: the kernel boundary (offsets and bases are complete).  The geometry of launch 1; the k-th transition of a
// segment lands at bases[d] + offset[s] + k, so the packed list ascends within a descriptor.  A store happens only below run_words.
__global__ __launch_bounds__(RLE_CG) void rle_write_kernel(const unsigned char* __restrict__ masks, const cris_eval_desc* __restrict__ descs,
                                                           size_t stride, const int* __restrict__ work, const long long* __restrict__ bases,
                                                           unsigned* __restrict__ runs, size_t run_words) {
    const cris_eval_desc d = descs[blockIdx.y];
    const unsigned char* __restrict__ M = masks + d.out_off;
    const int nb = (d.h_out + RLE_RB - 1) / RLE_RB, ncg = (d.w_out + RLE_CG - 1) / RLE_CG;
    const int* __restrict__ seg = work + (size_t)blockIdx.y * stride;
    const size_t first = (size_t)bases[blockIdx.y];
    for (long t = blockIdx.x; t < (long)ncg * nb; t += gridDim.x) {
        const int x = (int)(t / nb) * RLE_CG + (int)threadIdx.x, k = (int)(t % nb);
        if (x >= d.w_out) continue;
        size_t at = first + (size_t)seg[(size_t)x * nb + k];
        const unsigned col = (unsigned)x * (unsigned)d.h_out;               // x * h + y < h * w < 2^31
        rle_walk(M, d, x, k, [&](int y) {
            if (at < run_words) runs[at] = col + (unsigned)y;
            ++at;
        });
    }
}

// what both entry points read from the host copy of the descriptors: every address the kernels form.  *stride = max w * nb,
// *tiles = max (column groups * bands)
static const char* rle_check_descs(const cris_eval_desc* descs_host, int n, size_t mask_bytes, size_t* stride, long* tiles) {
    *stride = 0;
    *tiles = 0;
    for (int i = 0; i < n; ++i) {
        const cris_eval_desc& d = descs_host[i];
        if (!(d.w_out > 0 && d.h_out > 0 && (long)d.w_out * d.h_out < (1L << 31))) return "descriptor: bad output size";
        if (!(d.pitch >= d.w_out && (d.pitch & 3) == 0 && (long)d.pitch * d.h_out < (1L << 31)))
            return "descriptor: the pitch must be a multiple of 4, >= w_out, pitch * h_out < 2^31";
        if (!(d.out_off >= 0 && (size_t)d.out_off + (size_t)d.pitch * d.h_out <= mask_bytes)) return "descriptor: output outside the buffer";
        const long nb = (d.h_out + RLE_RB - 1) / RLE_RB, ncg = (d.w_out + RLE_CG - 1) / RLE_CG;
        if ((size_t)(d.w_out * nb) > *stride) *stride = (size_t)(d.w_out * nb);
        if (ncg * nb > *tiles) *tiles = ncg * nb;
    }
    return nullptr;
}

static size_t rle_seg_bytes(size_t stride, int n) { return ((size_t)n * stride * 4 + 7) & ~(size_t)7; }

extern "C" size_t cris_rle_work_bytes(const cris_eval_desc* descs_host, int n) {
    if (!descs_host || n <= 0 || n > 65535) return 0;
    size_t stride = 0;
    for (int i = 0; i < n; ++i) {                                           // (bad descriptors count nothing: cris_rle_encode names them)
        const cris_eval_desc& d = descs_host[i];
        if (!(d.w_out > 0 && d.h_out > 0 && (long)d.w_out * d.h_out < (1L << 31))) continue;
        const size_t segs = (size_t)d.w_out * (size_t)((d.h_out + RLE_RB - 1) / RLE_RB);
        if (segs > stride) stride = segs;
    }
    return rle_seg_bytes(stride, n) + 8 * (size_t)n;
}

extern "C" int cris_rle_encode(const unsigned char* masks, size_t mask_bytes, const cris_eval_desc* descs_host,
                               const cris_eval_desc* descs_dev, int n, void* work, size_t work_bytes, unsigned* runs, size_t run_words,
                               long long* totals, void* stream) {
    CRIS_CHECK_ARG(masks && descs_host && descs_dev && work && runs && totals, "null operand");
    CRIS_CHECK_ARG(n > 0 && n <= 65535, "n must be in 1 .. 65535");
    CRIS_CHECK_ARG(((uintptr_t)work & 7) == 0 && ((uintptr_t)runs & 3) == 0 && ((uintptr_t)totals & 7) == 0,
                   "work and totals must be 8-byte, runs 4-byte aligned");
    size_t stride = 0;
    long tiles = 0;
    const char* bad = rle_check_descs(descs_host, n, mask_bytes, &stride, &tiles);
    CRIS_CHECK_ARG(!bad, bad);
    CRIS_CHECK_ARG(work_bytes >= rle_seg_bytes(stride, n) + 8 * (size_t)n, "the work buffer is too small");
    int* seg = reinterpret_cast<int*>(work);
    long long* bases = reinterpret_cast<long long*>(reinterpret_cast<char*>(work) + rle_seg_bytes(stride, n));
    const int cap = 8192 / n > 32 ? 8192 / n : 32;                  // one-wave blocks: four times the block count of the 256-thread grids
    const dim3 grid(cris_grid_1d(tiles, 1, cap), n);
    hipLaunchKernelGGL(rle_count_kernel, grid, dim3(RLE_CG), 0, (hipStream_t)stream, masks, descs_dev, stride, seg);
    CRIS_LAUNCH_CHECK();
    hipLaunchKernelGGL(rle_scan_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, descs_dev, stride, seg, totals);
    CRIS_LAUNCH_CHECK();
    hipLaunchKernelGGL(rle_totals_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, n, totals, bases);
    CRIS_LAUNCH_CHECK();
    hipLaunchKernelGGL(rle_write_kernel, grid, dim3(RLE_CG), 0, (hipStream_t)stream, masks, descs_dev, stride, (const int*)seg,
                       (const long long*)bases, runs, run_words);
    CRIS_LAUNCH_CHECK();
    return 0;
}
