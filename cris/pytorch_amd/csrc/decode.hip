// Encoded masks decoded on the device: the inverse of csrc/rle.hip and of csrc/polygon.hip / csrc/simplify.hip.  A table
// of cris_mask_src rows names one mask each - where it goes (dst_off, pitch, h, w), where its payload lies and which kind it is - and
// the two entry points write, for the rows of their kind, h rows of pitch bytes: 0 / 255 at x < w, 0 at w <= x < pitch, the bytes
// EvalStaging.pack would have uploaded.  Nothing else is written: not the gap to the next slot, not the tail of the buffer, and no
// slot of a row of the other kind.  rle.decode / polygon.decode are the definitions; decode_core.h holds the arithmetic.
//
// cris_rle_decode, two launches:
//   1 decode_scan     one block per mask: inclusive scan of its counts (uint32, COCO order) into run ends, in its work slot; chunks of
//                     256 with a carry, as rle_scan_kernel
//   2 decode_store    one thread per dword of the slot (4 adjacent pixels of a row): pixel (x, y) is foreground iff the number of run
//                     ends <= x * h + y is odd - an upper-bound search, the next pixel's starts where the last one ended
// cris_polygon_fill, one memset and two launches:
//   0 hipMemsetAsync  the work buffer: every mask's bit plane (h rows of ceil(w / 64) 64-bit words, morph.hip's layout) is zero
//   1 decode_toggle   one thread per vertex = per edge to the ring's next vertex: for every centre line the edge crosses, bit px of
//                     that row's words flips (atomicXor, 64-bit integer: any order gives the same plane); px = w flips nothing
//   2 decode_store    the same geometry as above: bit x of a row's inclusive prefix parity - a shift-XOR doubling inside the word and
//                     the popcount parity of the row's earlier words - is the pixel
// Every cross-block dependency is a kernel boundary (the memset is a stream operation like a launch); no block waits for another.
// Integers only; the only atomics are the XORs, which commute: the same bytes on every run.  blockIdx.y (blockIdx.x of the scan) is
// the mask, and its work slot is blockIdx.y * stride words, stride the maximum over the whole table, so both entry points may share
// one work buffer on one stream.  A thread writes only dwords of its own slot at offsets the host has checked; the payload decides
// values, never addresses: counts that do not sum to h * w or vertices outside the image cannot cause a write outside the slot
// (rows are clamped to [0, h), px to [0, w]).  The payload is only read.
#include "common.h"
#include "../../../include/cris_hip.h"
#include "decode_core.h"

#define DEC_T 256

// inclusive scan over the 256 threads of a block; *total = the block's sum.  lds: 4 words, free again on return
__device__ __forceinline__ unsigned dec_block_scan(unsigned v, unsigned* lds, unsigned* total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    if (lane == 63) lds[wv] = v;
    __syncthreads();
    unsigned add = 0, tot = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned s = lds[j];
        if (j < wv) add += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return v + add;
}

// RLE launch 1.  Visibility: the kernel boundary - the counts are an earlier copy's; block m alone writes mask m's slot.
__global__ __launch_bounds__(DEC_T) void decode_scan_kernel(const cris_mask_src* __restrict__ srcs, const unsigned* __restrict__ counts,
                                                            size_t stride, unsigned long long* __restrict__ work) {
    __shared__ unsigned lds[4];
    const cris_mask_src s = srcs[blockIdx.x];
    if (s.kind != CRIS_MASK_RLE) return;
    const unsigned* __restrict__ c = counts + s.pay_off;
    unsigned* __restrict__ ends = reinterpret_cast<unsigned*>(work + (size_t)blockIdx.x * stride);
    unsigned carry = 0;
    for (int base = 0; base < s.pay_len; base += DEC_T) {
        const int j = base + (int)threadIdx.x;
        const unsigned v = j < s.pay_len ? c[j] : 0u;
        unsigned tot;
        const unsigned incl = dec_block_scan(v, lds, &tot);
        if (j < s.pay_len) ends[j] = carry + incl;
        carry += tot;
    }
}

// Polygon launch 1.  Visibility: the stream order - the memset zeroed the planes, the vertices and rings are an earlier copy's; the
// XORs are device-scope atomics on words no other kind of access touches during this launch.
__global__ __launch_bounds__(DEC_T) void decode_toggle_kernel(const cris_mask_src* __restrict__ srcs, const int2* __restrict__ vertices,
                                                              const long long* __restrict__ rings, int ring_stride, size_t stride,
                                                              unsigned long long* __restrict__ work) {
    const cris_mask_src s = srcs[blockIdx.y];
    if (s.kind != CRIS_MASK_POLYGON || s.pay_len <= 0) return;
    const long first = s.pay_off, last = first + s.pay_len - 1;
    const long long v0 = rings[(size_t)first * ring_stride + 1];
    const long long nv = rings[(size_t)last * ring_stride + 1] + rings[(size_t)last * ring_stride + 2] - v0;
    unsigned long long* __restrict__ plane = work + (size_t)blockIdx.y * stride;
    const int wpr = (s.w + 63) >> 6;
    for (long long j = (long long)blockIdx.x * DEC_T + threadIdx.x; j < nv; j += (long long)gridDim.x * DEC_T) {
        const long long g = v0 + j;
        const long r = decode_ring_of(rings, ring_stride, first, s.pay_len, g);
        const long long off = rings[(size_t)r * ring_stride + 1], len = rings[(size_t)r * ring_stride + 2];
        const int2 a = vertices[g], b = vertices[g + 1 < off + len ? g + 1 : off];
        decode_edge(a.x, a.y, b.x, b.y, s.h, s.w, [&](int px, int py) {    // 0 <= py < h, 0 <= px < w: a word of this mask's plane
            atomicXor(&plane[(size_t)py * wpr + (px >> 6)], 1ull << (px & 63));
        });
    }
}

// Launch 2 of both.  Visibility: the kernel boundary (the run ends / the planes are complete); every dword has one writer.
// blockIdx.y = mask, blockIdx.x strides over its h * pitch / 4 dwords; a block of another kind's mask leaves at once.
template <int KIND>
__global__ __launch_bounds__(DEC_T) void decode_store_kernel(const cris_mask_src* __restrict__ srcs, size_t stride,
                                                             const unsigned long long* __restrict__ work, unsigned char* __restrict__ out) {
    const cris_mask_src s = srcs[blockIdx.y];
    if (s.kind != KIND) return;
    const unsigned long long* __restrict__ slot = work + (size_t)blockIdx.y * stride;
    const int dpr = s.pitch >> 2, wpr = (s.w + 63) >> 6;
    unsigned* __restrict__ dst = reinterpret_cast<unsigned*>(out + s.dst_off);
    const long items = (long)s.h * dpr;
    for (long t = (long)blockIdx.x * DEC_T + threadIdx.x; t < items; t += (long)gridDim.x * DEC_T) {
        const int y = (int)(t / dpr), x = (int)(t % dpr) * 4;
        const unsigned bits = KIND == CRIS_MASK_RLE ? decode_rle_bits(reinterpret_cast<const uint32_t*>(slot), s.pay_len, s.h, s.w, x, y)
                                                    : decode_plane_bits(slot + (size_t)y * wpr, s.w, x);
        dst[t] = decode_bytes(bits);                                    // t < h * pitch / 4: a dword of this mask's slot
    }
}

// what both entry points read from the host copy of the table: every address the kernels form that does not depend on `kind`'s
// payload.  *stride = 64-bit words of a work slot, *items = max dwords of a slot of kind `kind`, *any = rows of that kind
static const char* dec_check_srcs(const cris_mask_src* srcs_host, int n, size_t out_bytes, int kind, size_t* stride, long* items, int* any) {
    *stride = 1;
    *items = 0;
    *any = 0;
    for (int i = 0; i < n; ++i) {
        const cris_mask_src& s = srcs_host[i];
        if (!(s.kind == CRIS_MASK_RLE || s.kind == CRIS_MASK_POLYGON)) return "mask source: kind must be CRIS_MASK_RLE or CRIS_MASK_POLYGON";
        if (!(s.w > 0 && s.h > 0 && (long)s.w * s.h < (1L << 31))) return "mask source: bad size";
        if (s.kind == CRIS_MASK_POLYGON && !((long)(s.w + 1) * (s.h + 1) <= (1L << 28))) return "mask source: (h + 1) * (w + 1) of a polygon mask must be <= 2^28";
        if (!(s.pitch >= s.w && (s.pitch & 3) == 0 && (long)s.pitch * s.h < (1L << 31)))
            return "mask source: the pitch must be a multiple of 4, >= w, pitch * h < 2^31";
        if (!(s.dst_off >= 0 && (s.dst_off & 3) == 0 && (size_t)s.dst_off + (size_t)s.pitch * s.h <= out_bytes))
            return "mask source: slot outside the buffer (or not 4-byte aligned)";
        if (!(s.pay_off >= 0 && s.pay_len >= 0)) return "mask source: negative payload offset or length";
        const size_t words = s.kind == CRIS_MASK_RLE ? ((size_t)s.pay_len + 1) / 2 : (size_t)s.h * (size_t)((s.w + 63) >> 6);
        if (words > *stride) *stride = words;
        if (s.kind == kind) {
            *any = 1;
            const long it = (long)s.h * (s.pitch >> 2);
            if (it > *items) *items = it;
        }
    }
    return nullptr;
}

extern "C" size_t cris_mask_decode_work_bytes(const cris_mask_src* srcs_host, int n) {
    if (!srcs_host || n <= 0 || n > 65535) return 0;
    size_t stride = 1;
    for (int i = 0; i < n; ++i) {                                           // (bad rows count nothing: the launchers name them)
        const cris_mask_src& s = srcs_host[i];
        if (!(s.w > 0 && s.h > 0 && (long)s.w * s.h < (1L << 31) && s.pay_len >= 0)) continue;
        const size_t words = s.kind == CRIS_MASK_RLE ? ((size_t)s.pay_len + 1) / 2 : (size_t)s.h * (size_t)((s.w + 63) >> 6);
        if (words > stride) stride = words;
    }
    return (size_t)n * stride * 8;
}

static dim3 dec_store_grid(long items, int n) {
    const int cap = 8192 / n > 32 ? 8192 / n : 32;
    return dim3(cris_grid_1d(items, DEC_T, cap), n);
}

extern "C" int cris_rle_decode(const cris_mask_src* srcs_host, const cris_mask_src* srcs_dev, int n, const unsigned* counts,
                               size_t count_words, void* work, size_t work_bytes, unsigned char* out, size_t out_bytes, void* stream) {
    CRIS_CHECK_ARG(srcs_host && srcs_dev && counts && work && out, "null operand");
    CRIS_CHECK_ARG(n > 0 && n <= 65535, "n must be in 1 .. 65535");
    CRIS_CHECK_ARG(((uintptr_t)work & 7) == 0 && ((uintptr_t)counts & 3) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)srcs_dev & 7) == 0,
                   "work and the table must be 8-byte, counts and out 4-byte aligned");
    size_t stride = 0;
    long items = 0;
    int any = 0;
    const char* bad = dec_check_srcs(srcs_host, n, out_bytes, CRIS_MASK_RLE, &stride, &items, &any);
    CRIS_CHECK_ARG(!bad, bad);
    for (int i = 0; i < n; ++i)
        if (srcs_host[i].kind == CRIS_MASK_RLE)
            CRIS_CHECK_ARG((size_t)srcs_host[i].pay_off + (size_t)srcs_host[i].pay_len <= count_words, "mask source: counts outside the payload");
    CRIS_CHECK_ARG(work_bytes >= (size_t)n * stride * 8, "the work buffer is too small");
    if (!any) return 0;
    unsigned long long* w = reinterpret_cast<unsigned long long*>(work);
    hipLaunchKernelGGL(decode_scan_kernel, dim3(n), dim3(DEC_T), 0, (hipStream_t)stream, srcs_dev, counts, stride, w);
    CRIS_LAUNCH_CHECK();
    hipLaunchKernelGGL(decode_store_kernel<CRIS_MASK_RLE>, dec_store_grid(items, n), dim3(DEC_T), 0, (hipStream_t)stream, srcs_dev, stride,
                       (const unsigned long long*)w, out);
    CRIS_LAUNCH_CHECK();
    return 0;
}

extern "C" int cris_polygon_fill(const cris_mask_src* srcs_host, const cris_mask_src* srcs_dev, int n, const int* vertices, size_t vertex_pairs,
                                 const long long* rings_host, const long long* rings_dev, size_t ring_rows, int ring_stride, void* work,
                                 size_t work_bytes, unsigned char* out, size_t out_bytes, void* stream) {
    CRIS_CHECK_ARG(srcs_host && srcs_dev && vertices && rings_host && rings_dev && work && out, "null operand");
    CRIS_CHECK_ARG(n > 0 && n <= 65535, "n must be in 1 .. 65535");
    CRIS_CHECK_ARG(ring_stride >= 3 && ring_stride <= 8, "ring_stride must be in 3 .. 8 words");
    CRIS_CHECK_ARG(((uintptr_t)work & 7) == 0 && ((uintptr_t)vertices & 7) == 0 && ((uintptr_t)rings_dev & 7) == 0 && ((uintptr_t)out & 3) == 0 &&
                       ((uintptr_t)srcs_dev & 7) == 0,
                   "work, the table, vertices and rings must be 8-byte, out 4-byte aligned");
    size_t stride = 0;
    long items = 0;
    int any = 0;
    const char* bad = dec_check_srcs(srcs_host, n, out_bytes, CRIS_MASK_POLYGON, &stride, &items, &any);
    CRIS_CHECK_ARG(!bad, bad);
    long long most = 0;                                                     // vertices of the largest mask
    for (int i = 0; i < n; ++i) {
        const cris_mask_src& s = srcs_host[i];
        if (s.kind != CRIS_MASK_POLYGON) continue;
        CRIS_CHECK_ARG((size_t)s.pay_off + (size_t)s.pay_len <= ring_rows, "mask source: ring rows outside the table");
        long long next = -1, begin = 0;
        for (long r = s.pay_off; r < s.pay_off + s.pay_len; ++r) {          // the rows of a mask: its own, packed and ascending
            const long long* row = rings_host + (size_t)r * ring_stride;
            CRIS_CHECK_ARG(row[0] == i, "ring table: a row names another mask than the one that lists it");
            CRIS_CHECK_ARG(row[1] >= 0 && row[2] >= 1 && (size_t)row[1] + (size_t)row[2] <= vertex_pairs, "ring table: vertices outside the payload");
            CRIS_CHECK_ARG(next < 0 || row[1] == next, "ring table: the rings of a mask must follow each other in the vertex list");
            if (next < 0) begin = row[1];
            next = row[1] + row[2];
        }
        if (next - begin > most) most = next - begin;
    }
    CRIS_CHECK_ARG(work_bytes >= (size_t)n * stride * 8, "the work buffer is too small");
    if (!any) return 0;
    unsigned long long* w = reinterpret_cast<unsigned long long*>(work);
    const hipError_t e = hipMemsetAsync(w, 0, (size_t)n * stride * 8, (hipStream_t)stream);
    if (e != hipSuccess) {
        cris_set_error("%s: memset failed: %s", __func__, hipGetErrorString(e));
        return (int)e;
    }
    if (most > 0) {
        const int cap = 8192 / n > 32 ? 8192 / n : 32;
        hipLaunchKernelGGL(decode_toggle_kernel, dim3(cris_grid_1d(most, DEC_T, cap), n), dim3(DEC_T), 0, (hipStream_t)stream, srcs_dev,
                           reinterpret_cast<const int2*>(vertices), rings_dev, ring_stride, stride, w);
        CRIS_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(decode_store_kernel<CRIS_MASK_POLYGON>, dec_store_grid(items, n), dim3(DEC_T), 0, (hipStream_t)stream, srcs_dev, stride,
                       (const unsigned long long*)w, out);
    CRIS_LAUNCH_CHECK();
    return 0;
}
