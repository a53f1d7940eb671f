// Douglas-Peucker simplification of the traced rings on the device (the definition, its tie order and the 64-bit
// bound: simplify_core.h; the host restatement: polygon.simplify).  Input is what cris_polygon_trace left on the device - packed
// vertices, the ring table (descriptor, offset, length, 2 A) and the header - and nothing is read by the host in between: the
// ring count comes from the device header and the rings are distributed over the grids by strided loops.
//
// cris_polygon_simplify, 3 or 4 launches, none depending on the content:
//   1 sp_select<64>   one wave (a block of 64) per ring of at most SP_WAVE_RING vertices
//   2 sp_select<256>  one block per longer ring (launched when the batch has more than SP_WAVE_RING vertices)
//                     Both: stage the ring as one word per position 0 .. k (x, y and two flag bits; position k is v_0 again) in LDS
//                     while k <= SP_LDS_RING, in the ring's slice of a global plane of the work buffer otherwise; find the
//                     anchor; then rounds until one keeps nothing.  A thread owns a contiguous chunk of positions.  Per round:
//                       A  the owner turns last round's winners into kept vertices, clears the key slot of every kept vertex
//                          and the block scans the last / first kept position of the chunks: every chunk learns the kept
//                          position before and after it
//                       C  every run of unkept positions reduces its keys and sends one integer max to the slot of its
//                          segment's first vertex
//                       D  the owner of a segment's first vertex reads the slot, applies the split test and marks the winner
//                     Every round but the last keeps at least one vertex, so the loop ends.  Then the kept vertices are
//                     counted, ranked (exclusive scan) and 2 A of the kept ring is summed; a ring left with fewer than 3 counts 0.
//   3 sp_offsets      one block: exclusive scan of the per-ring counts (removed rings count 0) to new ring rows and vertex
//                     offsets; rings and vertices of the result to the output header
//   4 sp_compact      one wave per ring: kept vertex p goes to offset + rank[p], lane 0 writes the row (descriptor, offset,
//                     length, 2 A of the simplified ring, hole flag of the traced ring)
// Integers only.  Every word has one writer per launch phase, except the key slots and the anchor slot, which receive integer
// maxima (atomicMax: the result does not depend on the order), and the round's "something was kept" word, to which every
// writer stores 1.  Every cross-block dependency is a kernel boundary, no block waits for another: the same words on every
// run.  Every store is guarded by the capacity the host passed, every index read from scratch is clamped, and every scratch word
// is written before it is read, so a rerun over dirty scratch gives the same output.  The traced vertices and table are only read.
#include "common.h"
#include "simplify_core.h"
#include "../../../include/cris_hip.h"

#define SP_WAVE_RING 256       // rings of at most this many vertices take one wave
#define SP_LDS_RING 4096       // rings of at most this many vertices are staged in LDS (12 bytes per position: 48 KiB of the CU's 160)
#define SP_KEPT 0x80000000u    // the flag bits of a staged word: x in bits 0 .. 14, y in bits 16 .. 30
#define SP_NEW 0x00008000u     // won this round's split test: kept from the next round on
#define SP_RING_WORDS 4        // per ring in the work buffer: kept count, 2 A, rounds, (row << 32) + offset
#define SP_HEADER_WORDS 4      // rings, vertices, traced rings, the rounds of the deepest ring
#define SP_ROW_WORDS 5

__device__ __forceinline__ int sp_x(unsigned w) { return (int)(w & 0x7fffu); }
__device__ __forceinline__ int sp_y(unsigned w) { return (int)((w >> 16) & 0x7fffu); }

// exclusive scan of `v` over the G threads of the block, forwards (thread t gets op over the threads before it) or backwards
// (over the threads after it); *total = op over all.  lds: G / 64 words, free again on return.  Called by every thread.
template <int G, bool REV, typename T, typename Op>
__device__ __forceinline__ T sp_scan_excl(T v, T ident, T* lds, Op op, T* total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T u = REV ? __shfl_down(v, o, 64) : __shfl_up(v, o, 64);
        if (REV ? lane + o < 64 : lane >= o) v = op(v, u);
    }
    T mine = REV ? __shfl_down(v, 1, 64) : __shfl_up(v, 1, 64);
    if (lane == (REV ? 63 : 0)) mine = ident;
    T carry = ident, tot;
    if (G > 64) {
        if (lane == (REV ? 0 : 63)) lds[wv] = v;
        __syncthreads();
        tot = ident;
#pragma unroll
        for (int j = 0; j < G / 64; ++j) {
            const T s = lds[j];
            if (REV ? j > wv : j < wv) carry = op(carry, s);
            tot = op(tot, s);
        }
        __syncthreads();
    } else {
        tot = __shfl(v, REV ? 0 : 63, 64);
    }
    *total = tot;
    return op(carry, mine);
}

struct sp_max_op { template <typename T> __device__ T operator()(T a, T b) const { return a > b ? a : b; } };
struct sp_min_op { template <typename T> __device__ T operator()(T a, T b) const { return a < b ? a : b; } };
struct sp_add_op { template <typename T> __device__ T operator()(T a, T b) const { return a + b; } };

// Launches 1 and 2.  Visibility: the kernel boundary towards the trace; inside a block every phase ends at a __syncthreads, which
// orders LDS and - for a ring staged in the global plane, whose slice only this block touches - global memory for the block.
// per_ring, rank: written for the rings this launch owns only (the two launches own disjoint rings).
template <int G>
__global__ __launch_bounds__(G) void sp_select_kernel(const long long* __restrict__ header, const int* __restrict__ verts, long long total,
                                                      const long long* __restrict__ rings, long long ring_cap, int q,
                                                      long long* __restrict__ per_ring, int* __restrict__ rank,
                                                      unsigned* __restrict__ plane_w, unsigned long long* __restrict__ plane_b) {
    constexpr int CAP = G == 64 ? SP_WAVE_RING : SP_LDS_RING;
    __shared__ unsigned s_w[CAP + 1];
    __shared__ unsigned long long s_b[CAP + 1];
    __shared__ unsigned long long s_key;
    __shared__ int s_any;
    __shared__ long long s_scan[G / 64];
    int* s_scan_i = reinterpret_cast<int*>(s_scan);
    const int tid = (int)threadIdx.x;
    long long count = header[0];
    count = count < 0 ? 0 : count > ring_cap ? ring_cap : count;
    for (long long r = blockIdx.x; r < count; r += gridDim.x) {
        const long long off = rings[4 * r + 1], len = rings[4 * r + 2];
        const bool ok = off >= 0 && len >= 4 && len <= total && off <= total - len;
        if ((G == 64) != (!ok || len <= SP_WAVE_RING)) continue;           // the other launch's ring (a bad row: the wave launch's)
        if (!ok) {                                                        // no such ring among the vertices: removed
            if (tid == 0) per_ring[SP_RING_WORDS * r] = per_ring[SP_RING_WORDS * r + 1] = per_ring[SP_RING_WORDS * r + 2] = 0;
            continue;
        }
        const int k = (int)len;
        unsigned* W = k <= CAP ? s_w : plane_w + off + r;                 // k + 1 positions: rings before this one took off + r
        unsigned long long* B = k <= CAP ? s_b : plane_b + off + r;
        const int* __restrict__ V = verts + 2 * off;
        const int x0 = V[0] & 0x7fff, y0 = V[1] & 0x7fff;
        unsigned long long far = 0;
        for (int p = tid; p <= k; p += G) {                               // stage; the anchor's key on the way
            const int s = p == k ? 0 : p, x = V[2 * s] & 0x7fff, y = V[2 * s + 1] & 0x7fff;
            W[p] = (unsigned)x | ((unsigned)y << 16) | (p == 0 || p == k ? SP_KEPT : 0u);
            if (p < k) {
                const unsigned long long key = sp_anchor_key(sp_len2(x0, y0, x, y), p);
                far = key > far ? key : far;
            }
        }
        if (tid == 0) s_key = 0;
        __syncthreads();
        atomicMax(&s_key, far);
        __syncthreads();
        int a = (int)sp_anchor_index(s_key);
        a = a < 1 ? 1 : a > k - 1 ? k - 1 : a;
        if (tid == 0) W[a] |= SP_KEPT;
        __syncthreads();
        const int chunk = (k + 1 + G - 1) / G;
        const int lo = min(tid * chunk, k + 1), hi = min(lo + chunk, k + 1);
        int prev = -1, next = k + 1, rounds = 0;
        for (;;) {
            // A
            int last = -1, first = k + 1, unused;
            for (int p = lo; p < hi; ++p) {
                unsigned w = W[p];
                if (w & SP_NEW) W[p] = w = (w & ~SP_NEW) | SP_KEPT;
                if (w & SP_KEPT) {
                    first = first > k ? p : first;
                    last = p;
                    B[p] = 0;
                }
            }
            if (tid == 0) s_any = 0;
            prev = sp_scan_excl<G, false>(last, -1, s_scan_i, sp_max_op(), &unused);
            next = sp_scan_excl<G, true>(first, k + 1, s_scan_i, sp_min_op(), &unused);
            __syncthreads();
            // C
            int i = prev;
            for (int p = lo; p < hi;) {
                if (W[p] & SP_KEPT) {
                    i = p++;
                    continue;
                }
                int e = p;
                while (e < hi && !(W[e] & SP_KEPT)) ++e;
                const int j = e < hi ? e : next;
                if (i >= 0 && j <= k && j - i >= 2) {
                    const unsigned wi = W[i], wj = W[j];
                    unsigned long long best = 0;
                    for (int m = p; m < e; ++m) {
                        const unsigned wm = W[m];
                        const unsigned long long key = sp_key(sp_cross(sp_x(wi), sp_y(wi), sp_x(wj), sp_y(wj), sp_x(wm), sp_y(wm)), i, j, m);
                        best = key > best ? key : best;
                    }
                    atomicMax(&B[i], best);
                }
                p = e;
            }
            __syncthreads();
            // D
            bool any = false;
            int j = next;
            for (int p = hi - 1; p >= lo; --p) {
                const unsigned wp = W[p];
                if (!(wp & SP_KEPT)) continue;
                if (j <= k && j - p >= 2) {
                    const unsigned long long key = B[p];
                    const long long c = sp_key_cross(key), m = sp_key_index(key, p, j);
                    if (c > 0 && m > p && m < j) {
                        const unsigned wj = W[j];
                        if (sp_split(c, q, sp_len2(sp_x(wp), sp_y(wp), sp_x(wj), sp_y(wj)))) {
                            W[m] = W[m] | SP_NEW;                         // m is unkept and inside this segment alone: one writer
                            any = true;
                        }
                    }
                }
                j = p;
            }
            if (any) s_any = 1;
            __syncthreads();
            const int go = s_any;
            __syncthreads();
            ++rounds;
            if (!go) break;
        }
        // the last round kept nothing: prev / next are those of the final flags
        long long mine = 0, area = 0, kept, area2;
        int j = next;
        for (int p = hi - 1; p >= lo; --p) {
            const unsigned wp = W[p];
            if (!(wp & SP_KEPT)) continue;
            if (p < k && j <= k) {
                const unsigned wj = W[j];
                ++mine;
                area += (long long)sp_x(wp) * sp_y(wj) - (long long)sp_x(wj) * sp_y(wp);
            }
            j = p;
        }
        long long at = sp_scan_excl<G, false>(mine, 0ll, s_scan, sp_add_op(), &kept);
        sp_scan_excl<G, false>(area, 0ll, s_scan, sp_add_op(), &area2);
        const bool stays = kept >= 3;
        for (int p = lo; p < hi && p < k; ++p) rank[off + p] = stays && (W[p] & SP_KEPT) ? (int)at++ : -1;
        if (tid == 0) {
            per_ring[SP_RING_WORDS * r] = stays ? kept : 0;
            per_ring[SP_RING_WORDS * r + 1] = stays ? area2 : 0;
            per_ring[SP_RING_WORDS * r + 2] = rounds;
        }
        __syncthreads();                                                  // the LDS is staged again for the block's next ring
    }
}

// Launch 3.  Visibility: the kernel boundary (both select launches).  One block; (rows << 32) + vertices scanned at once: the
// vertices of a batch are < 2^31, so the low word never carries.
__global__ __launch_bounds__(256) void sp_offsets_kernel(const long long* __restrict__ header, long long ring_cap, long long* __restrict__ per_ring,
                                                         long long* __restrict__ out_header) {
    __shared__ long long lds[4];
    long long count = header[0];
    count = count < 0 ? 0 : count > ring_cap ? ring_cap : count;
    long long carry = 0;
    int deepest = 0;
    for (long long base = 0; base < count; base += 256) {
        const long long r = base + threadIdx.x;
        long long v = 0, tot;
        if (r < count) {
            const long long kept = per_ring[SP_RING_WORDS * r];
            v = kept >= 3 ? (1ll << 32) + kept : 0;
            const long long rounds = per_ring[SP_RING_WORDS * r + 2];
            deepest = max(deepest, (int)(rounds < 0 ? 0 : rounds > 0x7fffffff ? 0x7fffffff : rounds));
        }
        const long long before = sp_scan_excl<256, false>(v, 0ll, lds, sp_add_op(), &tot);
        if (r < count) per_ring[SP_RING_WORDS * r + 3] = carry + before;
        carry += tot;
    }
    int all;
    sp_scan_excl<256, false>(deepest, 0, reinterpret_cast<int*>(lds), sp_max_op(), &all);
    if (threadIdx.x == 0) {
        out_header[0] = carry >> 32;
        out_header[1] = carry & 0xffffffffll;
        out_header[2] = count;
        out_header[3] = all;
    }
}

// Launch 4.  Visibility: the kernel boundary (the offsets).  One wave per ring; a vertex has one writer, a row lane 0 of its wave.
__global__ __launch_bounds__(256) void sp_compact_kernel(const long long* __restrict__ header, const int* __restrict__ verts, long long total,
                                                         const long long* __restrict__ rings, long long ring_cap,
                                                         const long long* __restrict__ per_ring, const int* __restrict__ rank,
                                                         int* __restrict__ out_verts, size_t out_vertex_cap, long long* __restrict__ out_rings,
                                                         size_t out_ring_cap) {
    const int lane = threadIdx.x & 63;
    long long count = header[0];
    count = count < 0 ? 0 : count > ring_cap ? ring_cap : count;
    for (long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); r < count; r += (long long)gridDim.x * 4) {
        const long long kept = per_ring[SP_RING_WORDS * r];
        const long long off = rings[4 * r + 1], len = rings[4 * r + 2];
        if (kept < 3 || !(off >= 0 && len >= 4 && len <= total && off <= total - len)) continue;
        const long long place = per_ring[SP_RING_WORDS * r + 3], row = place >> 32, at = place & 0xffffffffll;
        for (long long p = lane; p < len; p += 64) {
            const long long rk = rank[off + p], o = at + rk;
            if (rk >= 0 && rk < kept && o >= 0 && (size_t)o < out_vertex_cap) {
                out_verts[2 * o] = verts[2 * (off + p)];
                out_verts[2 * o + 1] = verts[2 * (off + p) + 1];
            }
        }
        if (lane == 0 && row >= 0 && (size_t)row < out_ring_cap) {
            out_rings[SP_ROW_WORDS * row] = rings[4 * r];
            out_rings[SP_ROW_WORDS * row + 1] = at;
            out_rings[SP_ROW_WORDS * row + 2] = kept;
            out_rings[SP_ROW_WORDS * row + 3] = per_ring[SP_RING_WORDS * r + 1];
            out_rings[SP_ROW_WORDS * row + 4] = rings[4 * r + 3] < 0;
        }
    }
}

static size_t sp_round8(size_t b) { return (b + 7) & ~(size_t)7; }

// the work buffer: [ring_cap x 4 64-bit words per ring][total ranks][total + ring_cap staged words][total + ring_cap 64-bit key slots]
extern "C" size_t cris_polygon_simplify_work_bytes(long long total_vertices, long long ring_cap) {
    if (total_vertices < 4 || total_vertices > (1ll << 30) || ring_cap < 1 || ring_cap > (1ll << 28)) return 0;
    const size_t v = (size_t)total_vertices, r = (size_t)ring_cap;
    return 8 * SP_RING_WORDS * r + sp_round8(4 * v) + sp_round8(4 * (v + r)) + 8 * (v + r);
}

extern "C" int cris_polygon_simplify(const int* vertices, const long long* rings, const long long* header, long long total_vertices,
                                     long long ring_cap, int q, const cris_eval_desc* descs_host, int n, void* work, size_t work_bytes,
                                     int* out_vertices, size_t out_vertex_cap, long long* out_rings, size_t out_ring_cap,
                                     long long* out_header, void* stream) {
    CRIS_CHECK_ARG(vertices && rings && header && descs_host && work && out_vertices && out_rings && out_header, "null operand");
    CRIS_CHECK_ARG(((uintptr_t)rings & 7) == 0 && ((uintptr_t)header & 7) == 0 && ((uintptr_t)work & 7) == 0 && ((uintptr_t)out_rings & 7) == 0 &&
                       ((uintptr_t)out_header & 7) == 0 && ((uintptr_t)vertices & 3) == 0 && ((uintptr_t)out_vertices & 3) == 0,
                   "rings, header, work, out_rings and out_header must be 8-byte, vertices and out_vertices 4-byte aligned");
    CRIS_CHECK_ARG(q >= 1 && q <= SP_MAX_Q, "q = 4 * epsilon must be in 1 .. 256");
    CRIS_CHECK_ARG(total_vertices >= 4 && total_vertices <= (1ll << 30), "total_vertices must be in 4 .. 2^30");
    CRIS_CHECK_ARG(ring_cap >= 1 && ring_cap <= (1ll << 28), "ring_cap must be in 1 .. 2^28");
    CRIS_CHECK_ARG(n > 0 && n <= 65535, "n must be in 1 .. 65535");
    for (int i = 0; i < n; ++i)
        CRIS_CHECK_ARG(descs_host[i].h_out >= 1 && descs_host[i].w_out >= 1 && descs_host[i].h_out <= SP_MAX_SIDE && descs_host[i].w_out <= SP_MAX_SIDE,
                       "descriptor: h_out and w_out must be in 1 .. 32767 (the 64-bit bound of the split test)");
    CRIS_CHECK_ARG(work_bytes >= cris_polygon_simplify_work_bytes(total_vertices, ring_cap), "the work buffer is too small");
    CRIS_CHECK_ARG(out_vertex_cap >= (size_t)total_vertices && out_ring_cap >= (size_t)ring_cap,
                   "out_vertex_cap must be >= total_vertices and out_ring_cap >= ring_cap");
    const size_t v = (size_t)total_vertices, r = (size_t)ring_cap;
    char* w = reinterpret_cast<char*>(work);
    long long* per_ring = reinterpret_cast<long long*>(w);
    int* rank = reinterpret_cast<int*>(w + 8 * SP_RING_WORDS * r);
    unsigned* plane_w = reinterpret_cast<unsigned*>(w + 8 * SP_RING_WORDS * r + sp_round8(4 * v));
    unsigned long long* plane_b = reinterpret_cast<unsigned long long*>(w + 8 * SP_RING_WORDS * r + sp_round8(4 * v) + sp_round8(4 * (v + r)));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sp_select_kernel<64>, dim3(cris_grid_1d((long)ring_cap, 1, 4096)), dim3(64), 0, st, header, vertices, total_vertices, rings,
                       ring_cap, q, per_ring, rank, plane_w, plane_b);
    CRIS_LAUNCH_CHECK();
    if (total_vertices > SP_WAVE_RING) {                                    // a longer ring can exist
        const long longer = (long)(total_vertices / (SP_WAVE_RING + 2));
        hipLaunchKernelGGL(sp_select_kernel<256>, dim3(cris_grid_1d(longer < (long)ring_cap ? longer : (long)ring_cap, 1, 1024)), dim3(256), 0, st,
                           header, vertices, total_vertices, rings, ring_cap, q, per_ring, rank, plane_w, plane_b);
        CRIS_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(sp_offsets_kernel, dim3(1), dim3(256), 0, st, header, ring_cap, per_ring, out_header);
    CRIS_LAUNCH_CHECK();
    hipLaunchKernelGGL(sp_compact_kernel, dim3(cris_grid_1d((long)ring_cap, 4, 2048)), dim3(256), 0, st, header, vertices, total_vertices, rings,
                       ring_cap, (const long long*)per_ring, (const int*)rank, out_vertices, out_vertex_cap, out_rings, out_ring_cap);
    CRIS_LAUNCH_CHECK();
    return 0;
}
