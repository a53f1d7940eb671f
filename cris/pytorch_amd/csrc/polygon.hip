// Polygon tracing of the packed masks on the device: the rings of every descriptor's mask as ordered lists of the
// pixel corners at which the boundary turns, packed contiguously, plus one table row per ring; the host slices them into dicts
// (cris/pytorch_amd/polygon.py states the format).
//
// The masks are the bytes cris_predict_masks_batch / cris_filter_components / cris_fill_holes leave (descriptor d at d.out_off,
// d.h_out rows of d.pitch bytes).  A pixel is foreground iff its byte is != 0 and x < w_out, outside the image is background: no
// address at x >= w_out is ever formed, so the pitch padding is never read.  Vertices, cracks, corner visits and the turn-right
// rule are those of polygon_core.h.  Two facts carry the whole file (checked on the host against a per-crack follower):
//   - list the corner visits of a mask in row-major vertex order (a saddle's west copy first): entries 2 k and 2 k + 1 are the two
//     ends of one horizontal ring edge; in column-major order (north copy first) they are the two ends of one vertical edge;
//   - the smallest row-major index of a ring is its raster-first vertex, the start the format asks for.
// So the successor of visit i is its partner i ^ 1 in the list of the crack it leaves on (a mask's base is even: every per-mask
// total is even), and ring membership, the start and the rank follow by pointer jumping.
//
// cris_polygon_count, three launches in the shape of rle.hip (none depends on the content):
//   1 pg_count    one wave per tile of PG_CG vertex columns x PG_RB vertex rows: lane = column, the lanes walk down the rows
//                 together; per row the wave's visits go to the row segment (y, column group), per lane to the column segment
//                 (x, band) - the two segmentations the two lists need
//   2 pg_scan     one block per descriptor: exclusive scans of both arrays in place, the sum to totals[d]
//   3 pg_totals   one block: exclusive scan of totals[0 .. n) to the packed bases, the sum to totals[n]
// cris_polygon_trace, 7 + rounds launches, the host having read the totals:
//   4 pg_write    the walk of launch 1: R[i] (row-major) and C[j] (column-major), one word per visit
//   5 pg_link     succ0[i]: i ^ 1, or through C (two binary searches inside the mask's own range); label = i, dist = 0
//   6 pg_jump     x rounds, two buffers: (label, dist) = the smallest index among the next 2^r visits and the steps to its FIRST
//                 occurrence, succ = succ o succ.  A tie keeps the nearer one, so rounds beyond ceil(log2(ring length)) change nothing
//   7 pg_chunks   per chunk of PG_CHUNK visits: the ring starts in it and the sum of their ring lengths
//   8 pg_chunk_scan  one block: exclusive scan of the chunk sums; rings and vertices of the batch to the header
//   9 pg_bases    per chunk: ring index and ring base of every start (exclusive scan in raster order of the starts = ring order)
//  10 pg_scatter  vertex i to base[label] + rank; the start writes the ring's row (descriptor, offset, length)
//  11 pg_area     one wave per ring: 2 A = sum x_i y_i+1 - x_i+1 y_i over its now contiguous vertices
// Integers only, no atomics, every word has one writer per launch, every cross-block dependency is a kernel boundary, no block
// waits for another: the same words on every run.  Every store is guarded by the capacity the host passed and every index read
// from scratch is clamped into [0, total), whatever the scratch holds.
#include "common.h"
#include "polygon_core.h"
#include "../../../include/cris_hip.h"

#define PG_RB 32           // vertex rows of a band
#define PG_CG 64           // vertex columns of a tile: one wave, one column per lane
#define PG_CHUNK 1024      // visits per block of the ring-base scan (256 threads x 4)
#define PG_MAX_VERTS (1L << 28)     // (h + 1) * (w + 1) of a descriptor: a visit's key and its three bits fit one 32-bit word

struct pg_geom {
    int nb, ncg;
    __host__ __device__ pg_geom(int h, int w) : nb((h + 1 + PG_RB - 1) / PG_RB), ncg((w + 1 + PG_CG - 1) / PG_CG) {}
};

// f(x, y, a, b, c, d) for every vertex row y of band k, called by all 64 lanes together (x > w_out: all zero)
template <typename F>
__device__ __forceinline__ void pg_walk(const unsigned char* __restrict__ M, const cris_eval_desc& d, int g, int k, F f) {
    const int x = g * PG_CG + (int)threadIdx.x;
    const int y0 = k * PG_RB, y1 = min(d.h_out + 1, y0 + PG_RB);
    const bool left = x >= 1 && x <= d.w_out, right = x < d.w_out;        // pixel columns x - 1 and x exist
    int a = 0, b = 0;
    if (y0 > 0) {
        const unsigned char* row = M + (size_t)(y0 - 1) * d.pitch;
        a = left && row[x - 1] != 0;
        b = right && row[x] != 0;
    }
    for (int y = y0; y < y1; ++y) {
        int c = 0, e = 0;
        if (y < d.h_out) {
            const unsigned char* row = M + (size_t)y * d.pitch;
            c = left && row[x - 1] != 0;
            e = right && row[x] != 0;
        }
        f(x, y, a, b, c, e);
        a = c;
        b = e;
    }
}

// Launch 1.  Visibility: the kernel boundary - the mask bytes are the previous launch's; every work word has one writer.
__global__ __launch_bounds__(PG_CG) void pg_count_kernel(const unsigned char* __restrict__ masks, const cris_eval_desc* __restrict__ descs,
                                                         size_t stride_r, size_t stride_c, int* __restrict__ rows, int* __restrict__ cols) {
    const cris_eval_desc d = descs[blockIdx.y];
    const unsigned char* __restrict__ M = masks + d.out_off;
    const pg_geom G(d.h_out, d.w_out);
    int* __restrict__ rseg = rows + (size_t)blockIdx.y * stride_r;
    int* __restrict__ cseg = cols + (size_t)blockIdx.y * stride_c;
    for (long t = blockIdx.x; t < (long)G.ncg * G.nb; t += gridDim.x) {
        const int g = (int)(t / G.nb), k = (int)(t % G.nb);
        int mine = 0;
        pg_walk(M, d, g, k, [&](int, int y, int a, int b, int c, int e) {
            const int v = pg_visits(a, b, c, e);
            mine += v;
            const unsigned long long m1 = __ballot(v >= 1), m2 = __ballot(v == 2);
            if (threadIdx.x == 0) rseg[(size_t)y * G.ncg + g] = __popcll(m1) + __popcll(m2);
        });
        const int x = g * PG_CG + (int)threadIdx.x;
        if (x <= d.w_out) cseg[(size_t)x * G.nb + k] = mine;
    }
}

// inclusive scan over the 256 threads of a block; *total = the block's sum.  lds: 4 words, free again on return
template <typename T>
__device__ __forceinline__ T pg_block_scan(T v, T* lds, T* total) {
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

__device__ __forceinline__ int pg_scan_in_place(int* __restrict__ seg, long segs, int* lds) {
    int carry = 0;
    for (long base = 0; base < segs; base += 256) {
        const long s = base + threadIdx.x;
        const int v = s < segs ? seg[s] : 0;
        int tot;
        const int incl = pg_block_scan(v, lds, &tot);
        if (s < segs) seg[s] = carry + incl - v;
        carry += tot;
    }
    return carry;
}

// Launch 2.  Visibility: the kernel boundary (launch 1 wrote the counts); block d alone reads and writes descriptor d's two slots
// and totals[d].  A descriptor's sum is at most 2 (h + 1) (w + 1) <= 2^29: int.
__global__ __launch_bounds__(256) void pg_scan_kernel(const cris_eval_desc* __restrict__ descs, size_t stride_r, size_t stride_c,
                                                      int* __restrict__ rows, int* __restrict__ cols, long long* __restrict__ totals) {
    __shared__ int lds[4];
    const cris_eval_desc d = descs[blockIdx.x];
    const pg_geom G(d.h_out, d.w_out);
    const int sum = pg_scan_in_place(rows + (size_t)blockIdx.x * stride_r, (long)(d.h_out + 1) * G.ncg, lds);
    pg_scan_in_place(cols + (size_t)blockIdx.x * stride_c, (long)(d.w_out + 1) * G.nb, lds);
    if (threadIdx.x == 0) totals[blockIdx.x] = sum;
}

// Launch 3.  Visibility: the kernel boundary (launch 2 wrote totals[0 .. n)); one block.  bases[d] = sum of totals[< d], totals[n] = all.
__global__ __launch_bounds__(256) void pg_totals_kernel(int n, long long* __restrict__ totals, long long* __restrict__ bases) {
    __shared__ long long lds[4];
    long long carry = 0;
    for (int base = 0; base < n; base += 256) {
        const int i = base + (int)threadIdx.x;
        const long long v = i < n ? totals[i] : 0;
        long long tot;
        const long long incl = pg_block_scan(v, lds, &tot);
        if (i < n) bases[i] = carry + incl - v;
        carry += tot;
    }
    if (threadIdx.x == 0) totals[n] = carry;
}

// the two words of a visit.  R: ((y (w + 1) + x) 2 + he) 4 + vs 2 + outv, ascending in row-major order; C: ((x (h + 1) + y) 2 + vs) 2 + he,
// ascending in column-major order
__device__ __forceinline__ unsigned pg_r_word(const cris_eval_desc& d, int x, int y, int visit) {
    const unsigned key = ((unsigned)y * (unsigned)(d.w_out + 1) + (unsigned)x) * 2u + (visit & PG_HE ? 1u : 0u);
    return key * 4u + (visit & PG_VS ? 2u : 0u) + (visit & PG_OUTV ? 1u : 0u);
}
__device__ __forceinline__ unsigned pg_c_word(const cris_eval_desc& d, int x, int y, int visit) {
    const unsigned key = ((unsigned)x * (unsigned)(d.h_out + 1) + (unsigned)y) * 2u + (visit & PG_VS ? 1u : 0u);
    return key * 2u + (visit & PG_HE ? 1u : 0u);
}

// Launch 4.  Visibility: the kernel boundary (offsets and bases are complete).  The geometry of launch 1; a visit lands at
// bases[d] + offset of its segment + its rank in the segment, in both lists.  A store happens only below `total`.
__global__ __launch_bounds__(PG_CG) void pg_write_kernel(const unsigned char* __restrict__ masks, const cris_eval_desc* __restrict__ descs,
                                                         size_t stride_r, size_t stride_c, const int* __restrict__ rows,
                                                         const int* __restrict__ cols, const long long* __restrict__ bases,
                                                         unsigned* __restrict__ R, unsigned* __restrict__ C, long total) {
    const cris_eval_desc d = descs[blockIdx.y];
    const unsigned char* __restrict__ M = masks + d.out_off;
    const pg_geom G(d.h_out, d.w_out);
    const int* __restrict__ rseg = rows + (size_t)blockIdx.y * stride_r;
    const int* __restrict__ cseg = cols + (size_t)blockIdx.y * stride_c;
    const long first = (long)bases[blockIdx.y];
    const unsigned long long below = (1ull << threadIdx.x) - 1;
    for (long t = blockIdx.x; t < (long)G.ncg * G.nb; t += gridDim.x) {
        const int g = (int)(t / G.nb), k = (int)(t % G.nb);
        const int x0 = g * PG_CG + (int)threadIdx.x;
        long atc = x0 <= d.w_out ? first + cseg[(size_t)x0 * G.nb + k] : total;
        pg_walk(M, d, g, k, [&](int x, int y, int a, int b, int c, int e) {
            const int v = pg_visits(a, b, c, e);
            const unsigned long long m1 = __ballot(v >= 1), m2 = __ballot(v == 2);
            if (v == 0) return;
            long atr = first + rseg[(size_t)y * G.ncg + g] + __popcll(m1 & below) + __popcll(m2 & below);
            for (int j = 0; j < v; ++j, ++atr, ++atc) {
                if (atr >= 0 && atr < total) R[atr] = pg_r_word(d, x, y, pg_visit_row(a, b, c, e, j));
                if (atc >= 0 && atc < total) C[atc] = pg_c_word(d, x, y, pg_visit_col(a, b, c, e, j));
            }
        });
    }
}

// the index in list[lo .. hi) whose word >> shift is key (the lists ascend); lo when there is none - never outside [lo, hi)
__device__ __forceinline__ long pg_find(const unsigned* __restrict__ list, long lo, long hi, unsigned key, int shift) {
    long a = lo, b = hi;
    while (a < b) {
        const long m = a + (b - a) / 2;
        if ((list[m] >> shift) < key) a = m + 1;
        else b = m;
    }
    return a < hi ? a : lo;
}

// Launch 5.  Visibility: the kernel boundary (R and C are complete).  blockIdx.y = descriptor, the threads stride over its visits.
__global__ __launch_bounds__(256) void pg_link_kernel(const cris_eval_desc* __restrict__ descs, const long long* __restrict__ bases,
                                                      const long long* __restrict__ totals, const unsigned* __restrict__ R,
                                                      const unsigned* __restrict__ C, long total, int* __restrict__ succ0,
                                                      int* __restrict__ label, int* __restrict__ dist, int* __restrict__ succ) {
    const cris_eval_desc d = descs[blockIdx.y];
    long lo = (long)bases[blockIdx.y], hi = lo + (long)totals[blockIdx.y];
    lo = lo < 0 ? 0 : lo;
    hi = hi > total ? total : hi;
    const unsigned W1 = (unsigned)(d.w_out + 1), H1 = (unsigned)(d.h_out + 1);
    for (long i = lo + (long)blockIdx.x * 256 + threadIdx.x; i < hi; i += (long)gridDim.x * 256) {
        const unsigned r = R[i];
        long s = i ^ 1;                                                   // the other end of the horizontal edge
        if (r & 1u) {                                                     // leaves on the vertical crack: the same visit in C, its partner, back to R
            const unsigned vertex = r >> 3, x = vertex % W1, y = vertex / W1;
            const long j = pg_find(C, lo, hi, (x * H1 + y) * 2u + ((r >> 1) & 1u), 1);
            const long p = j ^ 1;
            const unsigned c = p >= lo && p < hi ? C[p] : C[j];
            const unsigned cv = c >> 2, px = cv / H1, py = cv % H1;
            s = pg_find(R, lo, hi, (py * W1 + px) * 2u + (c & 1u), 2);
        }
        if (s < lo || s >= hi) s = i;
        succ0[i] = (int)s;
        succ[i] = (int)s;
        label[i] = (int)i;
        dist[i] = 0;
    }
}

// Launch 6, once per round r = 0, 1, ...: hop = 2^r.  Visibility: the kernel boundary; reads the buffers of round r - 1, writes the
// others.  Before the round (label, dist)[i] = the smallest index among the `hop` visits from i on and the steps to its first
// occurrence, succ[i] = the visit `hop` steps on.  A strictly smaller label wins, so the nearer of two equal ones stays.
__global__ __launch_bounds__(256) void pg_jump_kernel(long total, int hop, const int* __restrict__ label, const int* __restrict__ dist,
                                                      const int* __restrict__ succ, int* __restrict__ label2, int* __restrict__ dist2,
                                                      int* __restrict__ succ2) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        int s = succ[i];
        s = s < 0 || s >= total ? (int)i : s;
        int l = label[i], dd = dist[i];
        const int l2 = label[s];
        if (l2 < l) {
            l = l2;
            dd = hop + dist[s];
        }
        int s2 = succ[s];
        s2 = s2 < 0 || s2 >= total ? s : s2;
        label2[i] = l;
        dist2[i] = dd;
        succ2[i] = s2;
    }
}

// is visit i the start of its ring, and how long is the ring: the start is `dist` steps on from its own successor
__device__ __forceinline__ int pg_ring_length(long i, long total, const int* __restrict__ label, const int* __restrict__ dist,
                                              const int* __restrict__ succ0) {
    if (label[i] != (int)i) return 0;
    int s = succ0[i];
    s = s < 0 || s >= total ? (int)i : s;
    const int len = dist[s] + 1;
    return len < 1 ? 1 : len;
}

// Launch 7.  Visibility: the kernel boundary (the last round).  chunk c: the starts among its visits and their rings' lengths
__global__ __launch_bounds__(256) void pg_chunks_kernel(long total, const int* __restrict__ label, const int* __restrict__ dist,
                                                        const int* __restrict__ succ0, long long* __restrict__ chunks) {
    __shared__ long long lds[4];
    const long c0 = (long)blockIdx.x * PG_CHUNK;
    long long mine = 0;                                                   // rings in the high word, vertices in the low one
    for (int j = 0; j < PG_CHUNK / 256; ++j) {
        const long i = c0 + j * 256 + threadIdx.x;
        if (i < total) {
            const int len = pg_ring_length(i, total, label, dist, succ0);
            if (len) mine += (1ll << 32) + len;
        }
    }
    long long tot;
    pg_block_scan(mine, lds, &tot);
    if (threadIdx.x == 0) chunks[blockIdx.x] = tot;
}

// Launch 8.  One block: exclusive scan of the chunk sums in place (both halves at once: the vertices of a batch are < 2^31, so the
// low word never carries); header[0] = rings, header[1] = vertices of the batch
__global__ __launch_bounds__(256) void pg_chunk_scan_kernel(long nchunks, long long* __restrict__ chunks, long long* __restrict__ header) {
    __shared__ long long lds[4];
    long long carry = 0;
    for (long base = 0; base < nchunks; base += 256) {
        const long i = base + threadIdx.x;
        const long long v = i < nchunks ? chunks[i] : 0;
        long long tot;
        const long long incl = pg_block_scan(v, lds, &tot);
        if (i < nchunks) chunks[i] = carry + incl - v;
        carry += tot;
    }
    if (threadIdx.x == 0) {
        header[0] = carry >> 32;
        header[1] = carry & 0xffffffffll;
    }
}

// Launch 9.  Visibility: the kernel boundary.  Thread t of chunk c owns the 4 consecutive visits c * PG_CHUNK + 4 t ..: the scan
// over the block is in index order.  ring_index / ring_base are written at the starts only and read at the starts only.
__global__ __launch_bounds__(256) void pg_bases_kernel(long total, const int* __restrict__ label, const int* __restrict__ dist,
                                                       const int* __restrict__ succ0, const long long* __restrict__ chunks,
                                                       int* __restrict__ ring_index, int* __restrict__ ring_base) {
    __shared__ long long lds[4];
    const long i0 = (long)blockIdx.x * PG_CHUNK + 4 * (long)threadIdx.x;
    int len[4];
    long long mine = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        len[j] = i0 + j < total ? pg_ring_length(i0 + j, total, label, dist, succ0) : 0;
        if (len[j]) mine += (1ll << 32) + len[j];
    }
    long long tot;
    long long at = chunks[blockIdx.x] + pg_block_scan(mine, lds, &tot) - mine;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (!len[j]) continue;
        ring_index[i0 + j] = (int)(at >> 32);
        ring_base[i0 + j] = (int)(at & 0xffffffffll);
        at += (1ll << 32) + len[j];
    }
}

// Launch 10.  Visibility: the kernel boundary.  Vertex i goes to the base of its ring + its rank, the start writes the ring's row.
__global__ __launch_bounds__(256) void pg_scatter_kernel(const cris_eval_desc* __restrict__ descs, int n, const long long* __restrict__ bases,
                                                         long total, const unsigned* __restrict__ R, const int* __restrict__ label,
                                                         const int* __restrict__ dist, const int* __restrict__ succ0,
                                                         const int* __restrict__ ring_index, const int* __restrict__ ring_base,
                                                         int* __restrict__ vertices, size_t vertex_cap, long long* __restrict__ rings,
                                                         size_t ring_cap) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        int st = label[i];
        st = st < 0 || st >= total ? (int)i : st;
        int s = succ0[st];
        s = s < 0 || s >= total ? st : s;
        const int len = max(dist[s] + 1, 1), dd = dist[i];
        const long rank = dd > 0 && dd < len ? len - dd : 0;
        int lo = 0, hi = n;                                               // the last descriptor whose base is <= i: the one that holds i
        while (hi - lo > 1) {
            const int m = (lo + hi) / 2;
            if (bases[m] <= i) lo = m;
            else hi = m;
        }
        const unsigned vertex = R[i] >> 3, W1 = (unsigned)(descs[lo].w_out + 1);
        const long at = (long)ring_base[st] + rank;
        if (at >= 0 && (size_t)at < vertex_cap) {
            vertices[2 * at] = (int)(vertex % W1);
            vertices[2 * at + 1] = (int)(vertex / W1);
        }
        if (st == (int)i) {
            const long row = ring_index[i];
            if (row >= 0 && (size_t)row < ring_cap) {
                rings[4 * row] = lo;
                rings[4 * row + 1] = ring_base[i];
                rings[4 * row + 2] = len;
                rings[4 * row + 3] = 0;
            }
        }
    }
}

// Launch 11.  Visibility: the kernel boundary (vertices and rows are complete).  One wave per ring; lane sums in a fixed order.
__global__ __launch_bounds__(256) void pg_area_kernel(const long long* __restrict__ header, const int* __restrict__ vertices, size_t vertex_cap,
                                                      long long* __restrict__ rings, size_t ring_cap) {
    const int lane = threadIdx.x & 63;
    long long count = header[0];
    if (count > (long long)ring_cap) count = (long long)ring_cap;
    for (long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); r < count; r += (long long)gridDim.x * 4) {
        const long long off = rings[4 * r + 1], len = rings[4 * r + 2];
        long long sum = 0;
        if (off >= 0 && len >= 1 && (size_t)(off + len) <= vertex_cap) {
            for (long long j = lane; j < len; j += 64) {
                const long long p = off + j, q = off + (j + 1 == len ? 0 : j + 1);
                sum += (long long)vertices[2 * p] * vertices[2 * q + 1] - (long long)vertices[2 * q] * vertices[2 * p + 1];
            }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 64);
        if (lane == 0) rings[4 * r + 3] = sum;
    }
}

// what the entry points read from the host copy of the descriptors: every address the kernels form
static const char* pg_check_descs(const cris_eval_desc* descs_host, int n, size_t mask_bytes, size_t* stride_r, size_t* stride_c, long* tiles) {
    *stride_r = *stride_c = 0;
    *tiles = 0;
    for (int i = 0; i < n; ++i) {
        const cris_eval_desc& d = descs_host[i];
        if (!(d.w_out > 0 && d.h_out > 0 && ((long)d.w_out + 1) * ((long)d.h_out + 1) <= PG_MAX_VERTS))
            return "descriptor: bad output size ((h_out + 1) * (w_out + 1) must be <= 2^28)";
        if (!(d.pitch >= d.w_out && (d.pitch & 3) == 0 && (long)d.pitch * d.h_out < (1L << 31)))
            return "descriptor: the pitch must be a multiple of 4, >= w_out, pitch * h_out < 2^31";
        if (!(d.out_off >= 0 && (size_t)d.out_off + (size_t)d.pitch * d.h_out <= mask_bytes)) return "descriptor: output outside the buffer";
        const pg_geom G(d.h_out, d.w_out);
        const size_t sr = (size_t)(d.h_out + 1) * G.ncg, sc = (size_t)(d.w_out + 1) * G.nb;
        if (sr > *stride_r) *stride_r = sr;
        if (sc > *stride_c) *stride_c = sc;
        if ((long)G.ncg * G.nb > *tiles) *tiles = (long)G.ncg * G.nb;
    }
    return nullptr;
}

static size_t pg_round8(size_t b) { return (b + 7) & ~(size_t)7; }

// the count's scratch: [n * stride_r row segments][n * stride_c column segments][n bases]
static size_t pg_work_bytes(size_t stride_r, size_t stride_c, int n) {
    return pg_round8((size_t)n * stride_r * 4) + pg_round8((size_t)n * stride_c * 4) + 8 * (size_t)n;
}

extern "C" size_t cris_polygon_work_bytes(const cris_eval_desc* descs_host, int n) {
    if (!descs_host || n <= 0 || n > 65535) return 0;
    size_t stride_r = 0, stride_c = 0;
    for (int i = 0; i < n; ++i) {                                           // (bad descriptors count nothing: cris_polygon_count names them)
        const cris_eval_desc& d = descs_host[i];
        if (!(d.w_out > 0 && d.h_out > 0 && ((long)d.w_out + 1) * ((long)d.h_out + 1) <= PG_MAX_VERTS)) continue;
        const pg_geom G(d.h_out, d.w_out);
        const size_t sr = (size_t)(d.h_out + 1) * G.ncg, sc = (size_t)(d.w_out + 1) * G.nb;
        if (sr > stride_r) stride_r = sr;
        if (sc > stride_c) stride_c = sc;
    }
    return pg_work_bytes(stride_r, stride_c, n);
}

static long pg_chunk_count(long long total) { return (long)((total + PG_CHUNK - 1) / PG_CHUNK); }

// the trace's scratch: R, C, succ0 and two (label, dist, succ) buffers of `total` words each, then the chunk sums
extern "C" size_t cris_polygon_trace_work_bytes(long long total_vertices, int n) {
    if (total_vertices <= 0 || total_vertices > (1ll << 30) || n <= 0 || n > 65535) return 0;
    return 9 * pg_round8((size_t)total_vertices * 4) + 8 * (size_t)pg_chunk_count(total_vertices);
}

extern "C" int cris_polygon_count(const unsigned char* masks, size_t mask_bytes, const cris_eval_desc* descs_host,
                                  const cris_eval_desc* descs_dev, int n, void* work, size_t work_bytes, long long* totals, void* stream) {
    CRIS_CHECK_ARG(masks && descs_host && descs_dev && work && totals, "null operand");
    CRIS_CHECK_ARG(n > 0 && n <= 65535, "n must be in 1 .. 65535");
    CRIS_CHECK_ARG(((uintptr_t)work & 7) == 0 && ((uintptr_t)totals & 7) == 0, "work and totals must be 8-byte aligned");
    size_t stride_r = 0, stride_c = 0;
    long tiles = 0;
    const char* bad = pg_check_descs(descs_host, n, mask_bytes, &stride_r, &stride_c, &tiles);
    CRIS_CHECK_ARG(!bad, bad);
    CRIS_CHECK_ARG(work_bytes >= pg_work_bytes(stride_r, stride_c, n), "the work buffer is too small");
    int* rows = reinterpret_cast<int*>(work);
    int* cols = reinterpret_cast<int*>(reinterpret_cast<char*>(work) + pg_round8((size_t)n * stride_r * 4));
    long long* bases = reinterpret_cast<long long*>(reinterpret_cast<char*>(cols) + pg_round8((size_t)n * stride_c * 4));
    const int cap = 8192 / n > 32 ? 8192 / n : 32;
    const dim3 grid(cris_grid_1d(tiles, 1, cap), n);
    hipLaunchKernelGGL(pg_count_kernel, grid, dim3(PG_CG), 0, (hipStream_t)stream, masks, descs_dev, stride_r, stride_c, rows, cols);
    CRIS_LAUNCH_CHECK();
    hipLaunchKernelGGL(pg_scan_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, descs_dev, stride_r, stride_c, rows, cols, totals);
    CRIS_LAUNCH_CHECK();
    hipLaunchKernelGGL(pg_totals_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, n, totals, bases);
    CRIS_LAUNCH_CHECK();
    return 0;
}

extern "C" int cris_polygon_trace(const unsigned char* masks, size_t mask_bytes, const cris_eval_desc* descs_host,
                                  const cris_eval_desc* descs_dev, int n, const void* work, size_t work_bytes, const long long* totals,
                                  long long total_vertices, long long max_vertices_per_mask, int extra_rounds, void* trace_work,
                                  size_t trace_work_bytes, int* vertices, size_t vertex_cap, long long* rings, size_t ring_cap,
                                  long long* header, void* stream) {
    CRIS_CHECK_ARG(masks && descs_host && descs_dev && work && totals && trace_work && vertices && rings && header, "null operand");
    CRIS_CHECK_ARG(n > 0 && n <= 65535, "n must be in 1 .. 65535");
    CRIS_CHECK_ARG(((uintptr_t)work & 7) == 0 && ((uintptr_t)totals & 7) == 0 && ((uintptr_t)trace_work & 7) == 0 &&
                       ((uintptr_t)vertices & 3) == 0 && ((uintptr_t)rings & 7) == 0 && ((uintptr_t)header & 7) == 0,
                   "work, totals, trace_work, rings and header must be 8-byte, vertices 4-byte aligned");
    CRIS_CHECK_ARG(total_vertices > 0 && total_vertices <= (1ll << 30) && (total_vertices & 1) == 0,
                   "total_vertices must be even and in 2 .. 2^30 (a batch without foreground is not traced)");
    CRIS_CHECK_ARG(max_vertices_per_mask >= 4 && max_vertices_per_mask <= total_vertices, "max_vertices_per_mask must be in 4 .. total_vertices");
    CRIS_CHECK_ARG(extra_rounds >= 0 && extra_rounds <= 8, "extra_rounds must be in 0 .. 8");
    size_t stride_r = 0, stride_c = 0;
    long tiles = 0;
    const char* bad = pg_check_descs(descs_host, n, mask_bytes, &stride_r, &stride_c, &tiles);
    CRIS_CHECK_ARG(!bad, bad);
    CRIS_CHECK_ARG(work_bytes >= pg_work_bytes(stride_r, stride_c, n), "the work buffer is too small");
    CRIS_CHECK_ARG(trace_work_bytes >= cris_polygon_trace_work_bytes(total_vertices, n), "the trace work buffer is too small");
    const long total = (long)total_vertices, nchunks = pg_chunk_count(total_vertices);
    const int* rows = reinterpret_cast<const int*>(work);
    const int* cols = reinterpret_cast<const int*>(reinterpret_cast<const char*>(work) + pg_round8((size_t)n * stride_r * 4));
    const long long* bases = reinterpret_cast<const long long*>(reinterpret_cast<const char*>(cols) + pg_round8((size_t)n * stride_c * 4));
    const size_t plane = pg_round8((size_t)total * 4);
    char* tw = reinterpret_cast<char*>(trace_work);
    unsigned* R = reinterpret_cast<unsigned*>(tw);
    unsigned* C = reinterpret_cast<unsigned*>(tw + plane);
    int* succ0 = reinterpret_cast<int*>(tw + 2 * plane);
    int* buf[2][3];
    for (int s = 0; s < 2; ++s)
        for (int j = 0; j < 3; ++j) buf[s][j] = reinterpret_cast<int*>(tw + (3 + 3 * s + j) * plane);
    long long* chunks = reinterpret_cast<long long*>(tw + 9 * plane);
    int rounds = extra_rounds;
    for (long long m = 1; m < max_vertices_per_mask; m <<= 1) ++rounds;     // ceil(log2(max)): the window of the last round holds any ring
    hipStream_t st = (hipStream_t)stream;
    const int cap = 8192 / n > 32 ? 8192 / n : 32;
    hipLaunchKernelGGL(pg_write_kernel, dim3(cris_grid_1d(tiles, 1, cap), n), dim3(PG_CG), 0, st, masks, descs_dev, stride_r, stride_c, rows,
                       cols, bases, R, C, total);
    CRIS_LAUNCH_CHECK();
    const int per = cris_grid_1d((long)max_vertices_per_mask, 256, cap);
    hipLaunchKernelGGL(pg_link_kernel, dim3(per, n), dim3(256), 0, st, descs_dev, bases, totals, (const unsigned*)R, (const unsigned*)C, total,
                       succ0, buf[0][0], buf[0][1], buf[0][2]);
    CRIS_LAUNCH_CHECK();
    const int flat = cris_grid_1d(total, 256);
    int cur = 0;
    for (int r = 0; r < rounds; ++r, cur ^= 1) {
        const int hop = r < 30 ? 1 << r : 1 << 30;
        hipLaunchKernelGGL(pg_jump_kernel, dim3(flat), dim3(256), 0, st, total, hop, (const int*)buf[cur][0], (const int*)buf[cur][1],
                           (const int*)buf[cur][2], buf[cur ^ 1][0], buf[cur ^ 1][1], buf[cur ^ 1][2]);
        CRIS_LAUNCH_CHECK();
    }
    const int* label = buf[cur][0];
    const int* dist = buf[cur][1];
    int* ring_index = buf[cur ^ 1][0];                                      // the other buffer is free again
    int* ring_base = buf[cur ^ 1][1];
    hipLaunchKernelGGL(pg_chunks_kernel, dim3((unsigned)nchunks), dim3(256), 0, st, total, label, dist, (const int*)succ0, chunks);
    CRIS_LAUNCH_CHECK();
    hipLaunchKernelGGL(pg_chunk_scan_kernel, dim3(1), dim3(256), 0, st, nchunks, chunks, header);
    CRIS_LAUNCH_CHECK();
    hipLaunchKernelGGL(pg_bases_kernel, dim3((unsigned)nchunks), dim3(256), 0, st, total, label, dist, (const int*)succ0,
                       (const long long*)chunks, ring_index, ring_base);
    CRIS_LAUNCH_CHECK();
    hipLaunchKernelGGL(pg_scatter_kernel, dim3(flat), dim3(256), 0, st, descs_dev, n, bases, total, (const unsigned*)R, label, dist,
                       (const int*)succ0, (const int*)ring_index, (const int*)ring_base, vertices, vertex_cap, rings, ring_cap);
    CRIS_LAUNCH_CHECK();
    hipLaunchKernelGGL(pg_area_kernel, dim3(cris_grid_1d((long)(total / 4), 4, 2048)), dim3(256), 0, st, (const long long*)header,
                       (const int*)vertices, vertex_cap, rings, ring_cap);
    CRIS_LAUNCH_CHECK();
    return 0;
}
