// Exponential moving average of the weights, kept on the device inside the training step (NativeTrainer(ema_decay=...)):
//   cris_ema_advance   one thread: is this optimizer step an EMA step, and with which weight (warm-up included)?
//   cris_ema_update    one launch over a table of {p, ema}: ema += (p - ema) * weight, or nothing at all when the step is not one
// Both read what changes from step to step from device memory (the step counter, the 16-byte state record), so a captured graph or
// a recorded command list replays them unchanged.  The update is a pure HBM stream: read p, read ema, write ema.
#include "common.h"
#include "../../../include/cris_hip.h"

// No fused multiply-adds in this file: ema + (p - ema) * w is three separately rounded fp32 operations, so that torch's
// `e.add_((p - e) * w)` reproduces it bit for bit; hipcc contracts a*b+c by default (operators of HIP headers OUTSIDE this pragma
// would still get fused, csrc/evalpost.hip: everything below is written with the plain operators, inside it).
#pragma clang fp contract(off)
__device__ __forceinline__ float ema_lerp(float e, float p, float w) {
    const float d = p - e;
    const float s = d * w;
    return e + s;
}

#define EMA_ELEMS 8192                           // elements per block trip: the Adam kernels' partition (cris_adam_block_elems)
#define EMA_VECS (EMA_ELEMS / 4 / 256)           // 16-byte vectors per thread and trip

// the tensors are reached through pointers read from the table: telling the compiler that they are global memory turns its
// generic (flat) accesses into global ones
typedef const __attribute__((address_space(1))) f32x4* ema_gload4;
typedef __attribute__((address_space(1))) f32x4* ema_gstore4;
typedef const __attribute__((address_space(1))) float* ema_gload1;
typedef __attribute__((address_space(1))) float* ema_gstore1;
__device__ __forceinline__ f32x4 ema_lerp4(f32x4 e, f32x4 p, float w) {
    f32x4 o;
    o.x = ema_lerp(e.x, p.x, w); o.y = ema_lerp(e.y, p.y, w); o.z = ema_lerp(e.z, p.z, w); o.w = ema_lerp(e.w, p.w, w);
    return o;
}

struct ema_state { int updates; float weight; int active; int pad; };

__global__ void ema_advance_kernel(const int* __restrict__ step, int every, float decay, int warmup, ema_state* st) {
    const int s = step[0];                       // 1-based optimizer step (cris_step_advance[_micro] ran before)
    const int active = (s % every) == 0 ? 1 : 0;
    st->active = active;
    if (!active) return;                         // updates and weight stay as they are
    const int t = st->updates;
    st->updates = t + 1;
    float d = decay;
    if (warmup) {
        const float tf = (float)t;
        const float w = (1.0f + tf) / (10.0f + tf);          // correctly rounded division (no fast-math flag: build.py FLAGS)
        d = w < d ? w : d;
    }
    st->weight = 1.0f - d;
}

extern "C" int cris_ema_advance(const int32_t* step_dev, int every, float decay, int warmup, void* state, void* stream) {
    CRIS_CHECK_ARG(step_dev && state, "null step counter or state record");
    CRIS_CHECK_ARG(every >= 1, "every must be >= 1");
    CRIS_CHECK_ARG(decay > 0.f && decay < 1.f, "decay must lie in (0, 1)");
    CRIS_CHECK_ARG(!((uintptr_t)state & 15), "the state record must be 16-byte aligned");
    hipLaunchKernelGGL(ema_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, step_dev, every, decay, warmup ? 1 : 0, (ema_state*)state);
    CRIS_LAUNCH_CHECK();
    return 0;
}

// Block trip b of the table's partition (block_start prefix sums of cris_ema_blocks, as for cris_adam_step) owns elements
// [lb * 8192, (lb + 1) * 8192) of one tensor; the grid is capped and strides over the trips.  Every ema slice starts on a 16-byte
// boundary, so vector v of a tensor is aligned in ema; p is read with 16-byte loads when its own start is 16-byte aligned too (every
// torch allocation) and element by element otherwise (views at an odd offset).  The n & 3 tail elements, and every element of a
// row-skipping tensor whose rows are not whole vectors, go through scalar code.  One thread owns an element: no atomics.
__global__ __launch_bounds__(256) void ema_update_kernel(const cris_ema_desc* __restrict__ tab, int n_desc, int total_blocks,
                                                         const ema_state* __restrict__ st) {
    if (st->active == 0) return;                 // not an EMA step: the launch is the whole cost
    const float w = st->weight;
    for (int bid = blockIdx.x; bid < total_blocks; bid += gridDim.x) {
        int lo = 0, hi = n_desc - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (tab[mid].block_start <= bid) lo = mid; else hi = mid - 1;
        }
        const cris_ema_desc d = tab[lo];
        const long base = (long)(bid - d.block_start) * EMA_ELEMS;
        const long left = d.n - base;            // > 0 by the partition
        const unsigned char* live = d.row_live;
        if (live && (d.row_len & 3)) {
            // rows are not whole vectors: element by element (small tables only)
            for (int e = threadIdx.x; e < EMA_ELEMS && e < left; e += 256) {
                const long i = base + e;
                if (!live[i / d.row_len]) continue;
                ((ema_gstore1)d.ema)[i] = ema_lerp(((ema_gload1)d.ema)[i], ((ema_gload1)d.p)[i], w);
            }
            continue;
        }
        const ema_gload1 p = (ema_gload1)(d.p + base);
        const ema_gstore1 ema = (ema_gstore1)(d.ema + base);
        const bool p_vec = (((uintptr_t)d.p) & 15) == 0;      // (base is a multiple of 8192 elements)
        if (left >= EMA_ELEMS && p_vec && !live) {
            // the common trip: all loads of four vectors are issued before the first of their stores
#pragma unroll
            for (int h = 0; h < EMA_VECS; h += 4) {
                f32x4 pv[4], ev[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int v = threadIdx.x + 256 * (h + j);
                    pv[j] = ((ema_gload4)p)[v];
                    ev[j] = ((ema_gload4)ema)[v];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int v = threadIdx.x + 256 * (h + j);
                    ((ema_gstore4)ema)[v] = ema_lerp4(ev[j], pv[j], w);
                }
            }
            continue;
        }
        const int cnt = left < EMA_ELEMS ? (int)left : EMA_ELEMS;
        const int nvec = cnt >> 2;
        for (int v = threadIdx.x; v < nvec; v += 256) {
            if (live && !live[(base + 4 * (long)v) / d.row_len]) continue;      // (row_len % 4 == 0: a vector lies in one row)
            f32x4 pv;
            if (p_vec) pv = ((ema_gload4)p)[v];
            else { pv.x = p[4 * v]; pv.y = p[4 * v + 1]; pv.z = p[4 * v + 2]; pv.w = p[4 * v + 3]; }
            ((ema_gstore4)ema)[v] = ema_lerp4(((ema_gload4)ema)[v], pv, w);
        }
        const int e = 4 * nvec + threadIdx.x;    // tail: at most three elements
        if (e < cnt && !(live && !live[(base + e) / d.row_len])) ema[e] = ema_lerp(ema[e], p[e], w);
    }
}

// host: validates one descriptor and returns the block trips it occupies (block_start prefix sums); -1 and cris_last_error()
// for a descriptor the kernel must not see
extern "C" int cris_ema_blocks(const cris_ema_desc* d) {
    CRIS_CHECK_ARG(d && d->p && d->ema, "null descriptor, p or ema");
    CRIS_CHECK_ARG(d->n > 0, "n must be > 0");
    CRIS_CHECK_ARG(!((uintptr_t)d->ema & 15), "ema must be 16-byte aligned");
    CRIS_CHECK_ARG(!((uintptr_t)d->p & 3), "p must be 4-byte aligned");
    CRIS_CHECK_ARG(!d->row_live || d->row_len > 0, "row_live needs row_len > 0");
    CRIS_CHECK_ARG(d->n <= (long)EMA_ELEMS * 0x3fffffffL, "tensor too large for the block partition");
    return cris_cdiv(d->n, EMA_ELEMS);
}

// compute units of the current device (queried once per device; no stream operation, so legal during a capture)
static int ema_cu_count() {
    static int cached[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (!cached[dev]) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
        cached[dev] = cus;
    }
    return cached[dev];
}

extern "C" int cris_ema_update(const cris_ema_desc* dev_table, int n_desc, int total_blocks, const void* state, void* stream) {
    CRIS_CHECK_ARG(dev_table && state, "null table or state record");
    CRIS_CHECK_ARG(n_desc > 0 && total_blocks >= n_desc, "empty table (every descriptor occupies at least one block)");
    CRIS_CHECK_ARG(!((uintptr_t)state & 15), "the state record must be 16-byte aligned");
    // at most 8 blocks of 256 threads per CU, the rest by the grid-stride loop: more blocks add launch work, not bandwidth
    const int grid = cris_grid_1d(total_blocks, 1, 8 * ema_cu_count());
    hipLaunchKernelGGL(ema_update_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, dev_table, n_desc, total_blocks, (const ema_state*)state);
    CRIS_LAUNCH_CHECK();
    return 0;
}
