// Decoding of encoded masks: the per-pixel and per-edge arithmetic of csrc/decode.hip, host and device (the style of
// morph_core.h: the same functions compile for a host program that checks them against rle.decode / polygon.decode).
//
// RLE (rle.py): pixels in column-major order, i = x * h + y; ends[j] = counts[0] + ... + counts[j] is the pixel index at which run j
// ends; runs alternate background, foreground and start with background, so pixel i is foreground iff the number of ends <= i is
// odd (np.searchsorted(ends, i, side="right") & 1).  A run of length zero repeats an end: it is counted like any other.
//
// Polygons (polygon._decode_general, to the letter): doubled coordinates, every non-horizontal edge oriented downwards, the centre
// lines py = y0 .. y1 - 1 of an edge (x0, y0) -> (x1, y1), and on line py the crossing toggles the pixels at
//     x >= px,   px = x0 - floor((dy - num) / (2 dy)),   num = (2 py + 1 - 2 y0) dx,   dx = x1 - x0,   dy = y1 - y0 > 0
// with px clipped to [0, w]; a toggle at w changes no pixel.  dy - num is NEGATIVE for edges that lean right far enough: the quotient
// is a FLOOR (Python's //), which C++'s / - truncation towards zero - is not; decode_floor_div states the difference.  All of it in
// 64-bit integers: |num| < 2 (h + 1) (w + 1) <= 2^29 with the sides polygon.MAX_VERTICES allows.
//
// A bit plane is morph_core.h's: h rows of ceil(w / 64) 64-bit words, bit i of word c of row y is pixel (64 c + i, y).
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef CRIS_HD
#define CRIS_HD __host__ __device__ __forceinline__
#endif

// the number of ends[0 .. n) that are <= i (an upper bound; ends non-decreasing).  The loop ends after ceil(log2(n + 1)) steps and
// returns a value in [0, n] whatever the words hold
CRIS_HD int decode_upper_bound(const uint32_t* __restrict__ ends, int n, uint32_t i) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (ends[mid] <= i) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the same search restricted to [lo, n): for a pixel index that is not below the one that found `lo`
CRIS_HD int decode_upper_bound_from(const uint32_t* __restrict__ ends, int lo, int n, uint32_t i) {
    int hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (ends[mid] <= i) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

CRIS_HD bool decode_rle_pixel(const uint32_t* __restrict__ ends, int n, int h, int x, int y) {
    return decode_upper_bound(ends, n, (uint32_t)x * (uint32_t)h + (uint32_t)y) & 1;
}

// floor(a / b) for b > 0.  C++ truncates: -3 / 2 == -1, the floor is -2 - one less whenever a is negative and b does not divide it
CRIS_HD int64_t decode_floor_div(int64_t a, int64_t b) {
    const int64_t q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// the first pixel of row py that the edge (x0, y0) -> (x1, y1), y0 < y1, y0 <= py < y1, toggles: in [0, w]; w = none
CRIS_HD int decode_crossing(int64_t x0, int64_t y0, int64_t x1, int64_t y1, int64_t py, int w) {
    const int64_t dx = x1 - x0, dy = y1 - y0;
    const int64_t num = (2 * py + 1 - 2 * y0) * dx;
    const int64_t px = x0 - decode_floor_div(dy - num, 2 * dy);
    return (int)(px < 0 ? 0 : px > w ? w : px);
}

// every toggle of the edge a -> b in an h x w mask: toggle(px, py) for each centre line the edge crosses inside [0, h) whose
// crossing lies left of w.  Horizontal edges cross none; the others are oriented downwards first
template <typename F>
CRIS_HD void decode_edge(int ax, int ay, int bx, int by, int h, int w, F toggle) {
    if (ay == by) return;
    if (by < ay) {
        const int tx = ax, ty = ay;
        ax = bx;
        ay = by;
        bx = tx;
        by = ty;
    }
    const int ya = ay > 0 ? ay : 0, yb = by < h ? by : h;          // only rows of the mask
    for (int py = ya; py < yb; ++py) {
        const int px = decode_crossing(ax, ay, bx, by, py, w);
        if (px < w) toggle(px, py);
    }
}

// bit i = XOR of v's bits [0, i]: shift-and-XOR doubling
CRIS_HD uint64_t decode_prefix_parity(uint64_t v) {
    v ^= v << 1;
    v ^= v << 2;
    v ^= v << 4;
    v ^= v << 8;
    v ^= v << 16;
    v ^= v << 32;
    return v;
}

#if defined(__HIP_DEVICE_COMPILE__)
#define CRIS_DECODE_POPC(v) __popcll(v)
#else
#define CRIS_DECODE_POPC(v) __builtin_popcountll(v)
#endif

// What one thread of the store launch computes: bit k = pixel (x + k, y), k < 4, x a multiple of 4; the bits at x + k >= w are 0.
// RLE: four upper bounds, each starting where the last one ended (the pixel index grows by h from one to the next).
CRIS_HD unsigned decode_rle_bits(const uint32_t* __restrict__ ends, int n, int h, int w, int x, int y) {
    unsigned bits = 0;
    int at = 0;
    for (int k = 0; k < 4 && x + k < w; ++k) {
        at = decode_upper_bound_from(ends, at, n, (uint32_t)(x + k) * (uint32_t)h + (uint32_t)y);
        bits |= (unsigned)(at & 1) << k;
    }
    return bits;
}

// Polygon: the row's inclusive prefix parity at x .. x + 3.  row: the ceil(w / 64) words of the toggles of one row; the carry into
// word c is the popcount parity of the words before it.  No word is read when x >= w
CRIS_HD unsigned decode_plane_bits(const unsigned long long* __restrict__ row, int w, int x) {
    if (x >= w) return 0;
    const int c = x >> 6;
    unsigned carry = 0;
    for (int j = 0; j < c; ++j) carry ^= (unsigned)CRIS_DECODE_POPC(row[j]);
    const uint64_t v = decode_prefix_parity(row[c]) ^ ((carry & 1) ? ~0ull : 0ull);
    unsigned bits = (unsigned)(v >> (x & 63)) & 0xfu;
    if (x + 4 > w) bits &= (1u << (w - x)) - 1u;                    // the plane holds no toggle at x >= w, the parity runs on
    return bits;
}

// the dword of four mask bytes: byte k = 255 iff bit k
CRIS_HD uint32_t decode_bytes(unsigned bits) {
    return ((bits & 1u) ? 0xffu : 0u) | ((bits & 2u) ? 0xff00u : 0u) | ((bits & 4u) ? 0xff0000u : 0u) | ((bits & 8u) ? 0xff000000u : 0u);
}

// the ring of vertex g: the last row r of rows[first .. first + count) whose offset (word 1 of a row of `stride` words) is <= g.
// The rows' offsets ascend (the launcher checked them); count >= 1 and g >= the first row's offset
CRIS_HD long decode_ring_of(const long long* __restrict__ rows, int stride, long first, long count, long long g) {
    long lo = 0, hi = count;                                       // offsets[lo] <= g < offsets[hi]
    while (hi - lo > 1) {
        const long mid = lo + ((hi - lo) >> 1);
        if (rows[(size_t)(first + mid) * stride + 1] <= g) lo = mid;
        else hi = mid;
    }
    return first + lo;
}
