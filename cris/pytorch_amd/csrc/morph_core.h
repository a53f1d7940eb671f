// Square-structuring-element erosion on bit planes: the per-word arithmetic of csrc/morph.hip, host and device
// (the style of jpeg_core.h: the same functions compile for a host program that checks them against a per-pixel oracle).
//
// A bit plane holds a mask as h rows of wpr = ceil(w / 64) 64-bit words: bit i of word c of row y is pixel (64 c + i, y); the bits
// at x >= w of a row's last word are 0.  Outside the image is background.  Integers only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef CRIS_HD
#define CRIS_HD __host__ __device__ __forceinline__
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define CRIS_MORPH_CLZ(v) __clzll((long long)(v))
#define CRIS_MORPH_CTZ(v) (__ffsll((long long)(v)) - 1)
#else
#define CRIS_MORPH_CLZ(v) __builtin_clzll(v)
#define CRIS_MORPH_CTZ(v) __builtin_ctzll(v)
#endif

// true when the (2 d + 1)-square fits nowhere in an h x w image: the erosion is empty and no plane word is looked at.  Past this
// test d <= (min(h, w) - 1) / 2 < 2^30, so x + d and y + d stay inside int
CRIS_HD bool morph_empty(int h, int w, int d) { return 2 * (long)d + 1 > (long)(h < w ? h : w); }

// bit i = AND of v's bits [i - m + 1, i], 1 <= m <= 64, positions below 0 read as 1: shift-and-AND doubling, then one step for the rest
CRIS_HD uint64_t morph_win_left(uint64_t v, int m) {
    int p = 1;
    for (; 2 * p <= m; p *= 2) v &= (v << p) | ((1ull << p) - 1);
    const int r = m - p;
    if (r) v &= (v << r) | ((1ull << r) - 1);
    return v;
}

// bit i = AND of v's bits [i, i + m - 1], positions above 63 read as 1
CRIS_HD uint64_t morph_win_right(uint64_t v, int m) {
    int p = 1;
    for (; 2 * p <= m; p *= 2) v &= (v >> p) | (~0ull << (64 - p));
    const int r = m - p;
    if (r) v &= (v >> r) | (~0ull << (64 - r));
    return v;
}

// Row pass: word c of the row eroded along x by d (bit x survives iff the bits [x - d, x + d] are all inside [0, 64 wpr) and 1;
// the bits at x >= w are 0, so that is "inside [0, w)").  row: the wpr words of one row; 0 <= c < wpr; d >= 1, !morph_empty.
// Inside the word the window is the doubling above; beyond it only the NEAREST 0 on either side matters: the last 0 before the
// word (x = -1 counts) and the first after it (x = 64 wpr counts), found by walking at most ceil(d / 64) words each way - every
// index is clamped to [0, wpr).
CRIS_HD uint64_t morph_row_word(const uint64_t* __restrict__ row, int wpr, int c, int d) {
    const uint64_t v = row[c];
    if (v == 0) return 0;
    const int m = (d < 63 ? d : 63) + 1, H = (d + 63) / 64;
    uint64_t out = morph_win_left(v, m) & morph_win_right(v, m);
    const int lo = c - H > 0 ? c - H : 0, hi = c + H < wpr - 1 ? c + H : wpr - 1;
    long pz = 64L * lo - 1;                                       // the last 0 before the word, or a position out of the window's reach
    for (int j = c - 1; j >= lo; --j) {
        const uint64_t u = ~row[j];
        if (u) {
            pz = 64L * j + 63 - CRIS_MORPH_CLZ(u);
            break;
        }
    }
    long nz = 64L * (hi + 1);                                     // the first 0 after the word, likewise
    for (int j = c + 1; j <= hi; ++j) {
        const uint64_t u = ~row[j];
        if (u) {
            nz = 64L * j + CRIS_MORPH_CTZ(u);
            break;
        }
    }
    const long tl = pz + d + 1 - 64L * c;                         // bit i survives the left side iff 64 c + i - d > pz, i.e. i >= tl
    const long tr = nz - d - 64L * c;                             // and the right side iff 64 c + i + d < nz, i.e. i < tr
    if (tl >= 64 || tr <= 0) return 0;
    if (tl > 0) out &= ~0ull << tl;
    if (tr < 64) out &= (1ull << tr) - 1;
    return out;
}

// Column pass for the two rows y0 and y0 + 1 (y0 even) of word column c: e0 / e1 = AND of the row-eroded words of rows
// [y - d, y + d], 0 when that range leaves [0, h) (or y0 + 1 >= h).  The 2 d rows [y0 + 1 - d, y0 + d] are common to both windows
// and read once; each output adds one row.  plane: h rows of wpr words; d >= 1, !morph_empty.  No row outside [0, h) is read.
CRIS_HD void morph_col_pair(const uint64_t* __restrict__ plane, int wpr, int h, int y0, int c, int d, uint64_t* e0, uint64_t* e1) {
    const bool ok0 = y0 - d >= 0 && y0 + d < h, ok1 = y0 + 1 - d >= 0 && y0 + 1 + d < h;
    *e0 = *e1 = 0;
    if (!ok0 && !ok1) return;
    uint64_t core = ~0ull;
    for (int y = y0 + 1 - d; y <= y0 + d; ++y) core &= plane[(size_t)y * wpr + c];
    if (ok0) *e0 = core & plane[(size_t)(y0 - d) * wpr + c];
    if (ok1) *e1 = core & plane[(size_t)(y0 + 1 + d) * wpr + c];
}
