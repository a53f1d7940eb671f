// Square-structuring-element erosion (and, in the second half, dilation and clipped erosion) on bit planes: the per-word
// arithmetic of csrc/morph.hip, host and device (the style of jpeg_core.h: the same functions compile for a host
// program that checks them against a per-pixel oracle).
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

// ---- the dual window operation and the clipped erosion ("smoothing"): nothing outside the image exists ----
//     D_d(M)[p]  = OR  of M over the (2 d + 1)-square around p clipped to the image        (dilation)
//     E'_d(M)[p] = AND of M over the same clipped square = ~D_d(~M) on the image           (the adjoint erosion)
// Both keep the plane's rule: the bits at x >= w of a row's last word are 0 in what they write, and they never take those bits of
// what they read for pixels - every word is masked by morph_word_mask on the way in and on the way out.

// the bits of word c that are pixels of a row of w: all 64, or the low w - 64 c of the last word.  0 <= c < ceil(w / 64)
CRIS_HD uint64_t morph_word_mask(int w, int c) {
    const long n = (long)w - 64L * c;
    return n >= 64 ? ~0ull : (1ull << n) - 1;
}

// bit i = OR of v's bits [i - m + 1, i], 1 <= m <= 64, positions below 0 read as 0: shift-and-OR doubling, then one step for the rest
CRIS_HD uint64_t morph_or_left(uint64_t v, int m) {
    int p = 1;
    for (; 2 * p <= m; p *= 2) v |= v << p;
    const int r = m - p;
    if (r) v |= v << r;
    return v;
}

// bit i = OR of v's bits [i, i + m - 1], positions above 63 read as 0
CRIS_HD uint64_t morph_or_right(uint64_t v, int m) {
    int p = 1;
    for (; 2 * p <= m; p *= 2) v |= v >> p;
    const int r = m - p;
    if (r) v |= v >> r;
    return v;
}

// word j of a row as the window OR sees it: the row's own bits, or (inv) their complement ON THE IMAGE - a position at x >= w or in
// a word outside [0, wpr) is never a 1 either way, so it is no foreground for D and no background for E'
CRIS_HD uint64_t morph_load_word(const uint64_t* __restrict__ row, int w, int j, bool inv) {
    return (inv ? ~row[j] : row[j]) & morph_word_mask(w, j);
}

// Row pass of D (inv = false) and E' (inv = true: ~D(~row)): word c of the row's window OR along x over [x - d, x + d] clipped to
// [0, w).  row: the wpr = ceil(w / 64) words of one row; 0 <= c < wpr; d >= 1.  Inside the word the window is the doubling above;
// beyond it only the NEAREST 1 on either side matters, found by walking at most ceil(d / 64) words each way with every index
// clamped to [0, wpr) - no 1 within reach leaves a position no window touches.
CRIS_HD uint64_t morph_row_or_word(const uint64_t* __restrict__ row, int wpr, int w, int c, int d, bool inv) {
    const uint64_t v = morph_load_word(row, w, c, inv);
    const int m = (d < 63 ? d : 63) + 1, H = (d + 63) / 64;
    uint64_t out = morph_or_left(v, m) | morph_or_right(v, m);
    const int lo = c - H > 0 ? c - H : 0, hi = c + H < wpr - 1 ? c + H : wpr - 1;
    long p1 = -(1L << 40);                                        // the last 1 before the word, or a position out of every window's reach
    for (int j = c - 1; j >= lo; --j) {
        const uint64_t u = morph_load_word(row, w, j, inv);
        if (u) {
            p1 = 64L * j + 63 - CRIS_MORPH_CLZ(u);
            break;
        }
    }
    long n1 = 1L << 40;                                           // the first 1 after the word, likewise
    for (int j = c + 1; j <= hi; ++j) {
        const uint64_t u = morph_load_word(row, w, j, inv);
        if (u) {
            n1 = 64L * j + CRIS_MORPH_CTZ(u);
            break;
        }
    }
    const long tl = p1 + d - 64L * c;                             // bit i sees the 1 on its left iff 64 c + i - d <= p1, i.e. i <= tl
    const long tr = n1 - d - 64L * c;                             // and the one on its right iff 64 c + i + d >= n1, i.e. i >= tr
    if (tl >= 63) out = ~0ull;
    else if (tl >= 0) out |= (2ull << tl) - 1;
    if (tr <= 0) out = ~0ull;
    else if (tr < 64) out |= ~0ull << tr;
    return (inv ? ~out : out) & morph_word_mask(w, c);
}
CRIS_HD uint64_t morph_row_dilate_word(const uint64_t* __restrict__ row, int wpr, int w, int c, int d) {
    return morph_row_or_word(row, wpr, w, c, d, false);
}
CRIS_HD uint64_t morph_row_erode_clipped_word(const uint64_t* __restrict__ row, int wpr, int w, int c, int d) {
    return morph_row_or_word(row, wpr, w, c, d, true);
}

// Column pass of D for the two rows y0 and y0 + 1 (y0 even) of word column c: e0 / e1 = OR of the row-pass words of the rows
// [y - d, y + d] clipped to [0, h) (e1 = 0 when y0 + 1 >= h).  The rows [y0 + 1 - d, y0 + d], clipped, are common to both windows
// and read once; each output adds at most one row.  plane: h rows of wpr words; d >= 1.  No row outside [0, h) is read; the bits at
// x >= w stay 0 because they are 0 in every word read.
CRIS_HD void morph_col_pair_or(const uint64_t* __restrict__ plane, int wpr, int h, int y0, int c, int d, uint64_t* e0, uint64_t* e1) {
    const long a = (long)y0 + 1 - d > 0 ? (long)y0 + 1 - d : 0, b = (long)y0 + d < h - 1 ? (long)y0 + d : h - 1;
    uint64_t core = 0;
    for (long y = a; y <= b; ++y) core |= plane[(size_t)y * wpr + c];
    *e0 = *e1 = core;
    if ((long)y0 - d >= 0) *e0 |= plane[(size_t)(y0 - d) * wpr + c];
    if ((long)y0 + 1 + d < h) *e1 |= plane[(size_t)((long)y0 + 1 + d) * wpr + c];
    if (y0 + 1 >= h) *e1 = 0;
}

// Column pass of E': the same two windows with AND - a row outside [0, h) clips the window, it does not empty it
CRIS_HD void morph_col_pair_and_clipped(const uint64_t* __restrict__ plane, int wpr, int h, int y0, int c, int d, uint64_t* e0, uint64_t* e1) {
    const long a = (long)y0 + 1 - d > 0 ? (long)y0 + 1 - d : 0, b = (long)y0 + d < h - 1 ? (long)y0 + d : h - 1;
    uint64_t core = ~0ull;
    for (long y = a; y <= b; ++y) core &= plane[(size_t)y * wpr + c];
    *e0 = *e1 = core;
    if ((long)y0 - d >= 0) *e0 &= plane[(size_t)(y0 - d) * wpr + c];
    if ((long)y0 + 1 + d < h) *e1 &= plane[(size_t)((long)y0 + 1 + d) * wpr + c];
    if (y0 + 1 >= h) *e1 = 0;
}
