// The integer arithmetic of the Douglas-Peucker simplifier of traced rings: the distance key, its tie order, the split predicate and
// the anchor key of csrc/simplify.hip, host and device (the style of polygon_core.h: the same functions compile
// for a host program that checks them against a plain recursive oracle).
//
// A ring is v_0 .. v_k-1 with v_k = v_0; the kept set starts as {0, a}, a = the smallest index that maximises |v_i - v_0|^2.  For
// a segment (i, j), j - i >= 2, d = v_j - v_i and len2 = d.d, every m in (i, j) has c_m = |d.x (v_m - v_i).y - d.y (v_m - v_i).x|.
// The split candidate is the m of greatest c_m, among equals the one nearest the middle (smallest |2 m - (i + j)|), among those
// the smallest m; it is kept, and both halves go on, iff 16 c_m^2 > q^2 len2 (strict), q = 4 epsilon in 1 .. 256.
//
// The 64-bit bound.  Simplification needs h, w <= SP_MAX_SIDE = 32767 and the format has (h + 1) (w + 1) <= 2^28, so with every
// coordinate difference in [-w, w] x [-h, h]: |cross| <= 2 h w < 2^29, hence 16 cross^2 < 2^62; len2 <= h^2 + w^2 < 2^31 and
// q^2 <= 2^16, hence q^2 len2 < 2^47.  Every comparison below therefore fits a signed 64-bit integer, and a key - c in the high
// word, the tie order in the low one - fits an unsigned one as long as j - i < 2^31.
#pragma once

#ifndef CRIS_HD
#define CRIS_HD __host__ __device__ __forceinline__
#endif

#define SP_MAX_SIDE 32767       // h_out and w_out of a mask that is simplified
#define SP_MAX_Q 256            // q = 4 epsilon, epsilon a multiple of 0.25 in [0.25, 64]

// c_m of vertex m against the segment from vertex i to vertex j: < 2^29
CRIS_HD long long sp_cross(int xi, int yi, int xj, int yj, int xm, int ym) {
    const long long c = (long long)(xj - xi) * (ym - yi) - (long long)(yj - yi) * (xm - xi);
    return c < 0 ? -c : c;
}

CRIS_HD long long sp_len2(int xi, int yi, int xj, int yj) {
    return (long long)(xj - xi) * (xj - xi) + (long long)(yj - yi) * (yj - yi);
}

// the key of candidate m of segment (i, j): a greater key is a better candidate.  With t = 2 m - (i + j) the tie order (|t|, then
// m) is the order of u = 2 |t| + (t > 0), u < 2 (j - i) < 2^32
CRIS_HD unsigned long long sp_key(long long c, long long i, long long j, long long m) {
    const long long t = 2 * m - (i + j);
    const unsigned long long u = 2ull * (unsigned long long)(t < 0 ? -t : t) + (t > 0 ? 1ull : 0ull);
    return ((unsigned long long)c << 32) | (0xffffffffull - (u & 0xffffffffull));
}

CRIS_HD long long sp_key_cross(unsigned long long key) { return (long long)(key >> 32); }

// the m a key of segment (i, j) names (t + i + j = 2 m is even and >= 0)
CRIS_HD long long sp_key_index(unsigned long long key, long long i, long long j) {
    const long long u = (long long)(0xffffffffull - (key & 0xffffffffull));
    const long long t = (u & 1) ? (u >> 1) : -(u >> 1);
    return (t + i + j) / 2;
}

// is the candidate kept: 16 c^2 > q^2 len2, strictly (16 c^2 < 2^62, q^2 len2 < 2^47: see the bound above)
CRIS_HD bool sp_split(long long c, int q, long long len2) { return 16 * c * c > (long long)q * q * len2; }

// the key of vertex `index` as the anchor: the greatest squared distance from v_0 (< 2^31), then the smallest index (< 2^32)
CRIS_HD unsigned long long sp_anchor_key(long long dist2, long long index) {
    return ((unsigned long long)dist2 << 32) | (0xffffffffull - ((unsigned long long)index & 0xffffffffull));
}

CRIS_HD long long sp_anchor_index(unsigned long long key) { return (long long)(0xffffffffull - (key & 0xffffffffull)); }
