// Corner visits of the crack-following polygon tracer: the per-vertex arithmetic of csrc/polygon.hip, host and
// device (the style of morph_core.h: the same functions compile for a host program that checks them against a per-crack oracle).
//
// A vertex is a pixel corner (x, y), 0 <= x <= w, 0 <= y <= h; its 2x2 neighbourhood is a = pixel (x - 1, y - 1) [north-west],
// b = (x, y - 1) [north-east], c = (x - 1, y) [south-west], d = (x, y) [south-east], each 0 / 1, outside the image 0.  The unit
// cracks that meet at it: north iff a != b, south iff c != d, west iff a != c, east iff b != d.  Every crack is directed with the
// foreground on the right of travel (y grows downwards): north arrives (heads south) iff a, leaves iff b; south leaves iff c,
// arrives iff d; west leaves iff a, arrives iff c; east arrives iff b, leaves iff d.
//
// A corner visit is one passage of a ring through a vertex at which its direction changes: it uses one horizontal and one
// vertical crack.  A vertex with one of each is visited once; a saddle (a == d != b == c) has all four and is visited twice, each
// visit turning right around its own pixel (turn right before straight before left): for a == d == 1 the visits are {north, west}
// and {south, east}, for b == c == 1 they are {west, south} and {east, north}.  Every other vertex is no corner.
//
// A visit is three bits: PG_HE the horizontal crack is the east one, PG_VS the vertical crack is the south one, PG_OUTV the ring
// LEAVES the vertex on the vertical crack (else on the horizontal one).  Integers only.
#pragma once

#ifndef CRIS_HD
#define CRIS_HD __host__ __device__ __forceinline__
#endif

#define PG_HE 1
#define PG_VS 2
#define PG_OUTV 4

// the corner visits of a vertex: 0, 1 or 2
CRIS_HD int pg_visits(int a, int b, int c, int d) {
    const int horizontal = (a != c) + (b != d), vertical = (a != b) + (c != d);
    if (horizontal == 2 && vertical == 2) return 2;
    return horizontal == 1 && vertical == 1;
}

// the visit that uses the east (he = 1) or west (he = 0) crack; the vertex has that crack and is a corner
CRIS_HD int pg_visit_of_horizontal(int a, int b, int c, int d, int he) {
    int vs;
    if (a == d && b == c) vs = a ? he : !he;                              // saddle: the pairing of the turn-right rule
    else vs = c != d;
    const int outv = vs ? c : b;                                          // the south crack leaves iff c, the north one iff b
    return (he ? PG_HE : 0) | (vs ? PG_VS : 0) | (outv ? PG_OUTV : 0);
}

// visit k (0 <= k < pg_visits) in ROW-major order: the west-connected copy of a saddle before the east-connected one
CRIS_HD int pg_visit_row(int a, int b, int c, int d, int k) {
    const bool saddle = a == d && b == c;
    return pg_visit_of_horizontal(a, b, c, d, saddle ? k : (b != d));
}

// visit k in COLUMN-major order: the north-connected copy of a saddle before the south-connected one
CRIS_HD int pg_visit_col(int a, int b, int c, int d, int k) {
    const bool saddle = a == d && b == c;
    if (!saddle) return pg_visit_of_horizontal(a, b, c, d, b != d);
    return pg_visit_of_horizontal(a, b, c, d, a ? k : !k);               // vs == k: a == 1 pairs vs = he, b == 1 pairs vs = !he
}
