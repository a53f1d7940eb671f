// TEST INFRASTRUCTURE (built by tests/test_boundary_cpu.py with g++, address and undefined-behaviour sanitizers on): runs the
// per-word arithmetic of the erosion kernels - the very header csrc/morph.hip includes, csrc/morph_core.h - on the CPU, with loops in
// place of the launch grid, against a per-pixel loop over random and nearly full masks: widths and radii around the 64-bit word,
// heights around the window.  The planes are exact-size vectors, so an index outside a row or a plane is an error of the run.
//   probe <iterations>    prints "ok <bits compared>"
#define CRIS_HD inline
#define __restrict__
#include "../cris/pytorch_amd/csrc/morph_core.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

static uint64_t state = 0x9E3779B97F4A7C15ull;
static unsigned rnd(unsigned n) {                                           // (an LCG of its own: the same cases everywhere)
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(state >> 33) % n;
}

int main(int argc, char** argv) {
    const int iterations = argc > 1 ? atoi(argv[1]) : 1000;
    static const int widths[] = {1, 3, 63, 64, 65, 127, 128, 129, 200, 256, 320};
    long compared = 0;
    for (int it = 0; it < iterations; ++it) {
        int h = 1 + (int)rnd(140), w = 1 + (int)rnd(330), d = 1 + (int)rnd(70);
        if (it % 3 == 0) d = 1 + (int)rnd(4);
        if (it % 7 == 0) w = widths[rnd(11)];
        if (it % 5 == 0) h = 2 * d + (int)rnd(3);                           // one short of the window, the window, one more
        const int kind = (int)rnd(4);                                       // full, or one background pixel in 1000 / 300 / 50
        const unsigned one_in = kind == 1 ? 1000 : kind == 2 ? 300 : 50;
        std::vector<unsigned char> fg((size_t)h * w);
        for (auto& b : fg) b = kind == 0 ? 1 : rnd(one_in) != 0;
        const int wpr = (w + 63) / 64;
        std::vector<uint64_t> raw((size_t)h * wpr, 0), rowp((size_t)h * wpr, 0xdeadbeefdeadbeefull);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x)
                if (fg[(size_t)y * w + x]) raw[(size_t)y * wpr + x / 64] |= 1ull << (x % 64);
        const bool empty = morph_empty(h, w, d);
        for (int y = 0; y < h; ++y)
            for (int c = 0; c < wpr; ++c) rowp[(size_t)y * wpr + c] = empty ? 0 : morph_row_word(&raw[(size_t)y * wpr], wpr, c, d);
        std::vector<unsigned char> roww((size_t)h * 64 * wpr, 0);           // the row pass, pixel by pixel
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < 64 * wpr; ++x) {
                bool want = x < w;
                for (int s = -d; s <= d && want; ++s) want = x + s >= 0 && x + s < w && fg[(size_t)y * w + x + s];
                roww[(size_t)y * 64 * wpr + x] = want;
                if (!empty && (((rowp[(size_t)y * wpr + x / 64] >> (x % 64)) & 1) != 0) != want) {
                    printf("row pass: h %d w %d d %d y %d x %d\n", h, w, d, y, x);
                    return 1;
                }
            }
        for (int y0 = 0; y0 < h; y0 += 2)
            for (int c = 0; c < wpr; ++c) {
                uint64_t e[2] = {0, 0};
                if (!empty) morph_col_pair(rowp.data(), wpr, h, y0, c, d, &e[0], &e[1]);
                for (int k = 0; k < 2; ++k) {
                    const int y = y0 + k;
                    if (y >= h) {
                        if (e[k]) return 2;
                        continue;
                    }
                    for (int i = 0; i < 64; ++i) {
                        const int x = 64 * c + i;
                        bool want = x < w;
                        for (int s = -d; s <= d && want; ++s) want = y + s >= 0 && y + s < h && roww[(size_t)(y + s) * 64 * wpr + x];
                        if ((((e[k] >> i) & 1) != 0) != want) {
                            printf("column pass: h %d w %d d %d y %d x %d\n", h, w, d, y, x);
                            return 1;
                        }
                        ++compared;
                    }
                }
            }
    }
    printf("ok %ld\n", compared);
    return 0;
}
