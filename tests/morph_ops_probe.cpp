// TEST INFRASTRUCTURE (built by tests/test_morph_cpu.py with g++, address and undefined-behaviour sanitizers on): runs the per-word
// arithmetic of the dilation and of the clipped erosion - the very header csrc/morph.hip includes, csrc/morph_core.h - on the CPU,
// with loops in place of the launch grid, against per-pixel loops: the widths and radii of tests/morph_cases.py and random ones
// around the 64-bit word, heights around the window, sparse and dense masks.  The planes are exact-size vectors, so an index outside
// a row or a plane is an error of the run; the row plane's bits at x >= w must come out 0.
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

// one shape, one radius, one density: both operations, row pass then column pass.  -> bits compared, or -1
static long run(int h, int w, int d, unsigned one_in, bool dense) {
    std::vector<unsigned char> fg((size_t)h * w);
    for (auto& b : fg) b = one_in == 0 ? dense : ((rnd(one_in) == 0) != dense);          // sparse 1s for D, sparse 0s for E'
    const int wpr = (w + 63) / 64;
    std::vector<uint64_t> raw((size_t)h * wpr, 0);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
            if (fg[(size_t)y * w + x]) raw[(size_t)y * wpr + x / 64] |= 1ull << (x % 64);
    long compared = 0;
    for (int op = 0; op < 2; ++op) {                                        // 0: D, 1: E'
        std::vector<uint64_t> rowp((size_t)h * wpr, 0xdeadbeefdeadbeefull);
        for (int y = 0; y < h; ++y)
            for (int c = 0; c < wpr; ++c)
                rowp[(size_t)y * wpr + c] = op == 0 ? morph_row_dilate_word(&raw[(size_t)y * wpr], wpr, w, c, d)
                                                    : morph_row_erode_clipped_word(&raw[(size_t)y * wpr], wpr, w, c, d);
        std::vector<unsigned char> roww((size_t)h * w, 0);                  // the row pass, pixel by pixel
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < 64 * wpr; ++x) {
                const bool got = ((rowp[(size_t)y * wpr + x / 64] >> (x % 64)) & 1) != 0;
                if (x >= w) {
                    if (got) {
                        printf("row pass op %d: a bit at x >= w: h %d w %d d %d y %d x %d\n", op, h, w, d, y, x);
                        return -1;
                    }
                    continue;
                }
                bool want = op == 1;
                for (int s = -d; s <= d; ++s) {
                    if (x + s < 0 || x + s >= w) continue;                  // clipped: nothing outside the image exists
                    const bool b = fg[(size_t)y * w + x + s] != 0;
                    want = op == 0 ? (want || b) : (want && b);
                }
                roww[(size_t)y * w + x] = want;
                if (got != want) {
                    printf("row pass op %d: h %d w %d d %d y %d x %d\n", op, h, w, d, y, x);
                    return -1;
                }
                ++compared;
            }
        for (int y0 = 0; y0 < h; y0 += 2)
            for (int c = 0; c < wpr; ++c) {
                uint64_t e[2] = {0xdeadbeefdeadbeefull, 0xdeadbeefdeadbeefull};
                if (op == 0) morph_col_pair_or(rowp.data(), wpr, h, y0, c, d, &e[0], &e[1]);
                else morph_col_pair_and_clipped(rowp.data(), wpr, h, y0, c, d, &e[0], &e[1]);
                for (int k = 0; k < 2; ++k) {
                    const int y = y0 + k;
                    if (y >= h) {
                        if (e[k]) {
                            printf("column pass op %d: a row past the image is not 0: h %d w %d d %d\n", op, h, w, d);
                            return -1;
                        }
                        continue;
                    }
                    for (int i = 0; i < 64; ++i) {
                        const int x = 64 * c + i;
                        bool want = x < w && op == 1;
                        for (int s = -d; s <= d && x < w; ++s) {
                            if (y + s < 0 || y + s >= h) continue;
                            const bool b = roww[(size_t)(y + s) * w + x] != 0;
                            want = op == 0 ? (want || b) : (want && b);
                        }
                        if ((((e[k] >> i) & 1) != 0) != want) {
                            printf("column pass op %d: h %d w %d d %d y %d x %d\n", op, h, w, d, y, x);
                            return -1;
                        }
                        ++compared;
                    }
                }
            }
    }
    return compared;
}

int main(int argc, char** argv) {
    const int iterations = argc > 1 ? atoi(argv[1]) : 600;
    static const int widths[] = {1, 3, 63, 64, 65, 127, 128, 129, 200, 256, 320};
    static const int radii[] = {1, 2, 31, 32, 33, 63, 64, 65};
    long compared = 0;
    // every width of the cases at every radius of the cases, heights 1, 2 d, 2 d + 1, 2 d + 2 in turn
    int k = 0;
    for (int wi = 0; wi < 11; ++wi)
        for (int ri = 0; ri < 8; ++ri, ++k) {
            const int d = radii[ri], hs[4] = {1, 2 * d, 2 * d + 1, 2 * d + 2};
            const long n = run(hs[k % 4], widths[wi], d, 40, (k & 1) != 0);
            if (n < 0) return 1;
            compared += n;
        }
    for (int it = 0; it < iterations; ++it) {
        int h = 1 + (int)rnd(140), w = 1 + (int)rnd(330), d = 1 + (int)rnd(70);
        if (it % 3 == 0) d = 1 + (int)rnd(4);
        if (it % 7 == 0) w = widths[rnd(11)];
        if (it % 5 == 0) h = 2 * d + (int)rnd(3);
        if (it % 11 == 0) d = 100 + (int)rnd(400);                          // a window wider than the whole image
        const int kind = (int)rnd(5);                                       // uniform, or one odd pixel in 1000 / 300 / 50 / 3
        const unsigned one_in = kind == 0 ? 0 : kind == 1 ? 1000 : kind == 2 ? 300 : kind == 3 ? 50 : 3;
        const long n = run(h, w, d, one_in, rnd(2) != 0);
        if (n < 0) return 1;
        compared += n;
    }
    printf("ok %ld\n", compared);
    return 0;
}
