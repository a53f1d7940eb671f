// TEST INFRASTRUCTURE (built by tests/test_polygon_cpu.py with g++, address and undefined-behaviour sanitizers on): runs the per-vertex
// arithmetic of the polygon tracer - the very header csrc/polygon.hip includes, csrc/polygon_core.h - on the CPU, with loops in
// place of the launch grid, and prints both corner-visit lists of every mask for the test to compare with its per-crack oracle.
// The masks are exact-size vectors read with at(), so a pixel outside the image is an error of the run.
//   probe <file>    the file: the number of masks, then per mask "h w" and h rows of w characters 0 / 1
//   prints per mask "mask <index> <visits>", then "R x y he vs outv" per visit in row-major and "C x y he vs outv" in column-major order
#define CRIS_HD inline
#include "../cris/pytorch_amd/csrc/polygon_core.h"
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

struct Mask {
    int h, w;
    std::vector<unsigned char> px;
    int at(int x, int y) const { return x >= 0 && x < w && y >= 0 && y < h ? px.at((size_t)y * w + x) != 0 : 0; }
};

static void print_visit(char list, int x, int y, int bits) {
    std::printf("%c %d %d %d %d %d\n", list, x, y, bits & PG_HE ? 1 : 0, bits & PG_VS ? 1 : 0, bits & PG_OUTV ? 1 : 0);
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int n = 0;
    if (std::fscanf(f, "%d", &n) != 1 || n < 0) return 2;
    for (int i = 0; i < n; ++i) {
        Mask m;
        if (std::fscanf(f, "%d %d", &m.h, &m.w) != 2 || m.h < 1 || m.w < 1) return 2;
        m.px.resize((size_t)m.h * m.w);
        for (int y = 0; y < m.h; ++y) {
            char row[4096];
            if (m.w >= (int)sizeof(row) || std::fscanf(f, "%4095s", row) != 1 || (int)std::string(row).size() != m.w) return 2;
            for (int x = 0; x < m.w; ++x) m.px.at((size_t)y * m.w + x) = row[x] == '1';
        }
        long visits = 0;
        for (int y = 0; y <= m.h; ++y)
            for (int x = 0; x <= m.w; ++x) visits += pg_visits(m.at(x - 1, y - 1), m.at(x, y - 1), m.at(x - 1, y), m.at(x, y));
        std::printf("mask %d %ld\n", i, visits);
        for (int y = 0; y <= m.h; ++y)
            for (int x = 0; x <= m.w; ++x) {
                const int a = m.at(x - 1, y - 1), b = m.at(x, y - 1), c = m.at(x - 1, y), d = m.at(x, y);
                for (int k = 0; k < pg_visits(a, b, c, d); ++k) print_visit('R', x, y, pg_visit_row(a, b, c, d, k));
            }
        for (int x = 0; x <= m.w; ++x)
            for (int y = 0; y <= m.h; ++y) {
                const int a = m.at(x - 1, y - 1), b = m.at(x, y - 1), c = m.at(x - 1, y), d = m.at(x, y);
                for (int k = 0; k < pg_visits(a, b, c, d); ++k) print_visit('C', x, y, pg_visit_col(a, b, c, d, k));
            }
    }
    std::fclose(f);
    return 0;
}
