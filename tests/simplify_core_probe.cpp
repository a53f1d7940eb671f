// TEST INFRASTRUCTURE (built by tests/test_polygon_simplify_cpu.py with g++, address and undefined-behaviour sanitizers on): runs the
// arithmetic of the Douglas-Peucker simplifier - the very header csrc/simplify.hip includes, csrc/simplify_core.h - on the CPU, one
// segment at a time from a stack in place of the kernel's rounds, and prints the indices every ring keeps for the test to compare
// with its recursive oracle.  The rings are exact-size vectors read with at(), so an index outside a ring is an error of the run,
// and the undefined-behaviour sanitizer watches the 64-bit products of the split test.
//   probe <file>    the file: the number of rings, then per ring "k q" and k lines "x y"
//   prints per ring "ring <index> <kept>" and one line of the kept indices in ascending order
#define CRIS_HD inline
#include "../cris/pytorch_amd/csrc/simplify_core.h"
#include <algorithm>
#include <cstdio>
#include <utility>
#include <vector>

struct Ring {
    std::vector<int> x, y;      // k + 1 positions: position k is v_0 again
};

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int n = 0;
    if (std::fscanf(f, "%d", &n) != 1 || n < 0) return 2;
    for (int r = 0; r < n; ++r) {
        int k = 0, q = 0;
        if (std::fscanf(f, "%d %d", &k, &q) != 2 || k < 3 || q < 1 || q > SP_MAX_Q) return 2;
        Ring g;
        g.x.resize((size_t)k + 1);
        g.y.resize((size_t)k + 1);
        for (int i = 0; i < k; ++i)
            if (std::fscanf(f, "%d %d", &g.x.at(i), &g.y.at(i)) != 2 || g.x.at(i) < 0 || g.x.at(i) > SP_MAX_SIDE || g.y.at(i) < 0 || g.y.at(i) > SP_MAX_SIDE) return 2;
        g.x.at(k) = g.x.at(0);
        g.y.at(k) = g.y.at(0);
        unsigned long long far = 0;
        for (int i = 0; i < k; ++i) far = std::max(far, sp_anchor_key(sp_len2(g.x.at(0), g.y.at(0), g.x.at(i), g.y.at(i)), i));
        const int a = (int)sp_anchor_index(far);
        if (a < 1 || a >= k) return 3;
        std::vector<char> kept((size_t)k + 1, 0);
        kept.at(0) = kept.at(a) = 1;
        std::vector<std::pair<int, int>> todo{{0, a}, {a, k}};
        while (!todo.empty()) {
            const int i = todo.back().first, j = todo.back().second;
            todo.pop_back();
            if (j - i < 2) continue;
            unsigned long long best = 0;
            for (int m = i + 1; m < j; ++m)
                best = std::max(best, sp_key(sp_cross(g.x.at(i), g.y.at(i), g.x.at(j), g.y.at(j), g.x.at(m), g.y.at(m)), i, j, m));
            const long long c = sp_key_cross(best), m = sp_key_index(best, i, j);
            if (m <= i || m >= j) return 3;
            if (!sp_split(c, q, sp_len2(g.x.at(i), g.y.at(i), g.x.at(j), g.y.at(j)))) continue;
            kept.at((size_t)m) = 1;
            todo.push_back({i, (int)m});
            todo.push_back({(int)m, j});
        }
        std::printf("ring %d %d\n", r, (int)std::count(kept.begin(), kept.begin() + k, 1));
        for (int i = 0; i < k; ++i)
            if (kept.at(i)) std::printf("%d ", i);
        std::printf("\n");
    }
    std::fclose(f);
    return 0;
}
