// TEST INFRASTRUCTURE (built by tests/test_mask_decode_cpu.py with g++, address and undefined-behaviour sanitizers on): runs the
// arithmetic of the mask decoders - the very header csrc/decode.hip includes, csrc/decode_core.h - on the CPU, with loops in place of
// the launch grids, and prints every decoded mask for the test to compare with rle.decode / polygon.decode.  Run ends, planes and
// slots are exact-size vectors (the slot with a guard dword on either side), so an index outside them is an error of the run.
//   probe <file>    the file: the number of masks, then per mask either
//                       R h w n c_0 .. c_n-1                         an RLE of n counts
//                       P h w r  k_0 x y x y ..  k_1 x y ..          a polygon of r rings of k_i vertices
//   prints per mask "mask <index> <h> <w> <pitch>", then h rows of pitch characters 0 / 1 (the slot's bytes: 255 -> 1, 0 -> 0;
//   any other byte -> ?)
#define CRIS_HD inline
#include "../cris/pytorch_amd/csrc/decode_core.h"
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

static const uint32_t GUARD = 0x7f7f7f7fu;

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int n = 0;
    if (std::fscanf(f, "%d", &n) != 1 || n < 0) return 2;
    for (int i = 0; i < n; ++i) {
        char kind[4];
        int h, w, m;
        if (std::fscanf(f, "%1s %d %d %d", kind, &h, &w, &m) != 4 || h < 1 || w < 1 || m < 0) return 2;
        const int pitch = (w + 3) / 4 * 4, dpr = pitch / 4, wpr = (w + 63) / 64;
        std::vector<uint32_t> slot((size_t)h * dpr + 2, GUARD);                // [guard | h * pitch bytes | guard]
        if (kind[0] == 'R') {
            std::vector<uint32_t> counts(m), ends(m);
            for (int j = 0; j < m; ++j)
                if (std::fscanf(f, "%u", &counts.at(j)) != 1) return 2;
            uint32_t carry = 0;                                                 // the scan launch, one chunk of 256 at a time
            for (int base = 0; base < m; base += 256) {
                uint32_t run = 0;
                for (int j = base; j < m && j < base + 256; ++j) {
                    run += counts.at(j);
                    ends.at(j) = carry + run;
                }
                carry += run;
            }
            for (long t = 0; t < (long)h * dpr; ++t)                            // the store launch
                slot.at(1 + t) = decode_bytes(decode_rle_bits(ends.data(), m, h, w, (int)(t % dpr) * 4, (int)(t / dpr)));
        } else if (kind[0] == 'P') {
            std::vector<long long> rings;                                       // rows of (mask, offset, length)
            std::vector<int> xy;
            for (int r = 0; r < m; ++r) {
                int k;
                if (std::fscanf(f, "%d", &k) != 1 || k < 1) return 2;
                rings.insert(rings.end(), {(long long)i, (long long)(xy.size() / 2), (long long)k});
                for (int j = 0; j < 2 * k; ++j) {
                    int v;
                    if (std::fscanf(f, "%d", &v) != 1) return 2;
                    xy.push_back(v);
                }
            }
            std::vector<unsigned long long> plane((size_t)h * wpr, 0ull);       // the memset
            const long long nv = (long long)xy.size() / 2;
            for (long long g = 0; g < nv; ++g) {                                // the toggle launch: one thread per vertex
                const long r = decode_ring_of(rings.data(), 3, 0, m, g);
                const long long off = rings.at(3 * r + 1), len = rings.at(3 * r + 2);
                if (g < off || g >= off + len) return 3;                        // the search named another ring
                const long long nx = g + 1 < off + len ? g + 1 : off;
                decode_edge(xy.at(2 * g), xy.at(2 * g + 1), xy.at(2 * nx), xy.at(2 * nx + 1), h, w,
                            [&](int px, int py) { plane.at((size_t)py * wpr + (px >> 6)) ^= 1ull << (px & 63); });
            }
            for (long t = 0; t < (long)h * dpr; ++t) {                          // the store launch
                const int y = (int)(t / dpr), x = (int)(t % dpr) * 4;
                std::vector<unsigned long long> row(plane.begin() + (size_t)y * wpr, plane.begin() + (size_t)(y + 1) * wpr);   // exact size
                slot.at(1 + t) = decode_bytes(decode_plane_bits(row.data(), w, x));
            }
        } else {
            return 2;
        }
        if (slot.front() != GUARD || slot.back() != GUARD) return 4;
        std::printf("mask %d %d %d %d\n", i, h, w, pitch);
        const unsigned char* bytes = reinterpret_cast<const unsigned char*>(slot.data() + 1);
        std::string line((size_t)pitch, '0');
        for (int y = 0; y < h; ++y) {
            for (int x = 0; x < pitch; ++x) {
                const unsigned char b = bytes[(size_t)y * pitch + x];
                line[(size_t)x] = b == 255 ? '1' : b == 0 ? '0' : '?';
            }
            std::printf("%s\n", line.c_str());
        }
    }
    std::fclose(f);
    return 0;
}
