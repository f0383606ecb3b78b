// Host run of the per-word functions of csrc/mask_boundary.h, thread for thread as the two
// kernels of mask_boundary.hip call them: tests/test_boundary_cpu.py compiles this program (with
// the undefined-behaviour sanitizer) and compares its output with the NumPy rule.  The workspace
// starts as garbage and the output as ones, so a word read or left unwritten by mistake shows.
//   input  (binary file): int32 N, H, W, d; uint64 packed[N*H*Wq]; int32 extent[N*4]
//   output (binary file): uint64 out[N*H*Wq]; int32 area[N]
#include <cstdint>
#include <cstdio>
#include <vector>

#include "mask_boundary.h"

using namespace mrcnn_mb;

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[4];
    if (fread(hdr, sizeof(int32_t), 4, f) != 4) return 2;
    const int N = hdr[0], H = hdr[1], W = hdr[2], d = hdr[3];
    const int Wq = (W + 63) / 64;
    const size_t words = (size_t)N * H * Wq;
    std::vector<uint64_t> packed(words), eh(words, 0xA5A5A5A5A5A5A5A5ull), out(words, ~(uint64_t)0);
    std::vector<int32_t> extent((size_t)N * 4), area(N, -1);
    if (fread(packed.data(), sizeof(uint64_t), words, f) != words) return 2;
    if (fread(extent.data(), sizeof(int32_t), extent.size(), f) != extent.size()) return 2;
    fclose(f);
    const int q = d >> 6, r = d & 63;
    const int strips = (H + STRIP - 1) / STRIP;
    for (int n = 0; n < N; ++n) {
        const Window e = clamp_extent(extent.data() + 4 * n, H, Wq);
        const size_t base = (size_t)n * H * Wq;
        area[n] = 0;
        for (int y = e.y_lo; y < e.y_hi; ++y)                 // erode_rows_kernel
            for (int w = e.w_lo; w < e.w_hi; ++w)
                eh[base + (size_t)y * Wq + w] =
                    erode_row_word(packed.data() + base + (size_t)y * Wq, w, e, q, r);
        for (int s = 0; s < strips; ++s)                      // boundary_kernel
            for (int w = 0; w < Wq; ++w) {
                const int y0 = s * STRIP;
                const bool inside = w >= e.w_lo && w < e.w_hi && y0 < e.y_hi && y0 + STRIP > e.y_lo;
                uint64_t E[STRIP] = {};
                if (inside) erode_strip(eh.data() + base, Wq, w, y0, d, e, E);
                for (int i = 0; i < STRIP && y0 + i < H; ++i) {
                    const int y = y0 + i;
                    uint64_t b = 0;
                    if (inside && y >= e.y_lo && y < e.y_hi)
                        b = packed[base + (size_t)y * Wq + w] & ~E[i];
                    out[base + (size_t)y * Wq + w] = b;
                    area[n] += __builtin_popcountll(b);
                }
            }
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(out.data(), sizeof(uint64_t), words, f);
    fwrite(area.data(), sizeof(int32_t), area.size(), f);
    fclose(f);
    return 0;
}
