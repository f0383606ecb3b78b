// Per-word arithmetic of the mask-boundary kernels (mask_boundary.hip), kept free of HIP so
// that a host program (tests/mask_boundary_host.cpp) can run the same functions over a whole image
// and compare them with the rule.  Everything is 64-bit integer arithmetic on packed words
// (format: include/mrcnn_hip.h, "Packed masks"): bit b of word w is pixel x = 64 w + b, so a
// shift towards lower x is `>>`.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MRCNN_MB_HD __host__ __device__ __forceinline__
#else
#define MRCNN_MB_HD inline
#endif

namespace mrcnn_mb {

constexpr int STRIP = 8;   // output rows per thread of the vertical pass

// The extent of one mask clamped to the image, and its words with everything outside the
// extent reading as zero (the format's promise, so slack in the extent cannot change a result).
struct Window {
    int y_lo, y_hi, w_lo, w_hi;
};

MRCNN_MB_HD Window clamp_extent(const int32_t *e, int H, int Wq)
{
    Window r;
    r.y_lo = e[0] > 0 ? e[0] : 0;
    r.y_hi = e[1] < H ? e[1] : H;
    r.w_lo = e[2] > 0 ? e[2] : 0;
    r.w_hi = e[3] < Wq ? e[3] : Wq;
    return r;
}

MRCNN_MB_HD uint64_t word_at(const uint64_t *row, int w, const Window &e)
{
    return (w >= e.w_lo && w < e.w_hi) ? row[w] : 0;
}

// Low word of AND_{s = 0..k} ((hi:lo) >> s), 0 <= k <= 63: bit b is set iff bits b .. b+k of
// the 128-bit value are.  Doubling: after a step the value is the AND of c+1 shifts; the steps
// are 1, 2, 4, ... and one remainder, each at most 32.
MRCNN_MB_HD uint64_t window_and(uint64_t lo, uint64_t hi, int k)
{
    int c = 0;
    while (c < k) {
        const int s = (c + 1 < k - c) ? c + 1 : k - c;
        lo &= (lo >> s) | (hi << (64 - s));
        hi &= hi >> s;
        c += s;
    }
    return lo;
}

// A[w]: bit b set iff pixels x .. x+d of the row are foreground, x = 64 w + b, d = 64 q + r.
// [x, x+d] is q whole 64-pixel windows followed by one of r+1 pixels.  The loop ends at the
// first empty word, at the latest where the row does (words past the extent are zero).
MRCNN_MB_HD uint64_t run_word(const uint64_t *row, int w, const Window &e, int q, int r)
{
    if (w < e.w_lo || w >= e.w_hi) return 0;
    uint64_t a = ~(uint64_t)0;
    uint64_t cur = row[w];
    for (int j = 0; j < q; ++j) {
        const uint64_t next = word_at(row, w + j + 1, e);
        a &= window_and(cur, next, 63);
        if (!a) return 0;
        cur = next;
    }
    return a & window_and(cur, word_at(row, w + q + 1, e), r);
}

// Horizontal erosion of one word: Eh(x) = A(x) & A(x - d), zeros entering at both image ends
// (left: A of a negative word is zero; right: the pad bits and the words past the row are).
MRCNN_MB_HD uint64_t erode_row_word(const uint64_t *row, int w, const Window &e, int q, int r)
{
    const uint64_t a = run_word(row, w, e, q, r);
    if (!a) return 0;
    uint64_t shifted = run_word(row, w - q, e, q, r);
    if (r) shifted = (shifted << r) | (run_word(row, w - q - 1, e, q, r) >> (64 - r));
    return a & shifted;
}

// Vertical erosion of STRIP rows y0 .. y0+STRIP-1 of word column w from the horizontally
// eroded rows eh (row stride Wq words; only the extent's rows and words were written, the rest
// reads as zero): E(y) = AND_{|j| <= d} Eh(y + j).  The rows shared by all STRIP windows are
// combined once, the others as a suffix below and a prefix above: 2d + STRIP loads instead of
// STRIP (2d + 1).  Windows narrower than the strip (2d < STRIP - 1) are formed one by one.
MRCNN_MB_HD void erode_strip(const uint64_t *eh, int64_t Wq, int w, int y0, int d,
                             const Window &e, uint64_t E[STRIP])
{
    auto at = [&](int64_t y) -> uint64_t {
        return (y >= e.y_lo && y < e.y_hi) ? eh[y * Wq + w] : 0;
    };
    if (2 * (int64_t)d < STRIP - 1) {
        for (int i = 0; i < STRIP; ++i) {
            uint64_t v = ~(uint64_t)0;
            for (int j = -d; j <= d; ++j) v &= at((int64_t)y0 + i + j);
            E[i] = v;
        }
        return;
    }
    // a window reaching outside the extent's rows holds a zero row: nothing to read
    uint64_t core = ~(uint64_t)0;
    const int64_t c_lo = (int64_t)y0 + STRIP - 1 - d, c_hi = (int64_t)y0 + d;   // inclusive
    if (c_lo < e.y_lo || c_hi >= e.y_hi) core = 0;
    for (int64_t y = c_lo; core && y <= c_hi; ++y) core &= at(y);
    if (!core) {
        for (int i = 0; i < STRIP; ++i) E[i] = 0;
        return;
    }
    uint64_t low[STRIP];                       // low[i] = AND Eh(y0+i-d .. c_lo-1)
    low[STRIP - 1] = ~(uint64_t)0;
    for (int i = STRIP - 2; i >= 0; --i) low[i] = low[i + 1] & at((int64_t)y0 + i - d);
    uint64_t high = ~(uint64_t)0;              // AND Eh(c_hi+1 .. y0+i+d)
    for (int i = 0; i < STRIP; ++i) {
        if (i) high &= at((int64_t)y0 + i + d);
        E[i] = core & low[i] & high;
    }
}

}  // namespace mrcnn_mb
