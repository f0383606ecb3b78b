// Ignore regions of the train step (mask format: include/mrcnn_hip.h, "Packed masks"):
//   mask_union_pack — (G, H, W) uint8 masks -> ONE bit plane, their union (or base & ~union)
//   box_coverage    — per box, the number of set bits of a plane inside the rounded box, and the
//                     box's pixel count
// Replaces Detectron's crowd filter (roi_data_loader / roidb.py `_filter_crowd_proposals`: box
// overlap of every proposal with every crowd BOX, on the host) with the pixel coverage of the
// crowd MASKS; the reference trains with use_crowd=False and has neither.  Integer arithmetic
// after the rounding of the box (popcounts, shuffles): every result is exact and independent of
// scheduling.  No LDS, no atomics.
#include "common.h"

#include <math.h>

namespace {

constexpr int kWaves = 4;                             // wavefronts per workgroup, both kernels

// One wavefront per output word, one lane per pixel: a 64-lane __ballot of "any masks[g] byte of
// this pixel is nonzero" IS the word (bit l = lane l).  Lanes past W vote 0, so the pad bits of
// the row's last word are zero whatever base holds there.
__global__ void __launch_bounds__(64 * kWaves)
mask_union_pack_kernel(const uint8_t *__restrict__ masks, int G, int H, int W, int Wq,
                       const uint64_t *__restrict__ base, uint64_t *__restrict__ plane)
{
    const int lane = threadIdx.x & 63;
    const int64_t word = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);   // y * Wq + wq
    if (word >= (int64_t)H * Wq) return;              // wave-uniform
    const int y = (int)(word / Wq), wq = (int)(word - (int64_t)y * Wq);
    const int x = (wq << 6) + lane;
    const bool inside = x < W;
    bool any = false;
    if (inside) {
        const uint8_t *p = masks + (int64_t)y * W + x;
        const int64_t step = (int64_t)H * W;
        for (int g = 0; g < G; ++g) any |= p[g * step] != 0;
    }
    const uint64_t u = __ballot(any);
    const uint64_t valid = __ballot(inside);
    if (lane == 0) plane[word] = base ? (base[word] & ~u & valid) : u;
}

// Wave-wide integer sum (wave64).
__device__ __forceinline__ int wave_sum(int v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// round half to even, then clamp to [0, hi].  The first clamp is in float, to the largest float
// below 2^31, so that 1e30 or -1e30 never reaches the conversion; (float)hi itself may round UP,
// hence the exact clamp after it.  The caller has excluded NaN and the infinities.
__device__ __forceinline__ int round_clamp(float v, int hi)
{
    return min((int)fminf(fmaxf(rintf(v), 0.f), 2147483520.f), hi);
}

// One wavefront per box.  The rectangle spans words [wq0, wq1] of rows [y0, y1): the lanes stride
// over its (row, word) pairs, the first and last word of a row masked to columns [x0, x1).
__global__ void __launch_bounds__(64 * kWaves)
box_coverage_kernel(const uint64_t *__restrict__ plane, int H, int W, int Wq,
                    const float *__restrict__ boxes, int n, int32_t *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (b >= n) return;                               // wave-uniform
    const float *bx = boxes + 4 * (int64_t)b;
    const float fy0 = bx[0], fx0 = bx[1], fy1 = bx[2], fx1 = bx[3];
    int covered = 0, area = 0;
    if (isfinite(fy0) && isfinite(fx0) && isfinite(fy1) && isfinite(fx1)) {
        const int y0 = round_clamp(fy0, H), x0 = round_clamp(fx0, W);
        const int y1 = round_clamp(fy1, H), x1 = round_clamp(fx1, W);
        const int h = max(y1 - y0, 0), w = max(x1 - x0, 0);
        area = h * w;                                 // <= H * W < 2^31
        if (area > 0) {
            const int wq0 = x0 >> 6, wq1 = (x1 - 1) >> 6, nw = wq1 - wq0 + 1;
            const uint64_t first = ~0ull << (x0 & 63);
            const uint64_t last = ~0ull >> (63 - ((x1 - 1) & 63));
            const uint64_t *src = plane + (int64_t)y0 * Wq + wq0;
            const int total = h * nw;                 // <= H * Wq
            for (int i = lane; i < total; i += 64) {
                const int r = i / nw, k = i - r * nw;
                uint64_t bits = src[(int64_t)r * Wq + k];
                if (k == 0) bits &= first;
                if (k == nw - 1) bits &= last;
                covered += __popcll(bits);
            }
            covered = wave_sum(covered);
        }
    }
    if (lane == 0) *reinterpret_cast<int2 *>(out + 2 * (int64_t)b) = make_int2(covered, area);
}

}  // namespace

extern "C" int mrcnn_mask_union_pack(const uint8_t *masks, int G, int H, int W,
                                     const uint64_t *base, uint64_t *plane, void *stream)
{
    MRCNN_REQUIRE(G >= 0 && H > 0 && W > 0, "mask_union_pack: bad shape");
    MRCNN_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), "mask_union_pack: H*W >= 2^31");
    MRCNN_REQUIRE(plane && (masks || G == 0), "mask_union_pack: null pointer");
    MRCNN_REQUIRE((const uint64_t *)plane != base, "mask_union_pack: base may not alias plane");
    const int Wq = (W + 63) / 64;
    const int64_t words = (int64_t)H * Wq;
    hipLaunchKernelGGL(mask_union_pack_kernel, dim3((unsigned)mrcnn::ceil_div(words, kWaves)),
                       dim3(64 * kWaves), 0, mrcnn::as_stream(stream), masks, G, H, W, Wq, base,
                       plane);
    return mrcnn::check_launch("mask_union_pack");
}

extern "C" int mrcnn_box_coverage(const uint64_t *plane, int H, int W, const float *boxes, int n,
                                  int32_t *out, void *stream)
{
    MRCNN_REQUIRE(H > 0 && W > 0 && n >= 0, "box_coverage: bad shape");
    MRCNN_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), "box_coverage: H*W >= 2^31");
    if (n == 0) return 0;
    MRCNN_REQUIRE(plane && boxes && out, "box_coverage: null pointer");
    MRCNN_REQUIRE(((uintptr_t)out & 7) == 0, "box_coverage: out must be 8-byte aligned");
    const int Wq = (W + 63) / 64;
    hipLaunchKernelGGL(box_coverage_kernel, dim3((unsigned)mrcnn::ceil_div(n, kWaves)),
                       dim3(64 * kWaves), 0, mrcnn::as_stream(stream), plane, H, W, Wq, boxes, n,
                       out);
    return mrcnn::check_launch("box_coverage");
}
