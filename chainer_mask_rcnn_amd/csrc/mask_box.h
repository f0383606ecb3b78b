// Per-row mask records -> per-instance box and area: the second launch of mrcnn_mask_resize_crop
// (scale_jitter.hip) and the third of mrcnn_copy_paste (copy_paste.hip).  A mask kernel leaves one
// (x_lo, x_hi, count) record per output row (x_hi half-open; an empty row has count 0), reduced
// over a wave with the helpers below; mask_box_kernel reduces an instance's S records.  Integer
// min / max / sum only: the result is the same for any order.
#pragma once
#include "common.h"

namespace {

constexpr int kMaskBoxThreads = 256;
constexpr int kMaskBoxWaves = kMaskBoxThreads / 64;

__device__ __forceinline__ int wave_min(int v)
{
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ int wave_max(int v)
{
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ int wave_sum(int v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// One workgroup per instance: its S row records -> box (y_lo, x_lo, y_hi, x_hi) and area.
__global__ void __launch_bounds__(kMaskBoxThreads)
mask_box_kernel(const int32_t *__restrict__ row_stats, int S, int32_t *__restrict__ box,
                int32_t *__restrict__ area)
{
    __shared__ int s_part[kMaskBoxWaves][5];
    const int g = blockIdx.x;
    const int32_t *st = row_stats + (int64_t)g * S * 3;
    int y_lo = S, x_lo = S, y_hi = 0, x_hi = 0, sum = 0;
    for (int y = threadIdx.x; y < S; y += kMaskBoxThreads) {
        const int count = st[3 * y + 2];
        if (count > 0) {
            y_lo = min(y_lo, y);
            y_hi = y + 1;                             // y grows within a thread
            x_lo = min(x_lo, st[3 * y]);
            x_hi = max(x_hi, st[3 * y + 1]);
            sum += count;
        }
    }
    y_lo = wave_min(y_lo);
    x_lo = wave_min(x_lo);
    y_hi = wave_max(y_hi);
    x_hi = wave_max(x_hi);
    sum = wave_sum(sum);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_part[wave][0] = y_lo; s_part[wave][1] = x_lo; s_part[wave][2] = y_hi;
        s_part[wave][3] = x_hi; s_part[wave][4] = sum;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kMaskBoxWaves; ++w) {
            y_lo = min(y_lo, s_part[w][0]);
            x_lo = min(x_lo, s_part[w][1]);
            y_hi = max(y_hi, s_part[w][2]);
            x_hi = max(x_hi, s_part[w][3]);
            sum += s_part[w][4];
        }
        int32_t *b = box + 4 * g;
        const bool any = sum > 0;
        b[0] = any ? y_lo : 0;
        b[1] = any ? x_lo : 0;
        b[2] = any ? y_hi : 0;
        b[3] = any ? x_hi : 0;
        area[g] = sum;
    }
}

}  // namespace
