// Mask boundaries for Boundary IoU, cut from packed masks (format: include/mrcnn_hip.h,
// "Packed masks"):
//   mask_boundary — B = M & ~erode(M, d), erosion by the (2d+1) x (2d+1) square with the
//                   outside of the image as background, exact area of B
// Replaces boundary_iou.utils.boundary_utils.mask_to_boundary (cv2.copyMakeBorder + cv2.erode
// with a 3x3 kernel iterated d times, per mask on the host) behind COCOeval's iouType
// 'boundary' (Cheng et al., Boundary IoU, CVPR 2021).  The square erosion is separable: one
// launch erodes the rows into a caller-owned workspace, one erodes the columns of that, cuts
// the boundary and counts it.  Integer arithmetic only (shifts, ANDs, popcounts; integer
// atomics for the area alone), no LDS: every result is exact and independent of scheduling.
// The per-word functions are in mask_boundary.h.
#include "common.h"
#include "mask_boundary.h"

namespace {

using mrcnn_mb::STRIP;
using mrcnn_mb::Window;

// One thread per word (n = blockIdx.y; y, w flattened on x, w fastest).  Words outside the
// extent are neither read nor written: the vertical pass reads the workspace inside the extent
// only.  The mask's first thread zeroes the area the second launch accumulates.
__global__ void __launch_bounds__(256)
erode_rows_kernel(const uint64_t *__restrict__ packed, const int32_t *__restrict__ extent, int H,
                  int Wq, int q, int r, uint64_t *__restrict__ eh, int32_t *__restrict__ out_area)
{
    const int n = blockIdx.y;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx == 0) out_area[n] = 0;
    if (idx >= (int64_t)H * Wq) return;
    const int y = (int)(idx / Wq), w = (int)(idx - (int64_t)y * Wq);
    const Window e = mrcnn_mb::clamp_extent(extent + 4 * n, H, Wq);
    if (y < e.y_lo || y >= e.y_hi || w < e.w_lo || w >= e.w_hi) return;
    const int64_t row = ((int64_t)n * H + y) * Wq;
    eh[row + w] = mrcnn_mb::erode_row_word(packed + row, w, e, q, r);
}

// Wave-wide integer sum (wave64).
__device__ __forceinline__ int wave_sum(int v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// One thread per (strip of STRIP rows, word) of mask n = blockIdx.y, w fastest, so a wave's
// loads of one row are consecutive words.  Every word of out is written: zero outside the
// extent.  The wave's popcounts are summed in registers and added once to the mask's area.
__global__ void __launch_bounds__(256)
boundary_kernel(const uint64_t *__restrict__ packed, const uint64_t *__restrict__ eh,
                const int32_t *__restrict__ extent, int H, int Wq, int d,
                uint64_t *__restrict__ out, int32_t *__restrict__ out_area)
{
    const int n = blockIdx.y;
    const int strips = (H + STRIP - 1) / STRIP;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int count = 0;
    if (idx < (int64_t)strips * Wq) {
        const int s = (int)(idx / Wq), w = (int)(idx - (int64_t)s * Wq);
        const int y0 = s * STRIP;
        const Window e = mrcnn_mb::clamp_extent(extent + 4 * n, H, Wq);
        const int64_t base = (int64_t)n * H * Wq;
        const bool inside = w >= e.w_lo && w < e.w_hi && y0 < e.y_hi && y0 + STRIP > e.y_lo;
        uint64_t E[STRIP];
        if (inside) mrcnn_mb::erode_strip(eh + base, Wq, w, y0, d, e, E);
#pragma unroll
        for (int i = 0; i < STRIP; ++i) {
            const int y = y0 + i;
            if (y >= H) break;
            uint64_t b = 0;
            if (inside && y >= e.y_lo && y < e.y_hi)
                b = packed[base + (int64_t)y * Wq + w] & ~E[i];
            out[base + (int64_t)y * Wq + w] = b;
            count += __popcll(b);
        }
    }
    count = wave_sum(count);
    if ((threadIdx.x & 63) == 0 && count) atomicAdd(out_area + n, count);
}

}  // namespace

extern "C" int64_t mrcnn_mask_boundary_workspace_bytes(int N, int H, int W)
{
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    return (int64_t)N * H * ((W + 63) / 64) * (int64_t)sizeof(uint64_t);
}

extern "C" int mrcnn_mask_boundary(const uint64_t *packed, const int32_t *extent, int N, int H,
                                   int W, int d, uint64_t *out, int32_t *out_area,
                                   void *workspace, int64_t workspace_bytes, void *stream)
{
    MRCNN_REQUIRE(N >= 0 && H > 0 && W > 0, "mask_boundary: bad shape");
    MRCNN_REQUIRE(d >= 1, "mask_boundary: d must be >= 1");
    MRCNN_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), "mask_boundary: H*W >= 2^31");
    if (N == 0) return 0;
    MRCNN_REQUIRE(packed && extent && out && out_area && workspace, "mask_boundary: null pointer");
    MRCNN_REQUIRE(out != packed, "mask_boundary: out must not alias packed");
    MRCNN_REQUIRE(workspace_bytes >= mrcnn_mask_boundary_workspace_bytes(N, H, W),
                  "mask_boundary: workspace smaller than mrcnn_mask_boundary_workspace_bytes");
    MRCNN_REQUIRE(N <= 65535, "mask_boundary: more than 65535 masks in one call");
    const int Wq = (W + 63) / 64;
    const int strips = (H + STRIP - 1) / STRIP;
    hipStream_t s = mrcnn::as_stream(stream);
    uint64_t *eh = (uint64_t *)workspace;
    hipLaunchKernelGGL(erode_rows_kernel, dim3((unsigned)mrcnn::ceil_div((int64_t)H * Wq, 256), N),
                       dim3(256), 0, s, packed, extent, H, Wq, d >> 6, d & 63, eh, out_area);
    hipLaunchKernelGGL(boundary_kernel, dim3((unsigned)mrcnn::ceil_div((int64_t)strips * Wq, 256), N),
                       dim3(256), 0, s, packed, eh, extent, H, Wq, d, out, out_area);
    return mrcnn::check_launch("mask_boundary");
}
