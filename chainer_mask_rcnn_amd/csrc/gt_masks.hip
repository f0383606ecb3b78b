// Ground-truth masks of the train step from packed bits (format: include/mrcnn_hip.h, "Packed
// masks"):
//   mask_resize_nearest — packed source-size masks + row / column tables -> (G, outH, outW) uint8
// Replaces the host resize and flip of the mask stack in datasets/transforms.py:resize_nearest
// (the reference's chainer_mask_rcnn/datasets/transforms.py:40-46): the masks cross PCIe as bits
// and become the bytes mrcnn_mask_targets reads only here.  Integer arithmetic only.
#include "common.h"

namespace {

constexpr int kThreads = 256;

// One workgroup per output row (g, y).  The source row's words are staged in LDS; every thread
// then builds four output bytes at a time and stores them as one dword.  Dwords are aligned on
// the output ADDRESS, not on the row: outW is odd in the common case (1333), so a row starts at
// any byte.  The dwords that straddle the row's ends are written as single bytes — the neighbours
// belong to another workgroup.  Table entries are clamped, so every read stays inside the row.
__global__ void __launch_bounds__(kThreads)
mask_resize_nearest_kernel(const uint64_t *__restrict__ packed, int H, int W, int Wq,
                           const int32_t *__restrict__ ys, const int32_t *__restrict__ xs,
                           int outH, int outW, uint8_t *__restrict__ out)
{
    extern __shared__ uint64_t s_row[];               // (Wq) words of source row (g, ys[y])
    const int row = blockIdx.x;                       // g * outH + y
    const int g = row / outH, y = row - g * outH;
    const int sy = min(max(ys[y], 0), H - 1);
    const uint64_t *src = packed + ((int64_t)g * H + sy) * Wq;
    for (int w = threadIdx.x; w < Wq; w += kThreads) s_row[w] = src[w];
    __syncthreads();

    uint8_t *dst = out + (int64_t)row * outW;
    const int mis = (int)((uintptr_t)dst & 3);        // bytes between the dword boundary and dst
    const int n_dwords = (mis + outW + 3) >> 2;
    for (int d = threadIdx.x; d < n_dwords; d += kThreads) {
        const int x0 = 4 * d - mis;                   // dst + x0 is dword-aligned
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = x0 + j;
            if (x >= 0 && x < outW) {
                const int sx = min(max(xs[x], 0), W - 1);
                v |= (uint32_t)((s_row[sx >> 6] >> (sx & 63)) & 1) << (8 * j);
            }
        }
        if (x0 >= 0 && x0 + 4 <= outW) {
            *reinterpret_cast<uint32_t *>(dst + x0) = v;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x0 + j >= 0 && x0 + j < outW) dst[x0 + j] = (uint8_t)(v >> (8 * j));
        }
    }
}

}  // namespace

extern "C" int mrcnn_mask_resize_nearest(const uint64_t *packed, int G, int H, int W,
                                         const int32_t *ys, const int32_t *xs, int outH, int outW,
                                         uint8_t *out, void *stream)
{
    MRCNN_REQUIRE(G >= 0 && H > 0 && W > 0 && outH > 0 && outW > 0,
                  "mask_resize_nearest: bad shape");
    MRCNN_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), "mask_resize_nearest: H*W >= 2^31");
    MRCNN_REQUIRE((int64_t)G * outH * outW < ((int64_t)1 << 31),
                  "mask_resize_nearest: G*outH*outW >= 2^31");
    const int Wq = (W + 63) / 64;
    MRCNN_REQUIRE((int64_t)Wq * 8 <= 65536, "mask_resize_nearest: W > 524288 (one row in LDS)");
    if (G == 0) return 0;
    MRCNN_REQUIRE(packed && ys && xs && out, "mask_resize_nearest: null pointer");
    hipLaunchKernelGGL(mask_resize_nearest_kernel, dim3((unsigned)(G * outH)), dim3(kThreads),
                       (size_t)Wq * 8, mrcnn::as_stream(stream), packed, H, W, Wq, ys, xs, outH,
                       outW, out);
    return mrcnn::check_launch("mask_resize_nearest");
}
