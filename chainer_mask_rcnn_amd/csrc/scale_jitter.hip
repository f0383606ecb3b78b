// Large-scale jitter on the device: a fixed S x S training canvas cut out
// of (or padded around) the randomly resized example, without the resized example ever existing.
//   prepare_image_crop — window (oy, ox) of MaskRCNN.prepare's resized, mean-subtracted and
//                        optionally mirrored image, zero beyond its bottom / right edge
//   mask_resize_crop   — packed source-size masks + row / column tables in which a negative entry
//                        means "outside the resized mask" -> (G, S, S) uint8, and per instance the
//                        tight box and the area of what is left inside the canvas
// The reference has no scale augmentation: its transform
// (chainer_mask_rcnn/datasets/transforms.py:10-51) resizes to one fixed scale and flips.  These
// kernels extend the two that replace that resize and flip, mrcnn_prepare_image and
// mrcnn_mask_resize_nearest, by the crop window.  The image pixel is prepare_pixel.h's, the one
// mrcnn_prepare_image evaluates; the mask kernel keeps the rules of gt_masks.hip: integer
// arithmetic only, deterministic, no scratch.
// Built with -ffp-contract=off.
#include "common.h"
#include "mask_box.h"
#include "prepare_pixel.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxRows = 8;                           // output rows per workgroup (2 per wave)

// Canvas pixel (y, x) of image n is pixel (y + oy, x + ox) of the resized image (rH, rW), mirrored
// when flip_x, or 0 where that lies beyond the resized image.  Every pixel of the slot is written.
template <typename T>
__global__ void prepare_crop_kernel(const T *__restrict__ src, int C, int H, int W,
                                    double inv_scale, float m0, float m1, float m2,
                                    float *__restrict__ dst, int dstH, int dstW, int rH, int rW,
                                    int oy, int ox, int n, int flip_x)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= dstW || y >= dstH) return;
    float *o = dst + (((int64_t)n * dstH + y) * dstW + x) * C;
    const int ry = y + oy, rx = x + ox;
    if (ry < rH && rx < rW) {
        mrcnn::prepare_pixel(src, C, H, W, inv_scale, m0, m1, m2, ry, flip_x ? rW - 1 - rx : rx, o);
    } else {
        for (int c = 0; c < C; ++c) o[c] = 0.f;
    }
}

// One workgroup per `rows` consecutive output rows of one instance.  The source rows they read
// are staged in LDS together (a padded row, ys[y] < 0, stages nothing); then every wave builds
// whole output rows, four bytes per lane and step, stored as one dword.  As in gt_masks.hip the
// dwords are aligned on the output ADDRESS (S may be odd), and the dwords that straddle a row's
// ends are written as single bytes.  In-range table entries are clamped, so every read stays
// inside the buffers.  Lane 0 of the wave leaves the row's (x_lo, x_hi, count) in row_stats
// (x_hi half-open; an empty row has count 0): integer min / max / sum, the same for any order.
// mask_box.h's mask_box_kernel, shared with copy_paste.hip, reduces them per instance.
__global__ void __launch_bounds__(kThreads)
mask_resize_crop_kernel(const uint64_t *__restrict__ packed, int H, int W, int Wq,
                        const int32_t *__restrict__ ys, const int32_t *__restrict__ xs, int S,
                        int rows, int groups, uint8_t *__restrict__ out,
                        int32_t *__restrict__ row_stats)
{
    extern __shared__ uint64_t s_rows[];              // (rows, Wq) words
    const int g = blockIdx.x / groups;
    const int y_base = (blockIdx.x - g * groups) * rows;
    for (int i = threadIdx.x; i < rows * Wq; i += kThreads) {
        const int r = i / Wq, w = i - r * Wq;
        const int y = y_base + r;
        if (y < S) {
            const int sy = ys[y];
            if (sy >= 0) s_rows[i] = packed[((int64_t)g * H + min(sy, H - 1)) * Wq + w];
        }
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = wave; r < rows; r += kWaves) {
        const int y = y_base + r;
        if (y >= S) break;
        const bool inside = ys[y] >= 0;               // wave-uniform
        const uint64_t *s_row = s_rows + r * Wq;
        const int64_t row = (int64_t)g * S + y;
        uint8_t *dst = out + row * S;
        const int mis = (int)((uintptr_t)dst & 3);    // bytes between the dword boundary and dst
        const int n_dwords = (mis + S + 3) >> 2;
        int lo = S, hi = 0, count = 0;
        for (int d = lane; d < n_dwords; d += 64) {
            const int x0 = 4 * d - mis;               // dst + x0 is dword-aligned
            uint32_t v = 0;
            if (inside) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int x = x0 + j;
                    if (x >= 0 && x < S) {
                        const int t = xs[x];
                        const int sx = min(max(t, 0), W - 1);
                        const uint32_t bit = t >= 0 ? (uint32_t)((s_row[sx >> 6] >> (sx & 63)) & 1) : 0u;
                        v |= bit << (8 * j);
                        if (bit) {
                            lo = min(lo, x);
                            hi = x + 1;               // x grows within a lane
                            ++count;
                        }
                    }
                }
            }
            if (x0 >= 0 && x0 + 4 <= S) {
                *reinterpret_cast<uint32_t *>(dst + x0) = v;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (x0 + j >= 0 && x0 + j < S) dst[x0 + j] = (uint8_t)(v >> (8 * j));
            }
        }
        lo = wave_min(lo);
        hi = wave_max(hi);
        count = wave_sum(count);
        if (lane == 0) {
            int32_t *st = row_stats + row * 3;
            st[0] = lo;
            st[1] = hi;
            st[2] = count;
        }
    }
}

}  // namespace

extern "C" int mrcnn_prepare_image_crop(const void *src_chw, int src_is_u8, int C, int H, int W,
                                        double scale, const float *mean_host, float *dst_nhwc,
                                        int dstH, int dstW, int rH, int rW, int oy, int ox, int n,
                                        int flip_x, void *stream)
{
    MRCNN_REQUIRE(src_chw && dst_nhwc && mean_host, "prepare_image_crop: null pointer");
    MRCNN_REQUIRE(C == 3 && H > 0 && W > 0 && scale > 0.,
                  "prepare_image_crop: expects a 3-channel image");
    MRCNN_REQUIRE(dstH > 0 && dstW > 0 && dstH <= 65535 && rH > 0 && rW > 0 && n >= 0,
                  "prepare_image_crop: bad sizes");
    MRCNN_REQUIRE(oy >= 0 && oy < rH && ox >= 0 && ox < rW,
                  "prepare_image_crop: the offset lies outside the resized image");
    const dim3 grid((dstW + 255) / 256, dstH);
    if (src_is_u8)
        hipLaunchKernelGGL(prepare_crop_kernel<uint8_t>, grid, dim3(256), 0,
                           mrcnn::as_stream(stream), (const uint8_t *)src_chw, C, H, W, 1.0 / scale,
                           mean_host[0], mean_host[1], mean_host[2], dst_nhwc, dstH, dstW, rH, rW,
                           oy, ox, n, flip_x);
    else
        hipLaunchKernelGGL(prepare_crop_kernel<float>, grid, dim3(256), 0,
                           mrcnn::as_stream(stream), (const float *)src_chw, C, H, W, 1.0 / scale,
                           mean_host[0], mean_host[1], mean_host[2], dst_nhwc, dstH, dstW, rH, rW,
                           oy, ox, n, flip_x);
    return mrcnn::check_launch("prepare_image_crop");
}

extern "C" int mrcnn_mask_resize_crop(const uint64_t *packed, int G, int H, int W,
                                      const int32_t *ys, const int32_t *xs, int S, uint8_t *out,
                                      int32_t *box, int32_t *area, int32_t *row_stats,
                                      void *stream)
{
    MRCNN_REQUIRE(G >= 0 && H > 0 && W > 0 && S > 0, "mask_resize_crop: bad shape");
    MRCNN_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), "mask_resize_crop: H*W >= 2^31");
    MRCNN_REQUIRE((int64_t)G * S * S < ((int64_t)1 << 31), "mask_resize_crop: G*S*S >= 2^31");
    const int Wq = (W + 63) / 64;
    MRCNN_REQUIRE((int64_t)Wq * 8 <= 65536, "mask_resize_crop: W > 524288 (one row in LDS)");
    if (G == 0) return 0;
    MRCNN_REQUIRE(packed && ys && xs && out && box && area && row_stats,
                  "mask_resize_crop: null pointer");
    // as many rows per workgroup as 64 KB of LDS hold, kMaxRows at the most
    int rows = (int)(65536 / ((int64_t)Wq * 8));
    rows = rows < kMaxRows ? rows : kMaxRows;
    rows = rows < S ? rows : S;
    const int groups = (S + rows - 1) / rows;
    hipStream_t s = mrcnn::as_stream(stream);
    hipLaunchKernelGGL(mask_resize_crop_kernel, dim3((unsigned)(G * groups)), dim3(kThreads),
                       (size_t)rows * Wq * 8, s, packed, H, W, Wq, ys, xs, S, rows, groups, out,
                       row_stats);
    hipLaunchKernelGGL(mask_box_kernel, dim3((unsigned)G), dim3(kMaskBoxThreads), 0, s, row_stats, S,
                       box, area);
    return mrcnn::check_launch("mask_resize_crop");
}
