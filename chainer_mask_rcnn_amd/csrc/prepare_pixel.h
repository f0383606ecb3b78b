// One output pixel of MaskRCNN.prepare, shared by prepare_kernel (image.hip) and
// prepare_crop_kernel (scale_jitter.hip): both evaluate the same function, so a crop of the
// resized image equals the same window of the whole resized image bit for bit.
// Build the including files with -ffp-contract=off.
#pragma once
#include "bilinear.h"

namespace mrcnn {

// Pixel (y, x) of the image src (C,H,W) resized by 1 / inv_scale, minus the mean, to o[0..C).
// x is the column of the resized image to evaluate: the caller has already mirrored it for a
// flip.  fp32 sources take OpenCV's INTER_LINEAR float rule, uint8 sources its 8-bit path.
template <typename T>
__device__ __forceinline__ void prepare_pixel(const T *__restrict__ src, int C, int H, int W,
                                              double inv_scale, float m0, float m1, float m2,
                                              int y, int x, float *__restrict__ o)
{
    const Lin ly = lin_coord(y, inv_scale, H);
    const Lin lx = lin_coord(x, inv_scale, W);
    if constexpr (sizeof(T) == 1) {
        // OpenCV 8-bit path (imgproc/resize.cpp: HResizeLinear<uchar,int,short> +
        // VResizeLinear<uchar,int,short,FixedPtCast<int,uchar,22>>), see
        // oracle/np_infer.py:cv_resize_linear_u8.  Integer arithmetic: bit-exact vs the oracle.
        float fy = (float)(((double)y + 0.5) * inv_scale - 0.5);
        const int sy = (int)floorf(fy);
        fy -= (float)sy;                                     // vertical weight is NOT clamped
        const int y0 = min(max(sy, 0), H - 1), y1 = min(max(sy + 1, 0), H - 1);
        const int a0 = __float2int_rn((1.f - lx.t) * 2048.f), a1 = __float2int_rn(lx.t * 2048.f);
        const int b0 = __float2int_rn((1.f - fy) * 2048.f), b1 = __float2int_rn(fy * 2048.f);
        for (int c = 0; c < C; ++c) {
            const T *p = src + (int64_t)c * H * W;
            const int d0 = (int)p[y0 * W + lx.i0] * a0 + (int)p[y0 * W + lx.i1] * a1;
            const int d1 = (int)p[y1 * W + lx.i0] * a0 + (int)p[y1 * W + lx.i1] * a1;
            const int v = (((b0 * (d0 >> 4)) >> 16) + ((b1 * (d1 >> 4)) >> 16) + 2) >> 2;
            o[c] = (float)min(max(v, 0), 255) - (c == 0 ? m0 : (c == 1 ? m1 : m2));
        }
        return;
    }
    for (int c = 0; c < C; ++c) {
        const T *p = src + (int64_t)c * H * W;
        const float top = (float)p[ly.i0 * W + lx.i0] * (1.f - lx.t) + (float)p[ly.i0 * W + lx.i1] * lx.t;
        const float bot = (float)p[ly.i1 * W + lx.i0] * (1.f - lx.t) + (float)p[ly.i1 * W + lx.i1] * lx.t;
        const float v = top * (1.f - ly.t) + bot * ly.t;
        o[c] = v - (c == 0 ? m0 : (c == 1 ? m1 : m2));
    }
}

}  // namespace mrcnn
