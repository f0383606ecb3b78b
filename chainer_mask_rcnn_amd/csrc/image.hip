// Device-side image I/O at both ends of MaskRCNN.predict:
//   prepare      — cv2.resize(img, None, fx=scale, fy=scale) + mean subtraction + zero-padded
//                  batch assembly (/root/reference/chainer_mask_rcnn/models/mask_rcnn.py:152-176,
//                  datasets/concat_examples.py:20-26)
//   paste_masks  — segm_results / expand_boxes (models/mask_rcnn.py:44-107): pad the 14x14
//                  mask by one pixel, expand the box by (M+2)/M, truncate to int, bilinear
//                  resize to the box, threshold at 0.5, paste into the image.
// cv2 is not installable in the build container; both kernels restate OpenCV's INTER_LINEAR
// float path (src = (float)((dst + 0.5) * scale - 0.5), floor, clamp to the border, horizontal
// then vertical blend) exactly as oracle/np_infer.py does; uint8 sources take OpenCV's 8-bit
// fixed-point path (11-bit coefficients, result rounded to uint8 before the mean is subtracted),
// which is what cv2.resize runs for the decoded images MaskRCNNTransform feeds.
// Built with -ffp-contract=off.
#include "bilinear.h"
#include "common.h"
#include "prepare_pixel.h"

namespace {

using mrcnn::Lin;
using mrcnn::lin_coord;

// src (C,H,W) fp32 or uint8 -> dst image n of an (N, dstH, dstW, C) NHWC batch, rows/cols
// beyond (outH, outW) are left untouched (the caller zero-fills the batch).  flip_x writes
// the resized image mirrored left-right (chainercv random_flip after the resize).
template <typename T>
__global__ void prepare_kernel(const T *__restrict__ src, int C, int H, int W, double inv_scale,
                               float m0, float m1, float m2, float *__restrict__ dst, int dstH,
                               int dstW, int outH, int outW, int n, int flip_x)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= outW || y >= outH) return;
    float *o = dst + (((int64_t)n * dstH + y) * dstW + x) * C;
    mrcnn::prepare_pixel(src, C, H, W, inv_scale, m0, m1, m2, y, flip_x ? outW - 1 - x : x, o);
}

// Geometry of one detection's paste (expand_boxes on (x1, y1, x2, y2) = bbox[:, [1,0,3,2]],
// scale = (M + 2) / M, fp32): the expanded box truncated to int (rx1, ry1, w, h) and its clip
// to the image, [x_0, x_1) x [y_0, y_1).
struct PasteBox { int rx1, ry1, w, h, x_0, x_1, y_0, y_1; };

__device__ __forceinline__ PasteBox paste_box(const float *__restrict__ b, int M, int im_h, int im_w)
{
    const float scale = (float)(((double)M + 2.0) / (double)M);
    float w_half = (b[3] - b[1]) * .5f, h_half = (b[2] - b[0]) * .5f;
    const float x_c = (b[3] + b[1]) * .5f, y_c = (b[2] + b[0]) * .5f;
    w_half *= scale;
    h_half *= scale;
    PasteBox p;
    const int rx2 = (int)(x_c + w_half), ry2 = (int)(y_c + h_half);   // astype(int32): truncate
    p.rx1 = (int)(x_c - w_half);
    p.ry1 = (int)(y_c - h_half);
    p.w = max(rx2 - p.rx1 + 1, 1);
    p.h = max(ry2 - p.ry1 + 1, 1);
    p.x_0 = max(p.rx1, 0);
    p.x_1 = min(rx2 + 1, im_w);
    p.y_0 = max(p.ry1, 0);
    p.y_1 = min(ry2 + 1, im_h);
    return p;
}

// The pasted value of pixel (y, x) of detection d: 1 where the resized sigmoid exceeds 0.5
// inside the clipped box, 0 elsewhere.  Shared by paste_masks_kernel and the packed paste, so
// both make the same 0.5 decision for every pixel.
__device__ __forceinline__ uint8_t paste_pixel(const float *__restrict__ logits, int d, int M,
                                               int Kc, int ch, const PasteBox &p, int y, int x)
{
    if (!(x >= p.x_0 && x < p.x_1 && y >= p.y_0 && y < p.y_1)) return 0;
    const int P = M + 2;
    const Lin ly = lin_coord(y - p.ry1, (double)P / (double)p.h, P);
    const Lin lx = lin_coord(x - p.rx1, (double)P / (double)p.w, P);
    // padded_mask[1:-1, 1:-1] = sigmoid(logits[d, ch]); logits are (D, M, M, Kc) NHWC
    auto pm = [&](int py, int px) -> float {
        if (py < 1 || py > M || px < 1 || px > M) return 0.f;
        const float z = logits[(((int64_t)d * M + (py - 1)) * M + (px - 1)) * Kc + ch];
        // sigmoid in double, rounded once (as oracle/np_infer.py): the 0.5 threshold below
        // must not depend on the last ulp of a device expf
        return (float)(1.0 / (1.0 + exp(-(double)z)));
    };
    const float top = pm(ly.i0, lx.i0) * (1.f - lx.t) + pm(ly.i0, lx.i1) * lx.t;
    const float bot = pm(ly.i1, lx.i0) * (1.f - lx.t) + pm(ly.i1, lx.i1) * lx.t;
    return (top * (1.f - ly.t) + bot * ly.t) > 0.5f ? 1 : 0;
}

// one workgroup row per (detection, image row)
__global__ void paste_masks_kernel(const float *__restrict__ logits, const int32_t *__restrict__ label,
                                   const float *__restrict__ bbox, int D, int M, int Kc, int im_h,
                                   int im_w, uint8_t *__restrict__ out)
{
    const int d = blockIdx.z;
    const int y = blockIdx.y;
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= im_w) return;
    const PasteBox p = paste_box(bbox + 4 * d, M, im_h, im_w);
    out[((int64_t)d * im_h + y) * im_w + x] = paste_pixel(logits, d, M, Kc, label[d], p, y, x);
}

// Packed paste (mask format of include/mrcnn_hip.h): area 0 and extent = the clipped expanded
// box, word-aligned.  Written before paste_packed_kernel accumulates the areas.
__global__ void paste_packed_init_kernel(const float *__restrict__ bbox, int D, int M, int im_h,
                                         int im_w, int32_t *__restrict__ area,
                                         int32_t *__restrict__ extent)
{
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= D) return;
    const PasteBox p = paste_box(bbox + 4 * d, M, im_h, im_w);
    area[d] = 0;
    int32_t *e = extent + 4 * d;
    if (p.x_0 < p.x_1 && p.y_0 < p.y_1) {
        e[0] = p.y_0; e[1] = p.y_1; e[2] = p.x_0 >> 6; e[3] = ((p.x_1 - 1) >> 6) + 1;
    } else {
        e[0] = 0; e[1] = 0; e[2] = 0; e[3] = 0;
    }
}

// One 256-thread workgroup per (detection, image row); each wave builds one 64-pixel word per
// iteration with __ballot (bit l = lane l's pixel) and lane 0 stores it.  Words outside the box
// are stored as zero without evaluating a pixel.  Row popcounts go to area[d] with one integer
// atomic per row (exact, order-independent).
__global__ void __launch_bounds__(256)
paste_packed_kernel(const float *__restrict__ logits, const int32_t *__restrict__ label,
                    const float *__restrict__ bbox, int D, int M, int Kc, int im_h, int im_w,
                    int Wq, uint64_t *__restrict__ packed, int32_t *__restrict__ area)
{
    const int row = blockIdx.x;                       // d * im_h + y
    const int d = row / im_h, y = row - d * im_h;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const PasteBox p = paste_box(bbox + 4 * d, M, im_h, im_w);
    const int ch = label[d];
    const bool row_in = y >= p.y_0 && y < p.y_1;
    uint64_t *out = packed + (int64_t)row * Wq;
    int count = 0;
    for (int w = wave; w < Wq; w += 4) {
        const int x = (w << 6) + lane;
        uint64_t bits = 0;
        if (row_in && (w << 6) < p.x_1 && (w << 6) + 64 > p.x_0)
            bits = __ballot(x < im_w && paste_pixel(logits, d, M, Kc, ch, p, y, x));
        if (lane == 0) {
            out[w] = bits;
            count += __popcll(bits);
        }
    }
    if (lane == 0 && count) atomicAdd(area + d, count);
}

}  // namespace

extern "C" int mrcnn_prepare_image(const void *src_chw, int src_is_u8, int C, int H, int W,
                                   double scale, const float *mean_host, float *dst_nhwc, int dstH,
                                   int dstW, int outH, int outW, int n, int flip_x, void *stream)
{
    MRCNN_REQUIRE(src_chw && dst_nhwc && mean_host, "prepare_image: null pointer");
    MRCNN_REQUIRE(C == 3 && H > 0 && W > 0 && scale > 0., "prepare_image: expects a 3-channel image");
    MRCNN_REQUIRE(outH <= dstH && outW <= dstW && outH > 0 && outW > 0, "prepare_image: bad sizes");
    if (src_is_u8)
        hipLaunchKernelGGL(prepare_kernel<uint8_t>, dim3((outW + 255) / 256, outH), dim3(256), 0,
                           mrcnn::as_stream(stream), (const uint8_t *)src_chw, C, H, W, 1.0 / scale,
                           mean_host[0], mean_host[1], mean_host[2], dst_nhwc, dstH, dstW, outH,
                           outW, n, flip_x);
    else
        hipLaunchKernelGGL(prepare_kernel<float>, dim3((outW + 255) / 256, outH), dim3(256), 0,
                           mrcnn::as_stream(stream), (const float *)src_chw, C, H, W, 1.0 / scale,
                           mean_host[0], mean_host[1], mean_host[2], dst_nhwc, dstH, dstW, outH,
                           outW, n, flip_x);
    return mrcnn::check_launch("prepare_image");
}

extern "C" int mrcnn_paste_masks(const float *mask_logits, const int32_t *label, const float *bbox,
                                 int D, int M, int Kc, int im_h, int im_w, uint8_t *out,
                                 void *stream)
{
    MRCNN_REQUIRE(D >= 0 && M > 0 && Kc > 0 && im_h > 0 && im_w > 0, "paste_masks: bad shape");
    if (D == 0) return 0;
    MRCNN_REQUIRE(mask_logits && label && bbox && out, "paste_masks: null pointer");
    MRCNN_REQUIRE(D <= 65535 && im_h <= 65535, "paste_masks: grid too large");
    hipLaunchKernelGGL(paste_masks_kernel, dim3((im_w + 255) / 256, im_h, D), dim3(256), 0,
                       mrcnn::as_stream(stream), mask_logits, label, bbox, D, M, Kc, im_h, im_w, out);
    return mrcnn::check_launch("paste_masks");
}

extern "C" int mrcnn_paste_masks_packed(const float *mask_logits, const int32_t *label,
                                        const float *bbox, int D, int M, int Kc, int im_h,
                                        int im_w, uint64_t *packed, int32_t *area,
                                        int32_t *extent, void *stream)
{
    MRCNN_REQUIRE(D >= 0 && M > 0 && Kc > 0 && im_h > 0 && im_w > 0,
                  "paste_masks_packed: bad shape");
    MRCNN_REQUIRE((int64_t)im_h * im_w < ((int64_t)1 << 31), "paste_masks_packed: H*W >= 2^31");
    if (D == 0) return 0;
    MRCNN_REQUIRE(mask_logits && label && bbox && packed && area && extent,
                  "paste_masks_packed: null pointer");
    MRCNN_REQUIRE((int64_t)D * im_h < ((int64_t)1 << 31), "paste_masks_packed: grid too large");
    const int Wq = (im_w + 63) / 64;
    hipStream_t s = mrcnn::as_stream(stream);
    hipLaunchKernelGGL(paste_packed_init_kernel, dim3((D + 255) / 256), dim3(256), 0, s, bbox, D,
                       M, im_h, im_w, area, extent);
    hipLaunchKernelGGL(paste_packed_kernel, dim3(D * im_h), dim3(256), 0, s, mask_logits, label,
                       bbox, D, M, Kc, im_h, im_w, Wq, packed, area);
    return mrcnn::check_launch("paste_masks_packed");
}
