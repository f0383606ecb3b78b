// The per-class box decode of MaskRCNN._to_bboxes (models/mask_rcnn.py:220-240) for one (RoI, class)
// pair: the one statement of the expression behind mrcnn_decode_cls_boxes (proposal.hip) and
// mrcnn_decode_cls_boxes_views (test_aug.hip).  Both files are built with -ffp-contract=off, so the
// two entry points round alike.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mrcnn {

struct Norm4 { double v[4]; };

// a = roi (y_min, x_min, y_max, x_max) in the network's frame, lp = the class's 4 regression values
__device__ __forceinline__ float4 decode_cls_box(float4 a, const float *__restrict__ lp,
                                                 float inv_scale, const Norm4 &mean,
                                                 const Norm4 &stdv, float size_h, float size_w,
                                                 int use_div, float scale)
{
    // rois[keep] / scale  (models/mask_rcnn.py:220)
    if (use_div) { a.x = a.x / scale; a.y = a.y / scale; a.z = a.z / scale; a.w = a.w / scale; }
    else { a.x *= inv_scale; a.y *= inv_scale; a.z *= inv_scale; a.w *= inv_scale; }
    // (roi_cls_loc * std + mean).astype(float32) (:225-229): mean / std come from Python tuples,
    // i.e. float64 arrays — the product and sum are formed in double and rounded once
    const float dy = (float)((double)lp[0] * stdv.v[0] + mean.v[0]);
    const float dx = (float)((double)lp[1] * stdv.v[1] + mean.v[1]);
    const float dh = (float)((double)lp[2] * stdv.v[2] + mean.v[2]);
    const float dw = (float)((double)lp[3] * stdv.v[3] + mean.v[3]);
    const float h = a.z - a.x, w = a.w - a.y;
    const float cy = a.x + 0.5f * h, cx = a.y + 0.5f * w;
    const float ncy = dy * h + cy, ncx = dx * w + cx;
    const float nh = (float)exp((double)dh) * h;
    const float nw = (float)exp((double)dw) * w;
    float4 o;
    o.x = fminf(fmaxf(ncy - 0.5f * nh, 0.f), size_h);
    o.y = fminf(fmaxf(ncx - 0.5f * nw, 0.f), size_w);
    o.z = fminf(fmaxf(ncy + 0.5f * nh, 0.f), size_h);
    o.w = fminf(fmaxf(ncx + 0.5f * nw, 0.f), size_w);
    return o;
}

}  // namespace mrcnn
