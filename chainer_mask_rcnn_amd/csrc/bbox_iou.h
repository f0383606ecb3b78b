// Per-pair box IoU shared by the target creators (targets.hip) and the evaluation tables
// (bbox_eval.hip).  Build the including files with -ffp-contract=off: each function is a fixed
// sequence of IEEE operations that a NumPy statement of the same rule reproduces bit for bit.
#pragma once
#include <hip/hip_runtime.h>

namespace mrcnn {

// chainercv bbox_iou for one pair of (y1, x1, y2, x2) boxes, fp32 exactly as NumPy evaluates it
// (utils/bbox.py:bbox_iou): the product of the overlap's sides times the overlap
// predicate (so a NaN or an infinity survives the multiplication by zero as NumPy's does),
// divided by area_a + area_b - inter.
__device__ __forceinline__ float iou_pair(const float *a, const float *b)
{
    const float tl0 = fmaxf(a[0], b[0]), tl1 = fmaxf(a[1], b[1]);
    const float br0 = fminf(a[2], b[2]), br1 = fminf(a[3], b[3]);
    const float inter = (tl0 < br0 && tl1 < br1) ? (br0 - tl0) * (br1 - tl1) : 0.f * ((br0 - tl0) * (br1 - tl1));
    const float area_a = (a[2] - a[0]) * (a[3] - a[1]);
    const float area_b = (b[2] - b[0]) * (b[3] - b[1]);
    return inter / (area_a + area_b - inter);
}

// pycocotools bbIou (maskApi.c) for one detection d and one ground-truth box g, both
// (x, y, w, h) float64; the union of a crowd ground truth is the detection's area.
__device__ __forceinline__ double bb_iou_pair(const double *d, const double *g, bool crowd)
{
    const double da = d[2] * d[3], ga = g[2] * g[3];
    const double w = fmin(d[0] + d[2], g[0] + g[2]) - fmax(d[0], g[0]);
    if (w <= 0) return 0.0;
    const double h = fmin(d[1] + d[3], g[1] + g[3]) - fmax(d[1], g[1]);
    if (h <= 0) return 0.0;
    const double i = w * h;
    const double u = crowd ? da : da + ga - i;
    return i / u;
}

}  // namespace mrcnn
