// Half-pixel bilinear coordinate rule shared by the resize kernels (image.hip) and the report
// mosaic (visualize.hip).  Build the including files with -ffp-contract=off: the rule is
// restated bit for bit on the host.
#pragma once
#include <hip/hip_runtime.h>

namespace mrcnn {

struct Lin { int i0, i1; float t; };

// OpenCV resizeLinear coordinate rule for one axis: output index d of a resize by 1 / scale
// reads input rows i0 and i1 with weight t on i1; both clamp to [0, n_in).
__device__ __forceinline__ Lin lin_coord(int d, double scale, int n_in)
{
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= n_in - 1) { s = n_in - 1; f = 0.f; }
    Lin l;
    l.i0 = s;
    l.i1 = min(s + 1, n_in - 1);
    l.t = f;
    return l;
}

}  // namespace mrcnn
