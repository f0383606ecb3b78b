// What the three RoI feature extractors (roi_align.hip: ROIAlign; roi_pool_variants.hip: max
// pooling and crop-and-resize) share: the (R, 5) RoIs with bin_stride and order, the
// channels-last float / float4 dispatch, and the pixel-owner backward's workspace carved into
// 256-byte sections.  The kernels themselves stay in their files.
#pragma once
#include "common.h"

namespace mrcnn {
namespace roi {

// Streaming stores for the pooled output (written once, read by the next kernel after 200 MB of
// other traffic): keeps the feature map's taps resident in L2.
typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store_stream(float *p, float v) { __builtin_nontemporal_store(v, p); }
__device__ __forceinline__ void store_stream(float4 *p, float4 v)
{
    __builtin_nontemporal_store((f32x4){v.x, v.y, v.z, v.w}, reinterpret_cast<f32x4 *>(p));
}

// row index of the workgroup: an XCD (workgroup id mod 8) owns a contiguous run of (RoI, oh) rows
// or of pixel tiles, which re-read each other's inputs and so share one L2
__device__ __forceinline__ int xcd_row()
{
    const int per = ((int)gridDim.x + 7) / 8;
    return (int)(blockIdx.x % 8) * per + (int)(blockIdx.x / 8);
}

// inclusive prefix sum over the workgroup of one int per thread; *total = the workgroup's sum.
// Not for roi_align_bwd_owner_kernel, which keeps its two scans inlined: with this function its
// float4 instantiation went from 0 to 36 bytes/lane of scratch.
__device__ __forceinline__ int block_scan(int v, int *sWave, int *total)
{
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, nwaves = (int)blockDim.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(inc, d);
        if (lane >= d) inc += t;
    }
    __syncthreads();
    if (lane == 63) sWave[wave] = inc;
    __syncthreads();
    int off = 0, m = 0;
    for (int w = 0; w < nwaves; ++w) {
        const int cw = sWave[w];
        if (w < wave) off += cw;
        m += cw;
    }
    *total = m;
    return off + inc;
}

// lanes of a workgroup for cv channel vectors: whole waves, at most 256
inline int pick_threads(int cv)
{
    int t = ((cv + 63) / 64) * 64;
    return t > 256 ? 256 : (t < 64 ? 64 : t);
}

// bins produced along an axis of P bins: every bin_stride-th one
inline int out_bins(int P, int bin_stride) { return (P + bin_stride - 1) / bin_stride; }

// the shape check of every entry point; `what` names it in the message
inline int check(const char *what, const void *a, const void *b, const void *c, int N, int H, int W,
                 int C, int R, int PH, int PW, int bin_stride)
{
    MRCNN_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && R >= 0 && PH > 0 && PW > 0,
                  "%s: bad shape N=%d H=%d W=%d C=%d R=%d outh=%d outw=%d", what, N, H, W, C, R,
                  PH, PW);
    MRCNN_REQUIRE(bin_stride >= 1, "%s: bin_stride must be >= 1", what);
    MRCNN_REQUIRE(R == 0 || (a && b && c), "%s: null pointer", what);
    MRCNN_REQUIRE((int64_t)R * PH * PW < (int64_t)INT32_MAX, "%s: too many bins", what);
    return 0;
}

// a workspace's sections, each starting at a multiple of 256 bytes: take() returns the offset
// of the next one, `total` is the size to ask for
struct Carver {
    int64_t total = 0;
    int64_t take(int64_t bytes)
    {
        const int64_t at = total;
        total += (bytes + 255) / 256 * 256;
        return at;
    }
};

// f(float4()) when the tensors allow 16 B/lane accesses, f(float()) otherwise: a launch site is one
// generic lambda that reads its vector type off the tag
template <typename F> inline void dispatch_vec(bool vec, F &&f)
{
    if (vec)
        f(float4());
    else
        f(float());
}

}  // namespace roi
}  // namespace mrcnn
