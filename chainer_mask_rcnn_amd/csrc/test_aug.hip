// Test-time augmentation for gfx950 (Detectron's TEST.BBOX_AUG / TEST.MASK_AUG, core/test.py:
// im_detect_bbox_aug, im_detect_mask_aug): the device work that maps the results of an image's
// views (mirrored, other scales) back into the image frame and merges them.
//
//   mrcnn_decode_cls_boxes_views   every view's per-class decode + clip (decode_cls_box.h, the
//                                  expression of mrcnn_decode_cls_boxes) and, for a mirrored view,
//                                  the un-mirror x_min' = W - x_max, x_max' = W - x_min, written into
//                                  one union buffer: view after view, each in its own row order
//   mrcnn_mask_aug_combine         the views' mask-head logits (D,M,M,Kc) combined into one logit
//                                  map by one of Detectron's MASK_AUG.HEUR rules; a mirrored view is
//                                  read at column M-1-x
//
// Both are memory-bound maps (the largest real problem is 100 x 14 x 14 x 80 floats per view): one
// launch each, the view loop inside the thread, the views' pointers in a by-value struct, no
// atomics, no scratch.  Lanes run along the contiguous axis (n_class boxes of 16 bytes; Kc floats,
// four per lane where Kc % 4 == 0), so a mirrored read is as coalesced as a straight one: only
// the pixel moves, never the channel.
#include "common.h"
#include "decode_cls_box.h"

namespace {

constexpr int kMaxViews = MRCNN_TEST_AUG_MAX_VIEWS;
constexpr int kThreads = 256;

struct DecodeViews {
    const float4 *roi[kMaxViews];
    const float *loc[kMaxViews];
    int ld[kMaxViews];
    int end[kMaxViews];          // one past the view's last element (row * n_class) of the union
    float scale[kMaxViews];
    int flip[kMaxViews];
};

// grid (ceil(total / 256)), block 256; total = (sum R_v) * n_class < 2^31.
__global__ void __launch_bounds__(kThreads)
decode_views_kernel(DecodeViews views, int n_views, float4 *__restrict__ cls_bbox, int total,
                    int n_class, mrcnn::Norm4 mean, mrcnn::Norm4 stdv, float size_h, float size_w)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    // the view of element e: the last one that begins at or before it (an empty view begins where
    // the next one does).  Unrolled with constant indices, so the struct stays in scalar registers.
    const float4 *__restrict__ roi = views.roi[0];
    const float *__restrict__ loc = views.loc[0];
    int ld = views.ld[0], flip = views.flip[0], begin = 0;
    float scale = views.scale[0];
#pragma unroll
    for (int u = 1; u < kMaxViews; ++u) {
        if (u < n_views && e >= views.end[u - 1]) {
            roi = views.roi[u]; loc = views.loc[u]; ld = views.ld[u]; flip = views.flip[u];
            scale = views.scale[u]; begin = views.end[u - 1];
        }
    }
    const int local = e - begin;
    const int r = local / n_class, l = local % n_class;
    float4 o = mrcnn::decode_cls_box(roi[r], loc + (int64_t)r * ld + 4 * l, 1.f / scale, mean, stdv,
                                     size_h, size_w, 1, scale);
    if (flip) {
        // chainercv flip_bbox(x_flip=True) about the original width, in the image frame
        const float x_min = size_w - o.w, x_max = size_w - o.y;
        o.y = x_min;
        o.w = x_max;
    }
    cls_bbox[e] = o;
}

struct MaskViews {
    const float *map[kMaxViews];
    int flip[kMaxViews];
};

// sigmoid(l) and sigmoid(-l) through exp(-|l|): neither loses accuracy where the other saturates
__device__ __forceinline__ void sigmoid_pair(float l, double &p, double &q)
{
    const double e = exp(-fabs((double)l));
    const double big = 1.0 / (1.0 + e), small = e / (1.0 + e);
    p = l >= 0.f ? big : small;
    q = l >= 0.f ? small : big;
}

template <int HEUR> struct Combine {
    double a, b;
    float m;
    __device__ __forceinline__ void first(float l)
    {
        if (HEUR == MRCNN_MASK_AUG_SOFT_AVG) sigmoid_pair(l, a, b);
        else if (HEUR == MRCNN_MASK_AUG_LOGIT_AVG) a = (double)l;
        else m = l;
    }
    __device__ __forceinline__ void add(float l)
    {
        if (HEUR == MRCNN_MASK_AUG_SOFT_AVG) {
            double p, q;
            sigmoid_pair(l, p, q);
            a = a + p;
            b = b + q;
        } else if (HEUR == MRCNN_MASK_AUG_LOGIT_AVG) {
            a = a + (double)l;
        } else {
            m = l > m ? l : m;
        }
    }
    __device__ __forceinline__ float result(double n_views) const
    {
        if (HEUR == MRCNN_MASK_AUG_SOFT_AVG) return (float)(log(a / n_views) - log(b / n_views));
        if (HEUR == MRCNN_MASK_AUG_LOGIT_AVG) return (float)(a / n_views);
        return m;
    }
};

// One thread per W floats of the output (W = 4: 16-byte loads and stores, Kc % 4 == 0 and every
// pointer 16-byte aligned; W = 1 otherwise).  n_vec = D * M * M * (Kc / W) < 2^31.
template <int HEUR, int W>
__global__ void __launch_bounds__(kThreads)
mask_combine_kernel(MaskViews views, int n_views, int M, int kq, int64_t n_vec,
                    float *__restrict__ out)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_vec) return;
    const int64_t pix = e / kq;                  // (d * M + y) * M + x
    const int k = (int)(e - pix * kq);
    const int x = (int)(pix % M);
    const int64_t mirrored = (pix - x + (M - 1 - x)) * kq + k;
    Combine<HEUR> acc[W];
#pragma unroll
    for (int v = 0; v < kMaxViews; ++v) {
        if (v >= n_views) break;
        const int64_t at = views.flip[v] ? mirrored : e;
        float l[W];
        if constexpr (W == 4) {
            const float4 t = ((const float4 *)views.map[v])[at];
            l[0] = t.x; l[1] = t.y; l[2] = t.z; l[3] = t.w;
        } else {
            l[0] = views.map[v][at];
        }
#pragma unroll
        for (int i = 0; i < W; ++i) {
            if (v == 0) acc[i].first(l[i]);
            else acc[i].add(l[i]);
        }
    }
    float r[W];
#pragma unroll
    for (int i = 0; i < W; ++i) r[i] = acc[i].result((double)n_views);
    if constexpr (W == 4) ((float4 *)out)[e] = make_float4(r[0], r[1], r[2], r[3]);
    else out[e] = r[0];
}

template <int W>
void launch_combine(int heuristic, const MaskViews &views, int n_views, int M, int kq,
                    int64_t n_vec, float *out, hipStream_t s)
{
    const dim3 grid((unsigned)mrcnn::ceil_div(n_vec, kThreads)), block(kThreads);
    if (heuristic == MRCNN_MASK_AUG_SOFT_AVG)
        hipLaunchKernelGGL((mask_combine_kernel<MRCNN_MASK_AUG_SOFT_AVG, W>), grid, block, 0, s, views,
                           n_views, M, kq, n_vec, out);
    else if (heuristic == MRCNN_MASK_AUG_SOFT_MAX)
        hipLaunchKernelGGL((mask_combine_kernel<MRCNN_MASK_AUG_SOFT_MAX, W>), grid, block, 0, s, views,
                           n_views, M, kq, n_vec, out);
    else
        hipLaunchKernelGGL((mask_combine_kernel<MRCNN_MASK_AUG_LOGIT_AVG, W>), grid, block, 0, s, views,
                           n_views, M, kq, n_vec, out);
}

}  // namespace

extern "C" int mrcnn_decode_cls_boxes_views(const mrcnn_test_aug_view *views, int n_views,
                                            int n_class, const double *mean4, const double *std4,
                                            float size_h, float size_w, float *cls_bbox,
                                            void *stream)
{
    MRCNN_REQUIRE(n_views >= 0 && n_views <= kMaxViews,
                  "decode_cls_boxes_views: n_views must be in [0, %d], got %d", kMaxViews, n_views);
    MRCNN_REQUIRE(n_class > 0, "decode_cls_boxes_views: bad shape");
    if (n_views == 0) return 0;
    MRCNN_REQUIRE(views, "decode_cls_boxes_views: null pointer");
    DecodeViews dv = {};
    int64_t rows = 0;
    for (int v = 0; v < n_views; ++v) {
        const mrcnn_test_aug_view &w = views[v];
        MRCNN_REQUIRE(w.R >= 0, "decode_cls_boxes_views: view %d has R < 0", v);
        MRCNN_REQUIRE(w.R == 0 || (w.roi && w.cls_loc),
                      "decode_cls_boxes_views: view %d: null pointer", v);
        MRCNN_REQUIRE(w.R == 0 || w.ld_loc >= 4 * n_class,
                      "decode_cls_boxes_views: view %d: ld_loc %d < 4 * n_class", v, w.ld_loc);
        MRCNN_REQUIRE((uintptr_t)w.roi % 16 == 0,
                      "decode_cls_boxes_views: view %d: roi must be 16-byte aligned", v);
        rows += w.R;
        MRCNN_REQUIRE(rows * n_class < ((int64_t)1 << 31),
                      "decode_cls_boxes_views: more than 2^31 - 1 boxes");
        dv.roi[v] = (const float4 *)w.roi;
        dv.loc[v] = w.cls_loc;
        dv.ld[v] = w.ld_loc;
        dv.end[v] = (int)(rows * n_class);
        dv.scale[v] = w.scale;
        dv.flip[v] = w.flip_x != 0;
    }
    if (rows == 0) return 0;
    MRCNN_REQUIRE(cls_bbox && mean4 && std4, "decode_cls_boxes_views: null pointer");
    MRCNN_REQUIRE((uintptr_t)cls_bbox % 16 == 0,
                  "decode_cls_boxes_views: cls_bbox must be 16-byte aligned");
    mrcnn::Norm4 mean, stdv;
    for (int i = 0; i < 4; ++i) { mean.v[i] = mean4[i]; stdv.v[i] = std4[i]; }
    const int total = (int)(rows * n_class);
    hipLaunchKernelGGL(decode_views_kernel, dim3((unsigned)mrcnn::ceil_div(total, kThreads)),
                       dim3(kThreads), 0, mrcnn::as_stream(stream), dv, n_views,
                       (float4 *)cls_bbox, total, n_class, mean, stdv, size_h, size_w);
    return mrcnn::check_launch("decode_cls_boxes_views");
}

extern "C" int mrcnn_mask_aug_combine(const float *const *maps, const int32_t *flip_x, int n_views,
                                      int D, int M, int Kc, int heuristic, float *out,
                                      void *stream)
{
    MRCNN_REQUIRE(n_views >= 1 && n_views <= kMaxViews,
                  "mask_aug_combine: n_views must be in [1, %d], got %d", kMaxViews, n_views);
    MRCNN_REQUIRE(D >= 0 && M > 0 && Kc > 0, "mask_aug_combine: bad shape");
    MRCNN_REQUIRE(heuristic == MRCNN_MASK_AUG_SOFT_AVG || heuristic == MRCNN_MASK_AUG_SOFT_MAX ||
                  heuristic == MRCNN_MASK_AUG_LOGIT_AVG,
                  "mask_aug_combine: unknown heuristic %d", heuristic);
    if (D == 0) return 0;
    MRCNN_REQUIRE(maps && flip_x && out, "mask_aug_combine: null pointer");
    const int64_t n = (int64_t)D * M * M * Kc;
    MRCNN_REQUIRE(n < ((int64_t)1 << 31), "mask_aug_combine: more than 2^31 - 1 elements");
    MaskViews mv = {};
    uintptr_t bits = (uintptr_t)out;
    for (int v = 0; v < n_views; ++v) {
        MRCNN_REQUIRE(maps[v], "mask_aug_combine: view %d: null pointer", v);
        MRCNN_REQUIRE(maps[v] != out, "mask_aug_combine: view %d aliases the output (a mirrored "
                      "read would see written columns)", v);
        mv.map[v] = maps[v];
        mv.flip[v] = flip_x[v] != 0;
        bits |= (uintptr_t)maps[v];
    }
    hipStream_t s = mrcnn::as_stream(stream);
    if (Kc % 4 == 0 && bits % 16 == 0) launch_combine<4>(heuristic, mv, n_views, M, Kc / 4, n / 4, out, s);
    else launch_combine<1>(heuristic, mv, n_views, M, Kc, n, out, s);
    return mrcnn::check_launch("mask_aug_combine");
}
