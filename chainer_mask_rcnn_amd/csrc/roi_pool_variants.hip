// The two other RoI feature extractors of the reference's head (MaskRCNNResNet(pooling_func=...),
// examples/train_common.py:138-147): Fast R-CNN max pooling (chainer's F.roi_pooling_2d GPU
// kernel) and crop-and-resize (functions/crop_and_resize.py:7-41), NHWC, for gfx950.
//
// Forwards are laid out as the ROIAlign forward (roi_align.hip): one workgroup owns one output row
// of a RoI (roi, oh, all ow), the lanes run across channels (16 B/lane loads and stores when
// C % 4 == 0, one float per lane otherwise), every bin's geometry is wave-uniform arithmetic.
//
// Backwards are the pixel-owner form of mrcnn_roi_align_bwd_ws, with kernels of their own (the
// ROIAlign kernels sit at a register-allocation cliff); the host side of the contract is shared
// (roi_common.h):
//   pv_tables_kernel  (one thread per RoI)  per RoI: its pixel extent, and per produced bin row /
//                                           column either the pooling window [start, end) or the
//                                           two bilinear taps and their weights
//   pv_bwd_owner_kernel (8-pixel row tiles) one workgroup owns 8 pixels of one feature row x a
//                                           chunk of channels and walks the RoIs in index order:
//                                            A  ordered compaction of the RoIs that meet the tile
//                                            B  each such RoI's covering bins form a rectangle
//                                               [oh_lo, oh_hi] x [ow_lo, ow_hi] (the windows and
//                                               taps are monotone in the bin index); the
//                                               rectangles are written IN ORDER (RoI, oh, ow) into
//                                               an LDS list, in windows of kPvCap entries
//                                            C  every lane streams the list, kPvDepth independent
//                                               gy loads in flight
//   Every gx element is written exactly once: no atomics, no zero-fill, a fixed summation order
//   (RoI, then bin row, then bin column — the order of chainer's roi_pooling_2d backward kernel),
//   bit-reproducible run to run.
//
// Built with -ffp-contract=off: the forwards are bit-identical to the NumPy restatements of
// tests/pool_variants_ref.py.
#include <cstring>

#include "roi_common.h"

namespace {

using namespace mrcnn::roi;

constexpr int kPvXT = 8;          // pixels of a row per owner workgroup
constexpr int kPvThreads = 256;   // workgroup size bound (LDS list capacities)
constexpr int kPvCap = 512;       // LDS list entries per window
constexpr int kPvDepth = 4;       // gy loads in flight per lane

// ---- max pooling geometry (chainer F.roi_pooling_2d GPU kernel = Caffe's ROIPooling) ----------
struct PoolGeom {
    int batch, start_h, start_w;
    float bin_h, bin_w;
};

__device__ __forceinline__ PoolGeom pool_geom(const float *__restrict__ roi, float s, int PH, int PW)
{
    PoolGeom g;
    g.batch = (int)roi[0];
    // roundf: half away from zero, as the CUDA round() of chainer's kernel; the product in fp32
    g.start_w = (int)roundf(roi[1] * s);
    g.start_h = (int)roundf(roi[2] * s);
    const int end_w = (int)roundf(roi[3] * s);
    const int end_h = (int)roundf(roi[4] * s);
    const int roi_w = max(end_w - g.start_w + 1, 1);   // a malformed RoI becomes 1x1
    const int roi_h = max(end_h - g.start_h + 1, 1);
    g.bin_h = (float)roi_h / (float)PH;
    g.bin_w = (float)roi_w / (float)PW;
    return g;
}

// [lo, hi) of bin p along one axis, offset by the RoI start and clamped to [0, size]
__device__ __forceinline__ int2 pool_window(int p, float bin, int start, int size)
{
    int lo = (int)floorf((float)p * bin);
    int hi = (int)ceilf((float)(p + 1) * bin);
    lo = min(max(lo + start, 0), size);
    hi = min(max(hi + start, 0), size);
    return make_int2(lo, hi);
}

// ---- crop-and-resize geometry (functions/crop_and_resize.py:25-33, F.resize_images) -----------
struct CropGeom {
    int batch, y1, x1, hc, wc;
};

// crop start rint(v * s) (half to even, as Python 3's round), clamped into [0, size - 1]
// (extension: the reference wraps a negative start and fails on a start past the map); crop end
// max(rint(v2 * s), start + 1), truncated at the map edge as a Python slice
__device__ __forceinline__ int2 crop_axis(float v1, float v2, double s, int size)
{
    const int a = (int)fmin(fmax(rint((double)v1 * s), 0.0), (double)(size - 1));
    const int b = (int)fmin(fmax(rint((double)v2 * s), (double)(a + 1)), (double)size);
    return make_int2(a, b - a);
}

__device__ __forceinline__ CropGeom crop_geom(const float *__restrict__ roi, double s, int H, int W)
{
    CropGeom g;
    g.batch = (int)roi[0];
    const int2 ya = crop_axis(roi[2], roi[4], s, H);
    const int2 xa = crop_axis(roi[1], roi[3], s, W);
    g.y1 = ya.x;
    g.hc = ya.y;
    g.x1 = xa.x;
    g.wc = xa.y;
    return g;
}

struct LinTap {
    int i0, i1;
    float w0, w1;
};

// sample p of linspace(0, m - 1, n) (float64, numpy's i * step with the last point exact; 0 when
// n == 1): taps i0 = clip(floor(v), 0, m - 2), i1 = i0 + 1 (both 0 when m == 1), weights computed
// in float64 and rounded to fp32 once.  step = (m - 1) / (n - 1), precomputed by the caller.
__device__ __forceinline__ LinTap lin_tap(int p, int n, int m, double step)
{
    LinTap t;
    if (m == 1) {
        t.i0 = t.i1 = 0;
        t.w0 = 1.f;
        t.w1 = 0.f;
        return t;
    }
    const double v = n == 1 ? 0.0 : (p == n - 1 ? (double)(m - 1) : (double)p * step);
    int i0 = (int)floor(v);
    i0 = min(max(i0, 0), m - 2);
    const double d = v - (double)i0;
    t.i0 = i0;
    t.i1 = i0 + 1;
    t.w0 = (float)(1.0 - d);
    t.w1 = (float)d;
    return t;
}

__device__ __forceinline__ double lin_step(int n, int m) { return n > 1 ? (double)(m - 1) / (double)(n - 1) : 0.0; }

// ---- vector helpers -----------------------------------------------------------------------
template <typename V> struct PV;
template <> struct PV<float> {
    typedef int I;
    static __device__ __forceinline__ float splat(float v) { return v; }
    static __device__ __forceinline__ int isplat(int v) { return v; }
    static __device__ __forceinline__ void max_upd(float &m, int &a, float v, int idx)
    {
        if (v > m) { m = v; a = idx; }
    }
    // ((w00 v00 + w01 v01) + w10 v10) + w11 v11 in fp32 (no contraction)
    static __device__ __forceinline__ float bilin(float w00, float a, float w01, float b, float w10,
                                                  float c, float w11, float d)
    {
        return w00 * a + w01 * b + w10 * c + w11 * d;
    }
    static __device__ __forceinline__ float fma(float acc, float w, float v) { return acc + w * v; }
    static __device__ __forceinline__ float add_if(float acc, int a, int pix, float g)
    {
        return a == pix ? acc + g : acc;
    }
};
template <> struct PV<float4> {
    typedef int4 I;
    static __device__ __forceinline__ float4 splat(float v) { return make_float4(v, v, v, v); }
    static __device__ __forceinline__ int4 isplat(int v) { return make_int4(v, v, v, v); }
    static __device__ __forceinline__ void max_upd(float4 &m, int4 &a, float4 v, int idx)
    {
        PV<float>::max_upd(m.x, a.x, v.x, idx);
        PV<float>::max_upd(m.y, a.y, v.y, idx);
        PV<float>::max_upd(m.z, a.z, v.z, idx);
        PV<float>::max_upd(m.w, a.w, v.w, idx);
    }
    static __device__ __forceinline__ float4 bilin(float w00, float4 a, float w01, float4 b,
                                                   float w10, float4 c, float w11, float4 d)
    {
        return make_float4(PV<float>::bilin(w00, a.x, w01, b.x, w10, c.x, w11, d.x),
                           PV<float>::bilin(w00, a.y, w01, b.y, w10, c.y, w11, d.y),
                           PV<float>::bilin(w00, a.z, w01, b.z, w10, c.z, w11, d.z),
                           PV<float>::bilin(w00, a.w, w01, b.w, w10, c.w, w11, d.w));
    }
    static __device__ __forceinline__ float4 fma(float4 acc, float w, float4 v)
    {
        return make_float4(acc.x + w * v.x, acc.y + w * v.y, acc.z + w * v.z, acc.w + w * v.w);
    }
    static __device__ __forceinline__ float4 add_if(float4 acc, int4 a, int pix, float4 g)
    {
        return make_float4(PV<float>::add_if(acc.x, a.x, pix, g.x), PV<float>::add_if(acc.y, a.y, pix, g.y),
                           PV<float>::add_if(acc.z, a.z, pix, g.z), PV<float>::add_if(acc.w, a.w, pix, g.w));
    }
};

// ---- forwards -----------------------------------------------------------------------------
// y (R, OH, OW, C), argmax (R, OH, OW, C) int32: output bin (oh, ow) is bin (oh*BS, ow*BS) of the
// PH x PW grid.  An empty bin (or a RoI whose batch index is not in [0, N)) gives 0 / -1.
template <typename V>
__global__ void __launch_bounds__(256)
roi_pool_fwd_kernel(const V *__restrict__ x, const float *__restrict__ rois, V *__restrict__ y,
                    typename PV<V>::I *__restrict__ argmax, int N, int H, int W, int CV, int PH,
                    int PW, int OH, int OW, int BS, float spatial_scale, int R,
                    const int *__restrict__ order)
{
    typedef typename PV<V>::I I;
    const int row = xcd_row();
    if (row >= R * OH) return;
    const int oh = row % OH;
    const int n = order ? order[row / OH] : row / OH;
    if ((unsigned)n >= (unsigned)R) return;
    const PoolGeom g = pool_geom(rois + 5 * n, spatial_scale, PH, PW);
    const int2 hw = pool_window(oh * BS, g.bin_h, g.start_h, H);
    const bool ok = g.batch >= 0 && g.batch < N && hw.y > hw.x;
    for (int c = (int)(blockIdx.y * blockDim.x + threadIdx.x); c < CV; c += (int)(gridDim.y * blockDim.x)) {
        const V *__restrict__ img = x + (int64_t)(ok ? g.batch : 0) * H * W * CV + c;
        const int64_t o = ((int64_t)n * OH + oh) * OW * CV + c;
        for (int ow = 0; ow < OW; ++ow) {
            const int2 ww = pool_window(ow * BS, g.bin_w, g.start_w, W);
            V m = PV<V>::splat(0.f);
            I a = PV<V>::isplat(-1);
            if (ok && ww.y > ww.x) {
                m = PV<V>::splat(-1e37f);
                // h outer, w inner, ascending; strict > keeps the first maximum (NaN never wins).
                // Four loads in flight, then the four updates in order.
                for (int h = hw.x; h < hw.y; ++h) {
                    const V *__restrict__ rp = img + (int64_t)h * W * CV;
                    int w = ww.x;
                    for (; w + 4 <= ww.y; w += 4) {
                        const V v0 = rp[(int64_t)w * CV], v1 = rp[(int64_t)(w + 1) * CV];
                        const V v2 = rp[(int64_t)(w + 2) * CV], v3 = rp[(int64_t)(w + 3) * CV];
                        PV<V>::max_upd(m, a, v0, h * W + w);
                        PV<V>::max_upd(m, a, v1, h * W + w + 1);
                        PV<V>::max_upd(m, a, v2, h * W + w + 2);
                        PV<V>::max_upd(m, a, v3, h * W + w + 3);
                    }
                    for (; w < ww.y; ++w) PV<V>::max_upd(m, a, rp[(int64_t)w * CV], h * W + w);
                }
            }
            store_stream(&y[o + (int64_t)ow * CV], m);
            argmax[o + (int64_t)ow * CV] = a;
        }
    }
}

// y row out_rows[n] (identity when NULL) holds RoI n.  Four bins' 16 taps in flight per lane.
template <typename V>
__global__ void __launch_bounds__(256)
crop_resize_fwd_kernel(const V *__restrict__ x, const float *__restrict__ rois,
                       const int *__restrict__ out_rows, V *__restrict__ y, int N, int H, int W,
                       int CV, int PH, int PW, int OH, int OW, int BS, double spatial_scale, int R,
                       const int *__restrict__ order)
{
    const int row = xcd_row();
    if (row >= R * OH) return;
    const int oh = row % OH;
    const int n = order ? order[row / OH] : row / OH;
    if ((unsigned)n >= (unsigned)R) return;
    const int dst = out_rows ? out_rows[n] : n;
    if ((unsigned)dst >= (unsigned)R) return;
    const CropGeom g = crop_geom(rois + 5 * n, spatial_scale, H, W);
    const bool ok = g.batch >= 0 && g.batch < N;
    const LinTap ty = lin_tap(oh * BS, PH, g.hc, lin_step(PH, g.hc));
    const double sx = lin_step(PW, g.wc);
    for (int c = (int)(blockIdx.y * blockDim.x + threadIdx.x); c < CV; c += (int)(gridDim.y * blockDim.x)) {
        V *__restrict__ out = y + ((int64_t)dst * OH + oh) * OW * CV + c;
        if (!ok) {
            for (int ow = 0; ow < OW; ++ow) store_stream(&out[(int64_t)ow * CV], PV<V>::splat(0.f));
            continue;
        }
        const V *__restrict__ r0 = x + (((int64_t)g.batch * H + g.y1 + ty.i0) * W + g.x1) * CV + c;
        const V *__restrict__ r1 = x + (((int64_t)g.batch * H + g.y1 + ty.i1) * W + g.x1) * CV + c;
        for (int ow0 = 0; ow0 < OW; ow0 += 4) {
            V v[4][4];
            float w[4][4];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                if (ow0 + b >= OW) break;
                const LinTap tx = lin_tap((ow0 + b) * BS, PW, g.wc, sx);
                w[b][0] = ty.w0 * tx.w0;
                w[b][1] = ty.w0 * tx.w1;
                w[b][2] = ty.w1 * tx.w0;
                w[b][3] = ty.w1 * tx.w1;
                v[b][0] = r0[(int64_t)tx.i0 * CV];
                v[b][1] = r0[(int64_t)tx.i1 * CV];
                v[b][2] = r1[(int64_t)tx.i0 * CV];
                v[b][3] = r1[(int64_t)tx.i1 * CV];
            }
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                if (ow0 + b >= OW) break;
                store_stream(&out[(int64_t)(ow0 + b) * CV],
                             PV<V>::bilin(w[b][0], v[b][0], w[b][1], v[b][1], w[b][2], v[b][2], w[b][3], v[b][3]));
            }
        }
    }
}

// ---- pixel-owner backwards ------------------------------------------------------------------
// ext[r] = (ylo | yhi << 16, xlo | xhi << 16, batch or -1, output row of the RoI)
// rowt[r][oh] / colt[r][ow]:  max pool (start, end, 0, 0) of the window;
//                             crop-and-resize (tap0, tap1, bits of w0, bits of w1), map coordinates
template <bool POOL>
__global__ void __launch_bounds__(256)
pv_tables_kernel(const float *__restrict__ rois, const int *__restrict__ out_rows, int N, int H,
                 int W, int R, int PH, int PW, int OH, int OW, int BS, float fscale, double dscale,
                 int4 *__restrict__ ext, int4 *__restrict__ rowt, int4 *__restrict__ colt)
{
    const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (r >= R) return;
    const int dst = out_rows ? out_rows[r] : r;
    int batch, ylo = H, yhi = -1, xlo = W, xhi = -1;
    int4 *__restrict__ rt = rowt + (int64_t)r * OH;
    int4 *__restrict__ ct = colt + (int64_t)r * OW;
    if (POOL) {
        const PoolGeom g = pool_geom(rois + 5 * r, fscale, PH, PW);
        batch = g.batch;
        for (int oh = 0; oh < OH; ++oh) {
            const int2 w = pool_window(oh * BS, g.bin_h, g.start_h, H);
            rt[oh] = make_int4(w.x, w.y, 0, 0);
            if (w.y > w.x) { ylo = min(ylo, w.x); yhi = max(yhi, w.y - 1); }
        }
        for (int ow = 0; ow < OW; ++ow) {
            const int2 w = pool_window(ow * BS, g.bin_w, g.start_w, W);
            ct[ow] = make_int4(w.x, w.y, 0, 0);
            if (w.y > w.x) { xlo = min(xlo, w.x); xhi = max(xhi, w.y - 1); }
        }
    } else {
        const CropGeom g = crop_geom(rois + 5 * r, dscale, H, W);
        batch = g.batch;
        const double sy = lin_step(PH, g.hc), sx = lin_step(PW, g.wc);
        for (int oh = 0; oh < OH; ++oh) {
            const LinTap t = lin_tap(oh * BS, PH, g.hc, sy);
            rt[oh] = make_int4(g.y1 + t.i0, g.y1 + t.i1, __float_as_int(t.w0), __float_as_int(t.w1));
            ylo = min(ylo, g.y1 + t.i0);
            yhi = max(yhi, g.y1 + t.i1);
        }
        for (int ow = 0; ow < OW; ++ow) {
            const LinTap t = lin_tap(ow * BS, PW, g.wc, sx);
            ct[ow] = make_int4(g.x1 + t.i0, g.x1 + t.i1, __float_as_int(t.w0), __float_as_int(t.w1));
            xlo = min(xlo, g.x1 + t.i0);
            xhi = max(xhi, g.x1 + t.i1);
        }
    }
    const bool ok = batch >= 0 && batch < N && (unsigned)dst < (unsigned)R && yhi >= 0 && xhi >= 0;
    ext[r] = ok ? make_int4((int)((unsigned)ylo | ((unsigned)yhi << 16)),
                            (int)((unsigned)xlo | ((unsigned)xhi << 16)), batch, dst)
                : make_int4(0, 0, -1, 0);
}

// does row / column entry t of a RoI touch [lo, lo + len)?
template <bool POOL>
__device__ __forceinline__ bool pv_hits(const int4 t, int lo, int len)
{
    if (POOL) return t.y > lo && t.x < lo + len && t.y > t.x;
    return (t.x >= lo && t.x < lo + len) || (t.y >= lo && t.y < lo + len);
}

// crop-and-resize weight of row / column entry t on map coordinate p
__device__ __forceinline__ float pv_weight(const int4 t, int p)
{
    return (t.x == p ? __int_as_float(t.z) : 0.f) + (t.y == p ? __int_as_float(t.w) : 0.f);
}

template <typename V, bool POOL>
__global__ void __launch_bounds__(kPvThreads)
pv_bwd_owner_kernel(const V *__restrict__ gy, const typename PV<V>::I *__restrict__ argmax,
                    const int4 *__restrict__ ext, const int4 *__restrict__ rowt,
                    const int4 *__restrict__ colt, V *__restrict__ gx, int R, int N, int H, int W,
                    int CV, int OH, int OW)
{
    typedef typename PV<V>::I I;
    constexpr int XT = kPvXT;
    __shared__ int sList[kPvThreads];
    __shared__ int sWave[kPvThreads / 64];
    __shared__ int64_t sOff[kPvCap];                       // gy element offset of the bin's channel 0
    __shared__ __attribute__((aligned(16))) float sW[POOL ? 1 : kPvCap][XT];

    const int tiles_x = (W + XT - 1) / XT;
    const int total = tiles_x * H * N;
    const int logical = xcd_row();
    if (logical >= total) return;
    const int x0 = (logical % tiles_x) * XT;
    const int y = (logical / tiles_x) % H;
    const int n = logical / (tiles_x * H);
    const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
    const int nb = OH * OW;
    const int pix0 = y * W + x0;

    for (int c0 = (int)blockIdx.y * nthr; c0 < CV; c0 += (int)gridDim.y * nthr) {
        const int c = c0 + tid;
        const bool cok = c < CV;
        V acc[XT];
#pragma unroll
        for (int x = 0; x < XT; ++x) acc[x] = PV<V>::splat(0.f);

        for (int r0 = 0; r0 < R; r0 += nthr) {
            // A: the chunk's RoIs that meet this tile, in index order
            const int r = r0 + tid;
            bool in = false;
            if (r < R) {
                const int4 e = ext[r];
                const int ylo = e.x & 0xffff, yhi = (int)((unsigned)e.x >> 16);
                const int xlo = e.y & 0xffff, xhi = (int)((unsigned)e.y >> 16);
                in = e.z == n && y >= ylo && y <= yhi && xhi >= x0 && xlo <= x0 + XT - 1;
            }
            int m;
            const int pos = block_scan(in ? 1 : 0, sWave, &m) - (in ? 1 : 0);
            if (in) sList[pos] = r;
            __syncthreads();
            if (m == 0) continue;

            // B: thread i < m owns the i-th listed RoI: its rectangle of covering bins
            int rr = 0, oh_lo = 0, ow_lo = 0, ncol = 0, cnt = 0, dst = 0;
            if (tid < m) {
                rr = sList[tid];
                dst = ext[rr].w;
                int oh_hi = -1, ow_hi = -1;
                oh_lo = OH;
                ow_lo = OW;
                for (int oh = 0; oh < OH; ++oh)
                    if (pv_hits<POOL>(rowt[(int64_t)rr * OH + oh], y, 1)) { oh_lo = min(oh_lo, oh); oh_hi = oh; }
                for (int ow = 0; ow < OW; ++ow)
                    if (pv_hits<POOL>(colt[(int64_t)rr * OW + ow], x0, XT)) { ow_lo = min(ow_lo, ow); ow_hi = ow; }
                ncol = ow_hi >= ow_lo ? ow_hi - ow_lo + 1 : 0;
                cnt = oh_hi >= oh_lo ? (oh_hi - oh_lo + 1) * ncol : 0;
            }
            int ntot;
            const int off = block_scan(cnt, sWave, &ntot) - cnt;
            for (int win = 0; win < ntot; win += kPvCap) {
                if (cnt > 0) {
                    const int j0 = max(0, win - off), j1 = min(cnt, win + kPvCap - off);
                    for (int j = j0; j < j1; ++j) {
                        const int oh = oh_lo + j / ncol, ow = ow_lo + j % ncol;
                        const int k = off + j - win;
                        sOff[k] = ((int64_t)dst * nb + (int64_t)oh * OW + ow) * CV;
                        if (!POOL) {
                            const float ay = pv_weight(rowt[(int64_t)rr * OH + oh], y);
                            const int4 ct = colt[(int64_t)rr * OW + ow];
#pragma unroll
                            for (int x = 0; x < XT; ++x) sW[k][x] = ay * pv_weight(ct, x0 + x);
                        }
                    }
                }
                __syncthreads();
                // C: stream the window, kPvDepth loads in flight per lane
                const int nent = min(kPvCap, ntot - win);
                if (cok) {
                    for (int e = 0; e < nent; e += kPvDepth) {
                        V v[kPvDepth];
                        I a[kPvDepth];
#pragma unroll
                        for (int i = 0; i < kPvDepth; ++i) {
                            if (e + i < nent) {
                                v[i] = gy[sOff[e + i] + c];
                                if (POOL) a[i] = argmax[sOff[e + i] + c];
                            }
                        }
#pragma unroll
                        for (int i = 0; i < kPvDepth; ++i) {
                            if (e + i >= nent) break;
                            if (POOL) {
#pragma unroll
                                for (int x = 0; x < XT; ++x) acc[x] = PV<V>::add_if(acc[x], a[i], pix0 + x, v[i]);
                            } else {
#pragma unroll
                                for (int x = 0; x < XT; ++x) acc[x] = PV<V>::fma(acc[x], sW[e + i][x], v[i]);
                            }
                        }
                    }
                }
                __syncthreads();       // the window's list is consumed before the next one is written
            }
        }
        if (cok) {
            V *__restrict__ row = gx + (((int64_t)n * H + y) * W + x0) * CV + c;
#pragma unroll
            for (int x = 0; x < XT; ++x)
                if (x0 + x < W) row[(int64_t)x * CV] = acc[x];
        }
    }
}

// the family's shape check plus the limit of the variants' tables (16-bit extents, int pixel index)
int pv_check(const char *what, const void *a, const void *b, const void *c, int N, int H, int W,
             int C, int R, int PH, int PW, int bin_stride)
{
    if (int rc = check(what, a, b, c, N, H, W, C, R, PH, PW, bin_stride)) return rc;
    MRCNN_REQUIRE(H <= 32767 && W <= 32767 && (int64_t)H * W < (int64_t)INT32_MAX,
                  "%s: feature map too large (H, W <= 32767)", what);
    return 0;
}

// workspace sections of the pixel-owner backwards, 256-byte aligned
struct PvWs {
    int64_t ext, rowt, colt, total;
};
inline PvWs pv_ws(int R, int OH, int OW)
{
    PvWs w;
    Carver c;
    w.ext = c.take((int64_t)R * 16);
    w.rowt = c.take((int64_t)R * OH * 16);
    w.colt = c.take((int64_t)R * OW * 16);
    w.total = c.total;
    return w;
}

int64_t pv_ws_bytes(int N, int H, int W, int R, int PH, int PW, int bin_stride)
{
    if (N <= 0 || H <= 0 || W <= 0 || R <= 0 || PH <= 0 || PW <= 0 || bin_stride < 1) return 0;
    return pv_ws(R, out_bins(PH, bin_stride), out_bins(PW, bin_stride)).total;
}

template <bool POOL>
int pv_bwd(const char *what, const float *gy, const int *argmax, const float *rois,
           const int *out_rows, float *gx, int N, int H, int W, int C, int R, int PH, int PW,
           int bin_stride, float fscale, double dscale, void *ws, int64_t ws_bytes, void *stream)
{
    if (int rc = pv_check(what, gy, rois, POOL ? (const void *)argmax : (const void *)gy, N, H, W,
                          C, R, PH, PW, bin_stride))
        return rc;
    MRCNN_REQUIRE(gx != nullptr, "%s: null gx", what);
    MRCNN_REQUIRE(R == 0 || (ws != nullptr && (uintptr_t)ws % 16 == 0),
                  "%s: a 16-byte aligned workspace is required", what);
    MRCNN_REQUIRE(R == 0 || ws_bytes >= pv_ws_bytes(N, H, W, R, PH, PW, bin_stride),
                  "%s: workspace smaller than the size query", what);
    hipStream_t s = mrcnn::as_stream(stream);
    if (R == 0) {
        MRCNN_HIP_TRY(hipMemsetAsync(gx, 0, sizeof(float) * (size_t)N * H * W * C, s));
        return 0;
    }
    const int OH = out_bins(PH, bin_stride), OW = out_bins(PW, bin_stride);
    const int64_t tiles = (int64_t)((W + kPvXT - 1) / kPvXT) * H * N;
    MRCNN_REQUIRE(tiles + 8 < (int64_t)INT32_MAX, "%s: feature map too large", what);
    const PvWs w = pv_ws(R, OH, OW);
    int4 *ext = (int4 *)((char *)ws + w.ext);
    int4 *rowt = (int4 *)((char *)ws + w.rowt);
    int4 *colt = (int4 *)((char *)ws + w.colt);
    hipLaunchKernelGGL(pv_tables_kernel<POOL>, dim3((R + 255) / 256), dim3(256), 0, s, rois,
                       out_rows, N, H, W, R, PH, PW, OH, OW, bin_stride, fscale, dscale, ext, rowt, colt);
    const bool vec = C % 4 == 0 && (uintptr_t)gx % 16 == 0 && (uintptr_t)gy % 16 == 0 &&
                     (!POOL || (uintptr_t)argmax % 16 == 0);
    const int cv = vec ? C / 4 : C;
    const int nthr = pick_threads(cv);
    const dim3 grid((unsigned)((tiles + 7) / 8 * 8), (unsigned)((cv + nthr - 1) / nthr));
    dispatch_vec(vec, [&](auto tag) {
        typedef decltype(tag) V;
        hipLaunchKernelGGL((pv_bwd_owner_kernel<V, POOL>), grid, dim3(nthr), 0, s, (const V *)gy,
                           (const typename PV<V>::I *)argmax, ext, rowt, colt, (V *)gx, R, N, H, W, cv,
                           OH, OW);
    });
    return mrcnn::check_launch(what);
}

}  // namespace

extern "C" int mrcnn_roi_pool_fwd(const float *x, const float *rois, float *y, int *argmax, int N,
                                  int H, int W, int C, int R, int PH, int PW, int bin_stride,
                                  float spatial_scale, const int *order, void *stream)
{
    if (int rc = pv_check("roi_pool_fwd", x, rois, y, N, H, W, C, R, PH, PW, bin_stride)) return rc;
    MRCNN_REQUIRE(R == 0 || argmax, "roi_pool_fwd: null argmax");
    if (R == 0) return 0;
    const int OH = out_bins(PH, bin_stride), OW = out_bins(PW, bin_stride);
    hipStream_t s = mrcnn::as_stream(stream);
    const bool vec = C % 4 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)y % 16 == 0 &&
                     (uintptr_t)argmax % 16 == 0;
    const int cv = vec ? C / 4 : C;
    const int nthr = pick_threads(cv);
    const dim3 grid((R * OH + 7) / 8 * 8, (cv + nthr - 1) / nthr);
    dispatch_vec(vec, [&](auto tag) {
        typedef decltype(tag) V;
        hipLaunchKernelGGL(roi_pool_fwd_kernel<V>, grid, dim3(nthr), 0, s, (const V *)x, rois, (V *)y,
                           (typename PV<V>::I *)argmax, N, H, W, cv, PH, PW, OH, OW, bin_stride,
                           spatial_scale, R, order);
    });
    return mrcnn::check_launch("roi_pool_fwd");
}

extern "C" int64_t mrcnn_roi_pool_bwd_workspace_bytes(int N, int H, int W, int R, int PH, int PW,
                                                      int bin_stride)
{
    return pv_ws_bytes(N, H, W, R, PH, PW, bin_stride);
}

extern "C" int mrcnn_roi_pool_bwd_ws(const float *gy, const int *argmax, const float *rois,
                                     float *gx, int N, int H, int W, int C, int R, int PH, int PW,
                                     int bin_stride, float spatial_scale, void *ws,
                                     int64_t ws_bytes, void *stream)
{
    return pv_bwd<true>("roi_pool_bwd", gy, argmax, rois, nullptr, gx, N, H, W, C, R, PH, PW,
                        bin_stride, spatial_scale, 0.0, ws, ws_bytes, stream);
}

extern "C" int mrcnn_crop_resize_fwd(const float *x, const float *rois, const int *out_rows,
                                     float *y, int N, int H, int W, int C, int R, int PH, int PW,
                                     int bin_stride, double spatial_scale, const int *order,
                                     void *stream)
{
    if (int rc = pv_check("crop_resize_fwd", x, rois, y, N, H, W, C, R, PH, PW, bin_stride)) return rc;
    if (R == 0) return 0;
    const int OH = out_bins(PH, bin_stride), OW = out_bins(PW, bin_stride);
    hipStream_t s = mrcnn::as_stream(stream);
    const bool vec = C % 4 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)y % 16 == 0;
    const int cv = vec ? C / 4 : C;
    const int nthr = pick_threads(cv);
    const dim3 grid((R * OH + 7) / 8 * 8, (cv + nthr - 1) / nthr);
    dispatch_vec(vec, [&](auto tag) {
        typedef decltype(tag) V;
        hipLaunchKernelGGL(crop_resize_fwd_kernel<V>, grid, dim3(nthr), 0, s, (const V *)x, rois,
                           out_rows, (V *)y, N, H, W, cv, PH, PW, OH, OW, bin_stride, spatial_scale, R,
                           order);
    });
    return mrcnn::check_launch("crop_resize_fwd");
}

extern "C" int64_t mrcnn_crop_resize_bwd_workspace_bytes(int N, int H, int W, int R, int PH, int PW,
                                                         int bin_stride)
{
    return pv_ws_bytes(N, H, W, R, PH, PW, bin_stride);
}

extern "C" int mrcnn_crop_resize_bwd_ws(const float *gy, const float *rois, const int *out_rows,
                                        float *gx, int N, int H, int W, int C, int R, int PH,
                                        int PW, int bin_stride, double spatial_scale, void *ws,
                                        int64_t ws_bytes, void *stream)
{
    return pv_bwd<false>("crop_resize_bwd", gy, nullptr, rois, out_rows, gx, N, H, W, C, R, PH, PW,
                         bin_stride, 0.f, spatial_scale, ws, ws_bytes, stream);
}
