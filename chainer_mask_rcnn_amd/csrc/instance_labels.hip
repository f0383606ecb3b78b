// Instance label images <-> per-instance classes, boxes and masks (contract: include/mrcnn_hip.h,
// "Instance label images"):
//   label_scan      — value ranges of both images, presence bitmaps over the value windows and
//                     a popcount prefix that ranks every present value; n and the number of
//                     distinct classes land in meta[] (the caller's first synchronisation)
//   label_instances — per-(instance, class) pixel count and first raster position, boxes,
//                     the tie-broken majority class, the ascending ids, optional 0/1 masks
//   instances_to_label — painting (N, H, W) masks into (lbl_ins, lbl_cls)
// Replaces the per-instance loop of the reference's label2instance_boxes and the loop of
// instance_boxes2label (chainer_mask_rcnn/utils/geometry.py:94-147).  Every accumulation is an
// integer atomic (or, add, min, max), so the results are exact and do not depend on the
// order in which workgroups run.
#include <limits.h>

#include <algorithm>

#include "common.h"

namespace {

constexpr int kWindowBits = MRCNN_LABEL_WINDOW;          // 2^24 values per image
constexpr int kWindowWords = MRCNN_LABEL_WINDOW / 32;    // uint32 words of one bitmap

// Label value of pixel i: uint8 images store -1 as 255 (the VOC PNG "void" index).
__device__ __forceinline__ int label_at(const uint8_t *p, int64_t i)
{
    const int v = p[i];
    return v == 255 ? -1 : v;
}
__device__ __forceinline__ int label_at(const int32_t *p, int64_t i) { return p[i]; }

// Effective (instance, class) of pixel i: with mask_by_class, class -1 / 0 voids the instance.
template <typename TI, typename TC>
__device__ __forceinline__ void pixel_at(const TI *ins, const TC *cls, int64_t i, int mask_by_class,
                                         int &iv, int &cv)
{
    iv = label_at(ins, i);
    cv = label_at(cls, i);
    if (mask_by_class && (cv == -1 || cv == 0)) iv = -1;
}

// Number of bitmap words that cover [lo, hi] (0 when empty), clamped to the window: values
// beyond the window are never set, and the caller rejects such an image after reading meta.
__device__ __forceinline__ int window_words(int lo, int hi)
{
    if (hi < lo) return 0;
    const int64_t span = (int64_t)hi - lo + 1;
    return (int)min<int64_t>((span + 31) / 32, kWindowWords);
}

// Rank of a present value at offset d from the window's low end.
__device__ __forceinline__ int rank_of(const uint32_t *bm, const int32_t *pre, int d)
{
    const int w = d >> 5;
    return pre[w] + __popc(bm[w] & ((1u << (d & 31)) - 1u));
}

__device__ __forceinline__ int wave_min(int v)
{
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ int wave_max(int v)
{
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
    return v;
}

__device__ __forceinline__ int load_relaxed(const int32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t load_relaxed(const uint32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// meta = (ins_min, ins_max, cls_min, cls_max, n_ins, n_cls): empty ranges.
__global__ void meta_init_kernel(int32_t *meta)
{
    if (threadIdx.x == 0) {
        meta[0] = INT_MAX; meta[1] = INT_MIN;
        meta[2] = INT_MAX; meta[3] = INT_MIN;
        meta[4] = 0; meta[5] = 0;
    }
}

// Min / max of the instance values other than -1, and of the class values under them.  Each
// workgroup reduces in registers, across the wave and through LDS; one thread then issues the
// four global atomics.
template <typename TI, typename TC>
__global__ void __launch_bounds__(256)
range_kernel(const TI *__restrict__ ins, const TC *__restrict__ cls, int64_t HW, int mask_by_class,
             int32_t *__restrict__ meta)
{
    int imin = INT_MAX, imax = INT_MIN, cmin = INT_MAX, cmax = INT_MIN;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < HW; i += (int64_t)gridDim.x * 256) {
        int iv, cv;
        pixel_at(ins, cls, i, mask_by_class, iv, cv);
        if (iv != -1) {
            imin = min(imin, iv);
            imax = max(imax, iv);
            cmin = min(cmin, cv);
            cmax = max(cmax, cv);
        }
    }
    imin = wave_min(imin); imax = wave_max(imax);
    cmin = wave_min(cmin); cmax = wave_max(cmax);
    __shared__ int s[4][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s[0][wave] = imin; s[1][wave] = imax; s[2][wave] = cmin; s[3][wave] = cmax;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            imin = min(imin, s[0][w]); imax = max(imax, s[1][w]);
            cmin = min(cmin, s[2][w]); cmax = max(cmax, s[3][w]);
        }
        if (imin <= imax) {
            atomicMin(meta + 0, imin);
            atomicMax(meta + 1, imax);
            atomicMin(meta + 2, cmin);
            atomicMax(meta + 3, cmax);
        }
    }
}

// Clears the words of both bitmaps that the ranges in meta use.
__global__ void bitmap_clear_kernel(const int32_t *__restrict__ meta, uint32_t *__restrict__ bitmaps)
{
    const int which = blockIdx.y;
    const int words = window_words(meta[2 * which], meta[2 * which + 1]);
    uint32_t *bm = bitmaps + (int64_t)which * kWindowWords;
    for (int w = blockIdx.x * 256 + threadIdx.x; w < words; w += gridDim.x * 256) bm[w] = 0;
}

// Sets the presence bit of every instance value and of every class value under an instance.
// Consecutive lanes read consecutive pixels; a lane whose value equals its left neighbour's
// skips (one candidate per run of equal labels), and a bit already visible as set is not
// written again, so a large uniform region costs a handful of atomics, not one per pixel.
template <typename TI, typename TC>
__global__ void __launch_bounds__(256)
bitmap_set_kernel(const TI *__restrict__ ins, const TC *__restrict__ cls, int64_t HW,
                  int mask_by_class, const int32_t *__restrict__ meta, uint32_t *__restrict__ bitmaps)
{
    const int imin = meta[0], cmin = meta[2];
    const int lane = threadIdx.x & 63;
    uint32_t *bm_i = bitmaps, *bm_c = bitmaps + kWindowWords;
    // the trip count is uniform across the workgroup so that the shuffles see every lane
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < HW; base += stride) {
        const int64_t i = base + threadIdx.x;
        int iv = -1, cv = 0;
        if (i < HW) pixel_at(ins, cls, i, mask_by_class, iv, cv);
        const int piv = __shfl_up(iv, 1, 64), pcv = __shfl_up(cv, 1, 64);
        if (iv == -1) continue;
        const bool first_i = lane == 0 || piv != iv;
        const bool first_c = lane == 0 || piv == -1 || pcv != cv;
        const int64_t di = (int64_t)iv - imin, dc = (int64_t)cv - cmin;
        if (first_i && di < kWindowBits) {
            const uint32_t bit = 1u << (di & 31);
            uint32_t *w = bm_i + (di >> 5);
            if (!(load_relaxed(w) & bit)) atomicOr(w, bit);
        }
        if (first_c && dc < kWindowBits) {
            const uint32_t bit = 1u << (dc & 31);
            uint32_t *w = bm_c + (dc >> 5);
            if (!(load_relaxed(w) & bit)) atomicOr(w, bit);
        }
    }
}

// Exclusive popcount prefix of one bitmap per workgroup (blockIdx.x 0: instances, 1: classes)
// and the number of present values into meta[4 + blockIdx.x].  Thread t owns a contiguous
// chunk of words; the chunk totals are scanned through LDS.
__global__ void __launch_bounds__(1024)
bitmap_scan_kernel(int32_t *__restrict__ meta, const uint32_t *__restrict__ bitmaps,
                   int32_t *__restrict__ prefix)
{
    const int which = blockIdx.x;
    const int words = window_words(meta[2 * which], meta[2 * which + 1]);
    const uint32_t *bm = bitmaps + (int64_t)which * kWindowWords;
    int32_t *pre = prefix + (int64_t)which * kWindowWords;
    const int chunk = (words + 1023) / 1024;
    const int lo = min(words, (int)threadIdx.x * chunk), hi = min(words, lo + chunk);
    int sum = 0;
    for (int w = lo; w < hi; ++w) sum += __popc(bm[w]);
    // inclusive scan across the wave, then across the 16 wave totals
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = sum;
    for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_up(incl, off, 64);
        if (lane >= off) incl += v;
    }
    __shared__ int s_wave[16];
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wave; ++w) before += s_wave[w];
    int run = before + incl - sum;
    for (int w = lo; w < hi; ++w) {
        pre[w] = run;
        run += __popc(bm[w]);
    }
    if (threadIdx.x == 1023) meta[4 + which] = before + incl;
}

// count = 0 and first = INT_MAX for every (instance, class); boxes = empty (H, W, 0, 0) extents
// that the histogram pass narrows with integer min / max.
__global__ void table_init_kernel(int64_t cells, int n, int H, int W, int32_t *__restrict__ count,
                                  int32_t *__restrict__ first, int32_t *__restrict__ boxes)
{
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < cells; c += (int64_t)gridDim.x * 256) {
        count[c] = 0;
        first[c] = INT_MAX;
    }
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        int32_t *b = boxes + 4 * i;
        b[0] = H; b[1] = W; b[2] = 0; b[3] = 0;
    }
}

// ids[rank] = value of every set bit (blockIdx.y 0: instance ids, 1: class values).
__global__ void values_kernel(const int32_t *__restrict__ meta, const uint32_t *__restrict__ bitmaps,
                              const int32_t *__restrict__ prefix, int words_i, int words_c,
                              int32_t *__restrict__ ids, int32_t *__restrict__ cls_vals)
{
    const int which = blockIdx.y;
    const int words = which ? words_c : words_i;
    const int w = blockIdx.x * 256 + threadIdx.x;
    if (w >= words) return;
    const uint32_t bits = bitmaps[(int64_t)which * kWindowWords + w];
    int r = prefix[(int64_t)which * kWindowWords + w];
    int32_t *out = which ? cls_vals : ids;
    const int lo = meta[2 * which];
    for (uint32_t b = bits; b; b &= b - 1) out[r++] = lo + w * 32 + __ffs(b) - 1;
}

// Folds a run of `len` pixels of one (instance, class) cell starting at (y, x0) into the table
// and the instance's box.  The monotone updates read first and skip when they cannot change
// the value.
__device__ __forceinline__ void flush_run(int key, int len, int y, int x0, int W, int ncls,
                                          int32_t *__restrict__ count, int32_t *__restrict__ first,
                                          int32_t *__restrict__ boxes)
{
    if (key < 0) return;
    atomicAdd(count + key, len);
    const int pos = y * W + x0;
    if (load_relaxed(first + key) > pos) atomicMin(first + key, pos);
    int32_t *b = boxes + 4 * (key / ncls);
    if (load_relaxed(b + 0) > y) atomicMin(b + 0, y);
    if (load_relaxed(b + 1) > x0) atomicMin(b + 1, x0);
    if (load_relaxed(b + 2) < y + 1) atomicMax(b + 2, y + 1);
    if (load_relaxed(b + 3) < x0 + len) atomicMax(b + 3, x0 + len);
}

// One wave per image row, four rows per workgroup.  Each pixel gets the cell key
// rank(instance) * ncls + rank(class) (-1 outside every instance); the wave walks its row 64
// pixels at a time and reduces maximal runs of equal keys: a run that ends inside the 64
// pixels is flushed by its head lane, the run that reaches the last lane is carried (wave-
// uniform) into the next 64.  A row costs one flush per run, whatever the run lengths.
template <typename TI, typename TC>
__global__ void __launch_bounds__(256)
histogram_kernel(const TI *__restrict__ ins, const TC *__restrict__ cls, int H, int W,
                 int mask_by_class, const int32_t *__restrict__ meta,
                 const uint32_t *__restrict__ bitmaps, const int32_t *__restrict__ prefix, int ncls,
                 int32_t *__restrict__ count, int32_t *__restrict__ first, int32_t *__restrict__ boxes)
{
    const int y = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (y >= H) return;
    const int imin = meta[0], cmin = meta[2];
    const uint32_t *bm_i = bitmaps, *bm_c = bitmaps + kWindowWords;
    const int32_t *pre_i = prefix, *pre_c = prefix + kWindowWords;
    const int64_t row = (int64_t)y * W;
    int carry_key = -1, carry_len = 0, carry_x = 0;
    for (int x0 = 0; x0 < W; x0 += 64) {
        const int x = x0 + lane;
        int key = -1;
        if (x < W) {
            int iv, cv;
            pixel_at(ins, cls, row + x, mask_by_class, iv, cv);
            if (iv != -1)
                key = rank_of(bm_i, pre_i, iv - imin) * ncls + rank_of(bm_c, pre_c, cv - cmin);
        }
        const int left = __shfl_up(key, 1, 64);
        const bool head = lane == 0 ? key != carry_key : key != left;
        const uint64_t heads = __ballot(head);
        if (!heads) {                                   // the carried run spans all 64 lanes
            carry_len += 64;
            continue;
        }
        if (heads & 1ull) {                             // the carried run ended before lane 0
            if (lane == 0) flush_run(carry_key, carry_len, y, carry_x, W, ncls, count, first, boxes);
        } else {                                        // ... or continues up to the first head
            carry_len += __ffsll((unsigned long long)heads) - 1;
            if (lane == 0) flush_run(carry_key, carry_len, y, carry_x, W, ncls, count, first, boxes);
        }
        const int last = 63 - __clzll(heads);
        if (head && lane != last) {
            const uint64_t above = heads & ~((2ull << lane) - 1ull);
            const int next = __ffsll((unsigned long long)above) - 1;
            flush_run(key, next - lane, y, x, W, ncls, count, first, boxes);
        }
        carry_key = __shfl(key, last, 64);
        carry_len = 64 - last;
        carry_x = x0 + last;
    }
    // pixels past W carry key -1, so the carried run never counts them unless it is -1 itself
    if (lane == 0) flush_run(carry_key, carry_len, y, carry_x, W, ncls, count, first, boxes);
}

// One wave per instance: the class with the largest count, ties to the smallest first
// position (Counter insertion order of the reference).  classes[i] = that class's value.
__global__ void __launch_bounds__(256)
argmax_kernel(int n, int ncls, const int32_t *__restrict__ count, const int32_t *__restrict__ first,
              const int32_t *__restrict__ cls_vals, int32_t *__restrict__ classes)
{
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n) return;
    const int64_t base = (int64_t)i * ncls;
    int best_n = 0, best_f = INT_MAX, best_c = -1;
    for (int c = lane; c < ncls; c += 64) {
        const int cn = count[base + c], cf = first[base + c];
        if (cn > best_n || (cn == best_n && cn > 0 && cf < best_f)) {
            best_n = cn; best_f = cf; best_c = c;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const int on = __shfl_xor(best_n, off, 64), of = __shfl_xor(best_f, off, 64);
        const int oc = __shfl_xor(best_c, off, 64);
        if (on > best_n || (on == best_n && of < best_f)) {
            best_n = on; best_f = of; best_c = oc;
        }
    }
    if (lane == 0) classes[i] = best_c >= 0 ? cls_vals[best_c] : -1;
}

// masks[i, p] = (rank of pixel p's instance == i).  A thread ranks 16 consecutive pixels once
// and writes their 16 bytes for every instance, one 16-byte store per instance when H * W is
// a multiple of 16 (VEC), byte stores otherwise.
template <typename TI, typename TC, bool VEC>
__global__ void __launch_bounds__(256)
masks_kernel(const TI *__restrict__ ins, const TC *__restrict__ cls, int64_t HW, int mask_by_class,
             const int32_t *__restrict__ meta, const uint32_t *__restrict__ bitmaps,
             const int32_t *__restrict__ prefix, int n, uint8_t *__restrict__ masks)
{
    const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    if (p0 >= HW) return;
    const int cnt = (int)min<int64_t>(16, HW - p0);
    const int imin = meta[0];
    int r[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        r[k] = -1;
        if (k < cnt) {
            int iv, cv;
            pixel_at(ins, cls, p0 + k, mask_by_class, iv, cv);
            if (iv != -1) r[k] = rank_of(bitmaps, prefix, iv - imin);
        }
    }
    for (int i = 0; i < n; ++i) {
        uint8_t *dst = masks + (int64_t)i * HW + p0;
        if (VEC && cnt == 16) {
            uint32_t w[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                w[q] = (uint32_t)(r[4 * q] == i) | ((uint32_t)(r[4 * q + 1] == i) << 8) |
                       ((uint32_t)(r[4 * q + 2] == i) << 16) | ((uint32_t)(r[4 * q + 3] == i) << 24);
            *reinterpret_cast<uint4 *>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (k < cnt) dst[k] = r[k] == i;
        }
    }
}

// lbl_ins[p] = j and lbl_cls[p] = labels[order[j]] for the last j in painting order whose
// mask covers p; -1 and 0 where none does.
__global__ void __launch_bounds__(256)
paint_kernel(const uint8_t *__restrict__ masks, const int32_t *__restrict__ order,
             const int32_t *__restrict__ labels, int N, int64_t HW, int32_t *__restrict__ lbl_ins,
             int32_t *__restrict__ lbl_cls)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    int li = -1, lc = 0;
    for (int j = N - 1; j >= 0; --j) {
        const int m = order ? order[j] : j;
        if (masks[(int64_t)m * HW + p]) {
            li = j;
            lc = labels[m];
            break;
        }
    }
    lbl_ins[p] = li;
    lbl_cls[p] = lc;
}

template <typename TI, typename TC>
void launch_scan(const void *ins, const void *cls, int64_t HW, int mask_by_class, int32_t *meta,
                 uint32_t *bitmaps, int32_t *prefix, hipStream_t s)
{
    const int blocks = (int)std::min<int64_t>((HW + 2047) / 2048, 1024);
    hipLaunchKernelGGL(meta_init_kernel, dim3(1), dim3(64), 0, s, meta);
    hipLaunchKernelGGL((range_kernel<TI, TC>), dim3(blocks), dim3(256), 0, s, (const TI *)ins,
                       (const TC *)cls, HW, mask_by_class, meta);
    hipLaunchKernelGGL(bitmap_clear_kernel, dim3(256, 2), dim3(256), 0, s, meta, bitmaps);
    hipLaunchKernelGGL((bitmap_set_kernel<TI, TC>), dim3(blocks), dim3(256), 0, s, (const TI *)ins,
                       (const TC *)cls, HW, mask_by_class, meta, bitmaps);
    hipLaunchKernelGGL(bitmap_scan_kernel, dim3(2), dim3(1024), 0, s, meta, bitmaps, prefix);
}

template <typename TI, typename TC>
void launch_instances(const void *ins, const void *cls, int H, int W, int mask_by_class,
                      const int32_t *meta, const uint32_t *bitmaps, const int32_t *prefix, int n,
                      int ncls, int32_t *count, int32_t *first, int32_t *boxes, int32_t *classes,
                      const int32_t *cls_vals, uint8_t *masks, hipStream_t s)
{
    hipLaunchKernelGGL((histogram_kernel<TI, TC>), dim3((H + 3) / 4), dim3(256), 0, s,
                       (const TI *)ins, (const TC *)cls, H, W, mask_by_class, meta, bitmaps, prefix,
                       ncls, count, first, boxes);
    hipLaunchKernelGGL(argmax_kernel, dim3((n + 3) / 4), dim3(256), 0, s, n, ncls, count, first,
                       cls_vals, classes);
    if (!masks) return;
    const int64_t HW = (int64_t)H * W;
    const dim3 grid((unsigned)((HW + 4095) / 4096));
    if (HW % 16 == 0)
        hipLaunchKernelGGL((masks_kernel<TI, TC, true>), grid, dim3(256), 0, s, (const TI *)ins,
                           (const TC *)cls, HW, mask_by_class, meta, bitmaps, prefix, n, masks);
    else
        hipLaunchKernelGGL((masks_kernel<TI, TC, false>), grid, dim3(256), 0, s, (const TI *)ins,
                           (const TC *)cls, HW, mask_by_class, meta, bitmaps, prefix, n, masks);
}

}  // namespace

extern "C" int mrcnn_label_scan(const void *ins, int ins_bytes, const void *cls, int cls_bytes, int H,
                                int W, int mask_by_class, int32_t *meta, uint32_t *bitmaps,
                                int32_t *prefix, void *stream)
{
    MRCNN_REQUIRE(H > 0 && W > 0, "label_scan: bad shape");
    MRCNN_REQUIRE((ins_bytes == 1 || ins_bytes == 4) && (cls_bytes == 1 || cls_bytes == 4),
                  "label_scan: elem_bytes must be 1 or 4");
    MRCNN_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), "label_scan: H*W >= 2^31");
    MRCNN_REQUIRE(ins && cls && meta && bitmaps && prefix, "label_scan: null pointer");
    const int64_t HW = (int64_t)H * W;
    hipStream_t s = mrcnn::as_stream(stream);
    if (ins_bytes == 4 && cls_bytes == 4)
        launch_scan<int32_t, int32_t>(ins, cls, HW, mask_by_class, meta, bitmaps, prefix, s);
    else if (ins_bytes == 4)
        launch_scan<int32_t, uint8_t>(ins, cls, HW, mask_by_class, meta, bitmaps, prefix, s);
    else if (cls_bytes == 4)
        launch_scan<uint8_t, int32_t>(ins, cls, HW, mask_by_class, meta, bitmaps, prefix, s);
    else
        launch_scan<uint8_t, uint8_t>(ins, cls, HW, mask_by_class, meta, bitmaps, prefix, s);
    return mrcnn::check_launch("label_scan");
}

extern "C" int mrcnn_label_instances(const void *ins, int ins_bytes, const void *cls, int cls_bytes,
                                     int H, int W, int mask_by_class, const int32_t *meta,
                                     const uint32_t *bitmaps, const int32_t *prefix, int span_ins,
                                     int span_cls, int n, int ncls, int32_t *table, int32_t *ids,
                                     int32_t *classes, int32_t *boxes, uint8_t *masks, void *stream)
{
    MRCNN_REQUIRE(H > 0 && W > 0 && n >= 0 && ncls >= 0, "label_instances: bad shape");
    MRCNN_REQUIRE((ins_bytes == 1 || ins_bytes == 4) && (cls_bytes == 1 || cls_bytes == 4),
                  "label_instances: elem_bytes must be 1 or 4");
    MRCNN_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), "label_instances: H*W >= 2^31");
    if (n == 0) return 0;
    MRCNN_REQUIRE(ncls > 0, "label_instances: bad shape");
    MRCNN_REQUIRE(span_ins >= n && span_ins <= MRCNN_LABEL_WINDOW && span_cls >= ncls &&
                      span_cls <= MRCNN_LABEL_WINDOW,
                  "label_instances: value span outside [n, 2^24]");
    MRCNN_REQUIRE((int64_t)n * ncls <= MRCNN_LABEL_WINDOW,
                  "label_instances: instance x class table exceeds 2^24 entries");
    MRCNN_REQUIRE(ins && cls && meta && bitmaps && prefix && table && ids && classes && boxes,
                  "label_instances: null pointer");
    const int64_t HW = (int64_t)H * W;
    MRCNN_REQUIRE((HW + 4095) / 4096 < ((int64_t)1 << 31), "label_instances: grid too large");
    const int64_t cells = (int64_t)n * ncls;
    int32_t *count = table, *first = table + cells, *cls_vals = table + 2 * cells;
    hipStream_t s = mrcnn::as_stream(stream);
    const int words_i = (span_ins + 31) / 32, words_c = (span_cls + 31) / 32;
    hipLaunchKernelGGL(table_init_kernel, dim3((unsigned)std::min<int64_t>((cells + 255) / 256, 2048)),
                       dim3(256), 0, s, cells, n, H, W, count, first, boxes);
    hipLaunchKernelGGL(values_kernel, dim3((std::max(words_i, words_c) + 255) / 256, 2), dim3(256), 0, s,
                       meta, bitmaps, prefix, words_i, words_c, ids, cls_vals);
    if (ins_bytes == 4 && cls_bytes == 4)
        launch_instances<int32_t, int32_t>(ins, cls, H, W, mask_by_class, meta, bitmaps, prefix, n,
                                           ncls, count, first, boxes, classes, cls_vals, masks, s);
    else if (ins_bytes == 4)
        launch_instances<int32_t, uint8_t>(ins, cls, H, W, mask_by_class, meta, bitmaps, prefix, n,
                                           ncls, count, first, boxes, classes, cls_vals, masks, s);
    else if (cls_bytes == 4)
        launch_instances<uint8_t, int32_t>(ins, cls, H, W, mask_by_class, meta, bitmaps, prefix, n,
                                           ncls, count, first, boxes, classes, cls_vals, masks, s);
    else
        launch_instances<uint8_t, uint8_t>(ins, cls, H, W, mask_by_class, meta, bitmaps, prefix, n,
                                           ncls, count, first, boxes, classes, cls_vals, masks, s);
    return mrcnn::check_launch("label_instances");
}

extern "C" int mrcnn_instances_to_label(const uint8_t *masks, const int32_t *order,
                                        const int32_t *labels, int N, int H, int W,
                                        int32_t *lbl_ins, int32_t *lbl_cls, void *stream)
{
    MRCNN_REQUIRE(N >= 0 && H > 0 && W > 0, "instances_to_label: bad shape");
    MRCNN_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), "instances_to_label: H*W >= 2^31");
    MRCNN_REQUIRE(lbl_ins && lbl_cls && (N == 0 || (masks && labels)),
                  "instances_to_label: null pointer");
    const int64_t HW = (int64_t)H * W;
    hipLaunchKernelGGL(paint_kernel, dim3((unsigned)((HW + 255) / 256)), dim3(256), 0,
                       mrcnn::as_stream(stream), masks, order, labels, N, HW, lbl_ins, lbl_cls);
    return mrcnn::check_launch("instances_to_label");
}
