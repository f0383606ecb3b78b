// Simple Copy-Paste on the device: K instances of a source example pasted
// onto a target example, both already on the S x S canvas of large-scale jitter (section 18).
//   alpha             = OR over k of masks_s[idx[k]]
//   img_out           = alpha ? img_s : img_t            a select per pixel, never a blend
//   masks_out[g]      = masks_t[g] & ~alpha   (g < Gt)   occluded by the paste
//   masks_out[Gt + k] = masks_s[idx[k]]       (k < K)
//   box, area         = tight box and pixel count of each output mask
// Two launches on one stream: the masks and the image, each workgroup with the alpha of its own
// rows packed one bit per pixel in LDS; then the per-row records -> boxes and areas (mask_box.h,
// the kernel of mrcnn_mask_resize_crop).
// The reference has no copy-paste augmentation (chainer_mask_rcnn/datasets/transforms.py:10-51
// resizes and flips one example).  The rules are those of gt_masks.hip / scale_jitter.hip: integer
// arithmetic only on the mask side, no atomics, no scratch, the same result for
// any execution order, every byte of every output written.  The image is moved as 32-bit patterns, so NaN
// payloads and -0.0 survive and nothing of the unselected image reaches the output.
#include "common.h"
#include "mask_box.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRows = 8;                              // output rows per workgroup (2 per wave)
constexpr int kMinPlanes = 8, kMaxChunks = 4;         // planes of one row group are split at the most so

// each byte of v -> 1 if it is not 0 (no carry crosses a byte: 0x7f + 0x7f < 0x100)
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t v)
{
    return ((((v & 0x7f7f7f7fu) + 0x7f7f7f7fu) | v) & 0x80808080u) >> 7;
}

// p[0..3] as one dword, whatever the alignment of p (a source row starts anywhere: S may be odd)
__device__ __forceinline__ uint32_t load4(const uint8_t *p)
{
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

// bytes x0 .. x0+3 of a row of S, those outside [0, S) as 0
__device__ __forceinline__ uint32_t load_row4(const uint8_t *row, int x0, int S)
{
    if (x0 >= 0 && x0 + 4 <= S) return load4(row + x0);
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (x0 + j >= 0 && x0 + j < S) v |= (uint32_t)row[x0 + j] << (8 * j);
    return v;
}

// source instance of pasted plane k; clamped, so that no read leaves masks_s whatever idx holds
__device__ __forceinline__ int source_index(const int32_t *idx, int k, int Gs)
{
    return min(max(idx[k], 0), Gs - 1);
}

// Grid: groups of kRows canvas rows x chunks of planes; planes 0 .. Gt+K-1 are the output masks,
// plane Gt+K is the image.  A wave owns rows wave and wave + kWaves of the group, in every plane.
//
// First the alpha of the group's rows, one bit per pixel, in LDS (kRows, Wq): a step covers 256
// pixels, four per lane; the K selected source rows are ORed as bytes, four rows in flight where the
// whole step lies inside the row; a lane's four pixels become a nibble and an OR over each group of
// 16 lanes leaves one 64-bit word.  Bits past S are 0.  Nothing of it leaves the workgroup: a chunk
// of planes builds the alpha of its rows itself (the host keeps the chunks few), and a chunk that
// holds pasted planes only skips it.
//
// Then the planes.  Mask rows are built four bytes per lane and step.  As in
// mask_resize_crop_kernel the dwords are aligned on the output ADDRESS and the dwords that straddle
// a row's ends are written as single bytes; a source byte other than 0 counts as set and is written
// as 1; a target plane loses the pixels of alpha.  Lane 0 of the wave leaves the row's
// (x_lo, x_hi, count) in row_stats.  The image is one pixel of three dwords per lane and step, both
// sources loaded before the select.
__global__ void __launch_bounds__(kThreads)
paste_kernel(const uint32_t *__restrict__ img_t, const uint32_t *__restrict__ img_s,
             const uint8_t *__restrict__ masks_t, int Gt, const uint8_t *__restrict__ masks_s,
             int Gs, const int32_t *__restrict__ idx, int K, int S, int Wq, int groups,
             int planes_per_chunk, uint32_t *__restrict__ img_out,
             uint8_t *__restrict__ masks_out, int32_t *__restrict__ row_stats)
{
    extern __shared__ uint64_t s_alpha[];             // (kRows, Wq) words
    const int chunk = blockIdx.x / groups;
    const int y_base = (blockIdx.x - chunk * groups) * kRows;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = Gt + K;
    const int p_lo = chunk * planes_per_chunk, p_hi = min(p_lo + planes_per_chunk, n + 1);
    if (p_lo < Gt || p_hi > n) {                      // an occluded plane or the image: workgroup-uniform
        for (int r = wave; r < kRows; r += kWaves) {
            const int y = y_base + r;
            if (y >= S) break;
            const int64_t row_off = (int64_t)y * S;
            const int64_t plane = (int64_t)S * S;
            for (int c = 0; 256 * c < S; ++c) {
                const int x0 = 256 * c + 4 * lane;
                uint32_t v = 0;
                int k = 0;
                if (256 * c + 256 <= S) {             // wave-uniform: every lane loads a whole dword
                    for (; k + 4 <= K; k += 4) {
                        const uint32_t a = load4(masks_s + source_index(idx, k, Gs) * plane + row_off + x0);
                        const uint32_t b = load4(masks_s + source_index(idx, k + 1, Gs) * plane + row_off + x0);
                        const uint32_t e = load4(masks_s + source_index(idx, k + 2, Gs) * plane + row_off + x0);
                        const uint32_t f = load4(masks_s + source_index(idx, k + 3, Gs) * plane + row_off + x0);
                        v |= (a | b) | (e | f);
                    }
                }
                for (; k < K; ++k)
                    v |= load_row4(masks_s + source_index(idx, k, Gs) * plane + row_off, x0, S);
                const uint32_t nz = nonzero_bytes(v);
                const uint32_t nibble = (nz | nz >> 7 | nz >> 14 | nz >> 21) & 0xfu;
                uint64_t word = (uint64_t)nibble << (4 * (lane & 15));
                for (int off = 1; off < 16; off <<= 1) word |= __shfl_xor(word, off);
                const int w = 4 * c + (lane >> 4);
                if ((lane & 15) == 0 && w < Wq) s_alpha[r * Wq + w] = word;
            }
        }
    }
    __syncthreads();

    for (int p = p_lo; p < p_hi; ++p) {
        if (p == n) {
            for (int r = wave; r < kRows; r += kWaves) {
                const int y = y_base + r;
                if (y >= S) break;
                const uint64_t *arow = s_alpha + r * Wq;
                const int64_t base = (int64_t)y * S * 3;
                for (int x = lane; x < S; x += 64) {
                    const uint32_t *t = img_t + base + 3 * x, *s = img_s + base + 3 * x;
                    const uint32_t t0 = t[0], t1 = t[1], t2 = t[2];
                    const uint32_t s0 = s[0], s1 = s[1], s2 = s[2];
                    const bool pasted = (arow[x >> 6] >> (x & 63)) & 1;
                    uint32_t *o = img_out + base + 3 * x;
                    o[0] = pasted ? s0 : t0;
                    o[1] = pasted ? s1 : t1;
                    o[2] = pasted ? s2 : t2;
                }
            }
            continue;
        }
        const bool occlude = p < Gt;                  // workgroup-uniform
        const uint8_t *plane = occlude ? masks_t + (int64_t)p * S * S
                                       : masks_s + (int64_t)source_index(idx, p - Gt, Gs) * S * S;
        for (int r = wave; r < kRows; r += kWaves) {
            const int y = y_base + r;
            if (y >= S) break;
            const uint8_t *src = plane + (int64_t)y * S;
            const uint64_t *arow = s_alpha + r * Wq;
            const int64_t row = (int64_t)p * S + y;
            uint8_t *dst = masks_out + row * S;
            const int mis = (int)((uintptr_t)dst & 3);    // bytes between the dword boundary and dst
            const int n_dwords = (mis + S + 3) >> 2;
            int lo = S, hi = 0, count = 0;
            for (int d = lane; d < n_dwords; d += 64) {
                const int x0 = 4 * d - mis;           // dst + x0 is dword-aligned; -3 <= x0 < S
                uint32_t v = nonzero_bytes(load_row4(src, x0, S));
                if (occlude) {
                    const int xa = max(x0, 0), wi = xa >> 6, sh = xa & 63;
                    uint64_t bits = arow[wi] >> sh;   // alpha of pixels xa, xa + 1, ...
                    if (sh > 60 && wi + 1 < Wq) bits |= arow[wi + 1] << (64 - sh);
                    const uint32_t m = ((uint32_t)bits << (xa - x0)) & 0xfu;   // of x0 .. x0 + 3
                    v &= ~((m & 1u) | (m & 2u) << 7 | (m & 4u) << 14 | (m & 8u) << 21);
                }
                if (v) {                              // bytes outside the row are 0
                    lo = min(lo, x0 + ((__ffs((int)v) - 1) >> 3));
                    hi = x0 + ((31 - __clz((int)v)) >> 3) + 1;   // x grows within a lane
                    count += __popc(v);
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
}

struct Range {
    const char *lo, *hi;
    bool output;
};

Range range_of(const void *p, int64_t bytes, bool output)
{
    return Range{(const char *)p, (const char *)p + (p ? bytes : 0), output};
}

}  // namespace

extern "C" int mrcnn_copy_paste(const float *img_t, const float *img_s, const uint8_t *masks_t,
                                int Gt, const uint8_t *masks_s, int Gs, const int32_t *idx, int K,
                                int S, float *img_out, uint8_t *masks_out, int32_t *box,
                                int32_t *area, int32_t *row_stats, void *stream)
{
    MRCNN_REQUIRE(S > 0, "copy_paste: S <= 0");
    MRCNN_REQUIRE(Gt >= 0 && Gs >= 0 && K >= 0, "copy_paste: negative count");
    MRCNN_REQUIRE(K <= Gs, "copy_paste: K > Gs (more instances to paste than the source has)");
    const int64_t n = (int64_t)Gt + K, px = (int64_t)S * S;
    MRCNN_REQUIRE(n * px < ((int64_t)1 << 31), "copy_paste: (Gt+K)*S*S >= 2^31");
    MRCNN_REQUIRE(px * 3 < ((int64_t)1 << 31), "copy_paste: S*S*3 >= 2^31");
    MRCNN_REQUIRE(img_t && img_s && img_out, "copy_paste: null pointer");
    MRCNN_REQUIRE(Gt == 0 || masks_t, "copy_paste: null pointer");
    MRCNN_REQUIRE(K == 0 || (masks_s && idx), "copy_paste: null pointer");
    MRCNN_REQUIRE(n == 0 || (masks_out && box && area && row_stats), "copy_paste: null pointer");
    const int Wq = (S + 63) / 64;
    // No output or workspace may overlap an input or another output: the image is refused in
    // place too (img_out == img_t), although a pixel depends on its own position only.
    const Range ranges[] = {
        range_of(img_t, px * 12, false),        range_of(img_s, px * 12, false),
        range_of(masks_t, Gt * px, false),      range_of(masks_s, (K ? Gs : 0) * px, false),
        range_of(idx, (int64_t)K * 4, false),   range_of(img_out, px * 12, true),
        range_of(masks_out, n * px, true),      range_of(box, n * 16, true),
        range_of(area, n * 4, true),            range_of(row_stats, n * S * 12, true)};
    const int n_ranges = (int)(sizeof(ranges) / sizeof(ranges[0]));
    for (int a = 0; a < n_ranges; ++a)
        for (int b = a + 1; b < n_ranges; ++b) {
            const Range &p = ranges[a], &q = ranges[b];
            if (!(p.output || q.output) || p.lo == p.hi || q.lo == q.hi) continue;
            MRCNN_REQUIRE(p.hi <= q.lo || q.hi <= p.lo,
                          "copy_paste: an output or workspace overlaps an input or another output");
        }
    hipStream_t s = mrcnn::as_stream(stream);
    // Every chunk of planes builds the alpha of its rows again: few chunks, of 8 planes or more.
    const int groups = (S + kRows - 1) / kRows;
    int chunks = (int)((n + 1 + kMinPlanes - 1) / kMinPlanes);
    chunks = chunks < kMaxChunks ? chunks : kMaxChunks;
    const int planes_per_chunk = (int)((n + 1 + chunks - 1) / chunks);
    hipLaunchKernelGGL(paste_kernel, dim3((unsigned)(groups * chunks)), dim3(kThreads),
                       (size_t)kRows * Wq * 8, s, (const uint32_t *)img_t, (const uint32_t *)img_s,
                       masks_t, Gt, masks_s, Gs, idx, K, S, Wq, groups, planes_per_chunk,
                       (uint32_t *)img_out, masks_out, row_stats);
    if (n > 0)
        hipLaunchKernelGGL(mask_box_kernel, dim3((unsigned)n), dim3(kMaskBoxThreads), 0, s,
                           row_stats, S, box, area);
    return mrcnn::check_launch("copy_paste");
}
