// Packed instance masks for evaluation (mask format: include/mrcnn_hip.h, "Packed masks"):
//   mask_pack      — (N, H, W) uint8 / int32 masks -> one bit per pixel, exact areas, extents
//   mask_intersect — pairwise |A_p & B_g| over the overlap of the two extents
// Replaces the full-image np.bitwise_and / np.bitwise_or of the reference's get_mask_overlap
// (chainer_mask_rcnn/utils/geometry.py) and pycocotools' RLE intersection: only P x G integer
// counts and the areas leave the device.  Everything is integer arithmetic (popcounts, integer
// atomics), so every result is exact and independent of scheduling.
#include "common.h"

namespace {

// area 0 and an empty extent that the row atomics below widen: (y_lo, y_hi) = (H, 0),
// (wq_lo, wq_hi) = (Wq, 0).  A mask with no set bit keeps an empty extent (lo >= hi).
__global__ void pack_init_kernel(int N, int H, int Wq, int32_t *__restrict__ area,
                                 int32_t *__restrict__ extent)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    area[n] = 0;
    int32_t *e = extent + 4 * n;
    e[0] = H; e[1] = 0; e[2] = Wq; e[3] = 0;
}

// One 256-thread workgroup per (mask, row).  Each wave reads 64 consecutive pixels per
// iteration, __ballot turns them into one packed word (bit l = lane l, wave64: exactly one
// word), lane 0 stores it.  The row's popcount and its first / last nonzero word are reduced
// in LDS; one thread then folds them into area / extent with integer atomics.
template <typename T>
__global__ void __launch_bounds__(256)
pack_kernel(const T *__restrict__ masks, int H, int W, int Wq, uint64_t *__restrict__ packed,
            int32_t *__restrict__ area, int32_t *__restrict__ extent)
{
    const int row = blockIdx.x;                       // n * H + y
    const int n = row / H, y = row - n * H;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T *src = masks + (int64_t)row * W;
    uint64_t *out = packed + (int64_t)row * Wq;
    int count = 0, wlo = Wq, whi = -1;
    for (int w = wave; w < Wq; w += 4) {
        const int x = (w << 6) + lane;
        const uint64_t bits = __ballot(x < W && src[x] != 0);
        if (bits) {
            count += __popcll(bits);
            wlo = min(wlo, w);
            whi = max(whi, w);
        }
        if (lane == 0) out[w] = bits;
    }
    // bits, count, wlo and whi are uniform across a wave: lane 0 speaks for it
    __shared__ int s_count[4], s_lo[4], s_hi[4];
    if (lane == 0) {
        s_count[wave] = count;
        s_lo[wave] = wlo;
        s_hi[wave] = whi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0, lo = Wq, hi = -1;
        for (int i = 0; i < 4; ++i) {
            c += s_count[i];
            lo = min(lo, s_lo[i]);
            hi = max(hi, s_hi[i]);
        }
        if (c) {
            int32_t *e = extent + 4 * n;
            atomicAdd(area + n, c);
            atomicMin(e + 0, y);
            atomicMax(e + 1, y + 1);
            atomicMin(e + 2, lo);
            atomicMax(e + 3, hi + 1);
        }
    }
}

// Wave-wide integer sum (wave64).
__device__ __forceinline__ int wave_sum(int v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// One wave per (p, g) pair, four pairs per 256-thread workgroup.  The wave walks the words of
// the overlap rectangle of the two extents (clamped to the image) flattened row-major, 64
// words per step, and accumulates __popcll(a & b); a pair whose extents do not overlap stores
// 0 without reading the masks.
__global__ void __launch_bounds__(256)
intersect_kernel(const uint64_t *__restrict__ a, const int32_t *__restrict__ ext_a, int P,
                 const uint64_t *__restrict__ b, const int32_t *__restrict__ ext_b, int G, int H,
                 int Wq, int32_t *__restrict__ inter)
{
    const int64_t pair = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (pair >= (int64_t)P * G) return;
    const int p = (int)(pair / G), g = (int)(pair - (int64_t)p * G);
    const int32_t *ea = ext_a + 4 * p, *eb = ext_b + 4 * g;
    const int y0 = max(max(ea[0], eb[0]), 0), y1 = min(min(ea[1], eb[1]), H);
    const int w0 = max(max(ea[2], eb[2]), 0), w1 = min(min(ea[3], eb[3]), Wq);
    int count = 0;
    if (y0 < y1 && w0 < w1) {
        const int nw = w1 - w0;
        const int64_t total = (int64_t)(y1 - y0) * nw;
        const uint64_t *pa = a + (int64_t)p * H * Wq, *pb = b + (int64_t)g * H * Wq;
        // (y, w) of flat index i = lane + 64 k, advanced by 64 words per step without a division
        const int dq = 64 / nw, dr = 64 % nw;
        int y = y0 + lane / nw, w = w0 + lane % nw;
        for (int64_t i = lane; i < total; i += 64) {
            const int64_t off = (int64_t)y * Wq + w;
            count += __popcll(pa[off] & pb[off]);
            y += dq;
            w += dr;
            if (w >= w1) {
                w -= nw;
                ++y;
            }
        }
        count = wave_sum(count);
    }
    if (lane == 0) inter[pair] = count;
}

}  // namespace

extern "C" int mrcnn_mask_pack(const void *masks, int elem_bytes, int N, int H, int W,
                               uint64_t *packed, int32_t *area, int32_t *extent, void *stream)
{
    MRCNN_REQUIRE(N >= 0 && H > 0 && W > 0, "mask_pack: bad shape");
    MRCNN_REQUIRE(elem_bytes == 1 || elem_bytes == 4, "mask_pack: elem_bytes must be 1 or 4");
    MRCNN_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), "mask_pack: H*W >= 2^31");
    if (N == 0) return 0;
    MRCNN_REQUIRE(masks && packed && area && extent, "mask_pack: null pointer");
    MRCNN_REQUIRE((int64_t)N * H < ((int64_t)1 << 31), "mask_pack: grid too large");
    const int Wq = (W + 63) / 64;
    hipStream_t s = mrcnn::as_stream(stream);
    hipLaunchKernelGGL(pack_init_kernel, dim3((N + 255) / 256), dim3(256), 0, s, N, H, Wq, area,
                       extent);
    if (elem_bytes == 1)
        hipLaunchKernelGGL(pack_kernel<uint8_t>, dim3(N * H), dim3(256), 0, s,
                           (const uint8_t *)masks, H, W, Wq, packed, area, extent);
    else
        hipLaunchKernelGGL(pack_kernel<int32_t>, dim3(N * H), dim3(256), 0, s,
                           (const int32_t *)masks, H, W, Wq, packed, area, extent);
    return mrcnn::check_launch("mask_pack");
}

extern "C" int mrcnn_mask_intersect(const uint64_t *a, const int32_t *ext_a, int P,
                                    const uint64_t *b, const int32_t *ext_b, int G, int H,
                                    int W, int32_t *inter, void *stream)
{
    MRCNN_REQUIRE(P >= 0 && G >= 0 && H > 0 && W > 0, "mask_intersect: bad shape");
    MRCNN_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), "mask_intersect: H*W >= 2^31");
    const int Wq = (W + 63) / 64;
    if (P == 0 || G == 0) return 0;
    MRCNN_REQUIRE(a && ext_a && b && ext_b && inter, "mask_intersect: null pointer");
    const int64_t blocks = ((int64_t)P * G + 3) / 4;
    MRCNN_REQUIRE(blocks < ((int64_t)1 << 31), "mask_intersect: grid too large");
    hipLaunchKernelGGL(intersect_kernel, dim3((unsigned)blocks), dim3(256), 0,
                       mrcnn::as_stream(stream), a, ext_a, P, b, ext_b, G, H, Wq, inter);
    return mrcnn::check_launch("mask_intersect");
}
