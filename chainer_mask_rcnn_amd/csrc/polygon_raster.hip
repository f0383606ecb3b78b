// COCO polygons -> packed masks (mask format: include/mrcnn_hip.h, "Packed masks"; the rule:
// DESIGN.md section 25, arithmetic: polygon_walk.h).
//   polygon_strip  — one workgroup per (instance, 64-column word strip): for each ring of the
//                    instance, the crossings of the strip's pixel columns toggle bits of H words
//                    in LDS (atomic XOR), an XOR scan down the rows turns toggles into the even-odd
//                    fill, and the ring is ORed into the instance's words, also in LDS.  The
//                    words are stored once, with the strip's pixel count and tight bounds.
//   polygon_finish — one wavefront per instance: its strips' records -> area, extent, box.
// Work is per crossing, not per point of the dense walk: an edge crosses a column at most once, a
// shallow edge at a parameter known in closed form, a steep one at a parameter found by bisection
// (polygon_walk.h crossing_at).  XOR and OR commute, the reductions are integer min / max / sum:
// every output is exact and the same run to run.  No global atomics, no global toggle plane.
#include "common.h"
#include "mask_box.h"
#include "polygon_walk.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxH = 4000;               // two H-word arrays within 64 KiB of LDS
constexpr int kStats = 5;                 // per strip: y_lo, y_hi, x_lo, x_hi, count

// Inclusive XOR scan over the wavefront (wave64).
__device__ __forceinline__ uint64_t wave_xor_scan(uint64_t v, int lane)
{
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t o = __shfl_up((unsigned long long)v, off);
        if (lane >= off) v ^= o;
    }
    return v;
}

__global__ void __launch_bounds__(kThreads)
polygon_strip_kernel(const int32_t *__restrict__ xy5, const int32_t *__restrict__ ring_off,
                     const int32_t *__restrict__ inst_off, int H, int W, int Wq,
                     uint64_t *__restrict__ packed, int32_t *__restrict__ strip_stats)
{
    extern __shared__ uint64_t s_words[];             // toggles [H], then the instance's words [H]
    __shared__ uint64_t s_wave[kWaves];
    __shared__ int s_part[kWaves][kStats];
    uint64_t *tog = s_words, *acc = s_words + H;
    const int g = blockIdx.x / Wq, wq = blockIdx.x - g * Wq;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // this thread's rows, the same in every phase: [y0, y1)
    const int per = (H + kThreads - 1) / kThreads;
    const int y0 = min(tid * per, H), y1 = min(y0 + per, H);
    for (int y = y0; y < y1; ++y) { tog[y] = 0; acc[y] = 0; }
    __syncthreads();

    const int r0 = inst_off[g], r1 = inst_off[g + 1];
    for (int r = r0; r < r1; ++r) {                   // block-uniform
        const int v0 = ring_off[r], n = ring_off[r + 1] - v0;
        if (n < 3) continue;                          // a ring of fewer than 3 vertices sets nothing
        const int32_t *ring = xy5 + 2 * (int64_t)v0;
        for (int64_t i = tid; i < (int64_t)n * 64; i += kThreads) {
            const int j = (int)(i >> 6), k = (wq << 6) + (int)(i & 63);
            if (k >= W) continue;
            const int j1 = j + 1 == n ? 0 : j + 1;
            const mrcnn_pw::Edge e = mrcnn_pw::make_edge(ring[2 * j], ring[2 * j + 1],
                                                         ring[2 * j1], ring[2 * j1 + 1]);
            int y;
            if (mrcnn_pw::crossing_at(e, k, H, W, y) && y < H)       // y == H touches nothing
                atomicXor((unsigned long long *)&tog[y], 1ull << (k & 63));
        }
        __syncthreads();
        // even-odd fill: pixel (y, x) is set iff an odd number of toggles (y' <= y, x)
        uint64_t total = 0;
        for (int y = y0; y < y1; ++y) total ^= tog[y];
        const uint64_t incl = wave_xor_scan(total, lane);
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint64_t run = incl ^ total;                  // exclusive: the rows above this thread's
        for (int w = 0; w < wave; ++w) run ^= s_wave[w];
        for (int y = y0; y < y1; ++y) {
            run ^= tog[y];
            acc[y] |= run;
            tog[y] = 0;
        }
        __syncthreads();                              // toggles are zero again; s_wave is free
    }

    int y_lo = H, y_hi = 0, x_lo = W, x_hi = 0, count = 0;
    uint64_t *out = packed + ((int64_t)g * H) * Wq + wq;
    for (int y = y0; y < y1; ++y) {
        const uint64_t word = acc[y];                 // columns >= W are never toggled: pad bits 0
        out[(int64_t)y * Wq] = word;
        if (word) {
            y_lo = min(y_lo, y);
            y_hi = y + 1;                             // y grows within a thread
            x_lo = min(x_lo, (wq << 6) + __ffsll((unsigned long long)word) - 1);
            x_hi = max(x_hi, (wq << 6) + 64 - __clzll((long long)word));
            count += __popcll(word);
        }
    }
    y_lo = wave_min(y_lo);
    x_lo = wave_min(x_lo);
    y_hi = wave_max(y_hi);
    x_hi = wave_max(x_hi);
    count = wave_sum(count);
    if (lane == 0) {
        s_part[wave][0] = y_lo; s_part[wave][1] = y_hi; s_part[wave][2] = x_lo;
        s_part[wave][3] = x_hi; s_part[wave][4] = count;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kWaves; ++w) {
            y_lo = min(y_lo, s_part[w][0]);
            y_hi = max(y_hi, s_part[w][1]);
            x_lo = min(x_lo, s_part[w][2]);
            x_hi = max(x_hi, s_part[w][3]);
            count += s_part[w][4];
        }
        int32_t *st = strip_stats + (int64_t)blockIdx.x * kStats;
        st[0] = y_lo; st[1] = y_hi; st[2] = x_lo; st[3] = x_hi; st[4] = count;
    }
}

// One wavefront per instance: the Wq strip records -> area, extent (y_lo, y_hi, wq_lo, wq_hi) and
// box (y1, x1, y2, x2), both half-open and tight; an empty mask gets a box of zeros and the empty
// extent of mrcnn_mask_pack, (H, 0, Wq, 0).
__global__ void __launch_bounds__(kThreads)
polygon_finish_kernel(const int32_t *__restrict__ strip_stats, int G, int H, int W, int Wq,
                      int32_t *__restrict__ area, int32_t *__restrict__ extent,
                      int32_t *__restrict__ box)
{
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (g >= G) return;                               // wave-uniform
    int y_lo = H, y_hi = 0, x_lo = W, x_hi = 0, count = 0;
    for (int s = lane; s < Wq; s += 64) {
        const int32_t *st = strip_stats + ((int64_t)g * Wq + s) * kStats;
        if (st[4] > 0) {
            y_lo = min(y_lo, st[0]);
            y_hi = max(y_hi, st[1]);
            x_lo = min(x_lo, st[2]);
            x_hi = max(x_hi, st[3]);
            count += st[4];                           // <= H * W < 2^31
        }
    }
    y_lo = wave_min(y_lo);
    x_lo = wave_min(x_lo);
    y_hi = wave_max(y_hi);
    x_hi = wave_max(x_hi);
    count = wave_sum(count);
    if (lane == 0) {
        const bool any = count > 0;
        area[g] = count;
        int32_t *b = box + 4 * (int64_t)g, *e = extent + 4 * (int64_t)g;
        b[0] = any ? y_lo : 0;
        b[1] = any ? x_lo : 0;
        b[2] = any ? y_hi : 0;
        b[3] = any ? x_hi : 0;
        e[0] = y_lo;                                  // empty: (H, 0, Wq, 0), as mrcnn_mask_pack
        e[1] = y_hi;
        e[2] = any ? x_lo >> 6 : Wq;
        e[3] = any ? ((x_hi - 1) >> 6) + 1 : 0;
    }
}

}  // namespace

extern "C" int64_t mrcnn_polygon_rasterize_workspace_bytes(int G, int H, int W)
{
    if (G <= 0 || H <= 0 || W <= 0) return 0;
    return (int64_t)G * ((W + 63) / 64) * kStats * (int64_t)sizeof(int32_t);
}

extern "C" int mrcnn_polygon_rasterize(const int32_t *xy5, const int32_t *ring_off,
                                       const int32_t *inst_off, int G, int H, int W,
                                       uint64_t *packed, int32_t *area, int32_t *extent,
                                       int32_t *box, void *ws, void *stream)
{
    MRCNN_REQUIRE(G >= 0 && H > 0 && W > 0, "polygon_rasterize: bad shape");
    MRCNN_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), "polygon_rasterize: H*W >= 2^31");
    MRCNN_REQUIRE(H <= kMaxH, "polygon_rasterize: H > %d (two H-word arrays are kept in LDS)", kMaxH);
    if (G == 0) return 0;
    const int Wq = (W + 63) / 64;
    MRCNN_REQUIRE((int64_t)G * Wq < ((int64_t)1 << 31), "polygon_rasterize: G*ceil(W/64) >= 2^31");
    MRCNN_REQUIRE(ring_off && inst_off && packed && area && extent && box && ws,
                  "polygon_rasterize: null pointer");      // xy5 may be null: no vertices at all
    MRCNN_REQUIRE(((uintptr_t)ws & 3) == 0, "polygon_rasterize: ws must be 4-byte aligned");
    hipStream_t s = mrcnn::as_stream(stream);
    int32_t *stats = (int32_t *)ws;
    hipLaunchKernelGGL(polygon_strip_kernel, dim3((unsigned)((int64_t)G * Wq)), dim3(kThreads),
                       2 * (size_t)H * sizeof(uint64_t), s, xy5, ring_off, inst_off, H, W, Wq,
                       packed, stats);
    if (int rc = mrcnn::check_launch("polygon_rasterize (strips)")) return rc;
    hipLaunchKernelGGL(polygon_finish_kernel, dim3((unsigned)mrcnn::ceil_div(G, kWaves)),
                       dim3(kThreads), 0, s, (const int32_t *)stats, G, H, W, Wq, area, extent, box);
    return mrcnn::check_launch("polygon_rasterize (finish)");
}
