// Soft-NMS and bounding-box voting on score-sorted boxes for gfx950 (wave64): Detectron's two
// test-time options (TEST.SOFT_NMS, Bodla et al. 2017: utils/cython_nms.pyx:cpu_soft_nms;
// TEST.BBOX_VOTE: utils/boxes.py:box_voting with scoring method ID), decided on the device
// behind mrcnn_detect_sort and in front of mrcnn_detect_compact.
//
// Soft-NMS per group, as the sequential rule this file reproduces bit for bit:
//
//   s = sorted_prob[:n]; every row alive
//   repeat: i = the alive row with the largest s (ties: the lowest row);
//           stop if none is alive, or not (s[i] >= min_score), or `limit` picks were made;
//           emit i, alive[i] = false; for every alive j: s[j] = s[j] * w(iou_pair(box_i, box_j))
//   w hard:     iou >= Nt ? 0 : 1
//   w linear:   iou >= Nt ? 1 - iou : 1                                   (fp32)
//   w gaussian: iou > 0 ? (float)exp(-((double)iou * (double)iou) / (double)sigma) : 1
//
// (cpu_soft_nms prunes rows below min_score after every pick; scores only fall, so stopping at the
// first maximum below min_score emits the same rows.)  A NaN IoU (zero-area boxes) fails both
// predicates: weight 1.  IoU is bbox_iou.h's iou_pair, the fp32 operation sequence of the
// bit-mask NMS (nms.hip: iou_ge), so method hard keeps exactly the rows mrcnn_nms_sorted_batched
// keeps.  Input contract: scores are finite and non-negative (mrcnn_detect_sort's
// `prob > thresh` guarantees it); their bit patterns then order like their values.
//
// The picks are a serial chain: which row is picked next depends on every decay before it, so no
// suppression word can be precomputed as nms.hip does.  What one link costs is the design:
//   * one workgroup of 4 waves per group; a thread owns rows tid, tid + 256, ... and keeps their
//     boxes and live scores in registers for the whole problem (RPT = 1, 4 or 16 rows per thread);
//   * per pick one arg-max on the 64-bit key (score bits << 32) | ~row: RPT compares per thread,
//     six cross-lane steps per wave, then the wave's winning lane puts its key AND its box into the
//     wave's LDS slot, so that after the one barrier of the link every thread reads four keys and
//     the winner's box from LDS and nothing from global memory;
//   * the slots are double buffered: a slot written for pick t + 2 was last read for pick t, before
//     the barrier of pick t + 1, so one barrier per link is enough;
//   * every thread then decays its own alive rows; nobody else reads them.
// Rows below min_score keep decaying (the rule above says so, and soft_prob reports it); they can
// win the arg-max only when every alive row is below min_score, where the loop ends.
#include "common.h"
#include "bbox_iou.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSoftNmsMaxRows = 16 * kThreads;        // RPT = 16
constexpr int kVoteTile = 256;

struct __attribute__((aligned(16))) PickSlot {
    float box[4];
    unsigned long long key;
    unsigned long long pad;
};

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int off)
{
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off, 64);
    return ((unsigned long long)hi << 32) | lo;
}

template <int METHOD>
__device__ __forceinline__ float decay_weight(float iou, float nt, double sigma)
{
    if (METHOD == MRCNN_SOFT_NMS_HARD) return iou >= nt ? 0.f : 1.f;
    if (METHOD == MRCNN_SOFT_NMS_LINEAR) return iou >= nt ? 1.f - iou : 1.f;
    return iou > 0.f ? (float)exp(-((double)iou * (double)iou) / sigma) : 1.f;
}

// grid (groups), block 256.
template <int RPT, int METHOD>
__global__ void __launch_bounds__(kThreads)
soft_nms_kernel(const float4 *__restrict__ boxes_all, const float *__restrict__ prob_all,
                const int32_t *__restrict__ n_dev, int n_max, float nt, float sigma_f,
                float min_score, int limit, int32_t *__restrict__ keep_all,
                int32_t *__restrict__ n_keep_all, float *__restrict__ soft_all)
{
    __shared__ PickSlot slots[2][kWaves];
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float4 *__restrict__ boxes = boxes_all + (int64_t)g * n_max;
    const float *__restrict__ prob = prob_all + (int64_t)g * n_max;
    int32_t *__restrict__ keep = keep_all + (int64_t)g * n_max;
    float *__restrict__ soft = soft_all + (int64_t)g * n_max;
    const int n = max(min(n_dev[g], n_max), 0);
    const double sigma = (double)sigma_f;

    float box[RPT][4], s[RPT];
    uint32_t alive = 0;
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
        const int row = k * kThreads + tid;
        const bool ok = row < n;
        const float4 b = ok ? boxes[row] : make_float4(0.f, 0.f, 0.f, 0.f);
        box[k][0] = b.x; box[k][1] = b.y; box[k][2] = b.z; box[k][3] = b.w;
        s[k] = ok ? prob[row] : 0.f;
        if (ok) alive |= 1u << k;
    }

    int t = 0;
    for (;; ++t) {
        if (limit > 0 && t >= limit) break;
        // this thread's best alive row; the key of a dead row is 0, below every alive row's
        unsigned long long best = 0ull;
        float bb[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
            const uint32_t row = (uint32_t)(k * kThreads + tid);
            const unsigned long long key = ((alive >> k) & 1u)
                ? ((unsigned long long)__float_as_uint(s[k]) << 32) | (uint32_t)~row : 0ull;
            if (key > best) {
                best = key;
                bb[0] = box[k][0]; bb[1] = box[k][1]; bb[2] = box[k][2]; bb[3] = box[k][3];
            }
        }
        unsigned long long wmax = best;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = shfl_xor_u64(wmax, off);
            wmax = o > wmax ? o : wmax;
        }
        PickSlot *slot = &slots[t & 1][wave];
        if (wmax == 0ull ? lane == 0 : best == wmax) {       // keys are unique: exactly one lane
            slot->box[0] = bb[0]; slot->box[1] = bb[1]; slot->box[2] = bb[2]; slot->box[3] = bb[3];
            slot->key = wmax;
        }
        __syncthreads();
        unsigned long long gmax = slots[t & 1][0].key;
        int gw = 0;
#pragma unroll
        for (int w = 1; w < kWaves; ++w) {
            const unsigned long long o = slots[t & 1][w].key;
            if (o > gmax) { gmax = o; gw = w; }
        }
        if (gmax == 0ull) break;                              // nothing alive
        const float score = __uint_as_float((uint32_t)(gmax >> 32));
        if (!(score >= min_score)) break;
        const int row_i = (int)~(uint32_t)gmax;
        float bi[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) bi[c] = slots[t & 1][gw].box[c];
        if (tid == 0) {
            keep[t] = row_i;
            soft[row_i] = score;
        }
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
            if (k * kThreads + tid == row_i) alive &= ~(1u << k);
            if ((alive >> k) & 1u)
                s[k] = s[k] * decay_weight<METHOD>(mrcnn::iou_pair(bi, box[k]), nt, sigma);
        }
    }
    if (tid == 0) n_keep_all[g] = t;
    // rows never picked report the score they had decayed to
#pragma unroll
    for (int k = 0; k < RPT; ++k)
        if ((alive >> k) & 1u) soft[k * kThreads + tid] = s[k];
}

template <int RPT>
void launch_soft_nms(int method, int groups, hipStream_t s, const float4 *boxes, const float *prob,
                     const int32_t *n_dev, int n_max, float nt, float sigma, float min_score,
                     int limit, int32_t *keep, int32_t *n_keep, float *soft)
{
    if (method == MRCNN_SOFT_NMS_HARD)
        hipLaunchKernelGGL((soft_nms_kernel<RPT, MRCNN_SOFT_NMS_HARD>), dim3(groups), dim3(kThreads),
                           0, s, boxes, prob, n_dev, n_max, nt, sigma, min_score, limit, keep,
                           n_keep, soft);
    else if (method == MRCNN_SOFT_NMS_LINEAR)
        hipLaunchKernelGGL((soft_nms_kernel<RPT, MRCNN_SOFT_NMS_LINEAR>), dim3(groups),
                           dim3(kThreads), 0, s, boxes, prob, n_dev, n_max, nt, sigma, min_score,
                           limit, keep, n_keep, soft);
    else
        hipLaunchKernelGGL((soft_nms_kernel<RPT, MRCNN_SOFT_NMS_GAUSSIAN>), dim3(groups),
                           dim3(kThreads), 0, s, boxes, prob, n_dev, n_max, nt, sigma, min_score,
                           limit, keep, n_keep, soft);
}

// grid (ceil(n_max / 64), groups), block 64: thread q votes for the q-th kept row of its group.
// The candidates pass through LDS a tile at a time; every thread walks them in row order, so the
// float64 sums have one fixed order.
__global__ void __launch_bounds__(64)
box_vote_kernel(const float4 *__restrict__ boxes_all, const float *__restrict__ prob_all,
                const int32_t *__restrict__ n_dev, const int32_t *__restrict__ keep_all,
                const int32_t *__restrict__ n_keep_all, int n_max, float thresh,
                float4 *__restrict__ voted_all)
{
    __shared__ float4 tbox[kVoteTile];
    __shared__ float tprob[kVoteTile];
    const int g = blockIdx.y;
    const int n = max(min(n_dev[g], n_max), 0);
    const int nk = max(min(n_keep_all[g], n_max), 0);
    if ((int)blockIdx.x * 64 >= nk) return;                   // (block-uniform)
    const float4 *__restrict__ boxes = boxes_all + (int64_t)g * n_max;
    const float *__restrict__ prob = prob_all + (int64_t)g * n_max;
    const int q = blockIdx.x * 64 + threadIdx.x;
    int k = q < nk ? keep_all[(int64_t)g * n_max + q] : -1;
    if (k < 0 || k >= n_max) k = -1;                          // never index with a stray keep entry
    float bk[4] = {0.f, 0.f, 0.f, 0.f};
    if (k >= 0) {
        const float4 b = boxes[k];
        bk[0] = b.x; bk[1] = b.y; bk[2] = b.z; bk[3] = b.w;
    }
    double acc[4] = {0., 0., 0., 0.}, wsum = 0.;
    for (int j0 = 0; j0 < n; j0 += kVoteTile) {
        const int nt = min(kVoteTile, n - j0);
        __syncthreads();
        for (int j = threadIdx.x; j < nt; j += 64) {
            tbox[j] = boxes[j0 + j];
            tprob[j] = prob[j0 + j];
        }
        __syncthreads();
        if (k >= 0) {
            for (int j = 0; j < nt; ++j) {
                const float4 b = tbox[j];
                const float bj[4] = {b.x, b.y, b.z, b.w};
                if (mrcnn::iou_pair(bk, bj) >= thresh) {
                    const double w = (double)tprob[j];
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc[c] += w * (double)bj[c];
                    wsum += w;
                }
            }
        }
    }
    if (k >= 0) {
        float4 out = make_float4(bk[0], bk[1], bk[2], bk[3]);
        if (wsum != 0.)
            out = make_float4((float)(acc[0] / wsum), (float)(acc[1] / wsum),
                              (float)(acc[2] / wsum), (float)(acc[3] / wsum));
        voted_all[(int64_t)g * n_max + k] = out;
    }
}

}  // namespace

extern "C" int mrcnn_soft_nms_sorted_batched(const float *sorted_boxes, const float *sorted_prob,
                                             const int32_t *counts, int groups, int n_max,
                                             int method, float overlap_thresh, float sigma,
                                             float min_score, int limit, int32_t *keep,
                                             int32_t *n_keep, float *soft_prob, void *stream)
{
    MRCNN_REQUIRE(groups >= 0 && n_max >= 0, "soft_nms: bad shape");
    MRCNN_REQUIRE(method == MRCNN_SOFT_NMS_HARD || method == MRCNN_SOFT_NMS_LINEAR ||
                      method == MRCNN_SOFT_NMS_GAUSSIAN,
                  "soft_nms: method must be 0 (hard), 1 (linear) or 2 (gaussian), got %d", method);
    MRCNN_REQUIRE(method != MRCNN_SOFT_NMS_GAUSSIAN || sigma > 0.f,
                  "soft_nms: the gaussian method needs a positive sigma (got %g)", (double)sigma);
    MRCNN_REQUIRE(n_max <= kSoftNmsMaxRows, "soft_nms: n_max %d above the limit of %d rows per group",
                  n_max, kSoftNmsMaxRows);
    hipStream_t s = mrcnn::as_stream(stream);
    if (groups == 0) return 0;
    MRCNN_REQUIRE(n_keep, "soft_nms: null n_keep");
    if (n_max == 0) {
        MRCNN_HIP_TRY(hipMemsetAsync(n_keep, 0, 4 * (size_t)groups, s));
        return 0;
    }
    MRCNN_REQUIRE(sorted_boxes && sorted_prob && counts && keep && soft_prob, "soft_nms: null pointer");
    MRCNN_REQUIRE((uintptr_t)sorted_boxes % 16 == 0, "soft_nms: boxes must be 16-byte aligned");
    MRCNN_REQUIRE(groups <= 65535, "soft_nms: grid too large");
    const float4 *b4 = (const float4 *)sorted_boxes;
    if (n_max <= kThreads)
        launch_soft_nms<1>(method, groups, s, b4, sorted_prob, counts, n_max, overlap_thresh, sigma,
                           min_score, limit, keep, n_keep, soft_prob);
    else if (n_max <= 4 * kThreads)
        launch_soft_nms<4>(method, groups, s, b4, sorted_prob, counts, n_max, overlap_thresh, sigma,
                           min_score, limit, keep, n_keep, soft_prob);
    else
        launch_soft_nms<16>(method, groups, s, b4, sorted_prob, counts, n_max, overlap_thresh, sigma,
                            min_score, limit, keep, n_keep, soft_prob);
    return mrcnn::check_launch("soft_nms_sorted_batched");
}

extern "C" int mrcnn_box_vote(const float *sorted_boxes, const float *sorted_prob,
                              const int32_t *counts, const int32_t *keep, const int32_t *n_keep,
                              int groups, int n_max, float vote_thresh, float *voted_boxes,
                              void *stream)
{
    MRCNN_REQUIRE(groups >= 0 && n_max >= 0, "box_vote: bad shape");
    MRCNN_REQUIRE(vote_thresh == vote_thresh, "box_vote: vote_thresh is NaN");
    MRCNN_REQUIRE(n_max <= 65535 * 64, "box_vote: n_max %d above the limit of %d rows per group",
                  n_max, 65535 * 64);
    if (groups == 0 || n_max == 0) return 0;
    MRCNN_REQUIRE(sorted_boxes && sorted_prob && counts && keep && n_keep && voted_boxes,
                  "box_vote: null pointer");
    MRCNN_REQUIRE(((uintptr_t)sorted_boxes | (uintptr_t)voted_boxes) % 16 == 0,
                  "box_vote: boxes must be 16-byte aligned");
    MRCNN_REQUIRE(groups <= 65535, "box_vote: grid too large");
    hipLaunchKernelGGL(box_vote_kernel, dim3((n_max + 63) / 64, groups), dim3(64), 0,
                       mrcnn::as_stream(stream), (const float4 *)sorted_boxes, sorted_prob, counts,
                       keep, n_keep, n_max, vote_thresh, (float4 *)voted_boxes);
    return mrcnn::check_launch("box_vote");
}
