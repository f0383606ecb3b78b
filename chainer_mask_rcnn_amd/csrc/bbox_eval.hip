// Box IoU tables for detection evaluation: one launch per evaluation batch of images (ragged).
//   box_iou_voc  — (y1, x1, y2, x2) float32, +1 on both max corners, then chainercv's bbox_iou:
//                  replaces `bbox[:, 2:] += 1; bbox_iou(pred_bbox_l, gt_bbox_l)` of chainercv's
//                  calc_detection_voc_prec_rec (the NumPy call the reference's users run on the
//                  host per image and class)
//   box_iou_coco — (x, y, w, h) float64 with crowd flags: replaces pycocotools' maskUtils.iou
//                  on boxes (maskApi.c bbIou), called per image and category by COCOeval.computeIoU
// One thread per (detection, ground truth) pair of the whole batch; the thread finds its image
// by binary search in the int64 output offsets.  No atomics, no scratch, no LDS; the per-pair
// arithmetic (bbox_iou.h) is a fixed IEEE sequence (-ffp-contract=off), so every value is
// bit-identical to the NumPy statement of the same rule.
#include "bbox_iou.h"
#include "common.h"

namespace {

// The image of flat pair index t: the last i with out_off[i] <= t (images without pairs have
// out_off[i] == out_off[i + 1] and are skipped by taking the last).  Then the pair (p, g) inside
// the image's row-major (P_i, G_i) table.  false when the offsets do not describe t (the tables
// disagree with a_off / b_off, or a row would leave the box arrays): nothing is read or written.
struct Pair { int64_t a, b; };

__device__ __forceinline__ bool locate(int64_t t, const int32_t *__restrict__ a_off,
                                       const int32_t *__restrict__ b_off,
                                       const int64_t *__restrict__ out_off, int n_img, int n_a,
                                       int n_b, Pair *pair)
{
    int lo = 0, hi = n_img;                 // first i in (lo, hi] with out_off[i] > t
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (out_off[mid] <= t) lo = mid;
        else hi = mid;
    }
    const int64_t local = t - out_off[lo];
    const int P = a_off[lo + 1] - a_off[lo], G = b_off[lo + 1] - b_off[lo];
    if (local < 0 || P <= 0 || G <= 0 || local >= (int64_t)P * G) return false;
    const int p = (int)(local / G), g = (int)(local - (int64_t)p * G);
    pair->a = (int64_t)a_off[lo] + p;
    pair->b = (int64_t)b_off[lo] + g;
    return pair->a >= 0 && pair->a < n_a && pair->b >= 0 && pair->b < n_b;
}

__global__ void __launch_bounds__(256)
box_iou_voc_kernel(const float *__restrict__ boxes_a, const float *__restrict__ boxes_b,
                   const int32_t *__restrict__ a_off, const int32_t *__restrict__ b_off,
                   const int64_t *__restrict__ out_off, int n_img, int n_a, int n_b, int64_t total,
                   float *__restrict__ iou)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    Pair pr;
    if (!locate(t, a_off, b_off, out_off, n_img, n_a, n_b, &pr)) return;
    const float *a = boxes_a + 4 * pr.a, *b = boxes_b + 4 * pr.b;
    // bbox[:, 2:] += 1 in fp32, then bbox_iou
    const float a1[4] = {a[0], a[1], a[2] + 1.f, a[3] + 1.f};
    const float b1[4] = {b[0], b[1], b[2] + 1.f, b[3] + 1.f};
    iou[t] = mrcnn::iou_pair(a1, b1);
}

__global__ void __launch_bounds__(256)
box_iou_coco_kernel(const double *__restrict__ boxes_a, const double *__restrict__ boxes_b,
                    const uint8_t *__restrict__ crowd_b, const int32_t *__restrict__ a_off,
                    const int32_t *__restrict__ b_off, const int64_t *__restrict__ out_off,
                    int n_img, int n_a, int n_b, int64_t total, double *__restrict__ iou)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    Pair pr;
    if (!locate(t, a_off, b_off, out_off, n_img, n_a, n_b, &pr)) return;
    const double *d = boxes_a + 4 * pr.a, *g = boxes_b + 4 * pr.b;
    const double d4[4] = {d[0], d[1], d[2], d[3]}, g4[4] = {g[0], g[1], g[2], g[3]};
    iou[t] = mrcnn::bb_iou_pair(d4, g4, crowd_b != nullptr && crowd_b[pr.b] != 0);
}

int check_args(const char *what, const void *boxes_a, const void *boxes_b, const void *a_off,
               const void *b_off, const void *out_off, int n_img, int n_a, int n_b, int64_t total,
               const void *iou)
{
    MRCNN_REQUIRE(n_img >= 0 && n_a >= 0 && n_b >= 0 && total >= 0,
                  "%s: bad sizes (n_img=%d, n_a=%d, n_b=%d, total=%lld)", what, n_img, n_a, n_b,
                  (long long)total);
    MRCNN_REQUIRE(total <= (int64_t)n_a * n_b, "%s: total=%lld pairs from %d x %d boxes", what,
                  (long long)total, n_a, n_b);
    if (total == 0) return 0;
    MRCNN_REQUIRE(n_img > 0, "%s: %lld pairs in no image", what, (long long)total);
    MRCNN_REQUIRE(boxes_a && boxes_b && a_off && b_off && out_off && iou, "%s: null pointer", what);
    MRCNN_REQUIRE((total + 255) / 256 < ((int64_t)1 << 31), "%s: grid too large", what);
    return 0;
}

}  // namespace

extern "C" int mrcnn_box_iou_voc(const float *boxes_a, const float *boxes_b, const int32_t *a_off,
                                 const int32_t *b_off, const int64_t *out_off, int n_img, int n_a,
                                 int n_b, int64_t total, float *iou, void *stream)
{
    if (int rc = check_args("box_iou_voc", boxes_a, boxes_b, a_off, b_off, out_off, n_img, n_a,
                            n_b, total, iou))
        return rc;
    if (total == 0) return 0;
    hipLaunchKernelGGL(box_iou_voc_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       mrcnn::as_stream(stream), boxes_a, boxes_b, a_off, b_off, out_off, n_img,
                       n_a, n_b, total, iou);
    return mrcnn::check_launch("box_iou_voc");
}

extern "C" int mrcnn_box_iou_coco(const double *boxes_a, const double *boxes_b,
                                  const uint8_t *crowd_b, const int32_t *a_off,
                                  const int32_t *b_off, const int64_t *out_off, int n_img, int n_a,
                                  int n_b, int64_t total, double *iou, void *stream)
{
    if (int rc = check_args("box_iou_coco", boxes_a, boxes_b, a_off, b_off, out_off, n_img, n_a,
                            n_b, total, iou))
        return rc;
    if (total == 0) return 0;
    hipLaunchKernelGGL(box_iou_coco_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       mrcnn::as_stream(stream), boxes_a, boxes_b, crowd_b, a_off, b_off, out_off,
                       n_img, n_a, n_b, total, iou);
    return mrcnn::check_launch("box_iou_coco");
}
