/*
 * mrcnn_hip.h — C ABI of libmrcnn_hip.so, the MI355X (gfx950) implementation of
 * the Mask R-CNN ResNet-C4 hot path of wkentaro/chainer-mask-rcnn.
 *
 * The reference has no FFI of its own (it is 100 % Python; its device code is
 * CuPy kernel strings and third-party cuDNN/chainercv calls), so each entry
 * point below cites the reference interface it replaces (file:line under
 * /root/reference) and is what a ctypes binding on the reference side would
 * bind (INTEGRATION.md shows that binding).
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error (never throws,
 *     never aborts); mrcnn_last_error() returns a message for the calling thread.
 *   - all tensor pointers are DEVICE pointers owned by the caller (allocated by
 *     PyTorch-ROCm); the library neither frees nor retains them.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all work
 *     is enqueued asynchronously on it, no implicit device synchronisation.
 *   - activations are NHWC fp32 ("channels-last": the physical layout of a
 *     torch channels_last tensor whose logical shape is the reference's NCHW);
 *     conv filters are KRSC = (out, kh, kw, in) fp32 — the channels_last image
 *     of chainer's (out, in, kh, kw).
 *   - boxes are (y_min, x_min, y_max, x_max) fp32 as everywhere in the reference
 *     model (models/mask_rcnn.py:69); RoI rows for pooling are
 *     (batch_index, x1, y1, x2, y2) as functions/roi_align_2d.py:540-541.
 */
#ifndef MRCNN_HIP_H_
#define MRCNN_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- library ----------------------------------------------------------- */
const char *mrcnn_last_error(void);
int mrcnn_abi_version(void);
/* Number of compute units / device name of the current device (diagnostics). */
int mrcnn_device_info(int *n_cu, char *name, int name_len);

/* Kernel timer: HIP events recorded on the launch stream around every hot kernel while
 * enabled.  bench.py uses it to report roofline numbers (average launch duration and
 * algorithmic flops / bytes per kernel kind; kinds follow the kernel symbols rocprofv3
 * reports).  mrcnn_profile_enable(mode) clears the records; mode 0 = off, 1 = every kind,
 * 2 = only the forward-form 128x128 conv GEMM, the dominant kernel symbol (~48 instead of
 * ~500 event pairs per train step, so the timed region is barely perturbed; the other kinds
 * still count launches / flops / bytes), 3 = count launches / flops / bytes of every kind and
 * time nothing (no events on the stream at all); any other value is an error.
 * mrcnn_profile_summary sums the records (synchronise the stream first). */
int mrcnn_profile_enable(int on);
int mrcnn_profile_num_kinds(void);
const char *mrcnn_profile_kind_name(int kind);
int mrcnn_profile_summary(int kind, double *total_ms, double *total_flops,
                          double *total_bytes, int64_t *launches);

/* ---- ROIAlign ---------------------------------------------------------- */
/* Replaces ROIAlign2D.forward_gpu (functions/roi_align_2d.py:162-290).
 * x (N,H,W,C) NHWC, rois (R,5) = (batch, x1, y1, x2, y2), y (R,PH,PW,C). */
int mrcnn_roi_align_fwd(const float *x, const float *rois, float *y,
                        int N, int H, int W, int C, int R, int PH, int PW,
                        float spatial_scale, int sampling_ratio, void *stream);
/* Replaces ROIAlign2D.backward_gpu (functions/roi_align_2d.py:391-524).
 * gy (R,PH,PW,C) -> gx (N,H,W,C); gx is zero-filled by the call. */
int mrcnn_roi_align_bwd(const float *gy, const float *rois, float *gx,
                        int N, int H, int W, int C, int R, int PH, int PW,
                        float spatial_scale, int sampling_ratio, void *stream);

/* Strided-bin variants: only the bins (oh*bin_stride, ow*bin_stride) of the PH x PW grid are
 * produced / consumed, y and gy are (R, ceil(PH/bs), ceil(PW/bs), C).  res5's first block
 * reads the 14x14 RoI features through 1x1 stride-2 convolutions only
 * (models/mask_rcnn_resnet.py:131-133 with roi_size // 7 == 2), i.e. it uses just the even
 * bins; bin_stride = 2 skips the three quarters of the ROIAlign output nobody reads
 * (identical values for the bins that are read).
 *
 * order (may be NULL): a permutation of 0..R-1 on the device, the sequence in which the RoIs are
 * PROCESSED (results are written to their own rows and do not depend on it).  An XCD works on a
 * contiguous run of that sequence, so an order that keeps neighbouring RoIs together
 * (functions.roi_align_2d.spatial_order: image, 6-row band, x centre) lets it read its region of
 * the feature map from HBM once: 65 -> 52 us at the C2 shape. */
int mrcnn_roi_align_fwd_ex(const float *x, const float *rois, float *y,
                           int N, int H, int W, int C, int R, int PH, int PW, int bin_stride,
                           float spatial_scale, int sampling_ratio, const int *order,
                           void *stream);
/* ROIAlign with a fused per-channel epilogue: y = relu?(roi_align(x) * scale[c] + shift[c]).
 * Used where the head pools the OUTPUT of res5.a's 1x1 convolutions instead of their input
 * (models/mask_rcnn_resnet.py:131-133, 168-176: ROIAlign, then conv1 / the shortcut conv4, each 1x1,
 * followed by AffineChannel2D (+ ReLU)).  ROIAlign is linear over positions per channel and has no
 * constant term (skipped samples contribute zero, functions/roi_align_2d.py:228-236), a 1x1
 * convolution without bias is linear over channels per position, so
 *     affine(conv1x1(roi_align(x))) == affine(roi_align(conv1x1(x)))
 * in exact arithmetic: the convolution runs on the N*H*W map pixels instead of the R*7*7 pooled
 * ones (8 568 instead of 50 176 rows at the C2 shape) and this call applies the AffineChannel2D
 * (scale, shift: C floats each, both required) and the ReLU to the pooled values. */
int mrcnn_roi_align_fwd_affine(const float *x, const float *rois, float *y,
                               int N, int H, int W, int C, int R, int PH, int PW, int bin_stride,
                               float spatial_scale, int sampling_ratio, const int *order,
                               const float *scale, const float *shift, int relu, void *stream);
/* Backward, two forms.  ws = NULL (and mrcnn_roi_align_bwd): gather form with one atomic add
 * per (RoI patch pixel, channel) into a zero-filled gx — the order of the fp32 additions, like
 * the reference's atomicAdd kernel (:508-515), varies from run to run.  ws = a 16-byte aligned
 * workspace of mrcnn_roi_align_bwd_workspace_bytes(N, H, W, R, PH, PW, bin_stride): pixel-owner
 * form — per RoI the patch extent and the separable bilinear weights of every feature row and
 * column are tabulated once, then every gx pixel is summed in registers over the RoIs that cover
 * it (in RoI order, bins in row-major order) and stored once: no atomics, no zero-fill,
 * bit-reproducible, ~10x faster at the C2 shape (H, W <= 65535; otherwise the first form runs).
 * A bin is applied to the 8-pixel row tile it touches with weight 0 on the pixels it does not
 * touch: identical sums for finite gy; a non-finite gy element reaches those neighbours too. */
int64_t mrcnn_roi_align_bwd_workspace_bytes(int N, int H, int W, int R, int PH, int PW,
                                            int bin_stride);
int mrcnn_roi_align_bwd_ex(const float *gy, const float *rois, float *gx,
                           int N, int H, int W, int C, int R, int PH, int PW, int bin_stride,
                           float spatial_scale, int sampling_ratio, void *ws, void *stream);
/* Same call with the workspace's extent: fails (returns non-zero, mrcnn_last_error) when ws is
 * non-NULL and ws_bytes < mrcnn_roi_align_bwd_workspace_bytes(N, H, W, R, PH, PW, bin_stride) — a
 * caller that sized ws by an older formula gets an error instead of a table write past its buffer.
 * mrcnn_roi_align_bwd_ex is this call with the extent taken on trust. */
int mrcnn_roi_align_bwd_ws(const float *gy, const float *rois, float *gx,
                           int N, int H, int W, int C, int R, int PH, int PW, int bin_stride,
                           float spatial_scale, int sampling_ratio, void *ws, int64_t ws_bytes,
                           void *stream);
/* Which kernel mrcnn_roi_align_bwd_ws launches for this problem: 0 = pixel-owner, 1 = gather (one
 * atomic add per RoI patch pixel and channel), 2 = scatter (the reference's four atomic adds per
 * sample; taken when the gather form's tables of 4 (PH + (W + 4) PW) + 8 (W + 4) bytes exceed
 * 48 KB of LDS or R > 65535).  has_ws: a workspace is passed; ws_aligned: it is 16-byte aligned.
 * The function the launch itself consults; host only, needs no device.  -1 for a bad shape. */
int mrcnn_roi_align_bwd_form(int N, int H, int W, int R, int PH, int PW, int bin_stride,
                             int has_ws, int ws_aligned);

/* ---- RoI max pooling and crop-and-resize --------------------------------------------------
 * The two other RoI feature extractors the reference's head accepts as pooling_func
 * (examples/train_common.py:138-147: --pooling-func pooling / resize).  Same conventions as the
 * ROIAlign calls above: x (N,H,W,C), rois (R,5) = (batch, x1, y1, x2, y2), y (R,OH,OW,C) with
 * OH = ceil(PH / bin_stride), OW = ceil(PW / bin_stride) — only the bins (oh*bin_stride,
 * ow*bin_stride) of the PH x PW grid, whose geometry is that of the full grid; order (may be
 * NULL) is a processing permutation of the RoIs that does not change the result.  Validation
 * errors (outh / outw / C < 1, bin_stride < 1, a NULL pointer with R > 0) return non-zero with
 * mrcnn_last_error(); R == 0 is a successful no-op (the backwards zero-fill gx).  Backwards are
 * pixel-owner only: ws (16-byte aligned, at least the size query's bytes) is required, no
 * atomics, every gx element written once, bit-reproducible.  RoIs whose batch index is not in
 * [0, N) produce zeros (argmax -1) and receive no gradient. */
/* Replaces chainer's F.roi_pooling_2d forward GPU kernel (Caffe's Fast R-CNN ROIPooling), which
 * the reference selects as cmr.functions.roi_pooling_2d (examples/train_common.py:141-142).
 * Per bin, all in fp32: start = roundf(x1 * s) (half away from zero), roi size
 * max(end - start + 1, 1), window [floor(p * bin), ceil((p + 1) * bin)) + start clamped to
 * [0, size]; the first maximum in (h, w) ascending order, initial value -1e37 (a NaN never wins);
 * an empty window gives 0 and argmax -1.  argmax (R,OH,OW,C) int32 holds h * W + w. */
int mrcnn_roi_pool_fwd(const float *x, const float *rois, float *y, int *argmax,
                       int N, int H, int W, int C, int R, int PH, int PW, int bin_stride,
                       float spatial_scale, const int *order, void *stream);
/* Replaces chainer's F.roi_pooling_2d backward GPU kernel: gx[n,h,w,c] = the sum of gy[r,oh,ow,c]
 * over the bins whose argmax for channel c is h * W + w, in ascending (r, oh, ow) order — the
 * order of chainer's kernel.  gy / argmax as written by mrcnn_roi_pool_fwd. */
int64_t mrcnn_roi_pool_bwd_workspace_bytes(int N, int H, int W, int R, int PH, int PW,
                                           int bin_stride);
int mrcnn_roi_pool_bwd_ws(const float *gy, const int *argmax, const float *rois, float *gx,
                          int N, int H, int W, int C, int R, int PH, int PW, int bin_stride,
                          float spatial_scale, void *ws, int64_t ws_bytes, void *stream);
/* Replaces chainer_mask_rcnn.functions.crop_and_resize (functions/crop_and_resize.py:7-41): an
 * integer crop followed by F.resize_images (bilinear, aligned corners).  Crop start
 * rint(double(x1) * spatial_scale) (half to even, as Python's round), clamped into [0, W-1]
 * (extension: the reference wraps a negative start and fails on a start past the map); crop end
 * max(rint(double(x2) * spatial_scale), start + 1) truncated at W; the same along y.  Sample p of
 * linspace(0, crop - 1, PH) in float64 (0 when PH == 1), taps clip(floor(v), 0, crop - 2) and + 1
 * (one row when the crop is one row), per-axis weights in float64 rounded once to fp32, value
 * ((w00 v00 + w01 v01) + w10 v10) + w11 v11 in fp32 with w_ij = wy_i * wx_j.
 * out_rows (may be NULL = identity): the output row of each RoI — functions.crop_and_resize passes
 * the stable sort by batch index, the reference's output order (its per-image concat). */
int mrcnn_crop_resize_fwd(const float *x, const float *rois, const int *out_rows, float *y,
                          int N, int H, int W, int C, int R, int PH, int PW, int bin_stride,
                          double spatial_scale, const int *order, void *stream);
/* Adjoint of the four bilinear taps of mrcnn_crop_resize_fwd (the backward chainer derives for
 * F.resize_images), summed per gx pixel in (r, oh, ow) order. */
int64_t mrcnn_crop_resize_bwd_workspace_bytes(int N, int H, int W, int R, int PH, int PW,
                                              int bin_stride);
int mrcnn_crop_resize_bwd_ws(const float *gy, const float *rois, const int *out_rows, float *gx,
                             int N, int H, int W, int C, int R, int PH, int PW, int bin_stride,
                             double spatial_scale, void *ws, int64_t ws_bytes, void *stream);

/* ---- row-sparse backward of a 3x3 / stride 1 / pad 1 convolution --------------------------
 * The reference back-propagates the RPN losses through conv1 of
 * models/region_proposal_network.py:75-80 densely, although the losses ignore every anchor but
 * the <= 256 sampled ones per image (models/mask_rcnn_train_chain.py:150-166): the gradient of
 * conv1's output is exactly zero outside their map positions.  With the list of those positions
 * (`rows`, sorted indices into N*H*W, and `lookup`, position -> row or -1; both built where the
 * anchor targets are) the backward is: gather the rows' 3x3 input patches and gradient rows,
 * run weight and data gradient as the 1x1 problem (N = n_rows, C = 9*C_in) through
 * mrcnn_conv2d_wgrad / mrcnn_conv2d_dgrad_wt, and sum the patch gradients back per map pixel in
 * a fixed tap order (every gx element written once, no atomics).  x (N,H,W,C), g (N,H,W,K) NHWC,
 * patches (n_rows, 3, 3, C), g_rows (n_rows, K), g_patches (n_rows, 3, 3, C), gx (N,H,W,C). */
int mrcnn_sparse3x3_gather(const float *x, const float *g, const int32_t *rows, int n_rows,
                           int N, int H, int W, int C, int K, float *patches, float *g_rows,
                           void *stream);
int mrcnn_sparse3x3_scatter(const float *g_patches, const int32_t *lookup, int N, int H, int W,
                            int C, float *gx, void *stream);

/* ---- AffineChannel2D ---------------------------------------------------- */
/* Replaces AffineChannel2DFunction.forward / backward
 * (functions/affine_channel_2d.py:10-22, :38-56).  x,y (M,C) NHWC rows,
 * W,b (C).  Inside the model the affine is fused into the conv epilogue
 * (mrcnn_conv2d_fwd); these stand-alone entry points serve the public
 * `affine_channel_2d` function. gW/gb may be NULL (skipped). */
int mrcnn_affine_fwd(const float *x, const float *W, const float *b, float *y,
                     int64_t M, int C, void *stream);
int64_t mrcnn_colsum_workspace_bytes(int C);
int mrcnn_affine_bwd(const float *x, const float *W, const float *gy,
                     float *gx, float *gW, float *gb, int64_t M, int C,
                     void *ws /* mrcnn_colsum_workspace_bytes(C) */, void *stream);

/* ---- Proposal path (integer results) ------------------------------------ */
/* loc2bbox + clip + min-size validity: chainercv ProposalCreator steps 1-3
 * (call site models/region_proposal_network.py:135-138).
 * anchor (n,4), loc (n,4) -> roi (n,4); valid[i] = h>=min_size && w>=min_size. */
int mrcnn_decode_clip(const float *anchor, const float *loc, float *roi,
                      uint8_t *valid, int n, float img_h, float img_w,
                      float min_size, void *stream);
/* Stable descending top-k over valid entries: `argsort(score)[::-1][:k]` of
 * ProposalCreator (tie rule: lower index first).  order[j] = index of the j-th
 * best valid score (j < *n_out), n_out (device int32) = min(k, #valid).
 * valid may be NULL (all valid). */
int64_t mrcnn_topk_workspace_bytes(int n);
int mrcnn_topk_desc(const float *score, const uint8_t *valid, int n, int k,
                    int32_t *order, int32_t *n_out, void *ws, void *stream);
/* `groups` problems of the same size in one set of launches (a batch's images): score and
 * valid are (groups, n), order (groups, k), n_out (groups); ws holds
 * groups x round_up(mrcnn_topk_workspace_bytes(n), 64) bytes. */
int mrcnn_topk_desc_batched(const float *score, const uint8_t *valid, int groups, int n, int k,
                            int32_t *order, int32_t *n_out, void *ws, void *stream);
/* dst[j,:] = src[idx[j],:] for j < *n_dev (n_dev device int32, rows of `cols`
 * fp32); rows j >= *n_dev up to n_max are zero-filled. */
int mrcnn_gather_rows(const float *src, const int32_t *idx, const int32_t *n_dev,
                      int n_max, int cols, float *dst, void *stream);
/* chainercv non_maximum_suppression on score-sorted boxes (call
 * sites models/mask_rcnn.py:193-194 and ProposalCreator).  bbox (n_max,4)
 * sorted by descending score, *n_dev boxes valid.  Writes keep[0..*n_keep) =
 * indices into bbox (ascending = descending score), at most `limit` (<=0: no
 * limit).  mask_ws: caller-owned workspace of mrcnn_nms_workspace_bytes(n_max, 1). */
int64_t mrcnn_nms_workspace_bytes(int n_max, int groups);
int mrcnn_nms_sorted(const float *bbox, const int32_t *n_dev, int n_max,
                     float thresh, int limit, int32_t *keep, int32_t *n_keep,
                     void *mask_ws, void *stream);
/* Batched form for per-class NMS (MaskRCNN._suppress, models/mask_rcnn.py:178-202):
 * `groups` independent problems, group g has n_dev[g] boxes at bbox + g*n_max*4,
 * writes keep + g*n_max and n_keep[g]; workspace mrcnn_nms_workspace_bytes(n_max, groups). */
int mrcnn_nms_sorted_batched(const float *bbox, const int32_t *n_dev, int groups,
                             int n_max, float thresh, int limit, int32_t *keep,
                             int32_t *n_keep, void *mask_ws, void *stream);

/* ---- Convolution family (fp32 implicit GEMM on MFMA) ---------------------- */
/* Epilogue flags */
#define MRCNN_EPI_BIAS     1   /* y += bias[c]                                  */
#define MRCNN_EPI_AFFINE   2   /* y = y*scale[c] + shift[c]  (AffineChannel2D)  */
#define MRCNN_EPI_RESIDUAL 4   /* y += residual[m,c]                            */
#define MRCNN_EPI_RELU     8   /* y = max(y,0)                                  */
#define MRCNN_EPI_ACCUM    16  /* y += previous contents of y (dgrad fan-in)    */
#define MRCNN_EPI_EXACT_SIGNS 32 /* mrcnn_conv3x3_wino_fwd only, see there        */

typedef struct {
    int N, H, W, C;        /* input  (N,H,W,C)  NHWC                         */
    int K, R, S;           /* filter (K,R,S,C)  KRSC                         */
    int stride, pad;
    int P, Q;              /* output (N,P,Q,K)  NHWC                         */
} mrcnn_conv_desc;

/* Replaces chainer L.Convolution2D forward (cuDNN) + following AffineChannel2D,
 * residual add and ReLU of chainer's BottleneckA/B (call sites
 * models/region_proposal_network.py:75-80,124-131, models/mask_rcnn_resnet.py:131-143,
 * chainer ResNet50Layers via models/resnet_extractor.py:93).
 * y = epi( conv(x, w) ).  scale/shift/bias/residual may be NULL when unused.
 * split_ws (forward and backward-data entry points): NULL or a scratch buffer of
 * mrcnn_conv2d_split_workspace_bytes() bytes.  With it, a small-M problem whose 64x64 tiles
 * do not divide evenly over the 256 CUs (e.g. 536 tiles: the busiest CU would run 3, the
 * average 2.09) runs its leftover rows split along K into many short workgroups whose partial
 * sums are combined, in a fixed order, by a small epilogue kernel. */
int64_t mrcnn_conv2d_split_workspace_bytes(void);
/* Run-time tuning switches; an unknown name is an error.
 * Developer switches for A/B measurements (results are identical either way):
 *   "position_major_rows" (default 1): forward-form convolutions over many small maps (RoI
 *   features, 3x3 / pad 1 on 7x7) order their GEMM rows position-major so that the K slices of
 *   filter taps that fall into the zero padding for every row of a tile are skipped.
 *   "fused_tail" (default 512 = target number of pieces, 0 = off): the rows beyond the last full
 *   round of resident workgroups run as K-split pieces INSIDE the main launch (dispatched last,
 *   they fill the CUs while the final round drains) instead of a separate remainder launch;
 *   summation order of those rows differs between the two settings (both deterministic).
 * Arithmetic selection (NOT results-identical: same accuracy class, different rounding):
 *   "split_bf16" (default 3 since round 4; 0 = fp32 MFMA everywhere; bit 0: the 128x128
 *   forward-form and weight-gradient kernels, bit 1: the 64x64 forward-form kernel): operands are
 *   staged as three bf16 planes whose sum is the fp32 element exactly, six bf16 MFMAs per K step,
 *   fp32 accumulation.  Error against float64 is at (measured: below) the fp32-MFMA kernels' level
 *   (tests/test_gpu_split_bf16.py, tests/test_split_arithmetic_cpu.py).
 *   "split_planes" (default 3; legal 1, 2, 3 — any other value is an error and keeps the setting):
 *   how many of those planes the launches that "split_bf16" puts on the split kernels stage and
 *   multiply.  3: all six products, fp32-accurate.  2: hi and mid, the products mid*hi, hi*mid,
 *   hi*hi — operands of 16 significand bits, error about 3 x 2^-16 of sum |a||b|, half the
 *   matrix-pipe work.  1: hi only, the product hi*hi — bf16 operands, error about 2^-7 of
 *   sum |a||b|, one sixth.  fp32 accumulation, fp32 in / out and unrounded epilogue operands in
 *   all three.  No effect while "split_bf16" is 0, none on the kernels that run fp32 MFMA anyway,
 *   none on the launch plan (same route, tiles and K cuts for 1, 2 and 3), and none on the
 *   launches of the Winograd entry points (mrcnn_conv3x3_wino_*), which always run three planes.
 *   (tests/test_gpu_arithmetic_ladder.py, tests/test_arithmetic_ladder_cpu.py)
 *   "big_min_tiles" (default 384): fewest 128x128 tiles for which the 128x128 kernels are used
 *   (1 forces them; lets small test problems exercise the kernels of the full-size step).
 *   "big_split_k" (default -1 since round 6): with -1, a small-M, K-deep forward-form problem whose
 *   128x128 tiles cut along K fill one round of the resident workgroups (the batch-2 res4 3x3 layers)
 *   runs that way, slabs summed in order by the epilogue kernel, instead of as 64x64 tiles; 0 = off;
 *   k > 0 = aim at k workgroups (probe); "big_split_min_slices" (default 16): fewest K slices per slab.
 *   "tiny_split" (default 1): launches of <= 128 tiles and >= 32 K slices are cut along K.
 *   "small_m_split" (default 0 = off; k > 0): 64x64-tile problems of fewer than 256 k tiles and
 *   >= 16 K slices are cut along K to about 256 k workgroups.
 *   Summation order differs between these settings (each deterministic).
 *   "wino_ambiguity_ppb" (default 4000, parts per 1e9): rounding bound below which a Winograd
 *   forward output's sign counts as ambiguous and is recomputed directly.
 * Kernel selection (round 6):
 *   "w8" (default 1): large pointwise forward-form launches of the split arithmetic (K >= "w8_min_k",
 *   default 256, and at least 768 tiles) on 256x128 tiles / 512-thread workgroups.  Bit-identical
 *   either way unless the launch's last round runs as K-split tail pieces: W8 cuts that tail along K
 *   differently from the 128x128 kernels, so those rows are summed in another order.
 *   "pw" (default 3): bit 0 = pointwise (1x1 / stride 1) forward-form launches, bit 1 = 3x3 / stride 1 /
 *   pad 1 ones run instantiations with that geometry as compile-time constants; bit-identical.
 *   "roi_fwd_lanes" / "roi_bwd_lanes" (default 0 = 256): cap of the lanes per ROIAlign workgroup;
 *   0 or a multiple of 64 in [64, 256] (whole waves), any other value is an error and keeps the
 *   previous setting (the pixel-owner backward counts its RoI lists per wave). */
int mrcnn_set_tuning(const char *name, int value);
int mrcnn_conv2d_fwd(const mrcnn_conv_desc *d, const float *x, const float *w,
                     const float *bias, const float *scale, const float *shift,
                     const float *residual, float *y, int epi_flags, void *split_ws,
                     void *stream);
/* Gradient w.r.t. the input.  gy (N,P,Q,K) -> gx (N,H,W,C).  With
 * MRCNN_EPI_ACCUM gx += result (fan-in of several consumers). */
int mrcnn_conv2d_dgrad(const mrcnn_conv_desc *d, const float *gy, const float *w,
                       float *gx, int epi_flags, void *stream);
/* Gradient w.r.t. the filter, gw (K,R,S,C) (bias gradient: mrcnn_colsum of gy).
 * ws: split-K workspace of mrcnn_conv2d_wgrad_workspace_bytes(d) (NULL: no split). */
int64_t mrcnn_conv2d_wgrad_workspace_bytes(const mrcnn_conv_desc *d);
int mrcnn_conv2d_wgrad(const mrcnn_conv_desc *d, const float *x, const float *gy,
                       float *gw, void *ws, void *stream);
/* Extended backward entry points.  The backward of a conv's fused epilogue (AffineChannel2D
 * scale s[k], then ReLU with output y) is applied producer side, in the dgrad epilogue that
 * WRITES the gradient:
 *      gx = (acc * out_scale[c] + res_g * (res_y > 0)) * (out_mask_y > 0)
 *      out_mask_y / out_scale: ReLU output / affine scale of the conv that produced this
 *      conv's INPUT ((N,H,W,C) / (C); either may be NULL).  The next dgrad / wgrad down the
 *      chain then need no mask and run the three-workgroups-per-CU kernels.
 *      res_g (+ optional res_y): identity-shortcut gradient of a bottleneck, (N,H,W,C);
 *      stride 1 only.  With MRCNN_EPI_ACCUM the previous gx is added before the mask.
 *  A per-output-channel scale that cannot go to the producer (the block-top gradient feeds
 *  conv3, conv4 and the shortcut with different scales) is folded into the filter for dgrad
 *  (row_scale of mrcnn_filter_flip_transpose) and applied to the rows of gw in the wgrad
 *  epilogue (out_row_scale): gw[k] = s[k] * sum_m gy[m,k] x[m].
 * Used by functions/conv.py:_StageFn (a whole ResNet stage as one autograd node); chainer runs
 * each of these as separate elementwise kernels. */
int mrcnn_conv2d_dgrad_ex(const mrcnn_conv_desc *d, const float *gy, const float *w,
                          float *gx, int epi_flags, const float *res_g, const float *res_y,
                          const float *out_mask_y, const float *out_scale, void *split_ws,
                          void *stream);
int mrcnn_conv2d_wgrad_ex(const mrcnn_conv_desc *d, const float *x, const float *gy,
                          float *gw, void *ws, const float *out_row_scale, void *stream);
/* Winograd F(4x4,3x3) path (csrc/conv_winograd.h) for 3x3 / stride 1 / pad 1 convolutions —
 * the algorithm cuDNN selects for the same layers in the reference (chainer autotune off:
 * cudnnGetConvolutionForwardAlgorithm; call sites as mrcnn_conv2d_fwd).  A third of the MFMA
 * work of the direct form on the RoI head's 7x7 maps.  Interpolation points 0, +-1, 1/2, -2:
 * fp32 error max 3.4e-6 / rms 3.7e-7 of the tensor scale against an fp64 direct convolution
 * (direct fp32: 3.5e-7 / 5.7e-8), inside the 1e-4 parity tolerance.
 *   fwd:   y = epi(conv(x, w)), epi_flags: MRCNN_EPI_AFFINE (scale, shift) or MRCNN_EPI_BIAS
 *          (the bias in `shift`, scale NULL), and MRCNN_EPI_RELU.  With MRCNN_EPI_EXACT_SIGNS
 *          every output whose pre-activation lies within the propagated Winograd rounding
 *          bound of zero (a few in 10^5) is recomputed as a direct fp32 dot product, so the
 *          ReLU decisions — what a recorded graph's backward masks depend on — have the
 *          accuracy of the direct kernel (w must be given).  u: NULL (the filter is
 *          transformed per call) or the output of mrcnn_conv3x3_wino_filter for this w
 *          (mrcnn_conv3x3_wino_u_bytes(d) bytes; inference keeps it while w is unchanged, w may
 *          then be NULL).  v: NULL or a buffer of mrcnn_conv3x3_wino_v_bytes(d) that receives the
 *          transformed input (36 x tiles x C), which mrcnn_conv3x3_wino_wgrad consumes.
 *   dgrad: gx = (dgrad(gy * w_row_scale[k]) * out_scale[c]) masked by (out_mask_y > 0)
 *          (any of the three may be NULL; same meaning as in mrcnn_conv2d_dgrad_wt).
 *   wgrad: gw (K,3,3,C) from gy and exactly one of x (the raw input, transformed into the
 *          scratch) and v (the forward's kept transform); out_row_scale[k] (or NULL)
 *          multiplies gw's rows.
 * ws: scratch of mrcnn_conv3x3_wino_workspace_bytes(d), private to the stream. */
int64_t mrcnn_conv3x3_wino_v_bytes(const mrcnn_conv_desc *d);
int64_t mrcnn_conv3x3_wino_workspace_bytes(const mrcnn_conv_desc *d);
int64_t mrcnn_conv3x3_wino_u_bytes(const mrcnn_conv_desc *d);
int mrcnn_conv3x3_wino_filter(const mrcnn_conv_desc *d, const float *w, float *u, void *stream);
int mrcnn_conv3x3_wino_fwd(const mrcnn_conv_desc *d, const float *x, const float *w,
                           const float *u, const float *scale, const float *shift, float *y,
                           int epi_flags, float *v, void *ws, void *stream);
int mrcnn_conv3x3_wino_fixup_count(const mrcnn_conv_desc *d, const void *ws, void *stream,
                                   int *count);   /* diagnostics (synchronises): outputs the last
                                                     EXACT_SIGNS forward on ws found within the
                                                     rounding bound of zero.  The list behind the
                                                     forward's buffers holds cap = min(2^20,
                                                     (8 * 36 * K * C - 4) / 2) of them: min(count,
                                                     cap) outputs are recomputed, the rest keep
                                                     their Winograd value */
int mrcnn_conv3x3_wino_dgrad(const mrcnn_conv_desc *d, const float *gy, const float *w,
                             const float *w_row_scale, float *gx, const float *out_scale,
                             const float *out_mask_y, void *ws, void *stream);
int mrcnn_conv3x3_wino_wgrad(const mrcnn_conv_desc *d, const float *x, const float *v,
                             const float *gy, float *gw, const float *out_row_scale, void *ws,
                             void *stream);
/* Stride-1 dgrad expressed as a forward-form convolution of gy with the flipped, transposed
 * filter wT[c][R-1-r][S-1-s][k] = w[k][r][s][c] * row_scale[k] (both GEMM operands
 * K-contiguous).  mrcnn_filter_flip_transpose builds wT (C,R,S,K) from w (K,R,S,C)
 * (row_scale (K) or NULL); it moves R*S*K*C*8 bytes, negligible next to the dgrad.
 * Same extra arguments as _ex.  Round 6: mrcnn_conv2d_dgrad_wt also takes stride > 1 for 1x1 / pad 0
 * filters (the strided projections of res3.a / res4.a): gy is gathered densely, the rows are
 * scattered to the strided pixels of gx, which the call zero-fills unless MRCNN_EPI_ACCUM is set
 * (residual gradient / output mask arguments must be NULL there). */
int mrcnn_filter_flip_transpose(const float *w, float *wT, int K, int R, int S, int C,
                                const float *row_scale, void *stream);
/* The same for n filters in one launch (host arrays of n device pointers / sizes; row_scale
 * or its entries may be NULL): a ResNet stage's backward needs ~14 of them. */
int mrcnn_filter_flip_transpose_batched(int n, const void *const *w, void *const *wT,
                                        const int *K, const int *R, const int *S, const int *C,
                                        const void *const *row_scale, void *stream);
int mrcnn_conv2d_dgrad_wt(const mrcnn_conv_desc *d, const float *gy, const float *wT,
                          float *gx, int epi_flags, const float *res_g, const float *res_y,
                          const float *out_mask_y, const float *out_scale, void *split_ws,
                          void *stream);
/* Stem: conv1 7x7/2 pad 3 with bias of chainer ResNet50Layers (SURVEY.md A.1;
 * models/resnet_extractor.py:65-67) fused with bn1-as-affine and ReLU.  x4 is
 * the image padded to 4 channels (N,H,W,4); w784 is the filter laid out
 * (K,7,8,4) with zeros at s=7 and c=3.  Forward only (frozen, :86-87). */
int mrcnn_conv_stem_fwd(const float *x4, const float *w784, const float *bias,
                        const float *scale, const float *shift, float *y, int N,
                        int H, int W, int K, int epi_flags, void *stream);

/* Replaces chainer L.Deconvolution2D(2048,256,2,stride=2) (models/mask_rcnn_resnet.py:138-139,193).
 * x (N,H,W,C) -> y (N,2H,2W,K); filter w (C,2,2,K) = channels_last image of
 * chainer's (in,out,kh,kw).  Epilogue: bias + optional ReLU. */
int mrcnn_deconv2x2s2_fwd(const float *x, const float *w, const float *bias,
                          float *y, int N, int H, int W, int C, int K,
                          int epi_flags, void *stream);
/* The same forward on the TRANSPOSED filter wT (4K, C) = mrcnn_filter_flip_transpose(w, wT, C, 1, 1, 4K)
 * — a 1x1 convolution (both operands K-contiguous: the split-operand arithmetic) whose output columns
 * (a, b, o) the epilogue scatters to y[n, 2y + a, 2x + b, o].  Same values up to fp32 rounding. */
int mrcnn_deconv2x2s2_fwd_wt(const float *x, const float *wT, const float *bias,
                             float *y, int N, int H, int W, int C, int K, int epi_flags,
                             void *stream);
int mrcnn_deconv2x2s2_dgrad(const float *gy, const float *w, float *gx,
                            int N, int H, int W, int C, int K, void *stream);
int64_t mrcnn_deconv2x2s2_wgrad_workspace_bytes(int N, int H, int W, int C, int K);
int mrcnn_deconv2x2s2_wgrad(const float *x, const float *gy, float *gw,
                            int N, int H, int W, int C, int K, void *ws,
                            void *stream);
/* How the GEMM entry point mrcnn_<entry> would cut the call of descriptor d into kernel launches under
 * the knobs currently set, as one line of text in `out`; no device is touched and no pointer needed
 * (has_ws: the call would pass a split-K workspace).  entry: "conv2d_fwd", "conv_stem_fwd" (N, H, W, K
 * of d), "conv2d_dgrad", "conv2d_dgrad_ex", "conv2d_dgrad_wt" (either with the suffix "+res_g": the
 * call has a residual gradient), "conv2d_wgrad", "conv2d_wgrad_ex", and the "deconv2x2s2_*" entries, for
 * which d carries the input map (N, H, W, C) and K; and the Winograd route's "conv3x3_wino_fwd",
 * "conv3x3_wino_dgrad" and "conv3x3_wino_wgrad" (has_ws is not read: they always have their scratch),
 * whose GEMM rows are the 4x4 tiles of the maps (forward, data gradient) or K (weight gradient).  The
 * line names the branch of the policy (csrc/conv_gemm_plan.h) and, per GEMM launch, the kernel
 * instantiation, the row range, the grid (the Winograd entries add batch=36: the frequencies in
 * grid z), the K-slab depth and the fused-tail fields, then the slab sum if there is one.  The descriptor
 * checks are those of the entry point; an unknown entry, a rejected descriptor or a short buffer
 * returns non-zero. */
int mrcnn_conv_gemm_plan(const char *entry, const mrcnn_conv_desc *d, int has_ws, char *out,
                         int out_len);

/* ReLU / affine backward helper: g[m,c] = gy[m,c] * (y[m,c] > 0) * scale[c]
 * (scale NULL = 1; y NULL = no mask).  Backward of the fused conv epilogue. */
int mrcnn_epilogue_bwd(const float *gy, const float *y, const float *scale,
                       float *g, int64_t M, int C, void *stream);
/* Column sums: out[c] = sum_m g[m,c] (bias gradients); ws of
 * mrcnn_colsum_workspace_bytes(C). Deterministic (two-level fixed-order sum). */
int mrcnn_colsum(const float *g, float *out, int64_t M, int C, void *ws, void *stream);

/* ---- Pooling ------------------------------------------------------------ */
/* F.max_pooling_2d(x,3,stride=2,pad=1), cover_all=True (models/resnet_extractor.py:69).
 * x (N,H,W,C) -> y (N,P,Q,C), P = (H+2-3+1)/2+1. Forward only: the stem is
 * frozen (unchain_backward at res2, models/resnet_extractor.py:86-87). */
int mrcnn_maxpool3x3s2p1_fwd(const float *x, float *y, int N, int H, int W, int C,
                             int P, int Q, void *stream);
/* F.average_pooling_2d(res5, 7, stride=7) on a 7x7 map (models/mask_rcnn_resnet.py:188):
 * x (R,HW,C) -> y (R,C) mean over HW; backward broadcasts gy/HW. */
int mrcnn_avgpool_fwd(const float *x, float *y, int R, int HW, int C, void *stream);
int mrcnn_avgpool_bwd(const float *gy, float *gx, int R, int HW, int C,
                      int accumulate, void *stream);
/* Gradient entering res5's last block from the two consumers of its output y (R,HW,C)
 * (models/mask_rcnn_resnet.py:186-195: average pooling -> cls_loc / score, and deconv6 on the
 * foreground rows), already through y's ReLU — one pass instead of avgpool backward + row
 * scatter-add + ReLU mask (three passes over the 411 MB tensor):
 *   g[r,p,c] = (g_pool[r,c] / HW + (slot[r] >= 0 ? g_rows[slot[r],p,c] : 0)) * (y[r,p,c] > 0)
 * g_rows (F,HW,C) / slot (R) int32 may both be NULL (no row consumer).  Same operation order
 * as the three separate kernels, so the result is bit-identical to them. */
int mrcnn_head_tail_bwd(const float *g_pool, const float *g_rows, const int32_t *slot,
                        const float *y, float *g, int R, int HW, int C, void *stream);

/* ---- Losses (models/mask_rcnn_train_chain.py:163-181,192-213) -------------- */
/* All loss kernels write loss[0] (device scalar, already normalised) and, when gx
 * is non-NULL, the gradient of that scalar w.r.t. x (the total loss is a plain
 * sum, :180).  ws: workspace of mrcnn_loss_workspace_bytes(rows) bytes, rows = R
 * for softmax_ce, 0 otherwise.  No host synchronisation. */
int64_t mrcnn_loss_workspace_bytes(int rows);
/* F.sigmoid_cross_entropy(x, t), t in {-1,0,1}; x element i at x[i*x_stride + x_off(i)]:
 * plain form: x (n) contiguous. */
int mrcnn_sigmoid_ce(const float *x, const int32_t *t, int64_t n, float *loss,
                     float *gx, void *ws, void *stream);
/* mask form: x (R, Kc, HW) NHWC rows = (R, HW, Kc); selects channel label[r]-1
 * for row r (models/mask_rcnn_train_chain.py:176-178); t (R,HW) in {-1,0,1};
 * gx (R,HW,Kc) fully written (zeros elsewhere).  A background row (label 0) selects
 * channel Kc-1, as NumPy's index -1 does; its targets are normally all -1.
 * Nothing counted (every t == -1, or R == 0): loss 0, gx 0, as mrcnn_sigmoid_ce and
 * mrcnn_softmax_ce. */
int mrcnn_mask_sigmoid_ce(const float *x, const int32_t *label, const int32_t *t,
                          int R, int HW, int Kc, float *loss, float *gx,
                          void *ws, void *stream);
/* F.softmax_cross_entropy(x (R,ncls) with row stride ldx, t) ignore -1. */
int mrcnn_softmax_ce(const float *x, int ldx, const int32_t *t, int R, int ncls,
                     float *loss, float *gx, int ldg, void *ws, void *stream);
/* _fast_rcnn_loc_loss: pred (n,4) [row r at pred + r*ld + 4*cls[r] when cls != NULL],
 * gt_loc (n,4), gt_label (n); in_weight = label>0; normaliser = #(label>=0).
 * gx written with the same addressing (caller zero-fills the rest).
 * Nothing counted (every label < 0, or n == 0): loss is 0/0 = NaN, the original's
 * unguarded division by #(label>=0); gx stays 0 (no row has label > 0). */
int mrcnn_smooth_l1(const float *pred, int ld, const int32_t *cls,
                    const float *gt_loc, const int32_t *gt_label, int n,
                    float sigma, float *loss, float *gx, void *ws, void *stream);
/* F.softmax(x) row-wise (models/mask_rcnn.py:208) */
int mrcnn_softmax(const float *x, int ldx, float *y, int ldy, int R, int ncls,
                  void *stream);
/* Replaces chainer's reporter.Summary.add (`_x += value`) for the trainer's LogReport of the
 * reported losses (models/mask_rcnn_train_chain.py:182-188): sums[k] = sums[k] + *values[k]
 * for k < n, one fp32 add per key, one launch on `stream` (after the loss kernels), no host
 * synchronisation.  values: HOST array of n device pointers to float scalars, passed to the
 * kernel by value; sums: device float[n].  0 <= n <= MRCNN_MAX_OBSERVED. */
#define MRCNN_MAX_OBSERVED 8
int mrcnn_observe_accumulate(const float *const *values, int n, float *sums, void *stream);

/* ---- Optimizer (chainer MomentumSGD + WeightDecay, examples/train_common.py:176-180) */
/* g += wd*p; v = momentum*v - lr*g; p += v, over one flat arena of n floats.
 * grad_scale multiplies g first (1/world_size after an all-reduce sum). */
int mrcnn_sgd_momentum_wd(float *p, const float *g, float *v, int64_t n, float lr,
                          float momentum, float wd, float grad_scale,
                          void *stream);
/* Same update; with zero_grad != 0 the gradient arena is cleared in the same pass (chainer's
 * cleargrads() before the next backward, examples/train_common.py:226-231 via
 * StandardUpdater.update_core): a parameter whose backward does not run in the next step then
 * contributes a zero gradient instead of a stale one. */
int mrcnn_sgd_momentum_wd_ex(float *p, float *g, float *v, int64_t n, float lr,
                             float momentum, float wd, float grad_scale, int zero_grad,
                             void *stream);

/* ---- Global gradient norm and the step's control word (chainer's GradientClipping rule,
 * a non-finite guard, the logged norm) — three launches on one stream, no host round trip:
 * mrcnn_grad_sumsq per arena run, one mrcnn_grad_control, mrcnn_sgd_momentum_wd_ctl per run. */
/* partials[b], b < MRCNN_SUMSQ_PARTIALS: the sum of (double)g[i]^2 over chunk b of the n floats
 * (equal contiguous runs of whole 16-byte groups; the n % 4 tail belongs to the last chunk).
 * float64 from the square onward, a fixed order, no atomics: the same bits on every call,
 * whatever the device's CU count.  Every partial is written (empty chunks and n == 0: 0).
 * g: 16-byte aligned. */
#define MRCNN_SUMSQ_PARTIALS 1024
int mrcnn_grad_sumsq(const float *g, int64_t n, double *partials, void *stream);
/* ctl[4] from the partial slabs of one or more runs (n_partials doubles, summed in index order
 * in float64; sum = that total):
 *   NORM          (float)(sqrt(sum) * grad_scale): the norm of the averaged gradient; may be
 *                 inf / NaN, and may saturate to inf in float
 *   FACTOR        what the SGD launch multiplies g by: grad_scale bit for bit, or, when
 *                 clip > 0 and norm > clip, grad_scale * clip / norm (float64, rounded once) —
 *                 chainer's rate = threshold / norm, applied only when rate < 1
 *   SKIPPED       1.f if skip_nonfinite and the float64 sum is not finite, else 0.f (squares of
 *                 fp32 values cannot overflow float64: finite gradients are never skipped)
 *   NORM_REPORTED NORM, or 0 when the sum is not finite (keeps a log window's mean finite) */
#define MRCNN_CTL_NORM 0
#define MRCNN_CTL_FACTOR 1
#define MRCNN_CTL_SKIPPED 2
#define MRCNN_CTL_NORM_REPORTED 3
#define MRCNN_CTL_SIZE 4
int mrcnn_grad_control(const double *partials, int n_partials, float grad_scale, float clip,
                       int skip_nonfinite, float *ctl, void *stream);
/* mrcnn_sgd_momentum_wd_ex with grad_scale = ctl[MRCNN_CTL_FACTOR] read on the device (the same
 * update expression: the same bits for the same factor).  With ctl[MRCNN_CTL_SKIPPED] != 0, p and
 * v are left untouched; g is still cleared when zero_grad is set. */
int mrcnn_sgd_momentum_wd_ctl(float *p, float *g, float *v, int64_t n, float lr, float momentum,
                              float wd, const float *ctl, int zero_grad, void *stream);

/* Per-class `prob > thresh` filter + stable descending sort + gather, all foreground
 * classes in one launch: the first half of MaskRCNN._suppress (models/mask_rcnn.py:178-202).
 * prob (R, n_class), cls_bbox (R, n_class, 4) -> sorted_boxes (n_class-1, R, 4),
 * sorted_prob (n_class-1, R), counts (n_class-1); feed to mrcnn_nms_sorted_batched. */
int64_t mrcnn_detect_sort_workspace_bytes(int R, int n_class);
int mrcnn_detect_sort(const float *prob, const float *cls_bbox, int R, int n_class,
                      float thresh, float *sorted_boxes, float *sorted_prob,
                      int32_t *counts, void *ws, void *stream);

/* Soft-NMS (Bodla et al. 2017) in the place of mrcnn_nms_sorted_batched: replaces Detectron's
 * utils/cython_nms.pyx:cpu_soft_nms (TEST.SOFT_NMS), all classes in one launch.  sorted_boxes
 * (groups, n_max, 4), sorted_prob (groups, n_max) and counts (groups) as mrcnn_detect_sort writes
 * them.  Per group, with s an fp32 copy of the first counts[g] scores and every row alive:
 *   repeat: i = the alive row with the largest s (ties: the lowest row); stop if no row is alive,
 *           or not (s[i] >= min_score), or `limit` (> 0) picks were made; emit i, alive[i] = false;
 *           for every alive j: s[j] = s[j] * w(iou(box_i, box_j))        (one fp32 multiply)
 *   w hard:     iou >= overlap_thresh ? 0 : 1
 *   w linear:   iou >= overlap_thresh ? 1 - iou : 1                      (fp32)
 *   w gaussian: iou > 0 ? (float)exp(-((double)iou * (double)iou) / (double)sigma) : 1
 * iou is the fp32 expression of mrcnn_nms_sorted (a NaN IoU, from zero-area boxes, gives weight 1),
 * so method hard emits the rows mrcnn_nms_sorted_batched keeps.  cpu_soft_nms swaps the maximum to
 * the front and prunes rows below min_score after every pick; scores only fall, so this rule emits
 * the same rows in the same order with the same scores, and fixes the order of equal scores.
 * Writes keep (groups, n_max) = rows in emission order, n_keep (groups) and soft_prob
 * (groups, n_max) = the score every row had when it was emitted or, if it never was, when the loop
 * ended (rows >= counts[g] are not written); mrcnn_detect_compact takes soft_prob as its
 * sorted_prob.  Input contract: scores finite and non-negative (mrcnn_detect_sort's
 * `prob > thresh`), sigma > 0 for the gaussian method (unused by the others), n_max <= 4096. */
#define MRCNN_SOFT_NMS_HARD     0
#define MRCNN_SOFT_NMS_LINEAR   1
#define MRCNN_SOFT_NMS_GAUSSIAN 2
int mrcnn_soft_nms_sorted_batched(const float *sorted_boxes, const float *sorted_prob,
                                  const int32_t *counts, int groups, int n_max, int method,
                                  float overlap_thresh, float sigma, float min_score, int limit,
                                  int32_t *keep, int32_t *n_keep, float *soft_prob, void *stream);
/* Bounding-box voting behind either suppression: replaces Detectron's utils/boxes.py:box_voting
 * with scoring method ID (TEST.BBOX_VOTE; scores are not changed).  For every kept row
 * k = keep[g][q], q < n_keep[g]: over j = 0 .. counts[g] - 1 in row order, every j with
 * iou(box_k, box_j) >= vote_thresh adds w = (double)sorted_prob[g][j] (the undecayed score) to wsum
 * and w * (double)box_j[c] to acc[c]; voted_boxes[g][k][c] = (float)(acc[c] / wsum), or box_k
 * unchanged when wsum == 0 (a zero-area box overlaps nothing, itself included).  Only the kept rows
 * of voted_boxes (groups, n_max, 4) are written; mrcnn_detect_compact takes it as its
 * sorted_boxes. */
int mrcnn_box_vote(const float *sorted_boxes, const float *sorted_prob, const int32_t *counts,
                   const int32_t *keep, const int32_t *n_keep, int groups, int n_max,
                   float vote_thresh, float *voted_boxes, void *stream);

/* ---- Image I/O at both ends of predict (device restatement of the reference's cv2 calls) ---- */
/* MaskRCNN.prepare (models/mask_rcnn.py:152-176) for one image + its slot in the zero-padded
 * batch (datasets/concat_examples.py:20-26): bilinear resize by `scale` (OpenCV INTER_LINEAR
 * float rule) of src (C=3,H,W) — fp32, or uint8 as decoded when src_is_u8 — into image n of
 * dst (N,dstH,dstW,3) NHWC, minus the RGB mean (mean_host: HOST pointer to 3 floats).
 * (outH,outW) = rounded scaled size.  flip_x != 0 mirrors the resized image left-right: the
 * random_flip of datasets/transforms.py:38-40 folded into the same pass. */
int mrcnn_prepare_image(const void *src_chw, int src_is_u8, int C, int H, int W, double scale,
                        const float *mean_host, float *dst_nhwc, int dstH, int dstW,
                        int outH, int outW, int n, int flip_x, void *stream);
/* Large-scale jitter: mrcnn_prepare_image's arguments, with (rH,rW) the
 * rounded scaled size, plus a crop window.  Image n of dst (N,dstH,dstW,3) NHWC is the canvas:
 * canvas pixel (y,x) = pixel (y+oy, x+ox) of the (rH,rW) image mrcnn_prepare_image would write
 * with the same flip_x, and 0 where that lies beyond it; the whole slot is written, so the caller
 * need not zero it.  The pixel function is mrcnn_prepare_image's own (csrc/prepare_pixel.h), so
 * the result equals a slice of its output bit for bit, and the resized image (4 x the canvas at
 * twice the canvas size) never exists.  0 <= oy < rH, 0 <= ox < rW, dstH <= 65535.  The reference
 * has no scale augmentation (chainer_mask_rcnn/datasets/transforms.py:10-51 resizes to one
 * fixed scale); this extends the kernel that replaces its resize. */
int mrcnn_prepare_image_crop(const void *src_chw, int src_is_u8, int C, int H, int W, double scale,
                             const float *mean_host, float *dst_nhwc, int dstH, int dstW,
                             int rH, int rW, int oy, int ox, int n, int flip_x, void *stream);
/* segm_results / expand_boxes (models/mask_rcnn.py:44-107): mask_logits (D,M,M,Kc) NHWC head
 * outputs, label (D) foreground class per detection, bbox (D,4) yx in image coordinates ->
 * out (D,im_h,im_w) uint8 {0,1}: sigmoid, 1-pixel zero pad, box expanded by (M+2)/M and
 * truncated to int, INTER_LINEAR resize, threshold 0.5, paste. */
int mrcnn_paste_masks(const float *mask_logits, const int32_t *label, const float *bbox,
                      int D, int M, int Kc, int im_h, int im_w, uint8_t *out, void *stream);

/* ---- Packed masks for instance-segmentation evaluation (csrc/mask_eval.hip, image.hip) ---
 * Format: a set of N masks over an H x W image is uint64 (N, H, Wq), Wq = ceil(W / 64); bit
 * (x & 63) of word [n, y, x >> 6] is pixel (n, y, x), pad bits are zero — byte for byte
 * np.packbits(m, axis=-1, bitorder='little') of rows zero-padded to a multiple of 64.  Any
 * nonzero input value is foreground.  Each mask carries its exact area (int32 pixel count) and
 * an extent int32 (y_lo, y_hi, wq_lo, wq_hi): half-open row and word ranges that contain every
 * set bit (empty, lo >= hi, for a mask with none).  H * W < 2^31. */
/* Pack (N,H,W) masks of elem_bytes 1 (uint8 / bool) or 4 (int32): packed (N,H,Wq), area (N),
 * tight extent (N,4).  Replaces the per-mask work of get_mask_overlap
 * (chainer_mask_rcnn/utils/geometry.py) and pycocotools.mask.encode / area. */
int mrcnn_mask_pack(const void *masks, int elem_bytes, int N, int H, int W, uint64_t *packed,
                    int32_t *area, int32_t *extent, void *stream);
/* mrcnn_paste_masks written in the packed format: the bits equal pack(mrcnn_paste_masks(...))
 * exactly (one shared per-pixel function), area (D) exact, extent (D,4) = the clipped expanded
 * box widened to whole words.  Replaces segm_results (models/mask_rcnn.py:63-107) followed by
 * the host-side mask handling of the evaluators. */
int mrcnn_paste_masks_packed(const float *mask_logits, const int32_t *label, const float *bbox,
                             int D, int M, int Kc, int im_h, int im_w, uint64_t *packed,
                             int32_t *area, int32_t *extent, void *stream);
/* inter (P,G) int32 = |A_p & B_g| for packed A (P,H,Wq) and B (G,H,Wq) of an H x W image; only
 * the overlap of the two extents (clamped to the image) is read, a pair whose extents do not
 * overlap gives 0.  Replaces np.bitwise_and(...).sum() of get_mask_overlap and the RLE
 * intersection of pycocotools' rleIou; union = area_a + area_b - inter. */
int mrcnn_mask_intersect(const uint64_t *a, const int32_t *ext_a, int P, const uint64_t *b,
                         const int32_t *ext_b, int G, int H, int W, int32_t *inter,
                         void *stream);
/* Mask boundaries for Boundary IoU (csrc/mask_boundary.hip): out (N,H,Wq) = M & ~E, where
 * E(y,x) = 1 iff every pixel (y',x') with |y'-y| <= d and |x'-x| <= d lies inside the image and
 * is foreground; out_area (N) its exact bit count.  Replaces mask_to_boundary of the
 * boundary-iou-api (cv2.erode with a 3x3 kernel, d iterations, on the mask padded by a ring of
 * zeros) behind COCOeval's iouType 'boundary'.  Every word of out is written (zero outside the
 * extent and in the pad bits); the boundary set reuses the input extent (N,4), inside which
 * alone packed is read, so slack in the extent does not change the result; an empty extent gives
 * zeros and area 0.  d >= 1 and may exceed 63, W and H.  out must not alias packed.  workspace:
 * caller-owned scratch of at least mrcnn_mask_boundary_workspace_bytes(N, H, W) bytes (the
 * row-eroded masks between the two launches).  N <= 65535; N == 0 returns without a launch. */
int64_t mrcnn_mask_boundary_workspace_bytes(int N, int H, int W);
int mrcnn_mask_boundary(const uint64_t *packed, const int32_t *extent, int N, int H, int W,
                        int d, uint64_t *out, int32_t *out_area, void *workspace,
                        int64_t workspace_bytes, void *stream);

/* ---- Box IoU for evaluation (csrc/bbox_eval.hip) ---------------------------------------------
 * The IoU tables of a whole evaluation batch of images in one launch (ragged): boxes_a (n_a,4)
 * are the images' detections one after another, boxes_b (n_b,4) their ground-truth boxes; image i
 * owns rows a_off[i] .. a_off[i+1] of boxes_a (P_i of them) and b_off[i] .. b_off[i+1] of boxes_b
 * (G_i); a_off / b_off are (n_img+1) int32 prefix offsets, out_off (n_img+1) int64 with
 * out_off[i+1] - out_off[i] = P_i * G_i and total = out_off[n_img] (the host's copy).  Output: iou
 * (total) flat, image after image, each image's table row-major (P_i, G_i).  All arrays are device
 * pointers.  One thread per pair; every read is bounded by the offsets and by n_a / n_b (a pair
 * the offsets do not describe is left unwritten); total == 0 returns at once without a launch. */
/* VOC convention: (y1, x1, y2, x2) float32; 1 is added to both max corners, then chainercv's
 * bbox_iou, operation for operation (the per-pair function mrcnn_bbox_iou_argmax uses) —
 * bit-identical to utils.bbox.bbox_iou(a + [0,0,1,1], b + [0,0,1,1]).  Replaces the per-image,
 * per-class `bbox[:, 2:] += 1; bbox_iou(...)` of chainercv's calc_detection_voc_prec_rec. */
int mrcnn_box_iou_voc(const float *boxes_a, const float *boxes_b, const int32_t *a_off,
                      const int32_t *b_off, const int64_t *out_off, int n_img, int n_a, int n_b,
                      int64_t total, float *iou, void *stream);
/* COCO convention: (x, y, w, h) float64, crowd_b (n_b) uint8 or null (no crowds).  pycocotools'
 * bbIou: w = min(Dx+Dw, Gx+Gw) - max(Dx, Gx), 0 if w <= 0; h likewise; i = w*h; u = crowd ? Dw*Dh
 * : Dw*Dh + Gw*Gh - i; i / u.  Replaces maskUtils.iou(d, g, iscrowd) of COCOeval.computeIoU for
 * iouType 'bbox'. */
int mrcnn_box_iou_coco(const double *boxes_a, const double *boxes_b, const uint8_t *crowd_b,
                       const int32_t *a_off, const int32_t *b_off, const int64_t *out_off,
                       int n_img, int n_a, int n_b, int64_t total, double *iou, void *stream);

/* ---- COCO RLE of packed masks (csrc/mask_rle.hip) -----------------------------------------
 * Uncompressed counts: runs over the column-major pixel index p = x * H + y, alternating 0 / 1
 * starting with zeros (the first run may be 0), summing to H * W (pycocotools maskApi.c
 * rleEncode).  Compressed string (rleToString): from the fourth count on, count[i] - count[i-2]
 * is stored instead of count[i]; each value as 5-bit groups, low first, character = group + 48,
 * bit 5 (0x20) = more groups follow, the last group's bit 4 is the sign.  Characters 48..111.
 * Integer arithmetic only: outputs depend on the input alone. */
/* Encode N packed masks (N,H,Wq) whose extents (N,4) contain every set bit (pack_masks' tight
 * extents or paste_masks_packed's widened ones; only the extent's rows and words are read).
 * Caller-owned: chg_off int32 (N*Wq+1) scratch; val_off int32 (N+1): counts of mask n are
 * counts[val_off[n] .. val_off[n+1]); pos int32 (cap_values) scratch; counts int32
 * (cap_values); str_off int32 (N+1): the string of mask n is chars[str_off[n] .. str_off[n+1]).
 * val_off is always complete.  A mask whose counts end beyond cap_values writes no counts and
 * has an empty string; chars are written only for masks whose string ends within cap_chars.  A
 * caller that finds val_off[N] > cap_values or str_off[N] > cap_chars calls again with larger
 * buffers (at most 7 characters per count).  N * (H * W + 1) * 7 < 2^31. */
int mrcnn_rle_encode(const uint64_t *packed, const int32_t *extent, int N, int H, int W,
                     int32_t *chg_off, int32_t *val_off, int32_t *pos, int32_t *counts,
                     int cap_values, int32_t *str_off, char *chars, int cap_chars, void *stream);
/* Decode N masks of an H x W image: either chars (compressed strings, mask n =
 * chars[off[n] .. off[n+1])) or values (counts, values[off[n] .. off[n+1])), the other null.
 * starts int32 (off[N]) scratch; nval int32 (N) runs per mask; status int32 (N) MRCNN_RLE_*.
 * Output packed (N,H,Wq) (every word written; all zero for a mask whose status is not OK), exact
 * area (N) and tight extent (N,4): ready for mrcnn_mask_intersect.  Reads and writes stay
 * inside the buffers for any input. */
#define MRCNN_RLE_OK 0
#define MRCNN_RLE_BAD_CHAR 1        /* a character outside 48..111 */
#define MRCNN_RLE_UNTERMINATED 2    /* the string ends inside a value, or a value has > 7 groups */
#define MRCNN_RLE_NEGATIVE 3        /* a negative run */
#define MRCNN_RLE_BAD_SUM 4         /* the runs do not sum to H * W */
int mrcnn_rle_decode(const uint8_t *chars, const int32_t *values, const int32_t *off, int N,
                     int H, int W, int32_t *starts, int32_t *nval, int32_t *status,
                     uint64_t *packed, int32_t *area, int32_t *extent, void *stream);
/* Packed (N,H,Wq) -> (N,H,W) uint8 {0,1}. */
int mrcnn_mask_unpack(const uint64_t *packed, int N, int H, int W, uint8_t *out, void *stream);

/* ---- Instance label images (csrc/instance_labels.hip) --------------------------------------
 * Replaces label2instance_boxes and instance_boxes2label (chainer_mask_rcnn/utils/
 * geometry.py:94-147).  ins and cls are (H, W) label images of elem_bytes 4 (int32) or 1
 * (uint8, where 255 reads as -1: the VOC PNG "void" index); H * W < 2^31.  With
 * mask_by_class, pixels whose class is -1 or 0 have instance -1 (the datasets'
 * lbl_ins[np.isin(lbl_cls, [-1, 0])] = -1).  Instances are the distinct instance values other
 * than -1 (0 and other negatives included), ranked ascending.
 * Limits: the instance values and the class values under instances each span at most
 * MRCNN_LABEL_WINDOW (max - min + 1), and n_instances * n_classes <= MRCNN_LABEL_WINDOW. */
#define MRCNN_LABEL_WINDOW (1 << 24)
/* First half (queued, the caller then reads meta): meta int32[6] = (ins_min, ins_max,
 * cls_min, cls_max, n_instances, n_classes), ranges empty (min > max) without an instance
 * pixel; bitmaps uint32[2 * MRCNN_LABEL_WINDOW / 32] (instances, then classes) and prefix
 * int32[2 * MRCNN_LABEL_WINDOW / 32] are caller-owned scratch for mrcnn_label_instances.
 * A span over the window leaves counts for the in-window values only: the caller rejects it. */
int mrcnn_label_scan(const void *ins, int ins_bytes, const void *cls, int cls_bytes, int H, int W,
                     int mask_by_class, int32_t *meta, uint32_t *bitmaps, int32_t *prefix,
                     void *stream);
/* Second half, with n = meta[4], ncls = meta[5], span_ins = meta[1] - meta[0] + 1 and
 * span_cls = meta[3] - meta[2] + 1 read by the caller.  table int32[2 * n * ncls + ncls] is
 * scratch (pixel count and first row-major position per (instance, class), class values).
 * Outputs: ids (n) ascending instance values; classes (n) the majority class of each
 * instance, ties to the class whose first pixel in row-major order comes first (the
 * reference's Counter insertion order), -1 / 0 reported as they are; boxes (n, 4)
 * (y1, x1, y2, x2) half-open; masks (n, H, W) uint8 0/1 unless masks is NULL. */
int mrcnn_label_instances(const void *ins, int ins_bytes, const void *cls, int cls_bytes, int H,
                          int W, int mask_by_class, const int32_t *meta, const uint32_t *bitmaps,
                          const int32_t *prefix, int span_ins, int span_cls, int n, int ncls,
                          int32_t *table, int32_t *ids, int32_t *classes, int32_t *boxes,
                          uint8_t *masks, void *stream);
/* lbl_ins / lbl_cls (H, W) int32 from masks (N, H, W) uint8 painted in the order
 * order[0..N) (NULL: 0..N-1); the last mask covering a pixel wins: lbl_ins = its position j in
 * the painting order, lbl_cls = labels[order[j]]; -1 and 0 where no mask covers. */
int mrcnn_instances_to_label(const uint8_t *masks, const int32_t *order, const int32_t *labels,
                             int N, int H, int W, int32_t *lbl_ins, int32_t *lbl_cls,
                             void *stream);

/* ---- Instance drawing and the report mosaic (csrc/visualize.hip) ---------------------------
 * Replaces draw_instance_bboxes (chainer_mask_rcnn/utils/visualizations.py) and fcn's
 * get_tile_image as InstanceSegmentationVisReport (extensions/instance_segmentation_vis_
 * report.py) uses them.  The drawing contract, restated in NumPy by tests/visualize_ref.py:
 * for every instance i in order whose draw flag is set, inside its crop C_i = [y1, y2) x
 * [x1, x2) clipped to the image, a pixel with mask bit set becomes
 * trunc(double(v) * (1 - alpha) + t_i[c]) per channel (one fp64 multiply, one fp64 add), then
 * a pixel whose 3x3 neighbourhood clamped to C_i holds both mask values becomes (200, 200,
 * 200); the mask outside C_i is never read.  Then for every instance i in order: the pixels
 * within Chebyshev distance thickness / 2 of the 1-pixel rectangle through (x1, y1) and
 * (x2, y2) take its outline colour, then its caption coverage a (uint8) composites white:
 * v = (255 * a + v * (255 - a) + 127) / 255.  Each pixel depends only on its own value and
 * on mask bits: one thread per pixel, no atomics, bitwise deterministic. */
#define MRCNN_DRAW_MAX_INSTANCES 4096
#define MRCNN_TILE_MAX_CELLS 64
typedef struct mrcnn_draw_instance {
    double t[3];          /* mask colour term per channel: the fp32 color_inst * alpha, widened */
    int32_t box[4];       /* truncated (y1, x1, y2, x2), not clipped */
    int32_t draw;         /* nonzero: drawn; zero: skipped in both passes */
    uint32_t rgb;         /* outline colour r | g << 8 | b << 16 */
    int32_t cap[4];       /* caption rectangle (y0, x0, h, w) in image pixels; h or w 0: none */
    int64_t cap_offset;   /* byte offset of its (h, w) coverage in the atlas */
} mrcnn_draw_instance;    /* 72 bytes */
/* img (H, W, 3) uint8 drawn in place.  packed (N, H, Wq) masks in the packed format above
 * (NULL: no masks, pass 1 is skipped); extent (N, 4) their extents, used to skip tiles (NULL:
 * every tile of the crop is visited).  inst (N) device records, atlas the captions' coverage
 * bytes (atlas_bytes of them; a caption that reaches past them reads 0).  0 <= alpha <= 1,
 * 1 <= thickness <= 32767, N <= MRCNN_DRAW_MAX_INSTANCES, H * W < 2^31, H <= 4 * 65535. */
int mrcnn_draw_instances(uint8_t *img, int H, int W, const uint64_t *packed,
                         const int32_t *extent, int N, const mrcnn_draw_instance *inst,
                         const uint8_t *atlas, int64_t atlas_bytes, double alpha, int thickness,
                         void *stream);
typedef struct mrcnn_tile_cell {
    const uint8_t *src;   /* device (h, w, 3) uint8 image */
    int32_t h, w;         /* its size */
    int32_t oh, ow;       /* the size it is scaled to, inside the cell; 0: an empty cell */
    int32_t oy, ox;       /* offset of the scaled image in its cell */
} mrcnn_tile_cell;        /* 32 bytes */
/* out (rows * cell_h, cols * cell_w, 3) uint8: cell k = cells[k] (HOST array, k < n_cells,
 * row-major) scaled with the half-pixel bilinear rule of mrcnn_prepare_image (fp32, truncated
 * to uint8); margins and cells >= n_cells are 0.  n_cells <= rows * cols <=
 * MRCNN_TILE_MAX_CELLS, output H * W < 2^31 and H <= 65535.  Replaces fcn.utils.get_tile_image (bilinear instead of skimage's
 * anti-aliased resize). */
int mrcnn_tile_images(const mrcnn_tile_cell *cells, int n_cells, int rows, int cols, int cell_h,
                      int cell_w, uint8_t *out, void *stream);

/* Second half of MaskRCNN._suppress (models/mask_rcnn.py:195-202): the rows kept by
 * mrcnn_nms_sorted_batched (keep (G,R), n_keep (G)) of every class packed densely, class after
 * class and in keep order: bbox (<= G*R, 4), label, score, *total = number of rows. */
int mrcnn_detect_compact(const int32_t *keep, const int32_t *n_keep, const float *sorted_boxes,
                         const float *sorted_prob, int G, int R, float *bbox, int32_t *label,
                         float *score, int32_t *total, void *stream);

/* ---- Inference post-processing (models/mask_rcnn.py:204-265) ---------------- */
/* Per-class decode: cls_bbox[r,l,:] = clip(loc2bbox(roi[r]/scale,
 * cls_loc[r,l,:]*std+mean), 0, size) for all classes (:225-240). */
/* mean4/std4 are HOST pointers to 4 doubles (loc_normalize_mean/std): the reference builds
 * them from Python tuples, i.e. as float64 arrays, so `loc * std + mean` is evaluated in double
 * and rounded to fp32 once (pinned by tests/golden/to_bboxes.npz). */
int mrcnn_decode_cls_boxes(const float *roi, const float *cls_loc, int ld_loc,
                           float *cls_bbox, int R, int n_class, float scale,
                           const double *mean4, const double *std4, float size_h,
                           float size_w, void *stream);

/* ---- Test-time augmentation (csrc/test_aug.hip; Detectron TEST.BBOX_AUG / TEST.MASK_AUG) ----
 * An image is run through the network as up to MRCNN_TEST_AUG_MAX_VIEWS views (mirrored, other
 * scales); these two launches map the views' results back into the image frame and merge them. */
#define MRCNN_TEST_AUG_MAX_VIEWS 8
typedef struct {
    const float *roi;       /* (R,4) device: the view's RoIs (y_min, x_min, y_max, x_max) in the
                             * view's own (scaled, possibly mirrored) frame; 16-byte aligned */
    const float *cls_loc;   /* (R, >= 4*n_class) device: the head's regression outputs */
    int32_t ld_loc;         /* floats from one row of cls_loc to the next, >= 4*n_class */
    int32_t R;              /* rows of this view; 0 is legal (the pointers are then not read) */
    float scale;            /* the view's scale, as mrcnn_decode_cls_boxes takes it */
    int32_t flip_x;         /* != 0: the view saw the image mirrored left-right */
} mrcnn_test_aug_view;      /* 32 bytes */
/* One image's union of candidates over its views in one launch.  views: HOST array of n_views
 * records (0 <= n_views <= MRCNN_TEST_AUG_MAX_VIEWS), copied into the launch by value; mean4 / std4
 * HOST pointers to 4 doubles; cls_bbox (sum R_v, n_class, 4) device, 16-byte aligned.  The rows of
 * view v start at row sum_{u<v} R_u and keep the view's own row order.  Every row is
 *   1. the expression of mrcnn_decode_cls_boxes with the view's scale and (size_h, size_w) (one
 *      shared device function, csrc/decode_cls_box.h), then
 *   2. for a view with flip_x != 0, in fp32:  x_min' = size_w - x_max,  x_max' = size_w - x_min
 *      (boxes are (y_min, x_min, y_max, x_max): chainercv's flip_bbox about the original width,
 *      datasets/transforms.py:flip_bbox; clipped boxes stay inside [0, size_w]).
 * For an unmirrored view the rows equal mrcnn_decode_cls_boxes on that view bit for bit.  As in
 * Detectron the mirror is taken about the ORIGINAL width size_w: the view was mirrored about its
 * resized width round(size_w * scale), so its frame maps back to a width of
 * round(size_w * scale) / scale, and the difference to size_w (at most half a resized pixel,
 * 0.5 / scale) is ignored.  n_views == 0 or sum R_v == 0 launches nothing;
 * (sum R_v) * n_class < 2^31. */
int mrcnn_decode_cls_boxes_views(const mrcnn_test_aug_view *views, int n_views, int n_class,
                                 const double *mean4, const double *std4, float size_h,
                                 float size_w, float *cls_bbox, void *stream);
/* The views' mask-head outputs for the same D boxes combined into one map (Detectron
 * MASK_AUG.HEUR).  maps: HOST array of n_views device pointers to (D,M,M,Kc) fp32 NHWC logits, the
 * layout mrcnn_paste_masks reads; flip_x: HOST array of n_views flags; out (D,M,M,Kc) logits, so
 * mrcnn_paste_masks / mrcnn_paste_masks_packed take it as they take one view's map.  With
 * l_v = maps[v][d, y, flip_x[v] ? M-1-x : x, k], v = 0 .. n_views-1 in order, out[d,y,x,k] is
 *   LOGIT_AVG: (float)((l_0 + l_1 + ... ) / n_views)     sum in double in view order, one division
 *   SOFT_MAX:  the largest l_v (fp32; sigmoid is monotone, so the largest probability); of equal
 *              values the first view's (matters for -0 / +0 only)
 *   SOFT_AVG:  the logit of the mean probability, in double: e_v = exp(-|l_v|),
 *              p_v = sigmoid(l_v) and q_v = sigmoid(-l_v) taken as 1 / (1 + e_v) and e_v / (1 + e_v)
 *              (which is which by the sign of l_v), P = (sum p_v) / n_views, Q = (sum q_v) / n_views,
 *              out = (float)(log(P) - log(Q)); 1 - P is never formed, so the result stays accurate
 *              where the maps saturate (all views at -300 give -300, not -inf).
 * Input contract: finite logits, 1 <= n_views <= MRCNN_TEST_AUG_MAX_VIEWS, no map aliases out,
 * D * M * M * Kc < 2^31.  SOFT_AVG beyond the range of double: where every view's logit is below
 * about -745 (exp(-|l|) underflows to 0; it is subnormal from about -708), P is 0 and out is
 * -infinity, and likewise +infinity above +745; mrcnn_paste_masks' sigmoid reads them as 0 and 1.
 * D == 0 launches nothing.  16-byte loads and stores are used where Kc % 4 == 0 and every pointer
 * is 16-byte aligned, scalar ones otherwise; the result is the same. */
#define MRCNN_MASK_AUG_SOFT_AVG  0
#define MRCNN_MASK_AUG_SOFT_MAX  1
#define MRCNN_MASK_AUG_LOGIT_AVG 2
int mrcnn_mask_aug_combine(const float *const *maps, const int32_t *flip_x, int n_views, int D,
                           int M, int Kc, int heuristic, float *out, void *stream);

/* ---- Target creators: the device half ------------------------- */
/* The deterministic arithmetic of ProposalTargetCreator.__call__
 * (models/utils/proposal_target_creator.py:121-177) and chainercv's AnchorTargetCreator
 * (call site models/mask_rcnn_train_chain.py:153-158): IoU matrices, label rules, regression
 * targets, 14x14 mask targets.  The np.random draws stay with the caller (host), which reads
 * max_iou / the anchor labels back, draws, and passes the chosen indices in. */
/* chainercv bbox_iou(boxes_a (na,4), boxes_b (g,4)) reduced per row: max_iou (na), first
 * argmax (na); optional full matrix iou (na,g) and its column maxima col_max (g).
 * na == 0 returns at once and writes nothing: an empty column has no maximum (NumPy's max
 * raises), so col_max keeps its contents and the caller must not read it. */
int mrcnn_bbox_iou_argmax(const float *boxes_a, int na, const float *boxes_b, int g,
                          float *iou, float *max_iou, int32_t *argmax, float *col_max,
                          void *stream);
/* AnchorTargetCreator label rule before subsampling: -1 / 0 (max < neg) / 1 (row holds a
 * column maximum, or max >= pos). */
int mrcnn_anchor_labels(const float *iou, const float *max_iou, const float *gt_max, int na,
                        int g, float neg_iou_thresh, float pos_iou_thresh, int32_t *label,
                        void *stream);
/* label_inside[disabled[.]] = -1 (the host's draws), then the full-size targets: label (-1
 * outside the image) and loc = bbox2loc(anchor, bbox[argmax]) (0 outside). */
int mrcnn_anchor_targets_finish(const float *anchor_inside, const int32_t *inside_index,
                                int32_t *label_inside, const int32_t *argmax, const float *bbox,
                                int n_inside, const int32_t *disabled, int n_disabled,
                                int n_anchor, float *loc, int32_t *label, void *stream);
/* Rows chosen[0..n_sample) of the candidates (the first n_fg are foreground): sample_roi,
 * gt_roi_loc = (bbox2loc(roi, bbox[assigned]) - mean) / std, gt_roi_label (class + 1 | 0),
 * gt_index = assigned ground-truth box.  mean4 / std4 are HOST pointers to 4 floats. */
int mrcnn_proposal_targets_gather(const float *cand, const float *bbox, const int32_t *gt_label,
                                  const int32_t *assigned, const int32_t *chosen, int n_sample,
                                  int n_fg, const float *mean4_host, const float *std4_host,
                                  float *sample_roi, float *gt_roi_loc, int32_t *gt_roi_label,
                                  int32_t *gt_index, void *stream);
/* (n, M, M) int32 mask targets: rows < n_fg = crop of masks[gt_index] (uint8 (G,H,W)) at the
 * rounded RoI, cv2 INTER_LINEAR to M x M, > 0.5; other rows -1. */
int mrcnn_mask_targets(const uint8_t *masks, int G, int H, int W, const float *sample_roi,
                       const int32_t *gt_index, int n, int n_fg, int M, int32_t *out,
                       void *stream);
/* Ground-truth masks at the network size from packed source-size masks ("Packed masks" above):
 * packed (G,H,Wq) device, ys (outH) / xs (outW) device tables of the source row / column of each
 * output row / column -> out (G,outH,outW) uint8 {0,1}, out[g,y,x] = bit (g, ys[y], xs[x]); the
 * input mrcnn_mask_targets reads.  Replaces the host resize and flip of the dense mask stack,
 * datasets/transforms.py:resize_nearest (the reference's
 * chainer_mask_rcnn/datasets/transforms.py:36-38 `transforms.resize(mask, interpolation=0)` and
 * :45-49 `transforms.flip`): the caller builds the tables with the cv2 INTER_NEAREST index rule
 * and reverses xs for a horizontal flip, so only bits cross PCIe.  Table entries are clamped to
 * [0, H-1] / [0, W-1]: reads and writes stay inside the buffers whatever the tables hold.  G = 0
 * is a no-op.  H * W < 2^31, G * outH * outW < 2^31, W <= 524288 (a source row is staged in
 * LDS). */
int mrcnn_mask_resize_nearest(const uint64_t *packed, int G, int H, int W, const int32_t *ys,
                              const int32_t *xs, int outH, int outW, uint8_t *out, void *stream);
/* The same for the S x S canvas of large-scale jitter: ys / xs (S) device
 * tables in which a NEGATIVE entry means "outside the resized mask" (the canvas is padded there:
 * 0 is written); entries >= 0 are clamped to H-1 / W-1 as above, so no read leaves the buffers
 * whatever the tables hold.  out (G,S,S) uint8 {0,1}; box (G,4) int32 (y_lo, x_lo, y_hi, x_hi),
 * half-open and tight around the pixels of out[g], (0,0,0,0) for an empty mask; area (G) int32
 * pixel counts.  row_stats: (G,S,3) int32 of workspace (per-row x_lo, x_hi, count, reduced per
 * instance by a second launch on the same stream: integers, in a fixed order).  Replaces the
 * host resize and flip of datasets/transforms.py:resize_nearest followed by a crop / zero pad
 * and utils.mask_to_bbox of the result (the reference's
 * chainer_mask_rcnn/datasets/transforms.py:36-49 has the resize and flip only).  G = 0 is a no-op.
 * H * W < 2^31, G * S * S < 2^31, W <= 524288. */
int mrcnn_mask_resize_crop(const uint64_t *packed, int G, int H, int W, const int32_t *ys,
                           const int32_t *xs, int S, uint8_t *out, int32_t *box, int32_t *area,
                           int32_t *row_stats, void *stream);
/* Simple Copy-Paste (Ghiasi et al., 2021) on that canvas: the K instances
 * idx[0..K) of a source example pasted onto a target example.  img_t, img_s, img_out: (S,S,3)
 * NHWC fp32; masks_t (Gt,S,S), masks_s (Gs,S,S) uint8, a byte other than 0 counts as set; idx (K)
 * int32, clamped to [0, Gs) on the device, so no read leaves masks_s whatever it holds.
 *   alpha             = OR over k of masks_s[idx[k]]
 *   img_out           = alpha ? img_s : img_t      a select of 32-bit patterns, never a blend:
 *                                                  nothing of the unselected image reaches the output
 *   masks_out[g]      = masks_t[g] & ~alpha        g < Gt
 *   masks_out[Gt + k] = masks_s[idx[k]]            k < K, written as {0,1}
 * box (Gt+K,4) / area (Gt+K) int32: mrcnn_mask_resize_crop's convention for masks_out.  Every
 * byte of img_out, masks_out, box and area is written.  Workspace: row_stats (Gt+K,S,3) int32.
 * Two launches on the stream (masks and image, each workgroup with the alpha of its own rows one
 * bit per pixel in LDS; boxes), integers only on the mask side, no atomics.  K = 0, Gt = 0 and
 * Gt + K = 0 are legal (the image is still written); a pointer may be null only where its count
 * is 0.  K <= Gs, (Gt+K)*S*S < 2^31, and no output or workspace may overlap an input or another
 * output (img_out == img_t is refused).  The reference has no copy-paste augmentation
 * (chainer_mask_rcnn/datasets/transforms.py:10-51 transforms one example at a time). */
int mrcnn_copy_paste(const float *img_t, const float *img_s, const uint8_t *masks_t, int Gt,
                     const uint8_t *masks_s, int Gs, const int32_t *idx, int K, int S,
                     float *img_out, uint8_t *masks_out, int32_t *box, int32_t *area,
                     int32_t *row_stats, void *stream);

/* ---- Ignore regions of the train step (csrc/ignore_regions.hip) --------
 * A region that training must neither reward nor punish (a COCO `iscrowd` annotation) travels as
 * ONE bit plane of the network-size image, in the "Packed masks" format above.  Replaces the crowd
 * filter of Detectron (roidb.py `_filter_crowd_proposals`: host box overlaps against the crowd
 * BOXES); the reference (chainer_mask_rcnn/datasets/coco/coco_instance_segm.py, use_crowd=False)
 * drops crowd annotations before training sees them. */
/* plane (H,Wq) uint64, Wq = ceil(W/64), pad bits zero.
 * U = OR over g of (masks[g] != 0), masks (G,H,W) uint8.
 * base == NULL: plane = U.   base != NULL: plane = base & ~U   (base (H,Wq), may not alias plane;
 * its pad bits are cleared too).  Every word of plane is written.  G == 0: U is empty (plane = 0,
 * or a copy of base; masks may then be NULL).  H * W < 2^31. */
int mrcnn_mask_union_pack(const uint8_t *masks, int G, int H, int W, const uint64_t *base,
                          uint64_t *plane, void *stream);
/* out (n,2) int32 = (covered, area) per box.  boxes (n,4) float32 (y1,x1,y2,x2).
 * Integer rectangle: each coordinate rounded half to even (np.round, as mrcnn_mask_targets
 * rounds), then y clamped to [0,H] and x to [0,W]; rows [y0,y1) and columns [x0,x1).
 * area = max(y1-y0,0) * max(x1-x0,0);  covered = number of set bits of plane in the rectangle.
 * A box with a non-finite coordinate gives (0,0); the clamp is applied in float before the
 * conversion, so no coordinate overflows an int.  Only words of plane inside the clamped rectangle
 * are read.  out is 8-byte aligned (each row is one store).  n == 0 returns without a launch.
 * H * W < 2^31. */
int mrcnn_box_coverage(const uint64_t *plane, int H, int W, const float *boxes, int n,
                       int32_t *out, void *stream);

/* ---- COCO polygons -> packed masks (csrc/polygon_raster.hip) ----------
 * Ground-truth polygons drawn by COCO's own rule — pycocotools maskApi.c rleFrPoly: vertices
 * upsampled by 5, a dense walk of each edge, crossings of pixel-column centres, an even-odd fill
 * down each column — straight into the "Packed masks" format above, so that a polygon crosses
 * PCIe as its vertices and the mask never exists on the host.  The reference draws polygons with
 * PIL.ImageDraw (chainer_mask_rcnn/datasets/coco.py:136-143), which is a different rule. */
/* Scratch of mrcnn_polygon_rasterize for G instances of an H x W image (one record per instance
 * and 64-column strip), in bytes; 0 when G, H or W is not positive. */
int64_t mrcnn_polygon_rasterize_workspace_bytes(int G, int H, int W);
/* G instances, each the UNION of its rings (a ring by itself is filled even-odd).  xy5 (V,2)
 * int32: the rings' vertices (x, y) one ring after another, already upsampled as maskApi.c does,
 * X = (int)(5.0 * x + .5) in doubles, |X| < 2^30; ring_off (R+1) int32: ring r owns vertices
 * ring_off[r] .. ring_off[r+1]; inst_off (G+1) int32: instance g owns rings inst_off[g] ..
 * inst_off[g+1].  Both offset arrays are taken on trust (non-decreasing, from 0, ending at R and
 * V): they bound reads only; every write is bounded by G, H and W.  A ring of fewer than 3
 * vertices sets nothing; an instance may have no rings.  All arrays are device pointers; xy5 may
 * be null when V = 0.
 * Outputs: packed (G,H,Wq) — every word is written, pad bits are zero; area (G) exact; extent
 * (G,4) tight (y_lo, y_hi, wq_lo, wq_hi), (H, 0, Wq, 0) for an empty mask as mrcnn_mask_pack
 * leaves it; box (G,4) int32 the tight (y1, x1, y2, x2), half-open, zeros for an empty mask
 * (mrcnn_mask_resize_crop's convention, the dataset's mask_to_bbox).  ws: mrcnn_polygon_rasterize_workspace_bytes(G, H, W) bytes, 4-byte
 * aligned.  Two launches on the stream; LDS atomics and integer reductions only: the outputs are
 * exact and identical run to run.  Replaces pycocotools.mask.frPyObjects + merge + decode (packed),
 * area (area) and toBbox (box).  G == 0 returns without a launch.  H <= 4000 (a strip keeps two
 * H-word arrays in LDS), H * W < 2^31, G * Wq < 2^31; R and V are bounded by int32 only. */
int mrcnn_polygon_rasterize(const int32_t *xy5, const int32_t *ring_off, const int32_t *inst_off,
                            int G, int H, int W, uint64_t *packed, int32_t *area, int32_t *extent,
                            int32_t *box, void *ws, void *stream);

/* ---- Gradient exchange over RCCL / xGMI ---------------------------------------------- */
/* Replaces ChainerMN's communicator as the reference uses it
 * (examples/train_common.py:97-103 `chainermn.create_communicator('hierarchical')`, :178
 * `create_multi_node_optimizer`): bcast_data of the model before the first update and
 * allreduce_grad before every update.  One communicator per process (= per GPU).  RCCL
 * (ncclComm_t) is resolved at run time from the librccl.so already loaded into the process.
 * Collectives run on the communicator's OWN high-priority HIP stream, ordered against the
 * caller's streams with events only, so a bucket overlaps with the backward still running.
 *
 *   rank 0:   mrcnn_allreduce_unique_id(id)  -> 128 bytes, handed to every rank by the launcher
 *   all:      mrcnn_allreduce_init(id, rank, world, &comm)       (collective)
 *   per step: mrcnn_allreduce_bucket(comm, grads + lo, hi - lo, bucket, compute, side) ...
 *             mrcnn_allreduce_wait(comm, compute)  then the SGD launch (grad_scale = 1/world)
 */
#define MRCNN_COMM_ID_BYTES 128
int mrcnn_allreduce_unique_id(void *id128);
int mrcnn_allreduce_init(const void *id128, int rank, int world, void **comm);
int mrcnn_allreduce_destroy(void *comm);
/* rank / world of the communicator, RCCL version code, and which librccl was bound. */
int mrcnn_allreduce_info(void *comm, int *rank, int *world, int *rccl_version,
                         char *library, int library_len);
/* In-place SUM over ranks of buf[0..count) fp32, queued on the collective stream AFTER
 * everything queued so far on after_stream and (if non-NULL) after_stream2 — the compute
 * stream and the weight-gradient side stream.  bucket_id only labels the timing records. */
int mrcnn_allreduce_bucket(void *comm, float *buf, int64_t count, int bucket_id,
                           void *after_stream, void *after_stream2);
/* `stream` waits (device side) for every collective queued so far. */
int mrcnn_allreduce_wait(void *comm, void *stream);
/* rank `root`'s bytes to all ranks; ordered after and before `after_stream`. */
int mrcnn_allreduce_broadcast(void *comm, void *buf, int64_t bytes, int root,
                              void *after_stream);
/* HIP-event timing of the collectives: enable clears the records; bucket_times sums them
 * (bucket_id -1 = all) after the caller synchronised the device. */
int mrcnn_allreduce_timing(void *comm, int enable);
int mrcnn_allreduce_bucket_times(void *comm, int bucket_id, double *total_ms,
                                 double *total_bytes, int64_t *launches);

#ifdef __cplusplus
}
#endif
#endif /* MRCNN_HIP_H_ */
