// Implicit-GEMM convolution family on MFMA for gfx950 (NHWC / KRSC), fp32 in / out.
//
// Replaces every cuDNN call the reference makes through chainer's
// L.Convolution2D / L.Deconvolution2D / L.Linear and their backward passes
// (call sites /root/reference/chainer_mask_rcnn/models/region_proposal_network.py:75-80,
// models/mask_rcnn_resnet.py:131-143, chainer ResNet50Layers via
// models/resnet_extractor.py:93), plus the AffineChannel2D + residual + ReLU that
// follow each conv inside chainer's BottleneckA/B (fused into the epilogue here).
//
// One kernel body, three operand-gather modes:
//   FWD    y[m, k]   = sum_{r,s,c} x[pix(m,r,s), c] * w[k, r, s, c]
//   DGRAD  gx[m, c]  = sum_{r,s,k} gy[pix'(m,r,s), k] * w[k, r, s, c]
//   WGRAD  gw[k, rsc] = sum_m gy[m, k] * x[pix(m,r,s), c]      (split over m)
// Two arithmetics, both fp32 in / fp32 out / fp32 accumulate and fp32-roundoff-close to a CPU
// fp32 GEMM (there is no TF32 / xf32 on gfx950):
//   SPLIT (default, "split_bf16" knob): every operand element is staged as three bf16 values
//     whose sum is the element exactly, six v_mfma_f32_32x32x16_bf16 per 16-deep K step (see
//     SPLIT in conv_gemm_kernel.h); forward form 128x128 / 64x64 and the 128x128 weight gradient.
//   fp32 MFMA: v_mfma_f32_32x32x2_f32 (157 TF/s peak) — every other instantiation, and all of
//     them with split_bf16 = 0.
//   Below SPLIT, on request ("split_planes" knob, NP in the kernel's note): the same kernels staging
//     two planes and issuing three of the six products (16-bit-class operands), or one plane and
//     one product (bf16 operands); fp32 accumulate and fp32 in / out as ever.
// The description below is the fp32-MFMA body; the SPLIT instantiations replace its stage
// layout and its inner product loop only.
//
// Tiling (wave64): 256 threads = 2x2 waves, each wave owns TM x TN MFMA tiles of
// 32x32 (TM=TN=2 -> 128x128 block tile; TM=TN=1 -> 64x64 for small problems).
// K is consumed in 32-deep slices staged global -> registers -> LDS
// (double-buffered, one barrier per slice).  Operands whose K index is
// contiguous in memory sit in LDS as [row][32+4] and are fetched with one
// ds_read_b128 per 4 MFMAs; operands whose K index is the strided one sit as
// [k][row] and are fetched with conflict-free ds_read_b32.  Inside an 8-deep
// K block MFMA step t pairs k = 4*half + t of both operands (any pairing is
// valid as long as A and B agree).
#include <algorithm>
#include <cstring>

#include "conv_gemm_kernel.h"

namespace {

__global__ void splitk_reduce_kernel(const float *__restrict__ ws, int splits, int64_t n,
                                     int64_t stride, float *__restrict__ out)
{
    const int64_t nv = n / 4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv;
         i += (int64_t)gridDim.x * blockDim.x) {
        float4 a = reinterpret_cast<const float4 *>(ws)[i];
        int s = 1;
        // four slab loads in flight per step; the additions keep the slab order
        for (; s + 4 <= splits; s += 4) {
            const float4 v0 = reinterpret_cast<const float4 *>(ws + (s + 0) * stride)[i];
            const float4 v1 = reinterpret_cast<const float4 *>(ws + (s + 1) * stride)[i];
            const float4 v2 = reinterpret_cast<const float4 *>(ws + (s + 2) * stride)[i];
            const float4 v3 = reinterpret_cast<const float4 *>(ws + (s + 3) * stride)[i];
            a.x += v0.x; a.y += v0.y; a.z += v0.z; a.w += v0.w;
            a.x += v1.x; a.y += v1.y; a.z += v1.z; a.w += v1.w;
            a.x += v2.x; a.y += v2.y; a.z += v2.z; a.w += v2.w;
            a.x += v3.x; a.y += v3.y; a.z += v3.z; a.w += v3.w;
        }
        for (; s < splits; ++s) {
            const float4 v = reinterpret_cast<const float4 *>(ws + s * stride)[i];
            a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
        }
        reinterpret_cast<float4 *>(out)[i] = a;
    }
}

GemmKnobs g_knobs;     // mrcnn_set_tuning

// what the policy reads of a problem run in `mode`
inline GemmShape gemm_shape(const GemmParams &p, int mode, bool has_ws)
{
    GemmShape g = {};
    g.mode = mode;
    g.M = p.M; g.N = p.N; g.Kc = p.Kc;
    g.R = p.R; g.S = p.S; g.stride = p.stride; g.pad = p.pad;
    g.gp = p.gp; g.gq = p.gq; g.sh = p.sh; g.sw = p.sw;
    g.ldc = p.ldc; g.out_mode = p.out_mode; g.stem = p.stem; g.perm_n = p.perm_n;
    g.has_ws = has_ws;
    return g;
}

template <int TM, int TN, int MODE>
void launch_kernel(const GemmParams &p, GemmInst inst, int64_t tiles, int splits, hipStream_t s, int batch = 1)
{
    hipEvent_t ev0, ev1;          // kernel-only timing (ProfKernelScope of the caller), usually null
    mrcnn::prof_take(&ev0, &ev1);
    auto go = [&](auto kernel) {
        hipExtLaunchKernelGGL(kernel, dim3((unsigned)tiles, splits, batch), dim3(256), 0, s, ev0, ev1, 0, p);
    };
    if constexpr (TM == TN && ((MODE == WGRAD && TM == 2) || (MODE == FWD && (TM == 1 || TM == 2)))) {
        if (inst.split) {
            // one and two planes: the instantiations of conv_gemm_planes.hip
            const dim3 grid((unsigned)tiles, splits, batch);
            if (inst.planes == 1) return launch_planes<1>(p, 64 * TM, MODE, inst.variant, grid, s, ev0, ev1);
            if (inst.planes == 2) return launch_planes<2>(p, 64 * TM, MODE, inst.variant, grid, s, ev0, ev1);
            if constexpr (MODE == FWD) {
                if (inst.variant == INST_PW) return go(conv_gemm_kernel<TM, TN, MODE, false, 3, false, true>);
                if (inst.variant == INST_K3) return go(conv_gemm_kernel<TM, TN, MODE, false, 3, false, false, true>);
            }
            return go(conv_gemm_kernel<TM, TN, MODE, false, 3>);
        }
    }
    if constexpr (MODE == WGRAD) {
        if (inst.variant == INST_WPERM) return go(conv_gemm_kernel<TM, TN, MODE, true>);
    }
    go(conv_gemm_kernel<TM, TN, MODE>);
}

// a batched launch of conv_winograd.h: the 36 per-frequency problems in grid z, on the instantiation its
// plan (plan_wino_gemm / plan_wino_wgrad) picked
template <int TM, int TN, int MODE>
void launch_wino_kernel(const GemmParams &p, const GemmLaunch &l, hipStream_t s)
{
    launch_kernel<TM, TN, MODE>(p, l.inst, l.grid_x, l.grid_y, s, kWinoXi);
}

// ---- W8 launches (see the note above conv_gemm_kernel) -------------------------------------------
// (planes: the plan's; three on the Winograd launches of conv_winograd.h: the transforms amplify operand
// rounding, and six products on 36 / 16 of the outputs are already less matrix work than three on nine taps)
void launch_w8_kernel(const GemmParams &p, int64_t wgs, int batch, hipStream_t s, int planes = 3)
{
    hipEvent_t ev0, ev1;
    mrcnn::prof_take(&ev0, &ev1);
    const dim3 grid((unsigned)wgs, 1, batch);
    if (planes == 1) return launch_planes<1>(p, kW8BM, FWD, INST_W8, grid, s, ev0, ev1);
    if (planes == 2) return launch_planes<2>(p, kW8BM, FWD, INST_W8, grid, s, ev0, ev1);
    hipExtLaunchKernelGGL((conv_gemm_kernel<2, 2, FWD, false, 3, true>), grid, dim3(512), 0, s, ev0, ev1, 0, p);
}

// Profiler record of launch l of a problem: the operation and byte estimate of its rows, and the
// bucket of the kernel SYMBOL (what rocprofv3 reports): the forward-form instantiation runs forward
// convolutions and the transposed-filter dgrads alike
template <int MODE>
mrcnn::ProfKernelScope gemm_prof(const GemmParams &p, const GemmLaunch &l)
{
    const int small = l.tile >= 128 ? 0 : 1;
    if (MODE == WGRAD)
        return mrcnn::ProfKernelScope(mrcnn::PROF_CONV_WGRAD_128 + small, 2.0 * p.M * p.N * (double)p.Kc,
                                      4.0 * ((double)p.M * p.N + (double)p.Kc * (p.M + (double)p.cin)));
    const int64_t rows = l.m_hi - l.m_lo;
    const double kdepth = (double)p.R * p.S * (p.stem ? 21.0 : (double)p.Kc);
    const double flops = 2.0 * rows * p.N * kdepth;
    const double bytes = 4.0 * ((double)rows * p.N + (double)rows * p.Kc + (double)p.N * kdepth);
    const int kind = l.tile == kW8BM ? mrcnn::PROF_CONV_FWD_W8
                                     : (MODE == FWD ? mrcnn::PROF_CONV_FWD_128 : mrcnn::PROF_CONV_DGRAD_128) + small;
    return mrcnn::ProfKernelScope(kind, flops, bytes);
}

// ---- the ordered slab sum of the split-K launches (conv_gemm_plan.h) ------------------------
struct FixParams {
    const float *ws;
    float *C;
    const float *bias, *scale, *shift, *residual, *res_g, *res_y, *out_mask_y;
    int splits, rows, N, row0, ldc, flags;
    int perm_n, pq;      // position-major GEMM rows (see GemmParams::perm_n), positions per image
    int64_t stride;
};

__global__ void __launch_bounds__(256) splitk_epilogue_kernel(const FixParams f)
{
    const int n4 = f.N / 4;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)f.rows * n4) return;
    const int r = (int)(i / n4), c = (int)(i - (int64_t)r * n4) * 4;
    float4 a = *reinterpret_cast<const float4 *>(f.ws + (int64_t)r * f.N + c);
    for (int s = 1; s < f.splits; ++s) {
        const float4 v = *reinterpret_cast<const float4 *>(f.ws + s * f.stride + (int64_t)r * f.N + c);
        a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
    float v[4] = {a.x, a.y, a.z, a.w};
    int orow = f.row0 + r;
    if (f.perm_n > 0) {
        const PermRow pr = perm_row(orow, f.pq);
        if (pr.n >= f.perm_n) return;            // padding row of the last image block
        orow = pr.n * f.pq + pr.pos;
    }
    const int64_t off = (int64_t)orow * f.ldc + c;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float x = v[k];
        if (f.flags & MRCNN_EPI_BIAS) x += f.bias[c + k];
        if (f.flags & MRCNN_EPI_AFFINE) x = x * f.scale[c + k] + (f.shift ? f.shift[c + k] : 0.f);
        if (f.flags & MRCNN_EPI_RESIDUAL) x += f.residual[off + k];
        if (f.flags & MRCNN_EPI_ACCUM) x += f.C[off + k];
        if (f.res_g) x += (!f.res_y || f.res_y[off + k] > 0.f) ? f.res_g[off + k] : 0.f;
        if (f.flags & MRCNN_EPI_RELU) x = fmaxf(x, 0.f);
        if (f.out_mask_y) x = f.out_mask_y[off + k] > 0.f ? x : 0.f;
        v[k] = x;
    }
    *reinterpret_cast<float4 *>(f.C + off) = make_float4(v[0], v[1], v[2], v[3]);
}

// The ordered sum of the `splits` slabs of p.split_ws that hold rows [rows_lo, p.M), with p's
// epilogue, into p.C
template <int MODE>
void slab_sum(const GemmParams &p, int rows_lo, int splits, hipStream_t s)
{
    const int rows = p.M - rows_lo;
    FixParams f = {};
    f.ws = p.split_ws; f.C = p.C;
    f.bias = p.bias; f.scale = p.scale; f.shift = p.shift; f.residual = p.residual;
    f.res_g = p.res_g; f.res_y = p.res_y; f.out_mask_y = p.out_mask_y;
    f.splits = splits; f.rows = rows; f.N = p.N; f.row0 = rows_lo; f.ldc = p.ldc;
    f.flags = p.flags; f.stride = (int64_t)rows * p.N;
    f.perm_n = MODE == FWD ? p.perm_n : 0; f.pq = p.gp * p.gq;
    const int64_t n = (int64_t)rows * (p.N / 4);
    hipLaunchKernelGGL(splitk_epilogue_kernel, dim3((unsigned)mrcnn::ceil_div(n, 256)), dim3(256), 0, s, f);
}

// Runs `plan` on problem p (p.M = all rows, p.split_ws = the workspace the plan was made with; WGRAD:
// p.C = gw): per launch the row range, the slab or tail fields and the profiler record, then the
// ordered slab sum.
template <int MODE>
int run_plan(const GemmParams &p, const GemmPlan &plan, hipStream_t s)
{
    for (int i = 0; i < plan.n; ++i) {
        const GemmLaunch &l = plan.launch[i];
        GemmParams q = p;
        q.m_lo = l.m_lo;
        q.M = l.m_hi;
        if constexpr (MODE == WGRAD) {
            q.perm_n = plan.perm_n;
            q.split_len = l.split_len;
            q.split_stride = (int64_t)p.M * p.N;
            q.C = plan.sum_splits ? p.split_ws : p.C;
            q.split_ws = nullptr;
        } else if (l.split_len) {      // raw partial sums into slabs of the workspace
            q.C = p.split_ws;
            q.flags = 0;
            q.bias = q.scale = q.shift = q.residual = q.res_g = q.res_y = q.out_mask_y = nullptr;
            q.split_len = l.split_len;
            q.split_stride = (int64_t)(l.m_hi - l.m_lo) * p.N;
            q.out_row0 = l.m_lo;
            q.c_bytes = (unsigned)(q.split_stride * 4);
        }
        if (l.tail_splits) {
            q.tail_first = l.tail_first;
            q.tail_row0 = l.tail_row0;
            q.tail_splits = l.tail_splits;
            q.tail_split_len = l.tail_split_len;
            q.tail_ws = p.split_ws;
            q.tail_stride = (int64_t)(l.m_hi - l.tail_row0) * p.N;
            q.tail_bytes = (unsigned)(q.tail_stride * 4);
        }
        const auto prof = gemm_prof<MODE>(p, l);
        if (l.tile == kW8BM) {
            if constexpr (MODE == FWD) launch_w8_kernel(q, l.grid_x, 1, s, l.inst.planes);
        } else if (l.tile == 128) {
            launch_kernel<2, 2, MODE>(q, l.inst, l.grid_x, l.grid_y, s);
        } else {
            launch_kernel<1, 1, MODE>(q, l.inst, l.grid_x, l.grid_y, s);
        }
    }
    if constexpr (MODE == WGRAD) {
        // (Summing the slabs in the last-arriving workgroup of each tile instead was measured 4 ms per
        // train step slower: the agent-scope release every workgroup needs before it signals writes
        // back its XCD's whole dirty L2.)
        if (plan.sum_splits) {
            const int64_t gwsz = (int64_t)p.M * p.N;
            const int64_t blocks = mrcnn::ceil_div(gwsz / 4, 256);   // one float4 per thread
            hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, s,
                               (const float *)p.split_ws, plan.sum_splits, gwsz, gwsz, p.C);
        }
        return mrcnn::check_launch("conv_wgrad");
    } else {
        if (plan.sum_splits) slab_sum<MODE>(p, plan.sum_row0, plan.sum_splits, s);
        return mrcnn::check_launch("conv_gemm");
    }
}

// a forward-form / DGRAD problem under the policy of conv_gemm_plan.h
template <int MODE>
int launch(const GemmParams &p, hipStream_t s)
{
    return run_plan<MODE>(p, plan_gemm(gemm_shape(p, MODE, p.split_ws != nullptr), g_knobs), s);
}

int check_desc(const mrcnn_conv_desc *d)
{
    MRCNN_REQUIRE(d, "conv: null descriptor");
    MRCNN_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->C > 0 && d->K > 0 && d->R > 0 && d->S > 0 &&
                      d->stride > 0 && d->pad >= 0,
                  "conv: bad descriptor");
    MRCNN_REQUIRE(d->P == (d->H + 2 * d->pad - d->R) / d->stride + 1 &&
                      d->Q == (d->W + 2 * d->pad - d->S) / d->stride + 1,
                  "conv: output size (%d,%d) inconsistent with input (%d,%d) k=%d s=%d p=%d", d->P,
                  d->Q, d->H, d->W, d->R, d->stride, d->pad);
    MRCNN_REQUIRE(d->C % 4 == 0 && d->K % 4 == 0,
                  "conv: channel counts must be multiples of 4 (C=%d K=%d)", d->C, d->K);
    MRCNN_REQUIRE((int64_t)d->N * d->H * d->W * d->C < (int64_t)INT32_MAX &&
                      (int64_t)d->N * d->P * d->Q * d->K < (int64_t)INT32_MAX,
                  "conv: tensor exceeds 2^31 elements");
    return 0;
}

inline bool aligned16(const void *p) { return ((uintptr_t)p % 16) == 0; }

// buffer extents in floats -> bytes; 32-bit buffer offsets need every tensor < 2 GiB
int set_extents(GemmParams &p, int64_t a_floats, int64_t b_floats, int64_t c_floats)
{
    const int64_t lim = (int64_t)1 << 29;
    MRCNN_REQUIRE(a_floats < lim && b_floats < lim && c_floats < lim,
                  "conv: a tensor exceeds 2 GiB (%lld / %lld / %lld floats); split the batch",
                  (long long)a_floats, (long long)b_floats, (long long)c_floats);
    p.a_bytes = (unsigned)(a_floats * 4);
    p.b_bytes = (unsigned)(b_floats * 4);
    p.c_bytes = (unsigned)(c_floats * 4);
    return 0;
}

// ---- descriptor -> problem ------------------------------------------------------------------------
// The shape half of every entry point: the descriptor checks and every field of a zero-initialised
// GemmParams but the pointers and the epilogue flags, which the entry point checks and sets before it
// launches.  mrcnn_conv_gemm_plan plans the same problems without a pointer.

int fwd_problem(const mrcnn_conv_desc *d, GemmParams &p)
{
    if (int rc = check_desc(d)) return rc;
    p.M = d->N * d->P * d->Q; p.N = d->K; p.Kc = d->C;
    p.gp = d->P; p.gq = d->Q; p.sh = d->H; p.sw = d->W;
    p.R = d->R; p.S = d->S; p.stride = d->stride; p.pad = d->pad;
    p.lda = d->C; p.ldb = d->R * d->S * d->C; p.ldc = d->K;
    p.out_mode = OUT_PLAIN;
    p.perm_n = choose_perm(g_knobs, d->N, d->P, d->Q, d->R, d->S, d->stride, d->pad);
    if (p.perm_n) p.M = (int)(mrcnn::ceil_div(d->N, kPermBlock) * kPermBlock) * d->P * d->Q;
    return set_extents(p, (int64_t)d->N * d->H * d->W * d->C, (int64_t)d->K * d->R * d->S * d->C,
                       (int64_t)d->N * d->P * d->Q * d->K);
}

// Stem: conv1 7x7/2 pad 3 of chainer ResNet50Layers on an input
// padded to 4 channels; filter given as (K, 7, 8, 4) with zeros at s=7 / c=3.
int stem_problem(int N, int H, int W, int K, GemmParams &p)
{
    MRCNN_REQUIRE(N > 0 && H > 0 && W > 0 && K > 0 && K % 4 == 0, "conv_stem: bad shape");
    const int P = (H + 6 - 7) / 2 + 1, Q = (W + 6 - 7) / 2 + 1;
    p.M = N * P * Q; p.N = K; p.Kc = 32;
    p.gp = P; p.gq = Q; p.sh = H; p.sw = W;
    p.R = 7; p.S = 1; p.stride = 2; p.pad = 3;
    p.lda = 4; p.ldb = 7 * 32; p.ldc = K;
    p.out_mode = OUT_PLAIN; p.stem = 1;
    return set_extents(p, (int64_t)N * H * W * 4, (int64_t)K * 7 * 32, (int64_t)N * P * Q * K);
}

// K-strided data gradient; fused_grad: the call has a residual gradient or an output mask
int dgrad_problem(const mrcnn_conv_desc *d, bool fused_grad, GemmParams &p)
{
    if (int rc = check_desc(d)) return rc;
    MRCNN_REQUIRE(!fused_grad || d->stride == 1,
                  "conv2d_dgrad: residual gradient / output mask need stride 1");
    p.N = d->C; p.Kc = d->K; p.cin = d->C;
    p.R = d->R; p.S = d->S; p.pad = d->pad;
    p.lda = d->K; p.ldb = d->R * d->S * d->C; p.ldc = d->C;
    p.sh = d->P; p.sw = d->Q;
    if (d->stride == 1) {
        p.M = d->N * d->H * d->W; p.gp = d->H; p.gq = d->W; p.stride = 1;
        p.out_mode = OUT_PLAIN;
    } else {
        MRCNN_REQUIRE(d->R == 1 && d->S == 1 && d->pad == 0,
                      "conv2d_dgrad: stride>1 is implemented for 1x1/pad0 (the only strided "
                      "trainable convs of ResNet-C4) and the 2x2/2 adjoint (deconv entry points)");
        p.M = d->N * d->P * d->Q; p.gp = d->P; p.gq = d->Q; p.stride = d->stride;
        p.out_mode = OUT_STRIDED; p.oh = d->H; p.ow = d->W;
    }
    return set_extents(p, (int64_t)d->N * d->P * d->Q * d->K, (int64_t)d->K * d->R * d->S * d->C,
                       (int64_t)d->N * d->H * d->W * d->C);
}

// Data gradient as a forward-form convolution of gy with wT = flip-transpose(w) (C,R,S,K): both
// operands are K-contiguous (ds_read_b128 fragments, coalesced filter rows).
// 1x1 / pad 0 strided convolution: every output pixel of the convolution sends its gradient to ONE
// input pixel — the same forward-form GEMM on the transposed filter, its rows (the convolution's
// output pixels) scattered to the strided positions of a zero-filled gx (OUT_STRIDED in the
// per-element epilogue).
int dgrad_wt_problem(const mrcnn_conv_desc *d, bool fused_grad, GemmParams &p)
{
    if (int rc = check_desc(d)) return rc;
    const bool strided = d->stride > 1;
    MRCNN_REQUIRE(!strided || (d->R == 1 && d->S == 1 && d->pad == 0),
                  "conv2d_dgrad_wt: stride > 1 is implemented for 1x1 / pad 0 filters");
    MRCNN_REQUIRE(!strided || !fused_grad, "conv2d_dgrad_wt: residual gradient / output mask need stride 1");
    p.N = d->C; p.Kc = d->K;
    p.sh = d->P; p.sw = d->Q;
    p.R = d->R; p.S = d->S; p.stride = 1; p.pad = d->R - 1 - d->pad;
    p.lda = d->K; p.ldb = d->R * d->S * d->K; p.ldc = d->C;
    if (strided) {
        p.gp = d->P; p.gq = d->Q; p.ostride = d->stride;
        p.out_mode = OUT_STRIDED; p.oh = d->H; p.ow = d->W;
    } else {
        p.gp = d->H; p.gq = d->W;
        p.out_mode = OUT_PLAIN;
        p.perm_n = choose_perm(g_knobs, d->N, d->H, d->W, d->R, d->S, 1, p.pad);
    }
    p.M = d->N * p.gp * p.gq;
    if (p.perm_n) p.M = (int)(mrcnn::ceil_div(d->N, kPermBlock) * kPermBlock) * d->H * d->W;
    MRCNN_REQUIRE(d->S - 1 - d->pad == p.pad, "conv2d_dgrad_wt: square filters / symmetric padding only");
    return set_extents(p, (int64_t)d->N * d->P * d->Q * d->K, (int64_t)d->K * d->R * d->S * d->C,
                       (int64_t)d->N * d->H * d->W * d->C);
}

// Weight gradient gw[k, rsc] = sum over the pixels: M = K rows, N = R S C columns.  `shape` gets what
// plan_wgrad() reads beside the GemmParams fields.
int wgrad_problem(const mrcnn_conv_desc *d, GemmParams &p, GemmShape &shape)
{
    const int64_t pixels = (int64_t)d->N * d->P * d->Q;
    p.M = d->K; p.N = d->R * d->S * d->C; p.Kc = (int)pixels;
    p.gp = d->P; p.gq = d->Q; p.sh = d->H; p.sw = d->W;
    p.R = d->R; p.S = d->S; p.stride = d->stride; p.pad = d->pad;
    p.lda = d->C; p.ldg = d->K; p.cin = d->C; p.ldc = d->R * d->S * d->C;
    shape = gemm_shape(p, WGRAD, false);
    shape.pixels = pixels; shape.n_img = d->N; shape.C = d->C;
    return set_extents(p, pixels * d->K, (int64_t)d->N * d->H * d->W * d->C, (int64_t)d->K * d->R * d->S * d->C);
}

// ---- Deconvolution 2x2 stride 2 (= adjoint of a 2x2/2 convolution g: (N,2H,2W,K) -> (N,H,W,C)
//      with KRSC filter w (C,2,2,K)) -----------------------------------------------------------
inline mrcnn_conv_desc deconv_adjoint_desc(int N, int H, int W, int C, int K)
{
    return {N, 2 * H, 2 * W, K, C, 2, 2, 2, 0, H, W};
}

// The deconvolution forward as a 1x1 GEMM whose output columns (a, b, o) are scattered by the
// pixel-shuffle map of the epilogue: y[n, 2y + a, 2x + b, o] = sum_c x[n, y, x, c] w[c; (a, b, o)].
// wt = false: filter w (C, 4K), the K-strided DGRAD form (fp32 MFMA); wt = true: FORWARD form on the
// transposed filter wT (4K, C) — both operands K-contiguous, i.e. the split-operand kernels.
int deconv_problem(bool wt, int N, int H, int W, int C, int K, GemmParams &p)
{
    MRCNN_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && K > 0 && C % 4 == 0 && K % 4 == 0,
                  "%s: bad shape", wt ? "deconv_fwd_wt" : "deconv_fwd");
    p.M = N * H * W; p.N = 4 * K; p.Kc = C; p.cin = wt ? 0 : 4 * K;
    p.gp = H; p.gq = W; p.sh = H; p.sw = W;
    p.R = 1; p.S = 1; p.stride = 1; p.pad = 0;
    p.lda = C; p.ldb = wt ? C : 4 * K; p.ldc = K;
    p.out_mode = OUT_DECONV; p.ko = K;
    return set_extents(p, (int64_t)N * H * W * C, (int64_t)C * 4 * K, (int64_t)N * 4 * H * W * K);
}

int deconv_fwd(bool wt, const float *x, const float *w, const float *bias, float *y, int N, int H, int W,
               int C, int K, int epi_flags, void *stream)
{
    const char *who = wt ? "deconv_fwd_wt" : "deconv_fwd";
    GemmParams p = {};
    if (int rc = deconv_problem(wt, N, H, W, C, K, p)) return rc;
    MRCNN_REQUIRE(x && w && y, "%s: null pointer", who);
    MRCNN_REQUIRE(aligned16(x) && aligned16(w), "%s: x/%s must be 16-byte aligned", who, wt ? "wT" : "w");
    MRCNN_REQUIRE((epi_flags & ~(MRCNN_EPI_BIAS | MRCNN_EPI_RELU)) == 0, "%s: bad flags", who);
    MRCNN_REQUIRE(!(epi_flags & MRCNN_EPI_BIAS) || bias, "%s: bias flag without bias", who);
    p.A = x; p.B = w; p.C = y; p.bias = bias;
    p.flags = epi_flags;
    return wt ? launch<FWD>(p, mrcnn::as_stream(stream)) : launch<DGRAD>(p, mrcnn::as_stream(stream));
}

int wgrad_run(const mrcnn_conv_desc *d, const float *gy, const float *x, float *gw, void *ws,
              const float *out_row_scale, void *stream)
{
    GemmParams p = {};
    GemmShape shape;
    if (int rc = wgrad_problem(d, p, shape)) return rc;
    p.A = gy; p.B = x; p.C = gw;
    p.scale = out_row_scale;
    p.split_ws = (float *)ws;
    shape.has_ws = ws != nullptr;
    return run_plan<WGRAD>(p, plan_wgrad(shape, g_knobs), mrcnn::as_stream(stream));
}

extern float g_wino_ambiguity;
int wino_check(const mrcnn_conv_desc *d, const char *who);      // conv_winograd.h

}  // namespace

extern "C" int64_t mrcnn_conv2d_split_workspace_bytes(void) { return kSplitWsBytes; }

extern "C" int mrcnn_set_tuning(const char *name, int value)
{
    MRCNN_REQUIRE(name != nullptr, "set_tuning: null name");
    MRCNN_REQUIRE(knob_value_ok(name, value), "set_tuning: split_planes must be 1, 2 or 3, got %d (it stays %d)",
                  value, g_knobs.split_planes);
    if (set_knob(g_knobs, name, value)) return 0;
    if (strcmp(name, "wino_ambiguity_ppb") == 0) {
        g_wino_ambiguity = 1e-9f * (float)value;
        return 0;
    }
    if (int rc = mrcnn::roi_align_set_tuning(name, value); rc >= 0) return rc;   // roi_fwd_lanes / roi_bwd_lanes
    MRCNN_REQUIRE(false, "set_tuning: unknown option '%s'", name);
    return 1;
}

extern "C" int mrcnn_conv2d_fwd(const mrcnn_conv_desc *d, const float *x, const float *w,
                                const float *bias, const float *scale, const float *shift,
                                const float *residual, float *y, int epi_flags, void *split_ws,
                                void *stream)
{
    GemmParams p = {};
    if (int rc = fwd_problem(d, p)) return rc;
    MRCNN_REQUIRE(x && w && y, "conv2d_fwd: null pointer");
    MRCNN_REQUIRE(aligned16(x) && aligned16(w), "conv2d_fwd: x/w must be 16-byte aligned");
    MRCNN_REQUIRE(!(epi_flags & MRCNN_EPI_BIAS) || bias, "conv2d_fwd: bias flag without bias");
    MRCNN_REQUIRE(!(epi_flags & MRCNN_EPI_AFFINE) || (scale && shift), "conv2d_fwd: affine flag without scale/shift");
    MRCNN_REQUIRE(!(epi_flags & MRCNN_EPI_RESIDUAL) || residual, "conv2d_fwd: residual flag without residual");
    p.A = x; p.B = w; p.C = y;
    p.bias = bias; p.scale = scale; p.shift = shift; p.residual = residual;
    p.flags = epi_flags;
    p.split_ws = (float *)split_ws;
    return launch<FWD>(p, mrcnn::as_stream(stream));
}

extern "C" int mrcnn_conv_stem_fwd(const float *x4, const float *w784, const float *bias,
                                   const float *scale, const float *shift, float *y, int N, int H,
                                   int W, int K, int epi_flags, void *stream)
{
    GemmParams p = {};
    if (int rc = stem_problem(N, H, W, K, p)) return rc;
    MRCNN_REQUIRE(x4 && w784 && y, "conv_stem: null pointer");
    MRCNN_REQUIRE(aligned16(x4) && aligned16(w784), "conv_stem: pointers must be 16-byte aligned");
    p.A = x4; p.B = w784; p.C = y;
    p.bias = bias; p.scale = scale; p.shift = shift;
    p.flags = epi_flags;
    return launch<FWD>(p, mrcnn::as_stream(stream));
}

extern "C" int mrcnn_conv2d_dgrad_ex(const mrcnn_conv_desc *d, const float *gy, const float *w,
                                     float *gx, int epi_flags, const float *res_g,
                                     const float *res_y, const float *out_mask_y,
                                     const float *out_scale, void *split_ws, void *stream)
{
    GemmParams p = {};
    if (int rc = dgrad_problem(d, res_g || out_mask_y, p)) return rc;
    MRCNN_REQUIRE(!res_y || res_g, "conv2d_dgrad: res_y without res_g");
    MRCNN_REQUIRE(gy && w && gx, "conv2d_dgrad: null pointer");
    MRCNN_REQUIRE(aligned16(gy) && aligned16(w), "conv2d_dgrad: gy/w must be 16-byte aligned");
    MRCNN_REQUIRE((epi_flags & ~MRCNN_EPI_ACCUM) == 0, "conv2d_dgrad: only MRCNN_EPI_ACCUM is valid");
    hipStream_t s = mrcnn::as_stream(stream);
    p.A = gy; p.B = w; p.C = gx;
    p.res_g = res_g; p.res_y = res_y; p.out_mask_y = out_mask_y; p.scale = out_scale;
    p.flags = epi_flags | (out_scale ? MRCNN_EPI_AFFINE : 0);
    p.split_ws = (float *)split_ws;
    if (p.out_mode == OUT_STRIDED && !(epi_flags & MRCNN_EPI_ACCUM))
        MRCNN_HIP_TRY(hipMemsetAsync(gx, 0, sizeof(float) * (size_t)d->N * d->H * d->W * d->C, s));
    return launch<DGRAD>(p, s);
}

extern "C" int mrcnn_conv2d_dgrad(const mrcnn_conv_desc *d, const float *gy, const float *w,
                                  float *gx, int epi_flags, void *stream)
{
    return mrcnn_conv2d_dgrad_ex(d, gy, w, gx, epi_flags, nullptr, nullptr, nullptr, nullptr, nullptr,
                                 stream);
}


namespace {
// wT[c][R-1-r][S-1-s][k] = w[k][r][s][c] * row_scale[k]
__global__ void filter_flip_transpose_kernel(const float *__restrict__ w, float *__restrict__ wT,
                                             int K, int RS, int C,
                                             const float *__restrict__ row_scale)
{
    __shared__ float tile[32][33];
    const int rs = blockIdx.z;
    const int k0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    for (int j = ty; j < 32; j += 8) {
        const int k = k0 + j, c = c0 + tx;
        tile[j][tx] = (k < K && c < C)
                          ? w[((int64_t)k * RS + rs) * C + c] * (row_scale ? row_scale[k] : 1.f)
                          : 0.f;
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
        const int c = c0 + j, k = k0 + tx;
        if (c < C && k < K) wT[((int64_t)c * RS + (RS - 1 - rs)) * K + k] = tile[tx][j];
    }
}

// up to 32 filters per launch: a ResNet stage needs ~14 of these five-microsecond transposes,
// launch latency dominates them
constexpr int kFlipBatch = 32;
struct FlipBatch {
    const float *w[kFlipBatch];
    float *wT[kFlipBatch];
    const float *scale[kFlipBatch];
    int K[kFlipBatch], RS[kFlipBatch], C[kFlipBatch];
    int first_block[kFlipBatch + 1];
    int n;
};

__global__ void filter_flip_transpose_batched_kernel(const FlipBatch b)
{
    __shared__ float tile[32][33];
    int l = 0;
    while (l + 1 < b.n && (int)blockIdx.x >= b.first_block[l + 1]) ++l;
    const int K = b.K[l], RS = b.RS[l], C = b.C[l];
    int blk = blockIdx.x - b.first_block[l];
    const int ncb = (C + 31) / 32, nkb = (K + 31) / 32;
    const int cb = blk % ncb;
    blk /= ncb;
    const int kb = blk % nkb, rs = blk / nkb;
    const float *__restrict__ w = b.w[l];
    float *__restrict__ wT = b.wT[l];
    const float *__restrict__ row_scale = b.scale[l];
    const int k0 = kb * 32, c0 = cb * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int j = ty; j < 32; j += 8) {
        const int k = k0 + j, c = c0 + tx;
        tile[j][tx] = (k < K && c < C)
                          ? w[((int64_t)k * RS + rs) * C + c] * (row_scale ? row_scale[k] : 1.f)
                          : 0.f;
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
        const int c = c0 + j, k = k0 + tx;
        if (c < C && k < K) wT[((int64_t)c * RS + (RS - 1 - rs)) * K + k] = tile[tx][j];
    }
}
}  // namespace

extern "C" int mrcnn_filter_flip_transpose_batched(int n, const void *const *w, void *const *wT,
                                                   const int *K, const int *R, const int *S,
                                                   const int *C, const void *const *row_scale,
                                                   void *stream)
{
    MRCNN_REQUIRE(n >= 0 && (n == 0 || (w && wT && K && R && S && C)),
                  "filter_flip_transpose_batched: bad args");
    for (int i0 = 0; i0 < n; i0 += kFlipBatch) {
        FlipBatch b = {};
        b.n = std::min(kFlipBatch, n - i0);
        int blocks = 0;
        for (int i = 0; i < b.n; ++i) {
            const int j = i0 + i;
            MRCNN_REQUIRE(w[j] && wT[j] && K[j] > 0 && R[j] > 0 && S[j] > 0 && C[j] > 0,
                          "filter_flip_transpose_batched: bad entry %d", j);
            b.w[i] = (const float *)w[j];
            b.wT[i] = (float *)wT[j];
            b.scale[i] = row_scale ? (const float *)row_scale[j] : nullptr;
            b.K[i] = K[j]; b.RS[i] = R[j] * S[j]; b.C[i] = C[j];
            b.first_block[i] = blocks;
            blocks += ((C[j] + 31) / 32) * ((K[j] + 31) / 32) * R[j] * S[j];
        }
        b.first_block[b.n] = blocks;
        hipLaunchKernelGGL(filter_flip_transpose_batched_kernel, dim3(blocks), dim3(256), 0,
                           mrcnn::as_stream(stream), b);
    }
    return mrcnn::check_launch("filter_flip_transpose_batched");
}

extern "C" int mrcnn_filter_flip_transpose(const float *w, float *wT, int K, int R, int S, int C,
                                           const float *row_scale, void *stream)
{
    MRCNN_REQUIRE(w && wT && K > 0 && R > 0 && S > 0 && C > 0, "filter_flip_transpose: bad args");
    hipLaunchKernelGGL(filter_flip_transpose_kernel,
                       dim3((C + 31) / 32, (K + 31) / 32, R * S), dim3(256), 0,
                       mrcnn::as_stream(stream), w, wT, K, R * S, C, row_scale);
    return mrcnn::check_launch("filter_flip_transpose");
}

extern "C" int mrcnn_conv2d_dgrad_wt(const mrcnn_conv_desc *d, const float *gy, const float *wT,
                                     float *gx, int epi_flags, const float *res_g,
                                     const float *res_y, const float *out_mask_y,
                                     const float *out_scale, void *split_ws, void *stream)
{
    GemmParams p = {};
    if (int rc = dgrad_wt_problem(d, res_g || res_y || out_mask_y, p)) return rc;
    MRCNN_REQUIRE(gy && wT && gx, "conv2d_dgrad_wt: null pointer");
    MRCNN_REQUIRE(aligned16(gy) && aligned16(wT), "conv2d_dgrad_wt: gy/wT must be 16-byte aligned");
    MRCNN_REQUIRE((epi_flags & ~MRCNN_EPI_ACCUM) == 0, "conv2d_dgrad_wt: only MRCNN_EPI_ACCUM is valid");
    MRCNN_REQUIRE(!res_y || res_g, "conv2d_dgrad_wt: res_y without res_g");
    hipStream_t s = mrcnn::as_stream(stream);
    p.A = gy; p.B = wT; p.C = gx;
    p.res_g = res_g; p.res_y = res_y; p.out_mask_y = out_mask_y; p.scale = out_scale;
    p.flags = epi_flags | (out_scale ? MRCNN_EPI_AFFINE : 0);
    if (p.out_mode == OUT_STRIDED) {       // (the scattered rows are never cut along K: no workspace)
        if (!(epi_flags & MRCNN_EPI_ACCUM))
            MRCNN_HIP_TRY(hipMemsetAsync(gx, 0, sizeof(float) * (size_t)d->N * d->H * d->W * d->C, s));
    } else {
        p.split_ws = (float *)split_ws;
    }
    return launch<FWD>(p, s);
}

extern "C" int64_t mrcnn_conv2d_wgrad_workspace_bytes(const mrcnn_conv_desc *d)
{
    if (!d) return 0;
    const int64_t gwsz = (int64_t)d->K * d->R * d->S * d->C;
    return 64 * gwsz * 4;  // 64 split slabs
}

extern "C" int mrcnn_conv2d_wgrad_ex(const mrcnn_conv_desc *d, const float *x, const float *gy,
                                     float *gw, void *ws, const float *out_row_scale,
                                     void *stream)
{
    if (int rc = check_desc(d)) return rc;
    MRCNN_REQUIRE(x && gy && gw, "conv2d_wgrad: null pointer");
    MRCNN_REQUIRE(aligned16(x) && aligned16(gy) && aligned16(gw) && (!ws || aligned16(ws)),
                  "conv2d_wgrad: pointers must be 16-byte aligned");
    return wgrad_run(d, gy, x, gw, ws, out_row_scale, stream);
}

extern "C" int mrcnn_conv2d_wgrad(const mrcnn_conv_desc *d, const float *x, const float *gy,
                                  float *gw, void *ws, void *stream)
{
    return mrcnn_conv2d_wgrad_ex(d, x, gy, gw, ws, nullptr, stream);
}

extern "C" int mrcnn_deconv2x2s2_fwd(const float *x, const float *w, const float *bias, float *y,
                                     int N, int H, int W, int C, int K, int epi_flags,
                                     void *stream)
{
    return deconv_fwd(false, x, w, bias, y, N, H, W, C, K, epi_flags, stream);
}

extern "C" int mrcnn_deconv2x2s2_fwd_wt(const float *x, const float *wT, const float *bias, float *y,
                                        int N, int H, int W, int C, int K, int epi_flags,
                                        void *stream)
{
    return deconv_fwd(true, x, wT, bias, y, N, H, W, C, K, epi_flags, stream);
}

extern "C" int mrcnn_deconv2x2s2_dgrad(const float *gy, const float *w, float *gx, int N, int H,
                                       int W, int C, int K, void *stream)
{
    // gx = conv2x2/2(gy) with KRSC filter w (C,2,2,K)
    const mrcnn_conv_desc d = deconv_adjoint_desc(N, H, W, C, K);
    return mrcnn_conv2d_fwd(&d, gy, w, nullptr, nullptr, nullptr, nullptr, gx, 0, nullptr, stream);
}

extern "C" int64_t mrcnn_deconv2x2s2_wgrad_workspace_bytes(int N, int H, int W, int C, int K)
{
    return 64ll * C * 4 * K * 4;
}

extern "C" int mrcnn_deconv2x2s2_wgrad(const float *x, const float *gy, float *gw, int N, int H,
                                       int W, int C, int K, void *ws, void *stream)
{
    MRCNN_REQUIRE(x && gy && gw, "deconv_wgrad: null pointer");
    MRCNN_REQUIRE(aligned16(x) && aligned16(gy) && aligned16(gw) && (!ws || aligned16(ws)),
                  "deconv_wgrad: pointers must be 16-byte aligned");
    // gw[c, (a,b,o)] = sum_m x[m, c] * gy[pix(m,a,b), o] : wgrad of the adjoint conv with
    // "gy" := x and "x" := gy.
    const mrcnn_conv_desc d = deconv_adjoint_desc(N, H, W, C, K);
    return wgrad_run(&d, x, gy, gw, ws, nullptr, stream);
}

// The plan of one call as text, no device touched (tests/test_gemm_edge_cases_cpu.py parses it):
//   label=<branch> mode=<mode> M=<rows> N=<cols> k=<K extent the slabs cut>
//   | kind=<profiler kernel> tags=<instantiation> rows=<lo>:<hi> grid=<x>x<y> slab=<depth> tail=<first>,<row0>,<pieces>,<depth>
//   [| sum row0=<first row> slabs=<count>]
// The Winograd entries (conv3x3_wino_fwd / _dgrad / _wgrad: plan_wino_gemm / plan_wino_wgrad over the tiles of
// the maps) print batch=36 behind the grid of every launch.
extern "C" int mrcnn_conv_gemm_plan(const char *entry, const mrcnn_conv_desc *d, int has_ws, char *out,
                                    int out_len)
{
    MRCNN_REQUIRE(entry && d && out && out_len > 0, "conv_gemm_plan: null argument");
    const char *plus = strchr(entry, '+');
    const size_t len = plus ? (size_t)(plus - entry) : strlen(entry);
    auto is = [&](const char *name) { return strlen(name) == len && strncmp(entry, name, len) == 0; };
    const bool dgrad = is("conv2d_dgrad") || is("conv2d_dgrad_ex"), dgrad_wt = is("conv2d_dgrad_wt");
    MRCNN_REQUIRE(!plus || (strcmp(plus, "+res_g") == 0 && (dgrad || dgrad_wt)),
                  "conv_gemm_plan: unknown entry '%s'", entry);
    const bool fused_grad = plus != nullptr;
    const mrcnn_conv_desc adj = deconv_adjoint_desc(d->N, d->H, d->W, d->C, d->K);
    GemmParams p = {};
    GemmShape shape = {};
    int mode = FWD, rc = 0;
    bool wino = false;
    bool ws = has_ws != 0;                 // entry points without a workspace argument plan without one
    if (is("conv2d_fwd")) {
        rc = fwd_problem(d, p);
    } else if (is("conv_stem_fwd")) {
        rc = stem_problem(d->N, d->H, d->W, d->K, p);
        ws = false;
    } else if (dgrad) {
        mode = DGRAD;
        rc = dgrad_problem(d, fused_grad, p);
        ws = ws && is("conv2d_dgrad_ex");
    } else if (dgrad_wt) {
        rc = dgrad_wt_problem(d, fused_grad, p);
        ws = ws && p.out_mode == OUT_PLAIN;
    } else if (is("conv2d_wgrad") || is("conv2d_wgrad_ex")) {
        mode = WGRAD;
        rc = check_desc(d);
        if (!rc) rc = wgrad_problem(d, p, shape);
    } else if (is("deconv2x2s2_fwd") || is("deconv2x2s2_fwd_wt")) {
        mode = is("deconv2x2s2_fwd") ? DGRAD : FWD;
        rc = deconv_problem(mode == FWD, d->N, d->H, d->W, d->C, d->K, p);
        ws = false;
    } else if (is("deconv2x2s2_dgrad")) {
        rc = fwd_problem(&adj, p);
        ws = false;
    } else if (is("deconv2x2s2_wgrad")) {
        mode = WGRAD;
        rc = wgrad_problem(&adj, p, shape);
    } else if (is("conv3x3_wino_fwd") || is("conv3x3_wino_dgrad") || is("conv3x3_wino_wgrad")) {
        wino = true;
        mode = is("conv3x3_wino_wgrad") ? WGRAD : FWD;
        rc = wino_check(d, "conv_gemm_plan");
    } else {
        MRCNN_REQUIRE(false, "conv_gemm_plan: unknown entry '%s'", entry);
    }
    if (rc) return rc;
    GemmPlan plan;
    if (wino) {
        // rows = tiles of the maps; the data gradient's columns are the input channels
        const int64_t T = (int64_t)d->N * ((d->H + 3) / 4) * ((d->W + 3) / 4);
        const bool dgrad_form = is("conv3x3_wino_dgrad");
        p.M = mode == WGRAD ? d->K : (int)T;
        p.N = mode == WGRAD || dgrad_form ? d->C : d->K;
        plan = mode == WGRAD ? plan_wino_wgrad(T, d->K, d->C, g_knobs)
                             : plan_wino_gemm(T, p.N, dgrad_form ? d->K : d->C, g_knobs);
    } else {
        if (mode != WGRAD) shape = gemm_shape(p, mode, ws);
        shape.has_ws = ws;
        plan = mode == WGRAD ? plan_wgrad(shape, g_knobs) : plan_gemm(shape, g_knobs);
    }

    static const char *const modes[] = {"FWD", "DGRAD", "WGRAD"};
    static const char *const outs[] = {"OUT_PLAIN", "OUT_STRIDED", "OUT_DECONV"};
    static const char *const variants[] = {"general", "PW", "K3", "WPERM", "W8"};
    int at = snprintf(out, (size_t)out_len, "label=%s mode=%s M=%d N=%d k=%lld", plan.label, modes[mode], p.M, p.N,
                      (long long)plan.k_extent);
    for (int i = 0; i < plan.n && at < out_len; ++i) {
        const GemmLaunch &l = plan.launch[i];
        const bool w8 = l.tile == kW8BM;
        at += snprintf(out + at, (size_t)(out_len - at),
                       " | kind=conv_gemm_kernel<%d,%d,%s%s> tags=%s,%dx%d,%s,%s,%s%s%s rows=%d:%d grid=%lldx%d%s slab=%d "
                       "tail=%d,%d,%d,%d",
                       w8 ? 2 : l.tile / 64, w8 ? 2 : l.tile / 64, modes[mode], w8 ? ",W8" : "", modes[mode], l.tile,
                       w8 ? kW8BN : l.tile, outs[p.out_mode], l.inst.split ? "split" : "fp32", variants[l.inst.variant],
                       mode != WGRAD && p.perm_n > 0 ? ",perm" : "", mode != WGRAD && p.stem ? ",stem" : "", l.m_lo,
                       l.m_hi, (long long)l.grid_x, l.grid_y, wino ? " batch=36" : "", l.split_len, l.tail_first, l.tail_row0, l.tail_splits,
                       l.tail_split_len);
    }
    if (plan.sum_splits && at < out_len)
        at += snprintf(out + at, (size_t)(out_len - at), " | sum row0=%d slabs=%d", plan.sum_row0, plan.sum_splits);
    MRCNN_REQUIRE(at < out_len, "conv_gemm_plan: the plan needs %d bytes, the buffer has %d", at + 1, out_len);
    return 0;
}

#include "conv_winograd.h"
