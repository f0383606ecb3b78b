// The kernel of the implicit-GEMM convolution family (conv_gemm.hip describes it and launches it) and
// the launch record it takes.  A header because the instantiations are compiled in three translation
// units, so that the build parallelises: conv_gemm.hip holds fp32 MFMA (NP = 0) and the three-plane
// split (NP = 3), conv_gemm_planes.hip is compiled once for NP = 1 and once for NP = 2.
#pragma once
#include <type_traits>

#include "common.h"
#include "conv_gemm_plan.h"

namespace {

using namespace mrcnn::gemm;   // the launch policy, its constants (BK, Mode, OutMode, ...) and the knobs

typedef float f32x16 __attribute__((ext_vector_type(16)));

// minimum workgroups per CU the register allocation must allow (256-thread workgroups: one
// wave per SIMD each)
constexpr int min_blocks(int tm, int mode)
{
    if (!single_buffered(tm, mode)) return 1;
    return tm == 4 ? 2 : (tm == 2 ? 3 : 6);
}
constexpr int KPAD = 4;  // K-contiguous LDS rows are 36 floats (conflict-free b128)

constexpr bool is_fwd(int m) { return m == FWD; }

}  // namespace

namespace mrcnn {
namespace gemm {

struct GemmParams {
    const float *A;      // FWD: x      DGRAD: gy      WGRAD: gy
    const float *B;      // FWD: w      DGRAD: w       WGRAD: x
    float *C;            // FWD: y      DGRAD: gx      WGRAD: gw / split slabs
    const float *bias, *scale, *shift, *residual;
    int M, N;            // output tile space (rows, cols)
    int m_lo;            // first row handled by this launch (tail-split launches)
    int Kc;              // FWD: C_in   DGRAD: K_out   WGRAD: #pixels
    int gp, gq;          // pixel grid the rows (FWD/DGRAD) or K index (WGRAD) run over
    int sh, sw;          // spatial dims of the gathered tensor
    int R, S, stride, pad;
    int lda;             // channel stride (floats) of a pixel of the gathered tensor
    int ldb;             // FWD: row stride of w (R*S*C); DGRAD: R*S*C_in; WGRAD: unused
    int ldg;             // WGRAD: row stride of gy
    int cin;             // DGRAD/WGRAD: C_in
    int ldc;             // output row stride
    int flags;
    int out_mode;
    int oh, ow, ko;      // OUT_STRIDED: gx spatial dims; OUT_DECONV: ko = out channels
    int ostride;         // OUT_STRIDED: stride of the OUTPUT rows (0: `stride`; the forward-form strided dgrad gathers densely)
    int stem;            // FWD: stem gather (8 pixels x 4 ch per K slice)
    int split_len;       // WGRAD: pixels per split; FWD/DGRAD: K slices per split (0: no split)
    int64_t split_stride;// floats between split slabs
    int out_row0;        // FWD/DGRAD split launches: first row of the slab (subtracted)
    // Forward-form launches on many small maps (RoI features): GEMM rows ordered
    // (block of kPermBlock images, position, image in block): a 128-row tile holds ONE pixel
    // position of 128 images, so a filter tap that falls into the zero padding for that
    // position does so for EVERY row of the tile and its K slices are skipped (a 3x3 / pad 1
    // convolution on 7x7 maps: 18 % of all slices); consecutive tiles walk the positions of
    // the same image block, whose pixels therefore stay in the XCD's L2.  perm_n = number of
    // images (M is padded to whole blocks), 0 = natural (image, y, x) order.
    int perm_n;
    // backward-data epilogue: gx = (acc * scale[c] + res_g * (res_y > 0)) * (out_mask_y > 0)
    //   res_g / res_y : identity-shortcut gradient of a bottleneck (res_y NULL: res_g is added as is)
    //   out_mask_y    : output of the ReLU that produced this conv's INPUT, i.e. the epilogue-
    //                   backward of the NEXT conv down the chain applied where its incoming
    //                   gradient is produced (then that conv needs no mask staging at all)
    // WGRAD epilogue: gw[k, :] *= scale[k]
    const float *res_g, *res_y, *out_mask_y;
    float *split_ws;     // host only: caller's split-K workspace (kSplitWsBytes) or NULL
    unsigned a_bytes, b_bytes, c_bytes;  // buffer extents (bytes) of A, B, C
    // Fused tail (FWD / DGRAD, gridDim.y == 1): workgroups [0, tail_first) run whole tiles as
    // usual; the workgroups behind them run the tiles of the LEFTOVER rows — the rows beyond the
    // last full round of resident workgroups — each cut along K into tail_splits pieces that
    // write raw partial sums into slabs of tail_ws (summed, in order, by splitk_epilogue_kernel).
    // Dispatched last, the short pieces fill the CUs as the final round of whole tiles drains,
    // instead of a separate remainder launch that waits for the main launch to finish.
    int tail_first, tail_splits, tail_split_len, tail_row0;
    unsigned tail_bytes;
    float *tail_ws;
    int64_t tail_stride;
    // Batched launches (gridDim.z > 1; the 36 per-frequency GEMMs of the Winograd path,
    // winograd.hip): floats between consecutive problems of A, B and C.  The extents above
    // are then per problem.
    int64_t batch_a, batch_b, batch_c;
};

// GEMM row -> (image, position) under the block-position-major order of GemmParams::perm_n
struct PermRow { int n, pos; };
__host__ __device__ __forceinline__ PermRow perm_row(int m, int pq)
{
    const int q = m / kPermBlock, img = m - q * kPermBlock;
    const int blk = q / pq;
    PermRow r;
    r.pos = q - blk * pq;
    r.n = blk * kPermBlock + img;
    return r;
}

// conv_gemm_planes.hip: the NP-plane instantiation (NP = 1, 2) of a split-operand launch of the plan —
// tile 64 / 128 / kW8BM, mode FWD / WGRAD, variant GENERAL / PW / K3 / W8 — on `grid`
template <int NP>
void launch_planes(const GemmParams &p, int tile, int mode, int variant, dim3 grid, hipStream_t s, hipEvent_t ev0,
                   hipEvent_t ev1);
extern template void launch_planes<1>(const GemmParams &, int, int, int, dim3, hipStream_t, hipEvent_t, hipEvent_t);
extern template void launch_planes<2>(const GemmParams &, int, int, int, dim3, hipStream_t, hipEvent_t, hipEvent_t);

}  // namespace gemm
}  // namespace mrcnn

namespace {

template <int TM, int TN, int MODE>
struct Cfg {
    static constexpr int BM = 64 * TM, BN = 64 * TN;
    static constexpr bool A_KC = (MODE != WGRAD);  // A K-contiguous?
    static constexpr bool B_KC = is_fwd(MODE);
    static constexpr int A_FLOATS = A_KC ? BM * (BK + KPAD) : BK * BM;
    static constexpr int B_FLOATS = B_KC ? BN * (BK + KPAD) : BK * BN;
    static constexpr int A_V4 = BM * BK / 4 / 256;  // float4 per thread per slice
    static constexpr int B_V4 = BN * BK / 4 / 256;
};

// ---- buffer addressing -----------------------------------------------------------------
// Every global access of the kernel goes through a raw buffer descriptor: an element that
// must read as zero (image border of the im2col gather, tile tails in M / N / K) is given
// the byte offset kOOB, which lies beyond num_records, so the hardware returns 0 for loads
// and drops stores.  No per-element branch or select touches a loaded value, so every load
// of a K slice stays in flight across the slice's MFMAs.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
constexpr unsigned kOOB = 0x80000000u;

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void *p, unsigned bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, p ? bytes : 0u, 0x00020000);
}
__device__ __forceinline__ float4 bload4(__amdgpu_buffer_rsrc_t r, unsigned off)
{
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0);
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z),
                       __uint_as_float(v.w));
}
__device__ __forceinline__ float bload1(__amdgpu_buffer_rsrc_t r, unsigned off)
{
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0));
}
__device__ __forceinline__ void bstore1(__amdgpu_buffer_rsrc_t r, unsigned off, float v)
{
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), r, off, 0, 0);
}
__device__ __forceinline__ void bstore4(__amdgpu_buffer_rsrc_t r, unsigned off, float4 v)
{
    u32x4 u;
    u.x = __float_as_uint(v.x); u.y = __float_as_uint(v.y);
    u.z = __float_as_uint(v.z); u.w = __float_as_uint(v.w);
    __builtin_amdgcn_raw_buffer_store_b128(u, r, off, 0, 0);
}
__device__ __forceinline__ void bstore8(__amdgpu_buffer_rsrc_t r, unsigned off, unsigned a, unsigned b)
{
    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
    u32x2 u;
    u.x = a; u.y = b;
    __builtin_amdgcn_raw_buffer_store_b64(u, r, off, 0, 0);
}

// fp32 pair -> three packed bf16 pairs (low half = a, high half = b) with a = hi + mid + lo
// exactly: each conversion rounds to nearest, each residual is exact in fp32.
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pack_bf16(float a, float b)
{
    const f32x2 v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}
// a - b as ONE v_sub_f32: left to the compiler, adjacent subtractions are packed into v_pk_add_f32,
// which costs far more than its issue slot beside MFMAs (MI355X_MICROARCH.md, filler prices)
__device__ __forceinline__ float sub_f32(float a, float b)
{
    float r;
    asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// NP < 3: the first NP planes of the same split (the others are not computed and left unset)
template <int NP = 3>
__device__ __forceinline__ void split3(float a, float b, unsigned &h, unsigned &m, unsigned &l)
{
    h = pack_bf16(a, b);
    if constexpr (NP >= 2) {
        a = sub_f32(a, __uint_as_float(h << 16));
        b = sub_f32(b, __uint_as_float(h & 0xffff0000u));
        m = pack_bf16(a, b);
    }
    if constexpr (NP >= 3) {
        a = sub_f32(a, __uint_as_float(m << 16));
        b = sub_f32(b, __uint_as_float(m & 0xffff0000u));
        l = pack_bf16(a, b);
    }
}

// Round-3 tile-shape experiments, both bit-checked against this kernel and removed again
// (profiles/r03_exp_tiles.txt): 256 x 128 workgroup tiles (a wave owns 128 x 64, 255 VGPRs, two
// workgroups per CU) reach 85 vs 127 TFLOP/s on res5's 512 -> 2048 and 128 x 64 tiles (a wave
// owns 64 x 32, four workgroups per CU) 116 vs 127: with fp32 MFMA the number of interleaved
// waves per SIMD matters more than the bytes staged per MFMA, in both directions from 3.
// (A "ping-pong" variant — 512-thread workgroups running two tiles in antiphase, one group
// issuing MFMAs while the other stages — was measured slower, 110 vs 122 TFLOP/s on res5 3x3:
// one wave per SIMD cannot keep the fp32 MFMA pipe as full as interleaved free-running waves.
// Removed; see the history of this file.)
// WPERM: WGRAD with position-major pixel order (GemmParams::perm_n) — a separate instantiation
// because the natural-order kernel sits exactly at its 168-register budget.
// SPLIT (the default arithmetic; mrcnn_set_tuning("split_bf16", 0) selects fp32 MFMA everywhere;
// forward form 128x128 / 64x64 and the 128x128 natural-order weight gradient): the
// operands are staged as THREE bf16 planes each — a = a_hi + a_mid + a_lo EXACTLY (8 + 8 + 8
// significand bits) — and a K step runs six v_mfma_f32_32x32x16_bf16 (hi*hi, hi*mid, mid*hi,
// mid*mid, hi*lo, lo*hi; every product of two bf16 values is exact in fp32, accumulation is fp32).
// The three dropped cross terms are <= 2^-24 of |a*b| each, i.e. of the order of the rounding
// error of one fp32 multiply-add, so results stay fp32-accurate (tests/test_gpu_split_bf16.py
// measures the error against float64 next to the fp32 MFMA kernel's), while the matrix pipe
// does 6 x 32 instead of 8 x 64 cycles per 32x32x16 block.
// G groups of (MFMAs, one global load, LDS reads): the loads are dealt out evenly over ALL NM MFMAs
// of the K slice, the ND LDS reads (next K step's fragments) over the first NMD of them.
template <int G, int NM, int NMD, int ND, int I = 0>
__device__ __forceinline__ void sgb_interleave()
{
    if constexpr (I < G) {
        constexpr int m0 = NM * I / G, m1 = NM * (I + 1) / G;
        // LDS reads that belong in front of MFMA m1 (all of them once m1 >= NMD)
        constexpr int d0 = m0 >= NMD ? ND : ND * m0 / NMD, d1 = m1 >= NMD ? ND : ND * m1 / NMD;
        if constexpr (m1 > m0) __builtin_amdgcn_sched_group_barrier(0x008, m1 - m0, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        if constexpr (d1 > d0) __builtin_amdgcn_sched_group_barrier(0x100, d1 - d0, 0);
        sgb_interleave<G, NM, NMD, ND, I + 1>();
    }
}

// W8 (round 6; SPLIT forward form only): ONE 512-thread workgroup per CU on a 256 x 128 tile — eight
// waves of 64 x 64, i.e. the two co-resident 128 x 128 workgroups of the standard configuration
// stacked on top of each other so that they share the filter panel: 48 instead of 64 operand loads
// and 3/4 of the split arithmetic per CU and K slice.  Two LDS stages, ONE barrier per slice.  What
// two independent workgroups get from drifting apart — one stages while the other multiplies — the
// two halves of this workgroup get from running the barrier interval in OPPOSITE ORDER: waves 0-3
// multiply slice k and then split / store slice k + 1, waves 4-7 store first and multiply afterwards
// (both orders read stage k & 1 and write the other one, so the interval needs no further
// synchronisation); a SIMD hosts one wave of each half (MI355X_MICROARCH.md, wave placement).
//
// PW (forward form): the launch is a 1x1 / stride 1 / pad 0 gather in natural row order that writes
// plain rows (pw_plain() on the host) — the general gather (taps, image / y / x decomposition,
// position-major rows) and the strided / deconvolution output maps are compiled out, which frees
// the scalar registers the general instantiation spills (W8: 87 -> 0 spilled SGPRs, 250 -> 182
// VGPRs, +3 % on the head's 1x1 layers).  W8 implies it.  K3: the same for the 3x3 / stride 1 / pad 1
// launches in natural row order (k3_plain(): the backbone's 3x3 layers and their transposed-filter data
// gradients) — filter size, stride and padding are constants of the gather.  Same arithmetic, same bits.
//
// NP: the bf16 planes staged per operand element.  0: fp32 MFMA.  3: SPLIT as described above.
// 2 ("split_planes" = 2): hi and mid only, the products (mid,hi) (hi,mid) (hi,hi) — operands of
// 16 significand bits, half the matrix-pipe work.  1: hi only, the product (hi,hi) — plain bf16
// operands, one sixth.  The planes are the first NP of split3's and the products a suffix of the
// three-plane issue order; a plane no product reads is neither converted nor staged.  Everything
// else — tiles, K order, XCD remap, K cuts, epilogues — is the same code for every NP >= 1.
template <int TM, int TN, int MODE, bool WPERM = false, int NP = 0, bool W8 = false,
          bool PW = false, bool K3 = false>
__global__ void __launch_bounds__(W8 ? 512 : 256,
                                  NP > 0 ? (TM == 2 ? 2 : 4) : min_blocks(TM, MODE))
conv_gemm_kernel(const GemmParams p)
{
    static_assert(NP >= 0 && NP <= 3, "NP: 0 (fp32 MFMA) or 1 .. 3 bf16 planes");
    constexpr bool SPLIT = NP > 0;
    constexpr int NPROD = NP == 3 ? 6 : NP == 2 ? 3 : 1;    // bf16 MFMAs per K step and tile pair
    static_assert(!W8 || (SPLIT && MODE == FWD && TM == 2 && TN == 2),
                  "W8: the split-operand forward form on 64x64 wave tiles");
    static_assert(!WPERM || MODE == WGRAD, "WPERM is a WGRAD-only variant");
    static_assert(!PW || MODE == FWD, "PW: forward form only");
    static_assert(!K3 || (MODE == FWD && !W8 && !PW), "K3: forward form only");
    constexpr bool PWC = W8 || PW;
    // the launch geometry the gather and the output map use: compile-time facts in the PW / K3
    // instantiations (natural row order, no stem packing, plain output rows), the launch's fields otherwise
    constexpr bool GEO = PWC || K3;
    const int gR = PWC ? 1 : K3 ? 3 : p.R, gS = PWC ? 1 : K3 ? 3 : p.S;
    const int gStride = GEO ? 1 : p.stride, gPad = PWC ? 0 : K3 ? 1 : p.pad;
    const int gPermN = GEO ? 0 : p.perm_n;
    const bool gStem = !GEO && p.stem;
    constexpr bool ILV = SPLIT && MODE == FWD;
    static_assert(!SPLIT || (BK == 32 && TM == TN &&
                             ((MODE == FWD && (TM == 1 || TM == 2)) || (MODE == WGRAD && !WPERM && TM == 2))),
                  "SPLIT: forward form (128x128, 64x64) / weight gradient (128x128) only");
    constexpr bool SINGLEBUF = !W8 && (SPLIT || single_buffered(TM, MODE));
    using C_ = Cfg<TM, TN, MODE>;
    constexpr int NT = W8 ? 512 : 256;                  // threads of the workgroup
    constexpr int BM = (W8 ? 2 : 1) * C_::BM, BN = C_::BN;
    constexpr int AV = BM * BK / 4 / NT, BV = BN * BK / 4 / NT;   // float4 per thread per slice
    constexpr bool FWDLIKE = is_fwd(MODE);
    // SPLIT stage: 3 planes per operand of [row][32 bf16 + 8 pad] (80-byte rows: conflict-free b128)
    // forward form: 64-byte rows, 16-byte slots XOR-swizzled by (row >> 2) & 3 — conflict-free for
    // the b128 fragment reads (lane groups {0-3,12-15,20-27}, ...) AND for the b64 plane writes (a
    // 16-lane group writes two whole rows = one 128-byte bank row).  Weight gradient: 80-byte rows
    // (its transposing writes hit rows 4 apart; see swz).
    constexpr int SROW = MODE == WGRAD ? BK + 8 : BK;     // ushorts per plane row
    constexpr int PLA = BM * SROW, PLB = BN * SROW;       // ushorts per plane
    constexpr int STAGE_FLOATS = SPLIT ? 3 * (PLA + PLB) / 2 : C_::A_FLOATS + C_::B_FLOATS;
    __shared__ __attribute__((aligned(16))) float smem_all[1][SINGLEBUF ? 1 : 2][STAGE_FLOATS];

    float (*smem)[STAGE_FLOATS] = smem_all[0];
    // SPLIT WGRAD (80-byte rows, no swizzle): plane row 32 c + l holds channel 4 l + c of the tile
    // (WROWPERM).  The transposing writes of one instruction cover the channels 4 l + c of 32
    // lanes l: with the channel as the row they would sit 320 bytes apart — two bank positions
    // for the whole wave — and an XOR of the chunk index that spreads them breaks the b128
    // fragment reads instead (a read group spans rows r .. r + 27; round-4 PMC: half of the
    // LDS-active cycles of the former layout were bank conflicts).  With the permuted rows the
    // lanes of a write hit CONSECUTIVE rows (80 l mod 128: two-way, hidden by the store's own
    // register transfer) and a fragment read 16 rows with 16 different bank slots; the
    // permutation is undone where the tile is written (gw row 4 rr + .., column 4 li + ..).
    constexpr bool WROWPERM = SPLIT && MODE == WGRAD;
    auto swz = [](int row) { return !SPLIT || MODE == WGRAD ? 0 : ((row >> 2) & 3) << 1; };
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;

    const int64_t zb = blockIdx.z;                      // batched launches: problem index
    const __amdgpu_buffer_rsrc_t rA = make_rsrc(p.A + zb * p.batch_a, p.a_bytes);
    const __amdgpu_buffer_rsrc_t rB = make_rsrc(p.B + zb * p.batch_b, p.b_bytes);

    // tile -> (m0, n0).  Workgroup b runs on XCD b % 8 (observed dispatch order); remap so
    // that each XCD owns a contiguous run of tile ids — N fastest — and neighbouring tiles,
    // which share the gathered A rows and the filter panel, hit the same private L2.
    // WGRAD (grid = tiles x splits): the remap runs over the whole 2-D grid with the split as
    // the slow index, so the tiles of one split — which all stream the same pixel range of gy
    // and x — land on one or two XCDs instead of all eight.
    const int ntn = (p.N + BN - 1) / BN;
    int tile = blockIdx.x + blockIdx.y * gridDim.x;
    int split;
    int split_len = p.split_len;
    const bool tail = MODE != WGRAD && p.tail_splits > 0 && tile >= p.tail_first;   // uniform
    if (tail) {
        const int rem = tile - p.tail_first;
        split = rem % p.tail_splits;
        tile = p.tail_first + rem / p.tail_splits;
        split_len = p.tail_split_len;
    } else {
        const int nwg = (MODE != WGRAD && p.tail_splits > 0) ? p.tail_first : (int)(gridDim.x * gridDim.y);
        const int q = nwg >> 3, r = nwg & 7, xcd = tile & 7, idx = tile >> 3;
        tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
        split = tile / (int)gridDim.x;
        tile -= split * (int)gridDim.x;
    }
    // (Walking the tiles N-panel by N-panel so that an XCD's resident workgroups sweep a filter panel
    // that fits its L2 was measured in round 5 on res5's shapes, panels of 1 .. 8 N-tiles: every
    // layer within +-2 % of the plain N-fastest walk, profiles/r05c_npanel.txt; removed.)
    const int m0 = p.m_lo + (tile / ntn) * BM;
    const int n0 = (tile % ntn) * BN;

    // ---------------- per-thread gather state -----------------------------------
    constexpr int KC_C4 = BK / 4, KC_RPP = NT / KC_C4;    // float4 per row, rows per pass
    const int kc_row = tid / KC_C4, kc_c4 = tid % KC_C4;
    constexpr int NA = AV;                              // A rows a thread addresses
    auto a_row = [&](int i) { return kc_row + KC_RPP * i; };
    int a_n[NA], a_y[NA], a_x[NA];     // FWD/DGRAD: pixel coords of each A row
    // 1x1 / stride 1 / pad 0 forward-form launches (two thirds of the RoI head's GEMMs): GEMM row
    // m IS pixel m of the gathered tensor — no (image, y, x) decomposition, i.e. none of the
    // eight integer divisions of the general set-up
    // (PW / W8 launches are pointwise by the host's rule: the general gather is compiled out)
    const bool pointwise = PWC || (FWDLIKE && gR == 1 && gS == 1 && gStride == 1 && gPad == 0 &&
                                  gPermN == 0 && !gStem && p.gp == p.sh && p.gq == p.sw);   // uniform
    if (MODE != WGRAD && pointwise) {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int m = m0 + a_row(i);
            a_n[i] = m < p.M ? m : 0;          // (pixel index; folded into a_base below)
            a_x[i] = 0;
            a_y[i] = m < p.M ? 0 : -(1 << 28);
        }
    } else if (MODE != WGRAD) {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int m = m0 + a_row(i);
            const bool ok = m < p.M;
            const int mm = ok ? m : 0;
            int n, rem;
            bool img_ok = true;
            if (FWDLIKE && gPermN > 0) {
                const PermRow pr = perm_row(mm, p.gp * p.gq);
                n = pr.n; rem = pr.pos;
                img_ok = n < gPermN;           // padding rows of the last image block
            } else {
                n = mm / (p.gp * p.gq); rem = mm - n * (p.gp * p.gq);
            }
            const int gy = rem / p.gq, gx = rem - gy * p.gq;
            a_n[i] = n;
            if (FWDLIKE) { a_y[i] = gy * gStride - gPad; a_x[i] = gx * gStride - gPad; }
            else { a_y[i] = gy + gPad; a_x[i] = gx + gPad; }
            if (!ok || !img_ok) a_y[i] = -(1 << 28);   // no such row: every tap out of range
        }
    }
    constexpr int A_TPR = BM / 4, B_TPR = BN / 4;            // threads per k row (K-strided tiles)
    constexpr int A_RPP = 256 / A_TPR, B_RPP = 256 / B_TPR;  // k rows per pass
    const int wa_k = tid / A_TPR, wa_c4 = tid % A_TPR;
    const int wb_k = tid / B_TPR, wb_c4 = tid % B_TPR;
    // k row (pixel of the slice) of a thread's i-th load of a K-strided tile.  SPLIT: AV
    // CONSECUTIVE pixels per thread, so that the 4 channels x AV pixels it holds go to LDS as
    // [channel][pixel] rows (the layout the bf16 MFMA fragments are read from) with 8-byte writes.
    auto a_krow = [&](int i) { return SPLIT ? wa_k * AV + i : wa_k + A_RPP * i; };
    auto b_krow = [&](int i) { return SPLIT ? wb_k * BV + i : wb_k + B_RPP * i; };
    int wr = 0, ws_ = 0, wc = 0;
    int wy_lo = 0, wx_lo = 0, wnvx = 1;   // WGRAD position-major: valid-position rectangle
    int wr_u = 0, ws_u = 0, wnv = 1;      // ... the tile's tap and its position count, uniform
    bool wcol_ok = false;
    int pn[BV], py[BV], px[BV];
    int k_begin = 0, k_end = 0;
    if (MODE == WGRAD) {
        const int j = n0 + wb_c4 * 4;
        wcol_ok = j < p.N;
        const int jj = wcol_ok ? j : 0;
        const int rs = jj / p.cin;
        wc = jj - rs * p.cin;
        wr = rs / gS;
        ws_ = rs - wr * gS;
        k_begin = split * p.split_len;
        if (WPERM) {
            // Pixel order for the reduction: (block of BK images, position, image in block),
            // restricted to the positions whose tap (wr, ws_) lies inside the map — one K
            // slice = one position of BK consecutive images, and a block's positions follow
            // each other so its pixels stay in L2.  Every column of the tile belongs to the
            // same tap (cin % BN == 0, checked by the host): tile-uniform values live in SGPRs.
            wr_u = __builtin_amdgcn_readfirstlane(wr);
            ws_u = __builtin_amdgcn_readfirstlane(ws_);
            wy_lo = max(0, gPad - wr_u);
            wx_lo = max(0, gPad - ws_u);
            const int nvy = min(p.gp - 1, p.sh - 1 + gPad - wr_u) - wy_lo + 1;
            wnvx = max(min(p.gq - 1, p.sw - 1 + gPad - ws_u) - wx_lo + 1, 0);
            wnv = max(nvy, 0) * wnvx;
            const int nblk = (gPermN + BK - 1) / BK;
            k_end = min(nblk * wnv * BK, k_begin + p.split_len);
        } else {
            k_end = min(p.Kc, k_begin + p.split_len);
#pragma unroll
            for (int i = 0; i < BV; ++i) {
                const int m = k_begin + b_krow(i);
                const int n = m / (p.gp * p.gq);
                const int rem = m - n * (p.gp * p.gq);
                pn[i] = n;
                py[i] = rem / p.gq;
                px[i] = rem - py[i] * p.gq;
            }
        }
    }

    const int adv_x = BK % p.gq, adv_y = (BK / p.gq) % p.gp, adv_n = BK / (p.gp * p.gq);
    const int cprs = (MODE == WGRAD) ? 1 : (p.Kc + BK - 1) / BK;  // K slices per (r,s)
    // FWD/DGRAD split-K (leftover rows of a small-M problem, see plan_gemm()): this workgroup
    // runs slices [kt0, kt0 + nslices) and writes raw partial sums into its slab
    // position-major rows: the taps that are inside the map for at least one position of this
    // tile, as 4-bit indices packed into a word (wave-uniform)
    int ntaps = gR * gS;
    unsigned long long tap_list = 0;
    if (FWDLIKE && !GEO && gPermN > 0) {
        const int q_lo = m0 / kPermBlock;
        const int q_hi = min(p.M - 1, m0 + BM - 1) / kPermBlock;
        const int pq = p.gp * p.gq;
        ntaps = 0;
        for (int rs = 0; rs < gR * gS; ++rs) {
            const int r = rs / gS, s = rs - r * gS;
            bool hit = q_hi - q_lo > 3;              // many positions in the tile: keep all
            for (int qq = q_lo; qq <= q_hi && !hit; ++qq) {
                const int q = qq % pq;
                const int y = q / p.gq, x = q - y * p.gq;
                hit = (unsigned)(y * gStride - gPad + r) < (unsigned)p.sh &&
                      (unsigned)(x * gStride - gPad + s) < (unsigned)p.sw;
            }
            if (hit) {
                tap_list |= (unsigned long long)rs << (4 * ntaps);
                ++ntaps;
            }
        }
    }
    int kt0 = 0;
    int nslices = (MODE == WGRAD) ? (k_end - k_begin + BK - 1) / BK : ntaps * cprs;
    if (MODE != WGRAD && split_len > 0) {
        kt0 = split * split_len;
        nslices = max(0, min(nslices - kt0, split_len));
    }

    float4 ra[AV], rb[BV];

    // Loop-invariant parts of every load address (element offsets; an invalid row carries the
    // sentinel 0x20000000 so that 4 * offset lands beyond num_records and reads as zero).
    constexpr unsigned kBad = 0x20000000u;
    constexpr int NB = BV;
    unsigned a_base[NA], b_base[NB];
    if (MODE != WGRAD) {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const unsigned pix = pointwise ? (unsigned)a_n[i]
                                           : (unsigned)((a_n[i] * p.sh + a_y[i]) * p.sw + a_x[i]);
            a_base[i] = pix * (unsigned)p.lda + (unsigned)(kc_c4 * 4);
        }
        if (FWDLIKE) {
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const int n = n0 + kc_row + KC_RPP * i;
                b_base[i] = n < p.N ? (unsigned)(n * p.ldb + kc_c4 * 4) : kBad;
            }
        } else {
#pragma unroll
            for (int i = 0; i < BV; ++i) {
                const int n = n0 + wb_c4 * 4;
                b_base[i] = n < p.N ? (unsigned)((wb_k + B_RPP * i) * p.ldb + n) : kBad;
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < AV; ++i) {
            const int k = m0 + wa_c4 * 4;
            a_base[i] = k < p.M ? (unsigned)(a_krow(i) * p.ldg + k) : kBad;
        }
        if (!WPERM) {
#pragma unroll
            for (int i = 0; i < BV; ++i)
                b_base[i] = wcol_ok ? (unsigned)(b_krow(i) * p.lda + wc) : kBad;
        }
    }
    const bool wpoint = MODE == WGRAD && !WPERM && gR == 1 && gS == 1 && gStride == 1 && gPad == 0 &&
                        p.gp == p.sh && p.gq == p.sw;      // uniform
    const int RS = gR * gS;

    // ILV (SPLIT forward form): load_slice only computes the byte offsets of
    // the slice's loads; the loads themselves are issued INSIDE the following compute(), spread
    // between its MFMAs (issue_loads + the sched_group_barrier sequence there).  Issued as one
    // burst ahead of the MFMAs, the 8 .. 12 16-byte loads of every wave of the CU queue behind
    // each other in the texture path and the wave sits in their issue for 1000 - 1700 cycles
    // (s_memtime stamps) before its first MFMA.
    unsigned oa[ILV ? NA : 1], ob[ILV ? NB : 1];
    auto ldA = [&](int i, unsigned off) {
        if constexpr (ILV) {
            oa[i] = off;
        } else {
            ra[i] = bload4(rA, off);
        }
    };
    auto ldB = [&](int i, unsigned off) {
        if constexpr (ILV) ob[i] = off;
        else rb[i] = bload4(rB, off);
    };
    auto issue_loads = [&]() {
        if constexpr (ILV) {
#pragma unroll
            for (int i = 0; i < NA; ++i) ra[i] = bload4(rA, oa[i]);
#pragma unroll
            for (int i = 0; i < NB; ++i) rb[i] = bload4(rB, ob[i]);
        }
    };
    // issue the global loads of slice kt (nothing here consumes a loaded value).
    // FWD/DGRAD K order: channel chunk outer, filter tap (r,s) inner — consecutive slices re-read
    // the same 32-channel slab of neighbouring pixels, which stays in the CU's L1.
    auto load_slice = [&](int kt) {
        if (FWDLIKE && pointwise) {
            // 1x1 / stride 1: slice kt is channel chunk kt of the row's own pixel — none of the
            // tap / chunk divisions and bounds checks of the general gather (a quarter of the
            // instructions a wave issues per slice, all of them competing with the MFMAs of the
            // co-resident waves for issue slots)
            const int c0 = (kt + kt0) * BK;
            const int cc = c0 + kc_c4 * 4;
            const bool c_ok = cc < p.Kc;
#pragma unroll
            for (int i = 0; i < AV; ++i)
                ldA(i, (c_ok && a_y[i] == 0) ? 4u * (a_base[i] + (unsigned)c0) : kOOB);
#pragma unroll
            for (int i = 0; i < BV; ++i) ldB(i, c_ok ? 4u * (b_base[i] + (unsigned)c0) : kOOB);
            return;
        }
        if (FWDLIKE || MODE == DGRAD) {
            kt += kt0;
            int chunk, rs;
            if (FWDLIKE && gPermN > 0) {
                chunk = kt / ntaps;
                rs = (int)((tap_list >> (4 * (kt - chunk * ntaps))) & 15ull);
            } else {
                chunk = kt / RS;
                rs = kt - chunk * RS;
            }
            const int c0 = chunk * BK;
            const int r = rs / gS, s = rs - r * gS;
            const int cc = c0 + kc_c4 * 4;
            const bool c_ok = gStem || cc < p.Kc;
            // wave-uniform part of the A address for this slice
            const int tap = (FWDLIKE ? (r * p.sw + s) : -(r * p.sw + s)) * p.lda + c0;
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                int iy, ix;
                if (FWDLIKE) { iy = a_y[i] + r; ix = a_x[i] + s + (gStem ? (cc >> 2) : 0); }
                else { iy = a_y[i] - r; ix = a_x[i] - s; }
                const bool ok = c_ok && (unsigned)iy < (unsigned)p.sh && (unsigned)ix < (unsigned)p.sw;
                ldA(i, ok ? 4u * (a_base[i] + (unsigned)tap) : kOOB);
            }
            if (FWDLIKE) {
                const unsigned wofs = (unsigned)(rs * p.Kc + c0);
#pragma unroll
                for (int i = 0; i < BV; ++i) ldB(i, cc < p.Kc ? 4u * (b_base[i] + wofs) : kOOB);
            } else {
                const unsigned wofs = (unsigned)(c0 * p.ldb + rs * p.cin);
#pragma unroll
                for (int i = 0; i < BV; ++i) {
                    const int k = c0 + wb_k + B_RPP * i;
                    rb[i] = bload4(rB, k < p.Kc ? 4u * (b_base[i] + wofs) : kOOB);
                }
            }
        } else {
            const int kb = k_begin + kt * BK;
            if (WPERM) {
                // A and B rows of a thread are the same k rows (BM == BN); the slice's image
                // block and position are wave-uniform
                const int sidx = kb / BK;
                const int blk = sidx / max(wnv, 1), pos = sidx - blk * max(wnv, 1);
                const int yv = pos / max(wnvx, 1);
                const int y = wy_lo + yv, x = wx_lo + pos - yv * wnvx;
                const int a_col = m0 + wa_c4 * 4;
                const int pix_a = y * p.gq + x;
                const int pix_b = (y + wr_u - gPad) * p.sw + x + ws_u - gPad;
#pragma unroll
                for (int i = 0; i < BV; ++i) {
                    const int r = wb_k + B_RPP * i;
                    const int n = blk * BK + r;
                    const bool ok = kb + r < k_end && n < gPermN;
                    const unsigned offa = (unsigned)((n * (p.gp * p.gq) + pix_a) * p.ldg + a_col);
                    ra[i] = bload4(rA, ok && a_col < p.M ? 4u * offa : kOOB);
                    const unsigned offb = (unsigned)((n * (p.sh * p.sw) + pix_b) * p.lda + wc);
                    rb[i] = bload4(rB, ok && wcol_ok ? 4u * offb : kOOB);
                }
                return;
            }
            const unsigned gofs = (unsigned)(kb * p.ldg);
#pragma unroll
            for (int i = 0; i < AV; ++i) {
                const int m = kb + a_krow(i);
                ra[i] = bload4(rA, m < k_end ? 4u * (a_base[i] + gofs) : kOOB);
            }
            if (wpoint) {
                // 1x1 / stride 1: pixel m of gy is pixel m of x
                const unsigned xofs = (unsigned)(kb * p.lda);
#pragma unroll
                for (int i = 0; i < BV; ++i) {
                    const int m = kb + b_krow(i);
                    rb[i] = bload4(rB, m < k_end ? 4u * (b_base[i] + xofs) : kOOB);
                }
                return;
            }
#pragma unroll
            for (int i = 0; i < BV; ++i) {
                const int m = kb + b_krow(i);
                const int iy = py[i] * gStride - gPad + wr;
                const int ix = px[i] * gStride - gPad + ws_;
                const bool ok = wcol_ok && m < k_end && (unsigned)iy < (unsigned)p.sh &&
                                (unsigned)ix < (unsigned)p.sw;
                rb[i] = bload4(rB, ok ? 4u * (unsigned)(((pn[i] * p.sh + iy) * p.sw + ix) * p.lda + wc)
                                      : kOOB);
                // advance this row's pixel by BK for the next slice (two carries, no loops:
                // adv_x = BK % gq, adv_y = (BK / gq) % gp, adv_n = BK / (gp*gq))
                px[i] += adv_x;
                const int cx = px[i] >= p.gq;
                px[i] -= cx ? p.gq : 0;
                py[i] += adv_y + cx;
                const int cy = py[i] >= p.gp;
                py[i] -= cy ? p.gp : 0;
                pn[i] += adv_n + cy;
            }
        }
    };

    // registers -> LDS
    auto store_slice = [&](int buf) {
        if constexpr (SPLIT) {
            unsigned short *pa = reinterpret_cast<unsigned short *>(smem[buf]);
            unsigned short *pb = pa + 3 * PLA;
            auto put = [&](unsigned short *plane0, int plane_len, int row, float4 v) {
                unsigned h0, m0_, l0, h1, m1, l1;
                split3<NP>(v.x, v.y, h0, m0_, l0);
                split3<NP>(v.z, v.w, h1, m1, l1);
                unsigned short *q = plane0 + row * SROW + ((kc_c4 ^ swz(row)) << 2);
                *reinterpret_cast<uint2 *>(q) = make_uint2(h0, h1);
                if constexpr (NP >= 2) *reinterpret_cast<uint2 *>(q + plane_len) = make_uint2(m0_, m1);
                if constexpr (NP >= 3) *reinterpret_cast<uint2 *>(q + 2 * plane_len) = make_uint2(l0, l1);
            };
            if constexpr (MODE == WGRAD) {
                // a thread holds 4 channels x 4 consecutive pixels: transposed in registers, one
                // 8-byte write per channel and plane at [channel][pixel chunk ^ swz(channel)]
                static_assert(AV == 4 && BV == 4, "SPLIT WGRAD: 128x128 tiles");
                auto put_t = [&](unsigned short *plane0, int plane_len, int row0, int kchunk,
                                 const float4 (&r)[4]) {
                    auto e = [&](int i, int c) { return c == 0 ? r[i].x : c == 1 ? r[i].y : c == 2 ? r[i].z : r[i].w; };
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        unsigned h0, m0_, l0, h1, m1, l1;
                        split3<NP>(e(0, c), e(1, c), h0, m0_, l0);
                        split3<NP>(e(2, c), e(3, c), h1, m1, l1);
                        const int row = 32 * c + (row0 >> 2);      // channel row0 + c (WROWPERM)
                        unsigned short *q = plane0 + row * SROW + ((kchunk ^ swz(row)) << 2);
                        *reinterpret_cast<uint2 *>(q) = make_uint2(h0, h1);
                        if constexpr (NP >= 2) *reinterpret_cast<uint2 *>(q + plane_len) = make_uint2(m0_, m1);
                        if constexpr (NP >= 3) *reinterpret_cast<uint2 *>(q + 2 * plane_len) = make_uint2(l0, l1);
                    }
                };
                put_t(pa, PLA, wa_c4 * 4, wa_k, ra);
                put_t(pb, PLB, wb_c4 * 4, wb_k, rb);
                return;
            }
#pragma unroll
            for (int i = 0; i < AV; ++i) {
                put(pa, PLA, kc_row + KC_RPP * i, ra[i]);
            }
#pragma unroll
            for (int i = 0; i < BV; ++i) {
                put(pb, PLB, kc_row + KC_RPP * i, rb[i]);
            }
            return;
        }
        float *sa = smem[buf];
        float *sb = smem[buf] + C_::A_FLOATS;
#pragma unroll
        for (int i = 0; i < AV; ++i) {
            if (C_::A_KC)
                *reinterpret_cast<float4 *>(sa + (kc_row + KC_RPP * i) * (BK + KPAD) + kc_c4 * 4) = ra[i];
            else
                *reinterpret_cast<float4 *>(sa + (wa_k + A_RPP * i) * BM + wa_c4 * 4) = ra[i];
        }
        if (C_::B_KC) {
#pragma unroll
            for (int i = 0; i < BV; ++i)
                *reinterpret_cast<float4 *>(sb + (kc_row + KC_RPP * i) * (BK + KPAD) + kc_c4 * 4) = rb[i];
        } else {
#pragma unroll
            for (int i = 0; i < BV; ++i)
                *reinterpret_cast<float4 *>(sb + (wb_k + B_RPP * i) * BN + wb_c4 * 4) = rb[i];
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    const int li = lane & 31, lk = lane >> 5;

    // LDS -> MFMA fragments for the 8-deep K block kb of buffer `buf`
    auto load_frag = [&](const float *sa, const float *sb, int kb, float (&af)[TM][4],
                         float (&bf)[TN][4]) {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int row = wm * (32 * TM) + i * 32 + li;
            if (C_::A_KC) {
                const float4 v = *reinterpret_cast<const float4 *>(
                    sa + row * (BK + KPAD) + kb * 8 + lk * 4);
                af[i][0] = v.x; af[i][1] = v.y; af[i][2] = v.z; af[i][3] = v.w;
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t) af[i][t] = sa[(kb * 8 + lk * 4 + t) * BM + row];
            }
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int col = wn * (32 * TN) + j * 32 + li;
            if (C_::B_KC) {
                const float4 v = *reinterpret_cast<const float4 *>(
                    sb + col * (BK + KPAD) + kb * 8 + lk * 4);
                bf[j][0] = v.x; bf[j][1] = v.y; bf[j][2] = v.z; bf[j][3] = v.w;
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t) bf[j][t] = sb[(kb * 8 + lk * 4 + t) * BN + col];
            }
        }
    };

    // one K slice: fragments of block kb+1 are fetched while block kb's MFMAs issue
    auto compute_ = [&](int buf, auto issue_tag) {
        constexpr bool ISSUE = decltype(issue_tag)::value;   // issue the next slice's loads here
        if constexpr (SPLIT) {
            const unsigned short *pa = reinterpret_cast<const unsigned short *>(smem[buf]);
            const unsigned short *pb = pa + 3 * PLA;
            // (the stage keeps its three-plane layout for every NP: planes NP .. 2 are never touched)
            constexpr int NQ = SPLIT ? NP : 1;
            bf16x8 fa[2][TM][NQ], fb[2][TN][NQ];
            auto frag = [&](int ks, bf16x8 (&a)[TM][NQ], bf16x8 (&b)[TN][NQ]) {
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int q = 0; q < NQ; ++q)
                        a[i][q] = *reinterpret_cast<const bf16x8 *>(
                            pa + q * PLA + (wm * (32 * TM) + i * 32 + li) * SROW +
                            (((ks * 4 + lk * 2) ^ swz(wm * (32 * TM) + i * 32 + li)) << 2));
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int q = 0; q < NQ; ++q)
                        b[j][q] = *reinterpret_cast<const bf16x8 *>(
                            pb + q * PLB + (wn * (32 * TN) + j * 32 + li) * SROW +
                            (((ks * 4 + lk * 2) ^ swz(wn * (32 * TN) + j * 32 + li)) << 2));
            };
            frag(0, fa[0], fb[0]);
            if constexpr (ISSUE) issue_loads();
#pragma unroll
            for (int ks = 0; ks < BK / 16; ++ks) {
                if (ks + 1 < BK / 16) frag(ks + 1, fa[(ks + 1) & 1], fb[(ks + 1) & 1]);
                // smallest terms first: (hi,lo) (lo,hi) (mid,mid) (mid,hi) (hi,mid) (hi,hi); NP planes
                // issue the last NPROD of them, the products of the planes they stage
                constexpr int QA[6] = {0, 2, 1, 1, 0, 0}, QB[6] = {2, 0, 1, 0, 1, 0};
#pragma unroll
                for (int c = 6 - NPROD; c < 6; ++c)
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                                fa[ks & 1][i][QA[c]], fb[ks & 1][j][QB[c]], acc[i][j], 0, 0, 0);
            }
            if constexpr (ILV && !ISSUE) {
                // (W8, waves that multiply first: their next slice's loads are issued after the store)
                // first fragments, then one fragment read of the second K step per two MFMAs
                constexpr int NFR = NQ * (TM + TN), NMH = NPROD * TM * TN;
                __builtin_amdgcn_sched_group_barrier(0x100, NFR, 0);
#pragma unroll
                for (int g = 0; g < NFR; ++g) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                }
                constexpr int REST = NMH * (BK / 16) - 2 * NFR;     // (W8: 24 / 8 / 0 for 3 / 2 / 1 planes)
                static_assert(REST >= 0, "two MFMAs per fragment read");
                if constexpr (REST > 0) __builtin_amdgcn_sched_group_barrier(0x008, REST, 0);
            } else if constexpr (ILV) {
                // issue order: first fragments, then the first K step's MFMAs with one global load
                // and the second K step's fragment reads dealt out between them, then the rest
                constexpr int NFR = NQ * (TM + TN), NMH = NPROD * TM * TN;
                // MFMAs the second K step's fragment reads are dealt out over (one plane: fewer MFMAs
                // in the first K step than the two tile rows held back — behind its first group)
                constexpr int NMD = NMH * (BK / 16 - 1) - 2 * TM * TN > 0 ? NMH * (BK / 16 - 1) - 2 * TM * TN : 1;
                __builtin_amdgcn_sched_group_barrier(0x100, NFR, 0);
                // the CU's texture path takes ~64 cycles per 16-byte-per-lane wave load whoever
                // issues it (tools/exp/planes_probe.py ablations: kernel time = compute + 64 cycles
                // x loads): a wave whose load waits for its slot issues no MFMA either, so the
                // loads sit as far apart as the slice allows — one per NM / (NA + NB) MFMAs
                sgb_interleave<NA + NB, NMH * (BK / 16), NMD, NFR>();
            }
            return;
        }
        const float *sa = smem[buf];
        const float *sb = smem[buf] + C_::A_FLOATS;
        float af[2][TM][4], bf[2][TN][4];
        load_frag(sa, sb, 0, af[0], bf[0]);
        // DS read instructions per K block (b32 pairs are merged into ds_read2_b32)
        constexpr int NR = (C_::A_KC ? TM : 2 * TM) + (C_::B_KC ? TN : 2 * TN);
        constexpr int NMFMA = 4 * TM * TN;
        __builtin_amdgcn_sched_group_barrier(0x100, NR, 0);
#pragma unroll
        for (int kb = 0; kb < BK / 8; ++kb) {
            if (kb + 1 < BK / 8) load_frag(sa, sb, kb + 1, af[(kb + 1) & 1], bf[(kb + 1) & 1]);
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(
                            af[kb & 1][i][t], bf[kb & 1][j][t], acc[i][j], 0, 0, 0);
            // pin the issue order: the next block's LDS reads ride behind this block's first
            // MFMAs instead of being sunk in front of their consumers (which exposes the
            // LDS latency once per 4 MFMAs)
            if (kb + 1 < BK / 8) {
#define MRCNN_SGB_STEP(q)                                         \
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);            \
    __builtin_amdgcn_sched_group_barrier(0x100, (NR + 3 - (q)) / 4, 0);
                MRCNN_SGB_STEP(0) MRCNN_SGB_STEP(1) MRCNN_SGB_STEP(2) MRCNN_SGB_STEP(3)
#undef MRCNN_SGB_STEP
                __builtin_amdgcn_sched_group_barrier(0x008, NMFMA - 4, 0);
            } else {
                __builtin_amdgcn_sched_group_barrier(0x008, NMFMA, 0);
            }
        }
    };
    auto compute = [&](int buf) { compute_(buf, std::true_type()); };

    if (nslices > 0) {
        load_slice(0);
        issue_loads();
        store_slice(0);
    }
    if constexpr (W8) {
        // (see the W8 note above the kernel) stage k & 1 holds slice k; slice k + 1 is in registers
        // (or in flight) while slice k is multiplied
        auto no_loads = [&]() {
#pragma unroll
            for (int i = 0; i < NA; ++i) oa[i] = kOOB;
#pragma unroll
            for (int i = 0; i < NB; ++i) ob[i] = kOOB;
        };
        if (nslices > 1) {
            load_slice(1);
            issue_loads();
        }
        __syncthreads();
        const bool stage_first = wave >= 4;               // wave-uniform
        for (int kt = 0; kt < nslices; ++kt) {
            const int cur = kt & 1;
            const bool more = kt + 1 < nslices;
            if (stage_first) {
                if (more) store_slice(cur ^ 1);
                if (kt + 2 < nslices) load_slice(kt + 2); else no_loads();
                compute_(cur, std::true_type());          // (issues the loads of slice k + 2)
            } else {
                compute_(cur, std::false_type());
                if (more) store_slice(cur ^ 1);
                if (kt + 2 < nslices) {
                    load_slice(kt + 2);
                    issue_loads();
                }
            }
            __syncthreads();
        }
    } else if (SINGLEBUF) {
        // one LDS stage (37 KB -> three workgroups per CU, three waves per SIMD): a wave spends
        // ~40 % of a slice issuing MFMAs and ~60 % staging, so three interleaved waves are
        // needed to keep the pipe full; two barriers per slice instead of one.
        for (int kt = 0; kt < nslices; ++kt) {
            if (kt > 0) {
                __syncthreads();          // every wave is done reading the stage
                store_slice(0);
            }
            __syncthreads();
            if (kt + 1 < nslices) {
                load_slice(kt + 1);
            } else if constexpr (ILV) {      // (compute() issues the loads: none left)
#pragma unroll
                for (int i = 0; i < NA; ++i) oa[i] = kOOB;
#pragma unroll
                for (int i = 0; i < NB; ++i) ob[i] = kOOB;
            }
            compute(0);
        }
    } else {
        __syncthreads();
        for (int kt = 0; kt < nslices; ++kt) {
            const bool more = kt + 1 < nslices;
            if (more) load_slice(kt + 1);
            compute(kt & 1);
            if (more) store_slice((kt + 1) & 1);
            __syncthreads();
        }
    }

    // ---------------- epilogue ------------------------------------------------------
    // Per 32x32 MFMA tile: compute the 16 element offsets, issue every auxiliary load
    // (residual / accumulate / shortcut gradient) back to back, then combine and store.
    const float *out_base = tail ? p.tail_ws + (int64_t)split * p.tail_stride
                                 : p.C + zb * p.batch_c + (int64_t)split * p.split_stride;
    const __amdgpu_buffer_rsrc_t rC = make_rsrc(out_base, tail ? p.tail_bytes : p.c_bytes);
    const int e_flags = tail ? 0 : p.flags;              // tail pieces store raw partial sums
    const int e_row0 = tail ? p.tail_row0 : p.out_row0;
    const int e_ldc = tail ? p.N : p.ldc;
    const bool slab_rows = MODE != WGRAD && split_len > 0;   // slabs are indexed by GEMM row
    const __amdgpu_buffer_rsrc_t rRes = make_rsrc(p.residual, p.c_bytes);
    const __amdgpu_buffer_rsrc_t rResG = make_rsrc(p.res_g, p.c_bytes);
    const __amdgpu_buffer_rsrc_t rResY = make_rsrc(p.res_y, p.c_bytes);
    const __amdgpu_buffer_rsrc_t rOutM = make_rsrc(p.out_mask_y, p.c_bytes);
    const bool f_bias = (e_flags & MRCNN_EPI_BIAS) != 0, f_aff = (e_flags & MRCNN_EPI_AFFINE) != 0;
    const bool f_res = (e_flags & MRCNN_EPI_RESIDUAL) != 0, f_relu = (e_flags & MRCNN_EPI_RELU) != 0;
    const bool f_acc = (e_flags & MRCNN_EPI_ACCUM) != 0;
    const bool f_resg = MODE != WGRAD && !tail && p.res_g != nullptr;
    const bool f_resy = f_resg && p.res_y != nullptr;
    const bool f_outm = MODE != WGRAD && !tail && p.out_mask_y != nullptr;
    constexpr int EG = 8;       // accumulator rows handled per batch of auxiliary loads

    // (PW / W8 launches write plain rows in natural order by the host's rule)
    if (MODE == FWD && TM >= 2 && (GEO || p.out_mode == OUT_PLAIN)) {   // (uniform)
      if constexpr (MODE == FWD && TM >= 2) {
        // Forward-form launches: the accumulators (one column x 16 rows per lane) are turned
        // into row-major float4s through the wave's corner of the LDS stages, so the residual
        // / mask reads and the output stores are 16 B per lane — a quarter of the memory
        // instructions of the per-element path below.  K-short layers (a bottleneck's conv3:
        // 16 K slices, 411 MB written + 411 MB residual read) spend a quarter of their time here.
        constexpr int CW = 32 * TN;                 // columns of the wave's quadrant
        constexpr int LDW = CW + 4;                 // padded LDS row
        constexpr int F4 = CW / 4, RPI = 64 / F4;   // float4 per row, rows per pass of the wave
        constexpr int NK = 32 / RPI;                // passes per 32-row half
        constexpr int QG = TM >= 2 ? 4 : 2;         // passes whose loads are in flight together
        __syncthreads();                            // every wave is done with the K loop's LDS
        float *ep = &smem_all[0][0][0] + wave * (32 * LDW);
        const int c4 = lane % F4, r_in = lane / F4;
        const int col = n0 + wn * CW + c4 * 4;
        const bool col_ok = col < p.N;
        float4 bias4 = make_float4(0.f, 0.f, 0.f, 0.f), scale4 = make_float4(1.f, 1.f, 1.f, 1.f);
        float4 shift4 = bias4;
        if (col_ok) {
            if (f_bias) bias4 = *reinterpret_cast<const float4 *>(p.bias + col);
            if (f_aff) {
                scale4 = *reinterpret_cast<const float4 *>(p.scale + col);
                if (p.shift) shift4 = *reinterpret_cast<const float4 *>(p.shift + col);
            }
        }
        // The combine step is specialised at compile time for the flag combinations the model
        // launches (F >= 0: bit k of F = flag k below), selected by ONE workgroup-uniform switch:
        // with run-time flags every element went through a chain of eight add / select pairs
        // (about 120 VALU instructions per 16-byte store, a quarter of a 16-slice tile's
        // lifetime); F = -1 keeps that generic path for any other combination.  The operation
        // order per element is the same in every instantiation, so results are bit-identical.
        enum { C_BIAS = 1, C_AFF = 2, C_RES = 4, C_RELU = 8, C_ACC = 16, C_RESG = 32, C_RESY = 64,
               C_OUTM = 128 };
        auto run = [&](auto tag) {
            constexpr int F = decltype(tag)::value;
            const bool c_bias = F >= 0 ? (F & C_BIAS) != 0 : f_bias;
            const bool c_aff = F >= 0 ? (F & C_AFF) != 0 : f_aff;
            const bool c_res = F >= 0 ? (F & C_RES) != 0 : f_res;
            const bool c_relu = F >= 0 ? (F & C_RELU) != 0 : f_relu;
            const bool c_acc = F >= 0 ? (F & C_ACC) != 0 : f_acc;
            const bool c_resg = F >= 0 ? (F & C_RESG) != 0 : f_resg;
            const bool c_resy = F >= 0 ? (F & C_RESY) != 0 : f_resy;
            const bool c_outm = F >= 0 ? (F & C_OUTM) != 0 : f_outm;
            const bool natural = F >= 0 || GEO || !(gPermN > 0 && !slab_rows);   // F >= 0: natural row order
#pragma unroll
            for (int i = 0; i < TM; ++i) {
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e)
                        ep[((e & 3) + 8 * (e >> 2) + 4 * lk) * LDW + j * 32 + li] = acc[i][j][e];
                // same wave writes and reads: LDS operations of a wave execute in order
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
                for (int kg = 0; kg < NK; kg += QG) {
                    unsigned off[QG];
                    float4 v[QG], a0[QG], a1[QG], a2[QG], a3[QG];
#pragma unroll
                    for (int q = 0; q < QG; ++q) {
                        const int r = (kg + q) * RPI + r_in;
                        v[q] = *reinterpret_cast<const float4 *>(ep + r * LDW + c4 * 4);
                        const int row = m0 + wm * (32 * TM) + i * 32 + r;
                        int orow;
                        if (!natural) {
                            const PermRow pr = perm_row(row < p.M ? row : 0, p.gp * p.gq);
                            orow = pr.n < gPermN ? pr.n * (p.gp * p.gq) + pr.pos : -1;
                        } else {
                            orow = row - e_row0;
                        }
                        const bool ok = col_ok && row < p.M && orow >= 0;
                        off[q] = ok ? 4u * (unsigned)(orow * e_ldc + col) : kOOB;
                    }
                    if (c_res) {
#pragma unroll
                        for (int q = 0; q < QG; ++q) a0[q] = bload4(rRes, off[q]);
                    }
                    if (c_acc) {
#pragma unroll
                        for (int q = 0; q < QG; ++q) a1[q] = bload4(rC, off[q]);
                    }
                    if (c_resg) {
#pragma unroll
                        for (int q = 0; q < QG; ++q) a0[q] = bload4(rResG, off[q]);
                    }
                    if (c_resy) {
#pragma unroll
                        for (int q = 0; q < QG; ++q) a2[q] = bload4(rResY, off[q]);
                    }
                    if (c_outm) {
#pragma unroll
                        for (int q = 0; q < QG; ++q) a3[q] = bload4(rOutM, off[q]);
                    }
#pragma unroll
                    for (int q = 0; q < QG; ++q) {
                        float x[4] = {v[q].x, v[q].y, v[q].z, v[q].w};
                        const float b[4] = {bias4.x, bias4.y, bias4.z, bias4.w};
                        const float sc[4] = {scale4.x, scale4.y, scale4.z, scale4.w};
                        const float sh[4] = {shift4.x, shift4.y, shift4.z, shift4.w};
                        const float r0[4] = {a0[q].x, a0[q].y, a0[q].z, a0[q].w};
                        const float r1[4] = {a1[q].x, a1[q].y, a1[q].z, a1[q].w};
                        const float r2[4] = {a2[q].x, a2[q].y, a2[q].z, a2[q].w};
                        const float r3[4] = {a3[q].x, a3[q].y, a3[q].z, a3[q].w};
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            float y = x[t];
                            if (c_bias) y += b[t];
                            if (c_aff) y = y * sc[t] + sh[t];
                            if (c_res) y += r0[t];
                            if (c_acc) y += r1[t];
                            if (c_resy) y += r2[t] > 0.f ? r0[t] : 0.f;
                            else if (c_resg) y += r0[t];
                            if (c_relu) y = fmaxf(y, 0.f);
                            if (c_outm) y = r3[t] > 0.f ? y : 0.f;
                            x[t] = y;
                        }
                        bstore4(rC, off[q], make_float4(x[0], x[1], x[2], x[3]));
                    }
                }
            }
        };
        const int combo = (f_bias ? C_BIAS : 0) | (f_aff ? C_AFF : 0) | (f_res ? C_RES : 0) |
                          (f_relu ? C_RELU : 0) | (f_acc ? C_ACC : 0) | (f_resg ? C_RESG : 0) |
                          (f_resy ? C_RESY : 0) | (f_outm ? C_OUTM : 0);
        const bool permuted = !GEO && gPermN > 0 && !slab_rows;
#define MRCNN_EPI_CASE(F) case (F): run(std::integral_constant<int, (F)>()); break;
        switch (permuted ? -1 : combo) {       // workgroup-uniform
            MRCNN_EPI_CASE(0)
            MRCNN_EPI_CASE(C_AFF)
            MRCNN_EPI_CASE(C_AFF | C_RELU)
            MRCNN_EPI_CASE(C_AFF | C_RES | C_RELU)
            MRCNN_EPI_CASE(C_BIAS)
            MRCNN_EPI_CASE(C_BIAS | C_RELU)
            MRCNN_EPI_CASE(C_AFF | C_OUTM)
            MRCNN_EPI_CASE(C_RESG | C_OUTM)
            MRCNN_EPI_CASE(C_RESG)
            MRCNN_EPI_CASE(C_ACC | C_OUTM)
            MRCNN_EPI_CASE(C_ACC)
        default: run(std::integral_constant<int, -1>()); break;
        }
#undef MRCNN_EPI_CASE
        return;
      }
    }
    if constexpr (WROWPERM) {
        // tile rows / columns are in plane-row order: fragment row 32 c + l = channel 4 l + c.  A
        // lane's two column tiles (j = 0, 1) are the ADJACENT columns 4 li + 2 wn + j: one 8-byte
        // store per accumulator row.
        static_assert(TM == 2 && TN == 2, "SPLIT WGRAD: 128x128 tiles");
        const int col = n0 + 4 * li + 2 * wn;
        const bool col_ok = col < p.N;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int g = 0; g < 16 / EG; ++g) {
                unsigned off[EG];
                float row_scale[EG];
#pragma unroll
                for (int q = 0; q < EG; ++q) {
                    const int e = g * EG + q;
                    const int row = m0 + 4 * ((e & 3) + 8 * (e >> 2) + 4 * lk) + 2 * wm + i;
                    off[q] = (col_ok && row < p.M) ? 4u * (unsigned)(row * e_ldc + col) : kOOB;
                    row_scale[q] = (p.scale && row < p.M) ? p.scale[row] : 1.f;
                }
#pragma unroll
                for (int q = 0; q < EG; ++q) {
                    const float v0 = acc[i][0][g * EG + q] * row_scale[q];
                    const float v1 = acc[i][1][g * EG + q] * row_scale[q];
                    bstore8(rC, off[q], __float_as_uint(v0), __float_as_uint(v1));
                }
            }
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int col = n0 + wn * (32 * TN) + j * 32 + li;
        const bool col_ok = col < p.N;
        const int colc = col_ok ? col : 0;
        float bias = 0.f, scale = 1.f, shift = 0.f;
        if (MODE != WGRAD) {
            if (f_bias) bias = p.bias[!GEO && p.out_mode == OUT_DECONV ? colc % p.ko : colc];
            if (f_aff) { scale = p.scale[colc]; shift = p.shift ? p.shift[colc] : 0.f; }
        }
        int col_off = colc;
        if (MODE != WGRAD && !GEO && p.out_mode == OUT_DECONV) {
            const int ab = colc / p.ko, o = colc - ab * p.ko;
            col_off = ((ab >> 1) * (2 * p.gq) + (ab & 1)) * p.ko + o;
        }
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int g = 0; g < 16 / EG; ++g) {  // groups of EG accumulator rows
                unsigned off[EG];
#pragma unroll
                for (int q = 0; q < EG; ++q) {
                    const int e = g * EG + q;
                    const int row = m0 + wm * (32 * TM) + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lk;
                    int o;
                    if (MODE != WGRAD && !GEO && p.out_mode != OUT_PLAIN) {
                        const int rr = row < p.M ? row : 0;
                        const int n = rr / (p.gp * p.gq);
                        const int rem = rr - n * (p.gp * p.gq);
                        const int gy = rem / p.gq, gx = rem - gy * p.gq;
                        if (p.out_mode == OUT_STRIDED)
                            o = ((n * p.oh + gy * (p.ostride ? p.ostride : gStride)) * p.ow +
                                 gx * (p.ostride ? p.ostride : gStride)) * p.ldc + col_off;
                        else
                            o = ((n * (2 * p.gp) + 2 * gy) * (2 * p.gq) + 2 * gx) * p.ko + col_off;
                    } else if (FWDLIKE && !GEO && gPermN > 0 && !slab_rows) {
                        // position-major GEMM row -> (image, position) row of the NHWC tensor
                        // (split-K slabs stay indexed by GEMM row; the slab-sum kernel maps)
                        const PermRow pr = perm_row(row < p.M ? row : 0, p.gp * p.gq);
                        o = pr.n < gPermN ? (pr.n * (p.gp * p.gq) + pr.pos) * p.ldc + col_off : -1;
                    } else {
                        o = (row - e_row0) * e_ldc + col_off;
                    }
                    off[q] = (col_ok && row < p.M && o >= 0) ? 4u * (unsigned)o : kOOB;
                }
                float aux0[EG], aux1[EG], aux2[EG], aux3[EG];
                if (MODE != WGRAD) {
                    if (f_res) {
#pragma unroll
                        for (int q = 0; q < EG; ++q) aux0[q] = bload1(rRes, off[q]);
                    }
                    if (f_acc) {
#pragma unroll
                        for (int q = 0; q < EG; ++q) aux1[q] = bload1(rC, off[q]);
                    }
                    if (f_resg) {
#pragma unroll
                        for (int q = 0; q < EG; ++q) aux0[q] = bload1(rResG, off[q]);
                    }
                    if (f_resy) {
#pragma unroll
                        for (int q = 0; q < EG; ++q) aux2[q] = bload1(rResY, off[q]);
                    }
                    if (f_outm) {
#pragma unroll
                        for (int q = 0; q < EG; ++q) aux3[q] = bload1(rOutM, off[q]);
                    }
                }
                float row_scale[EG];
                if (MODE == WGRAD && p.scale) {
#pragma unroll
                    for (int q = 0; q < EG; ++q) {
                        const int e = g * EG + q;
                        const int row = m0 + wm * (32 * TM) + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lk;
                        row_scale[q] = row < p.M ? p.scale[row] : 0.f;
                    }
                }
#pragma unroll
                for (int q = 0; q < EG; ++q) {
                    float v = acc[i][j][g * EG + q];
                    if (MODE != WGRAD) {
                        if (f_bias) v += bias;
                        if (f_aff) v = v * scale + shift;
                        if (f_res) v += aux0[q];
                        if (f_acc) v += aux1[q];
                        if (f_resy) v += aux2[q] > 0.f ? aux0[q] : 0.f;
                        else if (f_resg) v += aux0[q];
                        if (f_relu) v = fmaxf(v, 0.f);
                        if (f_outm) v = aux3[q] > 0.f ? v : 0.f;
                    } else if (p.scale) {
                        v *= row_scale[q];
                    }
                    bstore1(rC, off[q], v);
                }
            }
        }
    }
}

}  // namespace
