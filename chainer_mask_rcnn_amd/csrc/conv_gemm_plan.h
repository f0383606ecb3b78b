// Launch policy of the convolution GEMM family: how one GEMM problem is cut into kernel launches.
//
// Plain C++17 and pure: a GemmPlan is a function of the problem's shape (GemmShape) and the
// mrcnn_set_tuning knobs (GemmKnobs) alone, so it can be computed, swept and compared where there is
// no device.  conv_gemm.hip builds the shape from a descriptor, runs the plan (run_plan) and prints it
// (mrcnn_conv_gemm_plan); tests/test_gemm_edge_cases_cpu.py holds it to tests/gemm_edge_cases.route().
// The Winograd route's launches (conv_winograd.h) have a policy of their own at the end of this file,
// planned, run, printed and tested the same way.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>

namespace mrcnn {
namespace gemm {

constexpr int BK = 32;                 // K slice staged per step
// The stride-1 dgrad is also run in FWD mode: a forward convolution of gy with the flipped,
// transposed filter (both operands K-contiguous).
enum Mode { FWD = 0, DGRAD = 1, WGRAD = 2 };
enum OutMode { OUT_PLAIN = 0, OUT_STRIDED = 1, OUT_DECONV = 2 };
// Workgroups resident at once: 128x128 tiles run 2 per CU (73 KB LDS), 64x64 tiles 4 per CU.
constexpr int64_t kSlotsBig = 512, kSlotsSmall = 1024;
constexpr int64_t kSplitWsBytes = 192ll << 20;   // >= 154 leftover tiles x 16 slabs; whole small-M outputs x splits
constexpr int kPermBlock = 128;        // images per block of the position-major row order (GemmParams::perm_n)
constexpr int kW8BM = 256, kW8BN = 128;   // W8 tile (see the note above conv_gemm_kernel)

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// The forward-form kernel fits 168 registers, so it runs with ONE LDS stage (37 KB) and three
// workgroups per CU: a wave spends ~40 % of a K slice issuing MFMAs and ~60 % staging (measured
// with s_memtime), so three interleaved waves per SIMD keep the pipe fuller than two (res5 3x3:
// 129 vs 122 TFLOP/s).  The K-strided DGRAD gather would spill at 168 and keeps two stages / two
// workgroups per CU.
constexpr bool single_buffered(int tm, int mode)
{
    if (tm == 1) return mode == 0;
    return tm >= 2 && (mode == 0 || mode == 2);
}

// mrcnn_set_tuning's GEMM switches (include/mrcnn_hip.h describes them)
struct GemmKnobs {
    int split_bf16 = 3;            // bit 0: 128x128 kernels, bit 1: 64x64 forward form on the split-operand
                                   // arithmetic (see SPLIT); 0 = fp32 MFMA everywhere
    int split_planes = 3;          // bf16 planes per operand of those launches (conv_gemm_kernel's NP): 3, 2 or 1.
                                   // Read by pick_inst() alone: the plan is the same for all three
    int big_split_k = -1;          // small-M problems as 128x128 tiles cut along K: -1 = the one-round rule of
                                   // plan_gemm(), 0 = off (64x64 tiles), k > 0 = aim at k workgroups
    int big_split_min_slices = 16; // fewest K slices per slab of the one-round rule
    int w8 = 1, w8_min_k = 256;    // W8 launches on / off, the shallowest K (input channels) they take
    int pw = 3;                    // bit 0: the PW instantiations, bit 1: the K3 instantiations
    int fused_tail = 512;          // 0 = off, else target number of tail pieces
    int big_min_tiles = 384;       // fewest 128x128 tiles that get 128x128 tiles
    int small_m_split = 0;         // target workgroups per CU (0 = off)
    int tiny_split = 1;            // K-split of launches with <= 128 tiles and >= 32 slices
    int position_major_rows = 1;   // position-major GEMM rows (choose_perm)
};

// Is `value` legal for the knob called `name`?  (Knobs without a closed value set take any.)
inline bool knob_value_ok(const char *name, int value)
{
    return strcmp(name, "split_planes") != 0 || (value >= 1 && value <= 3);
}

// Sets the knob called `name`; false when it is not one of GemmKnobs'.
inline bool set_knob(GemmKnobs &k, const char *name, int value)
{
    const struct { const char *name; int *at; } table[] = {
        {"split_bf16", &k.split_bf16}, {"split_planes", &k.split_planes}, {"big_split_k", &k.big_split_k},
        {"big_split_min_slices", &k.big_split_min_slices}, {"w8_min_k", &k.w8_min_k}, {"w8", &k.w8},
        {"pw", &k.pw}, {"fused_tail", &k.fused_tail}, {"big_min_tiles", &k.big_min_tiles},
        {"small_m_split", &k.small_m_split}, {"tiny_split", &k.tiny_split},
        {"position_major_rows", &k.position_major_rows}};
    for (const auto &t : table) {
        if (strcmp(name, t.name) != 0) continue;
        if (t.at == &k.fused_tail) value = value == 1 ? 512 : value;
        if (t.at == &k.position_major_rows) value = value != 0;
        *t.at = value;
        return true;
    }
    return false;
}

// What the policy reads of a problem (the fields of GemmParams of the same names)
struct GemmShape {
    int mode;                  // Mode
    int M, N, Kc;
    int R, S, stride, pad;
    int gp, gq, sh, sw;
    int ldc, out_mode, stem, perm_n;
    bool has_ws;               // the caller gave a split-K workspace
    // weight gradient only (M = K_out, N = R S C, gp x gq = P x Q; plan_wgrad() chooses perm_n)
    int64_t pixels;
    int n_img, C;
};

// Position-major row order (GemmParams::perm_n) pays when many small maps are convolved with
// a padded filter: n_img maps of gp x gq output positions, pad_eff = padding of the gathered
// tensor as the forward-form kernel sees it.
inline int choose_perm(const GemmKnobs &k, int n_img, int gp, int gq, int R, int S, int stride, int pad_eff)
{
    if (!k.position_major_rows || R * S <= 1 || R * S > 16 || stride != 1 || pad_eff <= 0) return 0;
    if (gp * gq > 256 || n_img < 64) return 0;
    return n_img;
}

// PW's launch rule (see the note above conv_gemm_kernel)
inline bool pw_plain(const GemmShape &p)
{
    return p.R == 1 && p.S == 1 && p.stride == 1 && p.pad == 0 && p.perm_n == 0 && !p.stem && p.gp == p.sh &&
           p.gq == p.sw && p.out_mode == OUT_PLAIN;
}

// K3's launch rule
inline bool k3_plain(const GemmShape &p)
{
    return p.R == 3 && p.S == 3 && p.stride == 1 && p.pad == 1 && p.perm_n == 0 && !p.stem &&
           p.out_mode == OUT_PLAIN;
}

// a forward-form launch (of `batch` problems in one grid) qualifies for W8: split-operand arithmetic,
// plain output rows, 1x1 / stride 1 gather, K >= 8 slices, at least three rounds of 256 tiles, rows that
// fill their tiles
inline bool w8_ok(const GemmShape &p, const GemmKnobs &k, int batch = 1)
{
    if (!k.w8 || !(k.split_bf16 & 1) || !pw_plain(p)) return false;
    const int64_t tm = cdiv(p.M, kW8BM), tn = cdiv(p.N, kW8BN);
    // (measured, profiles/r06b_w8_shapes.txt: the RoI head's 1x1 layers and their transposed-filter data
    // gradients gain 4 - 7 %; the batch-2 backbone's 270 - 530-tile, 2 - 8-slice launches lose 5 - 20 %)
    return p.N >= kW8BN && p.Kc >= k.w8_min_k && tm * tn * batch >= 768 && (p.M % kW8BM == 0 || p.M >= 16 * kW8BM);
}

// Which instantiation of conv_gemm_kernel a launch runs
enum Variant { INST_GENERAL = 0, INST_PW, INST_K3, INST_WPERM, INST_W8 };
struct GemmInst {
    bool split;      // split-operand arithmetic (SPLIT), else fp32 MFMA
    int variant;     // Variant
    int planes;      // split: bf16 planes per operand (GemmKnobs::split_planes), else 0
};

// the instantiation of a launch on 64 tm x 64 tm tiles
inline GemmInst pick_inst(const GemmShape &p, int tm, const GemmKnobs &k)
{
    if (p.mode == WGRAD) {
        if (tm == 2 && (k.split_bf16 & 1) && p.perm_n == 0) return {true, INST_GENERAL, k.split_planes};
        return {false, p.perm_n > 0 ? INST_WPERM : INST_GENERAL, 0};
    }
    if (p.mode == FWD && (k.split_bf16 & (tm == 2 ? 1 : 2))) {
        if ((k.pw & 1) && pw_plain(p)) return {true, INST_PW, k.split_planes};
        if ((k.pw & 2) && k3_plain(p)) return {true, INST_K3, k.split_planes};
        return {true, INST_GENERAL, k.split_planes};
    }
    return {false, INST_GENERAL, 0};
}

struct GemmLaunch {
    int tile;                  // 64, 128 (square tiles) or 256 (W8: 256x128)
    int m_lo, m_hi;            // GEMM rows [m_lo, m_hi)
    int64_t grid_x;            // tiles, plus the K pieces of the tail tiles
    int grid_y;                // K slabs
    // > 0: the launch writes raw partial sums, one slab of rows [m_lo, m_hi) per grid_y index into the
    // workspace, each split_len K slices (FWD / DGRAD) or pixels (WGRAD) deep
    int split_len;
    // fused tail (GemmParams::tail_*), tail_splits = 0: none.  Workgroups from tail_first on run the
    // tiles of rows [tail_row0, m_hi) as tail_splits K pieces of tail_split_len slices
    int tail_first, tail_row0, tail_splits, tail_split_len;
    GemmInst inst;
};

// A value: what to launch for one problem, in order, then the ordered sum of `sum_splits` slabs of rows
// [sum_row0, M) where sum_splits > 0
struct GemmPlan {
    const char *label;         // the branch taken (tests/gemm_edge_cases.py: FWD_LABELS, WGRAD_LABELS, OTHER_LABELS, WINO_LABELS)
    int n;
    GemmLaunch launch[2];
    int sum_row0, sum_splits;
    int64_t k_extent;          // what the slabs cut: K slices (FWD / DGRAD), pixels (WGRAD)
    int perm_n;                // WGRAD: position-major pixel order (the WPERM kernel), chosen here
};

// ---- split-K for the leftover rows of a small-M forward / dgrad ----------------------------
// 64x64 tiles are all resident at once, so a launch of T tiles costs ceil(T / 256) tile-times
// on the busiest CU (T = 536 -> 3, although the average CU has 2.09).  The rows of the whole
// multiples of 256 tiles run as usual; the leftover rows (< 154 tiles) are cut along K into
// `splits` short workgroups that spread over all CUs, write raw partial sums into slabs, and
// a small kernel sums the slabs in order and applies the epilogue (deterministic).
inline bool can_split_rows(const GemmShape &p)
{
    return p.has_ws && p.mode != WGRAD && p.out_mode == OUT_PLAIN && !p.stem && p.N % 4 == 0 &&
           p.ldc == p.N;
}

// fewer slabs while `splits` slabs of a rows x N output overflow the split-K workspace
inline int64_t fit_ws(int64_t splits, int64_t rows, int N)
{
    while (splits > 1 && rows * N * splits * 4 > kSplitWsBytes) --splits;
    return splits;
}

// K-split count of a split launch over `tiles` tiles of a rows x N output: about target_wgs
// workgroups, at most `cap` slabs, each at least depth_div K slices deep, within the workspace
inline int64_t k_splits(int total_slices, int depth_div, int64_t target_wgs, int64_t tiles, int64_t rows, int N,
                        int64_t cap)
{
    return fit_ws(std::min<int64_t>(std::min<int64_t>(cap, total_slices / depth_div), cdiv(target_wgs, tiles)),
                  rows, N);
}

inline int total_slices(const GemmShape &p) { return p.R * p.S * (int)cdiv(p.Kc, BK); }

// rows [m_lo, m_hi) as whole 64 tm x 64 tm tiles; nothing for an empty range
inline GemmLaunch *add_tiles(GemmPlan &g, const GemmShape &p, int tm, int m_lo, int m_hi, const GemmKnobs &k)
{
    const int64_t blocks = cdiv(m_hi - m_lo, 64 * tm) * cdiv(p.N, 64 * tm);
    if (blocks <= 0) return nullptr;
    GemmLaunch &l = g.launch[g.n++];
    l.tile = 64 * tm;
    l.m_lo = m_lo;
    l.m_hi = m_hi;
    l.grid_x = blocks;
    l.grid_y = 1;
    l.inst = pick_inst(p, tm, k);
    return &l;
}

// rows [rows_lo, p.M) as 64 tm x 64 tm tiles cut along K into `splits` slabs + the ordered slab sum;
// the slab count is re-derived from the slab depth
inline void add_split_rows(GemmPlan &g, const GemmShape &p, int tm, int rows_lo, int splits, const GemmKnobs &k)
{
    GemmLaunch *l = add_tiles(g, p, tm, rows_lo, p.M, k);
    if (!l) return;
    l->split_len = (int)cdiv(total_slices(p), splits);
    l->grid_y = (int)cdiv(total_slices(p), l->split_len);
    g.sum_row0 = rows_lo;
    g.sum_splits = l->grid_y;
}

// Rows [rows_main, m_hi) as the K-split pieces of a fused launch (GemmParams::tail_*) behind its
// first tail_first workgroups, tail_tiles tiles of `splits` pieces each (re-derived from the slab
// depth) + the ordered slab sum.
inline void set_tail(GemmPlan &g, GemmLaunch &l, int rows_main, int64_t tail_first, int64_t tail_tiles,
                     int slices, int64_t splits)
{
    l.tail_split_len = (int)cdiv(slices, splits);
    l.tail_splits = (int)cdiv(slices, l.tail_split_len);
    l.tail_first = (int)tail_first;
    l.tail_row0 = rows_main;
    l.grid_x = l.tail_first + tail_tiles * l.tail_splits;
    g.sum_row0 = rows_main;
    g.sum_splits = l.tail_splits;
}

// Rows [0, rows_main) as whole 64 tm x 64 tm tiles and rows [rows_main, p.M) as K-split pieces of the
// same tile shape in ONE launch, then the ordered slab sum.  Returns false (nothing planned) when the
// problem does not qualify.
inline bool add_fused_tail(GemmPlan &g, const GemmShape &p, int tm, int rows_main, const GemmKnobs &k)
{
    const int BM = 64 * tm;
    if (!k.fused_tail || !can_split_rows(p) || rows_main <= 0 || rows_main % BM != 0 || rows_main >= p.M)
        return false;
    const int64_t ntn = cdiv(p.N, BM);
    const int64_t main_tiles = (rows_main / BM) * ntn;
    const int64_t tail_tiles = cdiv(p.M - rows_main, BM) * ntn;
    const int64_t splits = k_splits(total_slices(p), 4, k.fused_tail, tail_tiles, p.M - rows_main, p.N, 16);
    if (splits < 2) return false;
    set_tail(g, *add_tiles(g, p, tm, 0, p.M, k), rows_main, main_tiles, tail_tiles, total_slices(p), splits);
    return true;
}

// The 64x64-tile remainder of a 128x128-tile launch (rows [rows_lo, M)) runs alone on the GPU
// after the main launch: few workgroups, each walking the whole K.  Cut along K so that about
// two workgroups per CU share the work.  Returns whether it is cut.
inline bool add_remainder(GemmPlan &g, const GemmShape &p, int rows_lo, const GemmKnobs &k)
{
    const int64_t left_tiles = cdiv(p.M - rows_lo, 64) * cdiv(p.N, 64);
    const int64_t splits = k_splits(total_slices(p), 8, 512, left_tiles, p.M - rows_lo, p.N, 16);
    if (!can_split_rows(p) || splits < 2) {
        add_tiles(g, p, 1, rows_lo, p.M, k);
        return false;
    }
    add_split_rows(g, p, 1, rows_lo, (int)splits, k);
    return true;
}

// One W8 launch for the whole problem: whole rounds of 256 tiles (one 512-thread workgroup per CU)
// and, when the last round would be less than ~60 % full, its rows as K-split pieces appended to
// the same grid + the ordered slab sum (the fused-tail scheme of add_fused_tail, with its own
// K partition: the W8 and the 128x128 tail pieces of a problem are not bit-identical).
inline void add_w8(GemmPlan &g, const GemmShape &p, const GemmKnobs &k)
{
    const int64_t tm = cdiv(p.M, kW8BM), tn = cdiv(p.N, kW8BN);
    const int64_t T = tm * tn, full = T / 256, rem = T - full * 256;
    const int slices = (int)cdiv(p.Kc, BK);
    int64_t main_rows_tiles = tm;
    if (rem > 0 && rem < 154 && full >= 1 && k.fused_tail && p.has_ws && p.N % 4 == 0 && p.ldc == p.N)
        main_rows_tiles = (full * 256) / tn;
    const int rows_main = (int)std::min<int64_t>(p.M, main_rows_tiles * kW8BM);
    const int64_t tail_tiles = cdiv(p.M - rows_main, kW8BM) * tn;
    const int64_t splits = rows_main < p.M ? k_splits(slices, 4, 256, tail_tiles, p.M - rows_main, p.N, 16) : 1;
    GemmLaunch &l = g.launch[g.n++];
    l.tile = kW8BM;
    l.m_lo = 0;
    l.m_hi = p.M;
    l.grid_x = T;
    l.grid_y = 1;
    l.inst = {true, INST_W8, k.split_planes};
    if (splits >= 2) set_tail(g, l, rows_main, main_rows_tiles * tn, tail_tiles, slices, splits);
}

// 64x64 tiles; returns the label
inline const char *add_small(GemmPlan &g, const GemmShape &p, const GemmKnobs &k)
{
    const int64_t tm = cdiv(p.M, 64), tn = cdiv(p.N, 64);
    const int64_t T = tm * tn, whole = (T / 256) * 256, rem = T - whole;
    const int slices = total_slices(p);
    // Occupancy-driven split-K: a wave of the 64x64 kernel spends only about a quarter of a K
    // slice issuing MFMAs, so a SIMD needs ~4 co-resident waves to keep its matrix pipe busy.
    // A small-M problem has only T / 256 workgroups per CU; cutting every tile along K into
    // `splits` slabs multiplies the resident waves (each at least 8 slices deep) at the price
    // of the ordered slab sum.
    // Tiny launches that are K-deep (the head's fused cls_loc / score layer: 1024 x 408 x 2048 = 112
    // tiles of 64 slices each on 112 of 256 CUs, 80 us of pure K-loop latency): cut along K so that
    // ~512 workgroups share the walk, ordered slab sum as for the leftover rows.
    if (k.tiny_split && can_split_rows(p) && T <= 128 && slices >= 32) {
        const int64_t splits = k_splits(slices, 8, 512, T, p.M, p.N, 16);
        if (splits >= 2) {
            add_split_rows(g, p, 1, 0, (int)splits, k);
            return "small/tiny_split";
        }
    }
    if (k.small_m_split > 0 && can_split_rows(p) && T < 256ll * k.small_m_split && slices >= 16) {
        const int64_t splits = k_splits(slices, 8, 256ll * k.small_m_split, T, p.M, p.N, 16);
        if (splits >= 2) {
            add_split_rows(g, p, 1, 0, (int)splits, k);
            return "small/m_split";
        }
    }
    const bool can_split = can_split_rows(p) && whole > 0 && whole <= 1024 && rem > 0 &&
                           rem < 154 && slices >= 8;   // beyond 4 tile-times per CU the
                                                       // two extra launches cost more than
                                                       // the imbalance
    const int rows_main = can_split ? (int)std::min<int64_t>(p.M, (whole / tn) * 64) : p.M;
    const int64_t left_tiles = cdiv(p.M - rows_main, 64) * tn;
    int splits = 1;
    // (two or more slabs need left_tiles < 256, so splits x left_tiles < 512 tiles of 16 KB: the
    // workspace clamp of k_splits never applies here)
    if (can_split && rows_main < p.M) splits = (int)k_splits(slices, 4, 256, left_tiles, p.M - rows_main, p.N, 16);
    if (splits < 2) {
        add_tiles(g, p, 1, 0, p.M, k);
        return "small/plain";
    }
    if (add_fused_tail(g, p, 1, rows_main, k)) return "small/fused_tail";
    add_tiles(g, p, 1, 0, rows_main, k);
    add_split_rows(g, p, 1, rows_main, splits, k);
    return "small/main+split_leftover";
}

// FWD / DGRAD launch policy.  With T 128x128 tiles and 512 resident workgroups a launch
// takes ceil(T/512) "rounds"; when the last round would be mostly empty (e.g. T = 536 or
// 1568) the rows of the full rounds run as 128x128 tiles and the leftover rows as a second,
// short launch of 64x64 tiles, instead of one nearly idle round of big tiles.
inline GemmPlan plan_gemm(const GemmShape &p, const GemmKnobs &k)
{
    GemmPlan g = {};
    g.k_extent = total_slices(p);
    const int64_t tm = cdiv(p.M, 128), tn = cdiv(p.N, 128);
    const int64_t T = tm * tn;
    const bool big_ok = p.N > 64 && p.M > 64;
    // Small-M, K-deep problems (the batch-2 backbone's 3x3 layers on res4: M = 8568, N = 256,
    // 72 K slices): 64x64 tiles load twice the operand bytes per MFMA of 128x128 tiles and reach
    // ~100 TFLOP/s whatever their occupancy (profiles/r05f_small_m.txt: K splits of the 64x64 tiles are
    // flat), while the 134 tiles of 128x128 fill half the CUs once.  When a K split puts those tiles
    // into ONE round of the 512 resident workgroups at >= 75 % fill with >= 16 slices each, the
    // 128x128 kernel plus the ordered slab sum is faster in isolation (98 -> 83 us forward, 97 -> 80 us
    // data gradient, profiles/r05d_big_split_k.txt); other counts land in a nearly empty second round
    // and lose.  In the R-50 train step the rule is worth 0.05 - 0.1 ms (12 launches), in the R-101
    // step (46 launches: 23 res4 blocks) 0.39 ms of 32.1 (same-box A/B, profiles/r06e_ab_big_split_k.txt):
    // the default since round 6 ("big_split_k" = 0 restores the 64x64 tiles).
    int64_t ksplits = 1;
    if (k.big_split_k != 0 && big_ok && T < k.big_min_tiles && can_split_rows(p)) {
        if (k.big_split_k > 0) {
            ksplits = k_splits(total_slices(p), 8, k.big_split_k, T, p.M, p.N, 8);
        } else {
            const int64_t fit = kSlotsBig / T;                 // splits that still make one round
            if (fit >= 2 && fit <= 8 && T * fit >= kSlotsBig * 3 / 4 && total_slices(p) / fit >= k.big_split_min_slices)
                ksplits = fit_ws(fit, p.M, p.N);
        }
    }
    if (p.mode == FWD && w8_ok(p, k)) {
        add_w8(g, p, k);
        g.label = "w8";
    } else if (ksplits >= 2) {
        add_split_rows(g, p, 2, 0, (int)ksplits, k);
        g.label = "big/one_round_ksplit";
    } else if (!big_ok || T < k.big_min_tiles) {
        g.label = add_small(g, p, k);
    } else {
        // whole "rounds" of k workgroups per CU (k = 3, 2, 1): pick the round size that leaves
        // the smallest leftover, run the leftover rows as 64x64 tiles
        // resident 128x128 workgroups per CU: 3 single-buffered fp32, 2 otherwise (and split-operand)
        const bool split_fwd = p.mode == FWD && (k.split_bf16 & 1);
        const int64_t max_per_cu = !split_fwd && single_buffered(2, p.mode) ? 3 : 2;
        int64_t main_tiles_m = tm, best_rem = T;
        for (int64_t per_cu = max_per_cu; per_cu >= 1; --per_cu) {
            const int64_t slots = 256 * per_cu, full = T / slots, rem = T - full * slots;
            if (full >= 1 && rem < best_rem) {
                best_rem = rem;
                main_tiles_m = rem > 0 && rem < 154 ? (full * slots) / tn : tm;
            }
        }
        const int rows_main = (int)std::min<int64_t>(p.M, main_tiles_m * 128);
        if (add_fused_tail(g, p, 2, rows_main, k)) {
            g.label = "big/fused_tail";
        } else {
            add_tiles(g, p, 2, 0, rows_main, k);
            if (rows_main >= p.M) g.label = "big/all_rows";
            else g.label = add_remainder(g, p, rows_main, k) ? "big/main+split_remainder" : "big/main+plain_remainder";
        }
    }
    return g;
}

inline int wgrad_splits(int64_t tiles, int64_t pixels, int64_t slots)
{
    // Pick the split count whose tiles*splits workgroups fill whole rounds of `slots`
    // resident workgroups best, each split at least 8 K slices deep, at most ~3 rounds.
    const int64_t maxs = std::min<int64_t>(64, std::max<int64_t>(1, pixels / (8 * BK)));
    int best = 1;
    double best_u = -1.;
    for (int64_t sp = 1; sp <= maxs; ++sp) {
        const int64_t blocks = tiles * sp;
        if (blocks > 3 * slots && sp > 1) break;
        const double u = (double)blocks / (double)(cdiv(blocks, slots) * slots);
        if (u > best_u + 1e-9) { best_u = u; best = (int)sp; }
    }
    return best;
}

// Weight-gradient policy: the tile size, the pixel order and the split over the pixels
inline GemmPlan plan_wgrad(const GemmShape &p0, const GemmKnobs &k)
{
    GemmShape p = p0;
    GemmPlan g = {};
    const int64_t big = cdiv(p.M, 128) * cdiv(p.N, 128);
    // The pixel (K) dimension supplies the parallelism through split-K, so 128x128 tiles are
    // used whenever tiles x achievable splits fills at least half of the resident slots and
    // the problem is at least one tile wide; otherwise 64x64 tiles.
    const int64_t small = cdiv(p.M, 64) * cdiv(p.N, 64);
    const int64_t max_splits = std::min<int64_t>(64, std::max<int64_t>(1, p.pixels / (8 * BK)));
    const bool use_big = p.N > 64 && p.M > 64 && (big * max_splits * 2 >= kSlotsBig || k.big_min_tiles <= 1);
    const int64_t tiles = use_big ? big : small;
    // block-position-major pixel order (WPERM kernel): border taps skip the positions where
    // they fall into the padding; the reduction then runs over whole blocks of BK images
    p.perm_n = 0;
    if (p.C % (use_big ? 128 : 64) == 0 && p.n_img >= BK)
        p.perm_n = choose_perm(k, p.n_img, p.gp, p.gq, p.R, p.S, p.stride, p.pad);
    g.perm_n = p.perm_n;
    g.k_extent = p.perm_n ? cdiv(p.n_img, BK) * BK * p.gp * p.gq : p.pixels;
    // resident 128x128 workgroups: 3 per CU single-buffered, 2 otherwise (and for the split-operand kernel)
    const bool split_kernel = (k.split_bf16 & 1) && p.perm_n == 0;
    const int64_t slots_big = !split_kernel && single_buffered(2, WGRAD) ? 768 : kSlotsBig;
    int splits = wgrad_splits(tiles, p.pixels, use_big ? slots_big : kSlotsSmall);
    if (!p.has_ws) splits = 1;
    GemmLaunch &l = g.launch[g.n++];
    l.tile = use_big ? 128 : 64;
    l.m_lo = 0;
    l.m_hi = p.M;
    l.grid_x = tiles;
    l.split_len = (int)(cdiv(cdiv(g.k_extent, splits), BK) * BK);
    l.grid_y = (int)cdiv(g.k_extent, l.split_len);
    l.inst = pick_inst(p, use_big ? 2 : 1, k);
    g.sum_splits = l.grid_y > 1 ? l.grid_y : 0;
    g.label = !p.has_ws ? "wgrad/no_ws"
              : p.perm_n ? (use_big ? "wgrad/wperm128" : "wgrad/wperm64")
              : use_big  ? (l.grid_y > 1 ? "wgrad128/split+reduce" : "wgrad128/one_slab")
                         : (l.grid_y > 1 ? "wgrad64/split+reduce" : "wgrad64/one_slab");
    return g;
}

// ---- the Winograd route (conv_winograd.h) -----------------------------------------------------------
// A pass runs its 36 per-frequency GEMMs as ONE grid (blockIdx.z = frequency): forward and data gradient
// M[xi] (T x N) = V[xi] (T x Kc) . U[xi]^T (N x Kc) over the T tiles of the maps, the weight gradient
// dU[xi] (K x C) summed over the T tiles.  The policy below is these launches' own; every launch has the
// batch kWinoXi, and the split-operand instantiations always run on three planes (launch_kernel's note in
// conv_gemm.hip).
constexpr int kWinoXi = 36;            // frequencies of F(4x4, 3x3)
constexpr int kWinoMaxSplits = 8;      // weight-gradient slabs the workspace holds (mrcnn_conv3x3_wino_workspace_bytes)

// one per-frequency GEMM as the policy reads it: a pointwise problem with plain output rows
inline GemmShape wino_shape(int mode, int M, int N, int Kc)
{
    GemmShape p = {};
    p.mode = mode;
    p.M = M; p.N = N; p.Kc = Kc;
    p.R = p.S = 1; p.stride = 1; p.pad = 0;
    p.gp = p.gq = p.sh = p.sw = 1;
    p.ldc = N; p.out_mode = OUT_PLAIN;
    return p;
}

inline GemmLaunch *add_wino_launch(GemmPlan &g, const GemmShape &p, int tile, int m_lo, int m_hi, int64_t grid_x,
                                   const GemmKnobs &k)
{
    GemmLaunch &l = g.launch[g.n++];
    l.tile = tile;
    l.m_lo = m_lo;
    l.m_hi = m_hi;
    l.grid_x = grid_x;
    l.grid_y = 1;
    l.inst = tile == kW8BM ? GemmInst{true, INST_W8, 3} : pick_inst(p, tile / 64, k);
    if (l.inst.split) l.inst.planes = 3;
    return &l;
}

// Forward / data gradient: T rows (tiles of the maps), N output channels, Kc input channels.
//   wino/small64         at most 64 rows or 64 columns: 64x64 tiles
//   wino/w8              w8_ok() over the 36 problems: 256x128 tiles on 512 threads
//   wino/main128+tail64  a last 128-row tile that is at most half full, from 256 rows on (the RPN's 546
//                        tiles of a 2 x 51 x 84 map: 4 x 128 + 34): rows [0, T - T % 128) as 128x128 tiles,
//                        the rest as one row of 64x64 tiles that starts at m_lo = T - T % 128
//   wino/big128          128x128 tiles
inline GemmPlan plan_wino_gemm(int64_t T, int N, int Kc, const GemmKnobs &k)
{
    GemmPlan g = {};
    const GemmShape p = wino_shape(FWD, (int)T, N, Kc);
    g.k_extent = total_slices(p);
    const bool big = p.M > 64 && p.N > 64;
    const int rem = p.M % 128;
    if (big && w8_ok(p, k, kWinoXi)) {
        add_wino_launch(g, p, kW8BM, 0, p.M, cdiv(p.M, kW8BM) * cdiv(p.N, kW8BN), k);
        g.label = "wino/w8";
    } else if (big && rem > 0 && rem <= 64 && p.M >= 256) {
        const int full = p.M - rem;
        add_wino_launch(g, p, 128, 0, full, (int64_t)(full / 128) * cdiv(p.N, 128), k);
        add_wino_launch(g, p, 64, full, p.M, cdiv(p.N, 64), k);
        g.label = "wino/main128+tail64";
    } else if (big) {
        add_wino_launch(g, p, 128, 0, p.M, cdiv(p.M, 128) * cdiv(p.N, 128), k);
        g.label = "wino/big128";
    } else {
        add_wino_launch(g, p, 64, 0, p.M, cdiv(p.M, 64) * cdiv(p.N, 64), k);
        g.label = "wino/small64";
    }
    return g;
}

// Weight gradient: K x C outputs per frequency, summed over the T tiles in at most kWinoMaxSplits slabs
// of whole K slices (wgrad_splits() over the 36 x tiles workgroups; the last slab may be short), then the
// ordered slab sum of wino_wgrad_finish_kernel.  128x128 tiles count 768 resident slots whatever the
// arithmetic.
inline GemmPlan plan_wino_wgrad(int64_t T, int K, int C, const GemmKnobs &k)
{
    GemmPlan g = {};
    const GemmShape p = wino_shape(WGRAD, K, C, (int)T);
    g.k_extent = T;
    const bool big = p.M > 64 && p.N > 64;
    const int64_t tiles = big ? cdiv(p.M, 128) * cdiv(p.N, 128) : cdiv(p.M, 64) * cdiv(p.N, 64);
    const int64_t slots = big ? (single_buffered(2, WGRAD) ? 768 : kSlotsBig) : kSlotsSmall;
    const int splits = std::min(kWinoMaxSplits, wgrad_splits(tiles * kWinoXi, T, slots));
    GemmLaunch &l = *add_wino_launch(g, p, big ? 128 : 64, 0, p.M, tiles, k);
    l.split_len = (int)(cdiv(cdiv(T, splits), BK) * BK);
    l.grid_y = (int)cdiv(T, l.split_len);
    g.sum_splits = l.grid_y > 1 ? l.grid_y : 0;
    g.label = big ? (l.grid_y > 1 ? "wino_wgrad128/split+sum" : "wino_wgrad128/one_slab")
                  : (l.grid_y > 1 ? "wino_wgrad64/split+sum" : "wino_wgrad64/one_slab");
    return g;
}

}  // namespace gemm
}  // namespace mrcnn
