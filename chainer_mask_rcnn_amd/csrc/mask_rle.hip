// COCO run-length (RLE) codec on packed masks (formats: include/mrcnn_hip.h, "Packed masks" and
// "COCO RLE"):
//   rle_encode — packed masks + extents -> uncompressed counts and compressed strings
//   rle_decode — compressed strings or counts -> packed masks, exact areas, extents
//   mask_unpack — packed masks -> (N, H, W) uint8
// Replaces pycocotools.mask.encode / frPyObjects / decode (maskApi.c rleEncode, rleToString,
// rleFrString, rleDecode) of the reference's _create_ann
// (chainer_mask_rcnn/utils/evaluations/eval_instance_segmentation_coco.py): only the strings
// leave the device.  Integer arithmetic only; every output is a function of the input alone.
#include "common.h"

namespace {

// A run boundary ("change") of mask n is a column-major pixel index p = x * H + y whose bit
// differs from the bit at p - 1 (bit -1 reads 0).  Counts are the differences of 0, the sorted
// changes and H * W.

// Wave-wide integer sum (wave64).
__device__ __forceinline__ int wave_sum(int v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Inclusive prefix sum over the 64 lanes of a wave.
__device__ __forceinline__ int wave_inclusive_scan(int v, int lane)
{
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(v, off, 64);
        if (lane >= off) v += t;
    }
    return v;
}

// Exclusive prefix sum over a 256-thread workgroup; *total gets the sum of all 256 values.
__device__ __forceinline__ int block_exclusive_scan(int v, int *total)
{
    __shared__ int s_wave[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int inc = wave_inclusive_scan(v, lane);
    __syncthreads();                                  // s_wave free from a previous call
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    int before = 0, all = 0;
    for (int i = 0; i < 4; ++i) {
        before += i < wave ? s_wave[i] : 0;
        all += s_wave[i];
    }
    *total = all;
    return before + inc - v;
}

// The extent of mask n clamped to the image: rows [y0, y1), words [w0, w1).
struct Extent { int y0, y1, w0, w1; };

__device__ __forceinline__ Extent clamped_extent(const int32_t *extent, int n, int H, int Wq)
{
    const int32_t *e = extent + 4 * n;
    return {max(e[0], 0), min(e[1], H), max(e[2], 0), min(e[3], Wq)};
}

// One wave walks word column wq of mask n over the extent's rows; lane l owns column
// x = 64 wq + l.  Each step loads the words of up to 64 rows (one per lane) and v_readlane
// broadcasts them row by row.  Returns the lane's number of changes; with out != nullptr the
// lane also stores its changes, ascending, at out[0..).  Rows outside the extent are zero by
// contract.  When the extent spans all rows, pixel (0, x) follows pixel (H-1, x-1) in the
// column-major order: the lane compares its first row with the previous column's last pixel,
// and the change at (x + 1) * H belongs to the lane of column x + 1 unless no lane walks that
// column.  Otherwise the column starts after a zero and its last run ends at x * H + y_hi.
// A change at H * W is the end of the mask, not a change.  Only words of the extent are read.
__device__ __forceinline__ int walk_column(const uint64_t *__restrict__ masks, const Extent &e,
                                           int n, int wq, int H, int W, int Wq, int lane,
                                           int32_t *__restrict__ out)
{
    const int x = (wq << 6) + lane;
    const bool in_w = x < W;
    const uint64_t *col = masks + (int64_t)n * H * Wq + wq;     // word (y, wq) = col[y * Wq]
    const bool full = e.y0 == 0 && e.y1 == H;
    // the lane of column x + 1 records the change at (x + 1) * H
    const bool next_walked = full && x + 1 < W && ((x + 1) >> 6) < e.w1;
    int prev = 0;
    if (full && in_w) {
        if (lane > 0) prev = (int)((col[(int64_t)(H - 1) * Wq] >> (lane - 1)) & 1);
        else if (wq - 1 >= e.w0) prev = (int)(col[(int64_t)(H - 1) * Wq - 1] >> 63);
    }
    const int32_t base = in_w ? x * H : 0;          // x * H < H * W < 2^31
    int k = 0;
    for (int y0 = e.y0; y0 < e.y1; y0 += 64) {
        const int rows = min(64, e.y1 - y0);
        const uint64_t mine = lane < rows ? col[(int64_t)(y0 + lane) * Wq] : 0;
        const int lo = (int)(uint32_t)mine, hi = (int)(uint32_t)(mine >> 32);
        for (int r = 0; r < rows; ++r) {
            const uint64_t word = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(hi, r) << 32)
                                  | (uint32_t)__builtin_amdgcn_readlane(lo, r);
            const int b = in_w ? (int)((word >> lane) & 1) : 0;
            if (b != prev) {
                if (out) out[k] = base + y0 + r;
                ++k;
                prev = b;
            }
        }
    }
    if (prev && !next_walked && (int64_t)base + e.y1 < (int64_t)H * W) {
        if (out) out[k] = base + e.y1;
        ++k;
    }
    return k;
}

// Pass 1: one wave per (mask, word column), four per workgroup: chg[n * Wq + wq] = the number
// of changes in that word column (0 outside the extent).
__global__ void __launch_bounds__(256)
rle_count_kernel(const uint64_t *__restrict__ masks, const int32_t *__restrict__ extent, int N,
                 int H, int W, int Wq, int32_t *__restrict__ chg)
{
    const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (item >= (int64_t)N * Wq) return;
    const int n = (int)(item / Wq), wq = (int)(item - (int64_t)n * Wq);
    const Extent e = clamped_extent(extent, n, H, Wq);
    int k = 0;
    if (e.y0 < e.y1 && wq >= e.w0 && wq < e.w1)
        k = wave_sum(walk_column(masks, e, n, wq, H, W, Wq, lane, nullptr));
    if (lane == 0) chg[item] = k;
}

// In-place exclusive scan of a[0..L) by one 256-thread workgroup; a[L] = the total.
__global__ void __launch_bounds__(256) rle_scan_kernel(int32_t *__restrict__ a, int L)
{
    int carry = 0;
    for (int i0 = 0; i0 < L; i0 += 256) {
        const int i = i0 + (int)threadIdx.x;
        const int v = i < L ? a[i] : 0;
        int total;
        const int ex = block_exclusive_scan(v, &total);
        if (i < L) a[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) a[L] = carry;
}

// val_off[n] = first count of mask n (mask n has changes + 1 counts), n = 0..N.
__global__ void rle_value_offsets_kernel(const int32_t *__restrict__ chg_off, int N, int Wq,
                                         int32_t *__restrict__ val_off)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n > N) return;
    val_off[n] = chg_off[(int64_t)n * Wq] + n;
}

// Pass 2: the same walk, storing each lane's changes at the word column's offset plus the lane's
// exclusive prefix.  Changes of mask n occupy pos[chg_off[n Wq] .. chg_off[(n+1) Wq]), in
// column-major order.  A mask whose counts do not fit cap_values stores nothing.
__global__ void __launch_bounds__(256)
rle_positions_kernel(const uint64_t *__restrict__ masks, const int32_t *__restrict__ extent,
                     int N, int H, int W, int Wq, const int32_t *__restrict__ chg_off,
                     const int32_t *__restrict__ val_off, int cap_values, int32_t *__restrict__ pos)
{
    const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (item >= (int64_t)N * Wq) return;
    const int n = (int)(item / Wq), wq = (int)(item - (int64_t)n * Wq);
    if (val_off[n + 1] > cap_values) return;
    const Extent e = clamped_extent(extent, n, H, Wq);
    if (!(e.y0 < e.y1 && wq >= e.w0 && wq < e.w1)) return;
    const int k = walk_column(masks, e, n, wq, H, W, Wq, lane, nullptr);
    const int before = wave_inclusive_scan(k, lane) - k;
    walk_column(masks, e, n, wq, H, W, Wq, lane, pos + chg_off[item] + before);
}

// Characters of one value in rleToString: 5 data bits each, the last one's bit 4 the sign.
__device__ __forceinline__ int rle_nchars(int32_t v)
{
    int c = 0;
    bool more = true;
    while (more) {
        const int d = v & 0x1f;
        v >>= 5;                                      // arithmetic shift: sign-extends
        more = (d & 0x10) ? v != -1 : v != 0;
        ++c;
    }
    return c;
}

// The value stored for count j: counts[j] - counts[j - 2] from the fourth count on.
__device__ __forceinline__ int32_t rle_delta(const int32_t *__restrict__ cnt, int j)
{
    return j > 2 ? cnt[j] - cnt[j - 2] : cnt[j];
}

// One 256-thread workgroup per mask: counts from the changes (0 in front, H * W at the end) and
// the string length of the mask (str_len[n], 0 for a mask that does not fit cap_values).
__global__ void __launch_bounds__(256)
rle_counts_kernel(const int32_t *__restrict__ val_off, const int32_t *__restrict__ pos, int N,
                  int32_t HW, int cap_values, int32_t *__restrict__ counts,
                  int32_t *__restrict__ str_len)
{
    const int n = blockIdx.x;
    const int vb = val_off[n], ve = val_off[n + 1];
    if (ve > cap_values) {
        if (threadIdx.x == 0) str_len[n] = 0;
        return;
    }
    const int nv = ve - vb, nchg = nv - 1;
    const int32_t *P = pos + (vb - n);               // changes of mask n
    int32_t *cnt = counts + vb;
    for (int j = threadIdx.x; j < nv; j += 256)
        cnt[j] = (j < nchg ? P[j] : HW) - (j > 0 ? P[j - 1] : 0);
    __syncthreads();                                  // rle_delta reads counts of other threads
    int len = 0;
    for (int j = threadIdx.x; j < nv; j += 256) len += rle_nchars(rle_delta(cnt, j));
    int total;
    block_exclusive_scan(len, &total);
    if (threadIdx.x == 0) str_len[n] = total;
}

// One 256-thread workgroup per mask: the characters of the mask's string at str_off[n], 256
// values per step, each value's place from a workgroup scan of the character counts.
__global__ void __launch_bounds__(256)
rle_string_kernel(const int32_t *__restrict__ val_off, const int32_t *__restrict__ counts, int N,
                  int cap_values, const int32_t *__restrict__ str_off, int cap_chars,
                  char *__restrict__ chars)
{
    const int n = blockIdx.x;
    const int vb = val_off[n], ve = val_off[n + 1];
    if (ve > cap_values || str_off[n + 1] > cap_chars) return;
    const int nv = ve - vb;
    const int32_t *cnt = counts + vb;
    int at = str_off[n];
    for (int j0 = 0; j0 < nv; j0 += 256) {
        const int j = j0 + (int)threadIdx.x;
        int32_t v = j < nv ? rle_delta(cnt, j) : 0;
        const int len = j < nv ? rle_nchars(v) : 0;
        int total;
        const int off = block_exclusive_scan(len, &total);
        char *o = chars + at + off;
        for (int i = 0; i < len; ++i) {
            int d = v & 0x1f;
            v >>= 5;
            if (i + 1 < len) d |= 0x20;
            o[i] = (char)(d + 48);
        }
        at += total;
    }
}

// Parse (one lane per mask).  STR: chars[off[n] .. off[n+1]) is a compressed string, else
// values[off[n] .. off[n+1]) are counts.  starts[off[n] + i] = the first pixel of run i (a string
// has at least one character per value, so the runs fit the input's own slots); nval[n] = the
// number of runs; status[n] = MRCNN_RLE_* (runs and starts are meaningless unless OK).
template <bool STR>
__global__ void rle_parse_kernel(const uint8_t *__restrict__ chars,
                                 const int32_t *__restrict__ values, const int32_t *__restrict__ off,
                                 int N, int64_t HW, int32_t *__restrict__ starts,
                                 int32_t *__restrict__ nval, int32_t *__restrict__ status)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const int b = off[n], e = off[n + 1];
    int64_t at = 0, c1 = 0, c2 = 0;                  // run start; counts[m - 1], counts[m - 2]
    int m = 0, st = MRCNN_RLE_OK;
    for (int p = b; p < e && st == MRCNN_RLE_OK;) {
        int64_t x = 0;
        if (STR) {
            int k = 0;
            bool more = true;
            while (more) {
                if (p >= e || k == 7) {               // 7 characters hold every 32-bit value
                    st = MRCNN_RLE_UNTERMINATED;
                    break;
                }
                const int c = (int)chars[p] - 48;
                if (c < 0 || c > 63) {
                    st = MRCNN_RLE_BAD_CHAR;
                    break;
                }
                x |= (int64_t)(c & 0x1f) << (5 * k);
                more = (c & 0x20) != 0;
                ++p;
                ++k;
                if (!more && (c & 0x10)) x |= (int64_t)-1 << (5 * k);
            }
            if (st != MRCNN_RLE_OK) break;
            if (m > 2) x += c2;
        } else {
            x = values[p++];
        }
        if (x < 0) {
            st = MRCNN_RLE_NEGATIVE;
            break;
        }
        starts[b + m] = (int32_t)at;
        at += x;
        if (at > HW) {
            st = MRCNN_RLE_BAD_SUM;
            break;
        }
        c2 = c1;
        c1 = x;
        ++m;
    }
    if (st == MRCNN_RLE_OK && at != HW) st = MRCNN_RLE_BAD_SUM;
    nval[n] = m;
    status[n] = st;
}

__global__ void rle_decode_init_kernel(int N, int H, int Wq, int32_t *__restrict__ area,
                                       int32_t *__restrict__ extent)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    area[n] = 0;
    int32_t *e = extent + 4 * n;
    e[0] = H; e[1] = 0; e[2] = Wq; e[3] = 0;
}

// Fill: one wave per (mask, word column), four per workgroup.  Lane l owns column
// x = 64 wq + l: a binary search finds the run holding pixel x * H, then the lane follows the runs
// down the rows; __ballot gives each row's word.  Lane r keeps the word of row y0 + r, so 64 rows
// are stored by one instruction.  Every word is written (zero for a mask whose status is not OK).
// Popcounts and the rows / words holding set bits go to area and extent with integer atomics.
__global__ void __launch_bounds__(256)
rle_fill_kernel(const int32_t *__restrict__ off, const int32_t *__restrict__ starts,
                const int32_t *__restrict__ nval, const int32_t *__restrict__ status, int N,
                int H, int W, int Wq, uint64_t *__restrict__ packed, int32_t *__restrict__ area,
                int32_t *__restrict__ extent)
{
    const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (item >= (int64_t)N * Wq) return;
    const int n = (int)(item / Wq), wq = (int)(item - (int64_t)n * Wq);
    uint64_t *col = packed + (int64_t)n * H * Wq + wq;
    const bool ok = status[n] == MRCNN_RLE_OK && nval[n] > 0;
    const int m = ok ? nval[n] : 0;
    const int32_t *S = starts + off[n];
    const int x = (wq << 6) + lane;
    const bool in_w = ok && x < W;
    const int32_t p0 = in_w ? x * H : 0;
    int i = 0;
    if (in_w) {                                       // largest i with S[i] <= p0 (S[0] = 0)
        int lo = 0, hi = m - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (S[mid] <= p0) lo = mid;
            else hi = mid - 1;
        }
        i = lo;
    }
    int count = 0, ylo = H, yhi = -1;
    for (int y0 = 0; y0 < H; y0 += 64) {
        const int rows = min(64, H - y0);
        uint64_t mine = 0;
        for (int r = 0; r < rows; ++r) {
            bool bit = false;
            if (in_w) {
                const int32_t p = p0 + y0 + r;
                while (i + 1 < m && S[i + 1] <= p) ++i;
                bit = (i & 1) != 0;
            }
            const uint64_t word = __ballot(bit);
            if (lane == r) mine = word;
            if (word) {
                count += __popcll(word);
                ylo = min(ylo, y0 + r);
                yhi = y0 + r;
            }
        }
        if (lane < rows) col[(int64_t)(y0 + lane) * Wq] = mine;
    }
    if (lane == 0 && count) {
        int32_t *e = extent + 4 * n;
        atomicAdd(area + n, count);
        atomicMin(e + 0, ylo);
        atomicMax(e + 1, yhi + 1);
        atomicMin(e + 2, wq);
        atomicMax(e + 3, wq + 1);
    }
}

// One 256-thread workgroup per (mask, row): bytes of the row from its packed words.
__global__ void __launch_bounds__(256)
unpack_kernel(const uint64_t *__restrict__ packed, int H, int W, int Wq, uint8_t *__restrict__ out)
{
    const int64_t row = blockIdx.x;
    const uint64_t *src = packed + row * Wq;
    uint8_t *dst = out + row * W;
    for (int x = threadIdx.x; x < W; x += 256) dst[x] = (uint8_t)((src[x >> 6] >> (x & 63)) & 1);
}

}  // namespace

extern "C" int mrcnn_rle_encode(const uint64_t *packed, const int32_t *extent, int N, int H, int W,
                                int32_t *chg_off, int32_t *val_off, int32_t *pos, int32_t *counts,
                                int cap_values, int32_t *str_off, char *chars, int cap_chars,
                                void *stream)
{
    MRCNN_REQUIRE(N >= 0 && H > 0 && W > 0 && cap_values >= 0 && cap_chars >= 0,
                  "rle_encode: bad shape");
    MRCNN_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), "rle_encode: H*W >= 2^31");
    const int Wq = (W + 63) / 64;
    // every offset (changes, counts, characters: at most 7 per count) stays below 2^31
    MRCNN_REQUIRE((int64_t)N * ((int64_t)H * W + 1) * 7 < ((int64_t)1 << 31),
                  "rle_encode: N*(H*W+1) too large for one call");
    if (N == 0) return 0;
    MRCNN_REQUIRE(packed && extent && chg_off && val_off && str_off, "rle_encode: null pointer");
    MRCNN_REQUIRE((cap_values == 0 || (pos && counts)) && (cap_chars == 0 || chars),
                  "rle_encode: null pointer");
    const int64_t items = (int64_t)N * Wq;
    hipStream_t s = mrcnn::as_stream(stream);
    const unsigned blocks = (unsigned)((items + 3) / 4);
    hipLaunchKernelGGL(rle_count_kernel, dim3(blocks), dim3(256), 0, s, packed, extent, N, H, W,
                       Wq, chg_off);
    hipLaunchKernelGGL(rle_scan_kernel, dim3(1), dim3(256), 0, s, chg_off, (int)items);
    hipLaunchKernelGGL(rle_value_offsets_kernel, dim3((N + 256) / 256), dim3(256), 0, s, chg_off,
                       N, Wq, val_off);
    hipLaunchKernelGGL(rle_positions_kernel, dim3(blocks), dim3(256), 0, s, packed, extent, N, H,
                       W, Wq, chg_off, val_off, cap_values, pos);
    hipLaunchKernelGGL(rle_counts_kernel, dim3(N), dim3(256), 0, s, val_off, pos, N,
                       (int32_t)(H * W), cap_values, counts, str_off);
    hipLaunchKernelGGL(rle_scan_kernel, dim3(1), dim3(256), 0, s, str_off, N);
    hipLaunchKernelGGL(rle_string_kernel, dim3(N), dim3(256), 0, s, val_off, counts, N, cap_values,
                       str_off, cap_chars, chars);
    return mrcnn::check_launch("rle_encode");
}

extern "C" int mrcnn_rle_decode(const uint8_t *chars, const int32_t *values, const int32_t *off,
                                int N, int H, int W, int32_t *starts, int32_t *nval,
                                int32_t *status, uint64_t *packed, int32_t *area, int32_t *extent,
                                void *stream)
{
    MRCNN_REQUIRE(N >= 0 && H > 0 && W > 0, "rle_decode: bad shape");
    MRCNN_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), "rle_decode: H*W >= 2^31");
    if (N == 0) return 0;
    MRCNN_REQUIRE((chars == nullptr) != (values == nullptr),
                  "rle_decode: exactly one of chars and values");
    MRCNN_REQUIRE(off && starts && nval && status && packed && area && extent,
                  "rle_decode: null pointer");
    const int Wq = (W + 63) / 64;
    const int64_t items = (int64_t)N * Wq;
    MRCNN_REQUIRE((items + 3) / 4 < ((int64_t)1 << 31), "rle_decode: grid too large");
    hipStream_t s = mrcnn::as_stream(stream);
    const int64_t HW = (int64_t)H * W;
    if (chars)
        hipLaunchKernelGGL(rle_parse_kernel<true>, dim3((N + 63) / 64), dim3(64), 0, s, chars,
                           values, off, N, HW, starts, nval, status);
    else
        hipLaunchKernelGGL(rle_parse_kernel<false>, dim3((N + 63) / 64), dim3(64), 0, s, chars,
                           values, off, N, HW, starts, nval, status);
    hipLaunchKernelGGL(rle_decode_init_kernel, dim3((N + 255) / 256), dim3(256), 0, s, N, H, Wq,
                       area, extent);
    hipLaunchKernelGGL(rle_fill_kernel, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, s, off,
                       starts, nval, status, N, H, W, Wq, packed, area, extent);
    return mrcnn::check_launch("rle_decode");
}

extern "C" int mrcnn_mask_unpack(const uint64_t *packed, int N, int H, int W, uint8_t *out,
                                 void *stream)
{
    MRCNN_REQUIRE(N >= 0 && H > 0 && W > 0, "mask_unpack: bad shape");
    MRCNN_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), "mask_unpack: H*W >= 2^31");
    if (N == 0) return 0;
    MRCNN_REQUIRE(packed && out, "mask_unpack: null pointer");
    MRCNN_REQUIRE((int64_t)N * H < ((int64_t)1 << 31), "mask_unpack: grid too large");
    hipLaunchKernelGGL(unpack_kernel, dim3((unsigned)(N * H)), dim3(256), 0,
                       mrcnn::as_stream(stream), packed, H, W, (W + 63) / 64, out);
    return mrcnn::check_launch("mask_unpack");
}
