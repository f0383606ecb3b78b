// Instance drawing and the report mosaic (contract: include/mrcnn_hip.h, "Instance drawing and
// the report mosaic"):
//   draw_instances — both passes of draw_instance_bboxes (chainer_mask_rcnn/utils/
//                    visualizations.py) in one launch: the masks' blend and boundaries, then
//                    the outlines and captions, instance after instance
//   tile_images    — fcn.utils.get_tile_image's mosaic with a bilinear resize
// Every output pixel is a function of its own input value, of mask bits and of the per-instance
// records, so one thread owns one pixel and walks the instances in order: no atomics, and the
// result is bitwise deterministic.  Built with -ffp-contract=off: the blend is one fp64
// multiply and one fp64 add, as the host restatement computes it.
#include "bilinear.h"
#include "common.h"

static_assert(sizeof(mrcnn_draw_instance) == 72, "mrcnn_draw_instance layout");
static_assert(sizeof(mrcnn_tile_cell) == 32, "mrcnn_tile_cell layout");

namespace {

constexpr int kTileRows = 4;                 // one wave per image row, one lane per column
constexpr int kThreads = 64 * kTileRows;

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// Does instance d touch the tile [ty0, ty1) x [tx0, tx1) in either pass?
__device__ __forceinline__ bool meets_tile(const mrcnn_draw_instance &d, const int32_t *ext,
                                           bool masks, int H, int W, int r, int ty0, int ty1,
                                           int tx0, int tx1)
{
    if (!d.draw) return false;
    const int y1 = d.box[0], x1 = d.box[1], y2 = d.box[2], x2 = d.box[3];
    if (masks) {
        // crop, clipped to the image and to the extent widened by the 3x3 neighbourhood
        int cy0 = max(max(y1, 0), ty0), cy1 = min(min(y2, H), ty1);
        int cx0 = max(max(x1, 0), tx0), cx1 = min(min(x2, W), tx1);
        if (ext) {
            cy0 = max(cy0, ext[0] - 1);
            cy1 = min(cy1, ext[1] + 1);
            cx0 = max(cx0, ext[2] * 64 - 1);
            cx1 = min(cx1, ext[3] * 64 + 1);
            if (ext[0] >= ext[1] || ext[2] >= ext[3]) cy1 = cy0;   // empty mask
        }
        if (cy0 < cy1 && cx0 < cx1) return true;
    }
    // outline band: the rectangle widened by r on every side
    if (min(y1, y2) - r < ty1 && max(y1, y2) + r >= ty0 && min(x1, x2) - r < tx1 &&
        max(x1, x2) + r >= tx0)
        return true;
    const int *c = d.cap;
    return c[2] > 0 && c[3] > 0 && c[0] < ty1 && c[0] + c[2] > ty0 && c[1] < tx1 &&
           c[1] + c[3] > tx0;
}

// Bit at column col of a row whose words q-1, q, q+1 are wp, wc, wn (x0 = 64 q).
__device__ __forceinline__ int mask_bit(uint64_t wp, uint64_t wc, uint64_t wn, int col, int x0)
{
    const int d = col - x0;
    if (d < 0) return (int)(wp >> 63);
    if (d >= 64) return (int)(wn & 1);
    return (int)((wc >> d) & 1);
}

__device__ __forceinline__ uint8_t blend(uint8_t v, double one_minus_alpha, double t)
{
    return (uint8_t)(int)((double)v * one_minus_alpha + t);
}

__device__ __forceinline__ uint8_t over_white(uint8_t v, int a)
{
    return (uint8_t)((255 * a + (int)v * (255 - a) + 127) / 255);
}

// One workgroup per 64-column x kTileRows tile: column block q is exactly packed word q.  The
// workgroup first lists, in LDS and in instance order, the instances that touch its tile (a
// ballot and a prefix over the waves per 256 instances); each wave then walks that list for
// its row.  Mask words, records and list entries are wave-uniform (scalar loads).
__global__ void __launch_bounds__(kThreads)
draw_instances_kernel(uint8_t *__restrict__ img, int H, int W, int Wq,
                      const uint64_t *__restrict__ packed, const int32_t *__restrict__ extent,
                      int N, const mrcnn_draw_instance *__restrict__ inst,
                      const uint8_t *__restrict__ atlas, int64_t atlas_bytes,
                      double one_minus_alpha, int r)
{
    __shared__ int16_t list[MRCNN_DRAW_MAX_INSTANCES];
    __shared__ int wave_count[kTileRows];
    const int q = blockIdx.x;
    const int tx0 = q * 64, tx1 = min(tx0 + 64, W);
    const int ty0 = blockIdx.y * kTileRows, ty1 = min(ty0 + kTileRows, H);
    const int lane = threadIdx.x & 63;
    const int wave = uniform(threadIdx.x >> 6);
    const bool masks = packed != nullptr;

    int n = 0;
    for (int base = 0; base < N; base += kThreads) {
        const int i = base + threadIdx.x;
        const bool hit = i < N && meets_tile(inst[i], extent ? extent + 4 * i : nullptr, masks,
                                             H, W, r, ty0, ty1, tx0, tx1);
        const uint64_t b = __ballot(hit);
        if (lane == 0) wave_count[wave] = __popcll(b);
        __syncthreads();
        int off = n, total = 0;
        for (int w = 0; w < kTileRows; ++w) {
            off += w < wave ? wave_count[w] : 0;
            total += wave_count[w];
        }
        if (hit) list[off + __popcll(b & ((1ull << lane) - 1ull))] = (int16_t)i;
        __syncthreads();
        n += total;
    }

    const int y = ty0 + wave;
    if (y >= H) return;                      // wave-uniform; no barrier follows
    const int x = tx0 + lane;
    const bool inside = x < W;
    uint8_t *px = img + ((int64_t)y * W + (inside ? x : 0)) * 3;
    uint8_t v0 = 0, v1 = 0, v2 = 0;
    if (inside) { v0 = px[0]; v1 = px[1]; v2 = px[2]; }

    // pass 1: masks
    if (masks) {
        for (int k = 0; k < n; ++k) {
            const int i = uniform(list[k]);
            const mrcnn_draw_instance &d = inst[i];
            const int cy0 = max(d.box[0], 0), cy1 = min(d.box[2], H);
            const int cx0 = max(d.box[1], 0), cx1 = min(d.box[3], W);
            if (y < cy0 || y >= cy1 || cx0 >= cx1) continue;
            const int ya = max(y - 1, cy0), yb = min(y + 1, cy1 - 1);
            const uint64_t *m = packed + (int64_t)i * H * Wq;
            uint64_t w[3][3];
            const int rows[3] = {ya, y, yb};
            uint64_t any_word = 0;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const uint64_t *row = m + (int64_t)rows[j] * Wq;
                w[j][0] = q > 0 ? row[q - 1] : 0;
                w[j][1] = row[q];
                w[j][2] = q + 1 < Wq ? row[q + 1] : 0;
                any_word |= w[j][0] | w[j][1] | w[j][2];
            }
            if (any_word == 0 || !inside || x < cx0 || x >= cx1) continue;
            const int xa = max(x - 1, cx0), xb = min(x + 1, cx1 - 1);
            int any = 0, all = 1;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int a = mask_bit(w[j][0], w[j][1], w[j][2], xa, tx0);
                const int b = mask_bit(w[j][0], w[j][1], w[j][2], x, tx0);
                const int c = mask_bit(w[j][0], w[j][1], w[j][2], xb, tx0);
                any |= a | b | c;
                all &= a & b & c;
            }
            if (mask_bit(w[1][0], w[1][1], w[1][2], x, tx0)) {
                v0 = blend(v0, one_minus_alpha, d.t[0]);
                v1 = blend(v1, one_minus_alpha, d.t[1]);
                v2 = blend(v2, one_minus_alpha, d.t[2]);
            }
            if (any && !all) v0 = v1 = v2 = 200;
        }
    }

    // pass 2: outline, then caption, instance by instance
    for (int k = 0; k < n; ++k) {
        const int i = uniform(list[k]);
        const mrcnn_draw_instance &d = inst[i];
        const int by0 = min(d.box[0], d.box[2]), by1 = max(d.box[0], d.box[2]);
        const int bx0 = min(d.box[1], d.box[3]), bx1 = max(d.box[1], d.box[3]);
        const bool outer = y >= by0 - r && y <= by1 + r && x >= bx0 - r && x <= bx1 + r;
        const bool inner = y > by0 + r && y < by1 - r && x > bx0 + r && x < bx1 - r;
        if (inside && outer && !inner) {
            v0 = (uint8_t)(d.rgb & 255);
            v1 = (uint8_t)((d.rgb >> 8) & 255);
            v2 = (uint8_t)((d.rgb >> 16) & 255);
        }
        const int cy = d.cap[0], cx = d.cap[1], ch = d.cap[2], cw = d.cap[3];
        if (ch > 0 && cw > 0 && y >= cy && y < cy + ch && inside && x >= cx && x < cx + cw) {
            const int64_t o = d.cap_offset + (int64_t)(y - cy) * cw + (x - cx);
            const int a = o >= 0 && o < atlas_bytes ? atlas[o] : 0;
            v0 = over_white(v0, a);
            v1 = over_white(v1, a);
            v2 = over_white(v2, a);
        }
    }
    if (inside) { px[0] = v0; px[1] = v1; px[2] = v2; }
}

struct TileArgs { mrcnn_tile_cell cells[MRCNN_TILE_MAX_CELLS]; };

// One thread per output pixel: its cell, then a half-pixel bilinear sample of that cell's
// image (fp32, horizontal then vertical, truncated), 0 in margins and empty cells.
__global__ void __launch_bounds__(256)
tile_images_kernel(TileArgs args, int n_cells, int cols, int cell_h, int cell_w, int OW,
                   uint8_t *__restrict__ out)
{
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= OW) return;
    const int gy = y / cell_h, gx = x / cell_w;
    const int k = gy * cols + gx;
    uint8_t o[3] = {0, 0, 0};
    if (k < n_cells) {
        const mrcnn_tile_cell &c = args.cells[k];
        const int ly = y - gy * cell_h - c.oy, lx = x - gx * cell_w - c.ox;
        if (ly >= 0 && ly < c.oh && lx >= 0 && lx < c.ow) {
            const mrcnn::Lin sy = mrcnn::lin_coord(ly, (double)c.h / (double)c.oh, c.h);
            const mrcnn::Lin sx = mrcnn::lin_coord(lx, (double)c.w / (double)c.ow, c.w);
            const uint8_t *r0 = c.src + (int64_t)sy.i0 * c.w * 3;
            const uint8_t *r1 = c.src + (int64_t)sy.i1 * c.w * 3;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float top = (float)r0[sx.i0 * 3 + ch] * (1.f - sx.t) +
                                  (float)r0[sx.i1 * 3 + ch] * sx.t;
                const float bot = (float)r1[sx.i0 * 3 + ch] * (1.f - sx.t) +
                                  (float)r1[sx.i1 * 3 + ch] * sx.t;
                o[ch] = (uint8_t)(int)(top * (1.f - sy.t) + bot * sy.t);
            }
        }
    }
    uint8_t *p = out + ((int64_t)y * OW + x) * 3;
    p[0] = o[0];
    p[1] = o[1];
    p[2] = o[2];
}

}  // namespace

extern "C" int mrcnn_draw_instances(uint8_t *img, int H, int W, const uint64_t *packed,
                                    const int32_t *extent, int N,
                                    const mrcnn_draw_instance *inst, const uint8_t *atlas,
                                    int64_t atlas_bytes, double alpha, int thickness, void *stream)
{
    MRCNN_REQUIRE(H > 0 && W > 0 && N >= 0, "draw_instances: bad shape");
    MRCNN_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), "draw_instances: H*W >= 2^31");
    MRCNN_REQUIRE(H <= 65535 * kTileRows, "draw_instances: H > %d", 65535 * kTileRows);
    MRCNN_REQUIRE(N <= MRCNN_DRAW_MAX_INSTANCES, "draw_instances: N > %d instances",
                  MRCNN_DRAW_MAX_INSTANCES);
    MRCNN_REQUIRE(alpha >= 0.0 && alpha <= 1.0, "draw_instances: alpha outside [0, 1]");
    MRCNN_REQUIRE(thickness >= 1 && thickness <= 32767, "draw_instances: thickness outside [1, 32767]");
    MRCNN_REQUIRE(atlas_bytes >= 0, "draw_instances: negative atlas_bytes");
    MRCNN_REQUIRE(img && (N == 0 || inst) && (atlas_bytes == 0 || atlas),
                  "draw_instances: null pointer");
    if (N == 0) return 0;
    const int Wq = (W + 63) / 64;
    hipLaunchKernelGGL(draw_instances_kernel, dim3((unsigned)Wq, (unsigned)((H + kTileRows - 1) / kTileRows)),
                       dim3(kThreads), 0, mrcnn::as_stream(stream), img, H, W, Wq, packed, extent,
                       N, inst, atlas, atlas_bytes, 1.0 - alpha, thickness / 2);
    return mrcnn::check_launch("draw_instances");
}

extern "C" int mrcnn_tile_images(const mrcnn_tile_cell *cells, int n_cells, int rows, int cols,
                                 int cell_h, int cell_w, uint8_t *out, void *stream)
{
    MRCNN_REQUIRE(rows > 0 && cols > 0 && cell_h > 0 && cell_w > 0 && n_cells >= 0,
                  "tile_images: bad shape");
    MRCNN_REQUIRE((int64_t)rows * cols <= MRCNN_TILE_MAX_CELLS && n_cells <= rows * cols,
                  "tile_images: more than rows * cols <= %d cells", MRCNN_TILE_MAX_CELLS);
    const int64_t OH = (int64_t)rows * cell_h, OW = (int64_t)cols * cell_w;
    MRCNN_REQUIRE(OH * OW < ((int64_t)1 << 31), "tile_images: output H*W >= 2^31");
    MRCNN_REQUIRE(OH <= 65535, "tile_images: output H > 65535");
    MRCNN_REQUIRE(out && (n_cells == 0 || cells), "tile_images: null pointer");
    TileArgs args = {};
    for (int k = 0; k < n_cells; ++k) {
        const mrcnn_tile_cell &c = cells[k];
        MRCNN_REQUIRE(c.oh >= 0 && c.ow >= 0 && c.oy >= 0 && c.ox >= 0 && c.oy + c.oh <= cell_h &&
                          c.ox + c.ow <= cell_w,
                      "tile_images: cell %d: scaled image outside its cell", k);
        MRCNN_REQUIRE(c.oh == 0 || c.ow == 0 || (c.src && c.h > 0 && c.w > 0),
                      "tile_images: cell %d: bad source (null pointer or empty)", k);
        MRCNN_REQUIRE((int64_t)c.h * c.w < ((int64_t)1 << 31), "tile_images: cell %d: h*w >= 2^31", k);
        args.cells[k] = c;
    }
    hipLaunchKernelGGL(tile_images_kernel, dim3((unsigned)((OW + 255) / 256), (unsigned)OH),
                       dim3(256), 0, mrcnn::as_stream(stream), args, n_cells, cols, cell_h,
                       cell_w, (int)OW, out);
    return mrcnn::check_launch("tile_images");
}
