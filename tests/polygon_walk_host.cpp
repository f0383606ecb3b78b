// Runs the arithmetic of csrc/polygon_walk.h on the host, as csrc/polygon_raster.hip calls it, and
// prints the crossings for tests/test_polygons_cpu.py to compare with the rule
// (tests/polygon_ref.py).  Build with -ffp-contract=off (the rule's doubles are not fused) and the
// address and undefined-behaviour sanitizers.
//
//   polygon_walk_host IN OUT
// IN:  one ring per line: h w k X0 Y0 X1 Y1 ... (k upsampled integer vertices)
// OUT: one line per ring: n x0 y0 x1 y1 ... — its n crossings sorted by (x, y), found per
//      (edge, column) with crossing_at(), the kernel's form.
// The dense walk of every edge with point() and crossing() — maskApi.c's form — must give the same
// crossings; exit status 3 names a ring where it does not.
#include <algorithm>
#include <cstdio>
#include <utility>
#include <vector>

#include "polygon_walk.h"

using Crossings = std::vector<std::pair<int, int>>;

static Crossings by_column(const std::vector<int> &xy, int h, int w)
{
    Crossings out;
    const int k = (int)xy.size() / 2;
    for (int j = 0; j < (k >= 3 ? k : 0); ++j) {
        const int j1 = j + 1 == k ? 0 : j + 1;
        const mrcnn_pw::Edge e = mrcnn_pw::make_edge(xy[2 * j], xy[2 * j + 1], xy[2 * j1], xy[2 * j1 + 1]);
        int y;
        for (int x = 0; x < w; ++x)                    // the kernel tries every column of the image
            if (mrcnn_pw::crossing_at(e, x, h, w, y)) out.emplace_back(x, y);
    }
    std::sort(out.begin(), out.end());
    return out;
}

static Crossings by_walk(const std::vector<int> &xy, int h, int w)
{
    Crossings out;
    const int k = (int)xy.size() / 2;
    for (int j = 0; j < (k >= 3 ? k : 0); ++j) {
        const int j1 = j + 1 == k ? 0 : j + 1;
        const mrcnn_pw::Edge e = mrcnn_pw::make_edge(xy[2 * j], xy[2 * j + 1], xy[2 * j1], xy[2 * j1 + 1]);
        int up, vp;
        mrcnn_pw::point(e, e.flip ? e.n : 0, up, vp);
        for (int d = 1; d <= e.n; ++d) {
            int u, v, x, y;
            mrcnn_pw::point(e, e.flip ? e.n - d : d, u, v);
            if (u != up && mrcnn_pw::crossing(up, vp, u, v, h, w, x, y)) out.emplace_back(x, y);
            up = u;
            vp = v;
        }
    }
    std::sort(out.begin(), out.end());
    return out;
}

int main(int argc, char **argv)
{
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 2;
    }
    std::FILE *in = std::fopen(argv[1], "r"), *out = std::fopen(argv[2], "w");
    if (!in || !out) {
        std::fprintf(stderr, "cannot open %s or %s\n", argv[1], argv[2]);
        return 2;
    }
    int h, w, k, ring = 0, status = 0;
    while (std::fscanf(in, "%d %d %d", &h, &w, &k) == 3) {
        std::vector<int> xy(2 * (size_t)k);
        for (int &c : xy)
            if (std::fscanf(in, "%d", &c) != 1) return 2;
        const Crossings a = by_column(xy, h, w), b = by_walk(xy, h, w);
        if (a != b) {
            std::fprintf(stderr, "ring %d: %zu crossings per column, %zu by the dense walk\n", ring,
                         a.size(), b.size());
            status = 3;
        }
        std::fprintf(out, "%zu", a.size());
        for (const auto &c : a) std::fprintf(out, " %d %d", c.first, c.second);
        std::fprintf(out, "\n");
        ++ring;
    }
    std::fclose(in);
    std::fclose(out);
    return status;
}
