// Per-point and per-crossing arithmetic of COCO's polygon rule (pycocotools maskApi.c rleFrPoly,
// DESIGN.md section 25), kept free of HIP so that a host program (tests/polygon_walk_host.cpp) can
// run the same functions and compare the crossings with the rule.  Vertices arrive upsampled by
// 5 as integers (|X| < 2^30).  Doubles are used only where maskApi.c uses them and the result
// depends on their rounding: the slope s and the two expressions ys + s*t + .5 / xs + s*t + .5
// (a multiply, an add, an add: compile with -ffp-contract=off).  Everything after them is integer.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MRCNN_PW_HD __host__ __device__ __forceinline__
#else
#define MRCNN_PW_HD inline
#endif

namespace mrcnn_pw {

// One edge after maskApi.c's swap: it walks t = 0 .. n from (xs, ys), n = max(dx, dy); `flip`
// says that the ring meets its points in the order t = n .. 0.
struct Edge {
    int xs, ys, xe, ye, dx, dy, n;
    bool flip, shallow;                   // shallow: dx >= dy, u = t + xs; else v = t + ys
    double s;
};

MRCNN_PW_HD Edge make_edge(int x0, int y0, int x1, int y1)
{
    Edge e;
    e.dx = x1 > x0 ? x1 - x0 : x0 - x1;
    e.dy = y1 > y0 ? y1 - y0 : y0 - y1;
    e.shallow = e.dx >= e.dy;
    e.flip = (e.shallow && x0 > x1) || (!e.shallow && y0 > y1);
    e.xs = e.flip ? x1 : x0;
    e.ys = e.flip ? y1 : y0;
    e.xe = e.flip ? x0 : x1;
    e.ye = e.flip ? y0 : y1;
    e.n = e.shallow ? e.dx : e.dy;
    // a zero-length edge has one point and no slope (0/0 in C; its v is never read)
    e.s = e.n == 0 ? 0. : (e.shallow ? (double)(e.ye - e.ys) / e.dx : (double)(e.xe - e.xs) / e.dy);
    return e;
}

// The point at parameter t, 0 <= t <= n.  The casts truncate towards zero, as C's do.
MRCNN_PW_HD void point(const Edge &e, int t, int &u, int &v)
{
    if (e.shallow) {
        u = t + e.xs;
        v = e.n == 0 ? e.ys : (int)(e.ys + e.s * t + .5);
    } else {
        v = t + e.ys;
        u = (int)(e.xs + e.s * t + .5);
    }
}

// Two consecutive points of the walk, (u_prev, v_prev) then (u, v), u != u_prev: the crossing of
// a pixel-column centre they make, if any.  maskApi.c in doubles:
//   xd = u < u_prev ? u : u - 1;  xd = (xd + .5) / 5 - .5;  kept iff floor(xd) == xd, 0 <= xd <= w-1
//   yd = min(v, v_prev);          yd = (yd + .5) / 5 - .5;  clamped to [0, h];  ceil
// (m + .5) / 5 - .5 is an integer exactly when m = 5 k + 2 (then it is k, exactly, in doubles too;
// the other residues land 0.2 or 0.4 from an integer, far beyond any rounding), so
//   x = (m - 2) / 5 where m = 5 k + 2,   y = clamp(ceil((min v - 2) / 5), 0, h).
MRCNN_PW_HD bool crossing(int u_prev, int v_prev, int u, int v, int h, int w, int &x, int &y)
{
    const int m = u < u_prev ? u : u - 1;
    if (m < 2 || (m - 2) % 5 != 0) return false;
    x = (m - 2) / 5;
    if (x > w - 1) return false;
    const int vm = v < v_prev ? v : v_prev;
    y = vm <= 2 ? 0 : (int)(((int64_t)vm + 2) / 5);   // ceil((vm - 2) / 5) for vm > 2
    if (y > h) y = h;
    return true;
}

// The crossing of column k by this edge: the one pair of consecutive points (t, t + 1) between
// which u passes from <= 5 k + 2 to >= 5 k + 3 (or back), handed to crossing() in the ring's
// walking order.  Shallow edge: u = t + xs, so t = 5 k + 2 - xs.  Steep edge: u is monotone in t
// (a rounded multiply, two rounded adds and a truncation, each monotone), found by bisection.
// An edge crosses a column at most once.
MRCNN_PW_HD bool crossing_at(const Edge &e, int k, int h, int w, int &y)
{
    if (e.n == 0 || k < 0 || k > w - 1) return false;
    const int64_t m = 5 * (int64_t)k + 2;
    int t;
    if (e.shallow) {
        const int64_t tt = m - e.xs;
        if (tt < 0 || tt > (int64_t)e.n - 1) return false;
        t = (int)tt;
    } else {
        int u, v;
        const bool up = e.s > 0;
        // P(t): the walk has passed the centre; false at 0, true at n, else no crossing here
        auto passed = [&](int q) {
            point(e, q, u, v);
            return up ? u > m : u <= m;
        };
        if (e.s == 0 || passed(0) || !passed(e.n)) return false;
        int lo = 0, hi = e.n;
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            if (passed(mid)) hi = mid; else lo = mid;
        }
        t = lo;
    }
    int u0, v0, u1, v1, x;
    point(e, t, u0, v0);
    point(e, t + 1, u1, v1);
    if (u0 == u1) return false;
    const bool hit = e.flip ? crossing(u1, v1, u0, v0, h, w, x, y) : crossing(u0, v0, u1, v1, h, w, x, y);
    return hit && x == k;
}

}  // namespace mrcnn_pw
