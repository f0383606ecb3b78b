"""Edge inputs of the target-creator kernels (csrc/targets.hip), shared by tests/test_gpu_targets.py
(the kernels) and tests/test_launch_ref_cpu.py (the references of tests/launch_ref.py on NumPy
emulations of right and wrong kernels), and the exact integer count of the hard cases they hold."""
import numpy as np

H, W = 800, 1333
SIDES = (1, 2, 3, 7, 13, 14, 15, 27, 28, 29, 56, 84, 200)


def mask_patterns(G, H=H, W=W):
    """(G, H, W) uint8: 1-px checkerboard, 2 x 3 blocks, 1-px vertical stripes, all ones, in turn;
    the foreground value cycles through 1, 2 and 255 (any non-zero value is foreground)."""
    yy, xx = np.mgrid[0:H, 0:W]
    base = [(yy + xx) % 2, (yy // 2 + xx // 3) % 2, xx % 2, np.ones((H, W), np.int64)]
    m = np.empty((G, H, W), np.uint8)
    for g in range(G):
        m[g] = base[g % 4] * (1, 2, 255)[(g // 4) % 3]
    return m


def crop_boxes(H=H, W=W):
    """(n, 4) float32 RoIs (y0, x0, y1, x1): every (h, w) of SIDES^2 at the top-left corner, at the
    bottom-right corner and at (101, 207); the same boxes with every coordinate moved to x.5; the
    whole image; one empty crop (zero height after rounding)."""
    rows = []
    for h in SIDES:
        for w in SIDES:
            rows += [(0, 0, h, w), (H - h, W - w, H, W), (101, 207, 101 + h, 207 + w)]
    b = np.asarray(rows, np.float32)
    return np.concatenate([b, b + np.float32(0.5),
                           np.asarray([(0, 0, H, W), (10, 10, 10, 30)], np.float32)], 0)


def mask_rows(G, per_crop=4):
    """The crop set against the mask patterns: (sample_roi (n, 4) f32, gt_index (n,) i32).  Row k
    of crop c reads mask (c + k) mod 4 + 4 j, j running over the G / 4 quadruples with c, so that
    every crop meets `per_crop` of the four patterns and gt_index covers all of G."""
    assert G % 4 == 0
    boxes = crop_boxes()
    roi = np.repeat(boxes, per_crop, 0)
    c = np.repeat(np.arange(len(boxes)), per_crop)
    k = np.tile(np.arange(per_crop), len(boxes))
    gt = ((c + k) % 4 + 4 * (c % (G // 4))).astype(np.int32)
    return roi, gt


def round_half_away(x):
    """roundf on non-negative coordinates."""
    return np.floor(np.asarray(x, np.float64) + 0.5)


def halfway_rows(roi):
    """Rows with a coordinate whose fraction is exactly .5 and whose two roundings differ."""
    return (np.round(roi.astype(np.float64)) != round_half_away(roi)).any(1)


def tie_stats(masks, roi, gt_index, M=14):
    """For M = 14 the bilinear weights are multiples of 1 / 28 ((2 d + 1) n - 14 over 28), so
    784 prob is an integer: returns (prob784 (n, M, M) int64, valid (n,) bool) in exact integer
    arithmetic for the correctly rounded (half-to-even) boxes; a tie is prob784 == 392."""
    assert M == 14
    Hh, Ww = masks.shape[1:]
    r = np.round(roi.astype(np.float64)).astype(np.int64)
    y0, y1 = np.clip(r[:, 0], 0, Hh), np.clip(r[:, 2], 0, Hh)
    x0, x1 = np.clip(r[:, 1], 0, Ww), np.clip(r[:, 3], 0, Ww)
    h, w = np.maximum(y1 - y0, 0), np.maximum(x1 - x0, 0)
    valid = (h > 0) & (w > 0)

    def axis(n_in, start, limit):
        n = np.maximum(n_in, 1)[:, None]
        P = (2 * np.arange(M)[None, :] + 1) * n - M             # 28 pos
        i0 = P // (2 * M)
        t = P - 2 * M * i0
        edge = (i0 < 0) | (i0 >= n - 1)
        t = np.where(edge, 0, t)
        i0 = np.clip(i0, 0, n - 1)
        i1 = np.minimum(i0 + 1, n - 1)
        s = start[:, None]
        return np.clip(i0 + s, 0, limit - 1), np.clip(i1 + s, 0, limit - 1), t

    ya, yb, ty = axis(h, y0, Hh)
    xa, xb, tx = axis(w, x0, Ww)
    g = np.asarray(gt_index)[:, None, None]
    f = lambda yy, xx: (masks[g, yy[:, :, None], xx[:, None, :]] != 0).astype(np.int64)
    tx_, ty_ = tx[:, None, :], ty[:, :, None]
    top = f(ya, xa) * (2 * M - tx_) + f(ya, xb) * tx_
    bot = f(yb, xa) * (2 * M - tx_) + f(yb, xb) * tx_
    return top * (2 * M - ty_) + bot * ty_, valid


def iou_boxes(na, g, seed=0, degenerate=False):
    """(a (na, 4), b (g, 4)) float32 in a 800 x 1333 image with, as far as na and g leave room:
    the last row of `a` equal to the last box of `b` (the only IoU 1 of that column), a[0] = b[0]
    and b[1] = b[0] (a tied row: first argmax), a row that overlaps nothing, a row that only
    touches b[0] (tl == br), a zero-area row; with `degenerate` also a zero-area ground-truth box
    (its column is 0 / 0 = NaN against the equal zero-area row, 0 elsewhere)."""
    rng = np.random.RandomState(seed * 1000003 + na * 101 + g)

    def boxes(n, lo, hi):
        y0, x0 = rng.uniform(0, H - lo, n), rng.uniform(0, W - lo, n)
        b = np.stack([y0, x0, np.minimum(y0 + rng.uniform(lo, hi, n), H),
                      np.minimum(x0 + rng.uniform(lo, hi, n), W)], 1)
        return b.astype(np.float32)

    b = boxes(g, 32, 400)
    a = boxes(na, 8, 500)
    if na:                                           # half of the rows near a ground-truth box
        k = rng.randint(0, g, na)
        near = b[k] + rng.uniform(-20, 20, (na, 4)).astype(np.float32)
        near[:, 2:] = np.maximum(near[:, 2:], near[:, :2] + 1)
        a[::2] = near[::2]
    if g >= 3:
        b[1] = b[0]
    if degenerate and g >= 2:
        b[g - 2] = (7, 7, 7, 7)
    special = []
    if g >= 2:
        special.append(b[0])
    special += [np.asarray((5000, 5000, 5010, 5010), np.float32),
                np.asarray((b[0, 2], b[0, 1], b[0, 2] + 10, b[0, 3]), np.float32),
                np.asarray((50, 50, 50, 80), np.float32)]
    if degenerate:
        special.append(np.asarray((7, 7, 7, 7), np.float32))
    if na > len(special):
        step = max((na - 1) // len(special), 1)
        for i, s in enumerate(special):
            a[i * step] = s
    if na:
        a[na - 1] = b[g - 1]
    return a, b
