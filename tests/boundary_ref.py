"""NumPy statement of Boundary IoU / Boundary AP (Cheng et al., CVPR 2021) as the
boundary-iou-api computes it, on plain full-image masks, written from the rule and sharing no code
with chainer_mask_rcnn_amd:

* d = max(int(round(ratio * sqrt(H^2 + W^2))), 1);
* E(y, x) = 1 iff every pixel within Chebyshev distance d lies inside the image and is foreground
  (cv2's 3x3 erosion iterated d times on the mask padded by a ring of zeros), as a summed-area test;
* B = M & ~E; boundary IoU = |B_a & B_b| / |B_a | B_b|, 0 where the intersection is 0;
* Boundary AP: the unchanged COCO / VOC evaluation of tests/instseg_eval_ref.py on
  min(mask IoU, boundary IoU), the crowd rule applied to each table before the min.

Also the generator of the crafted evaluation set of the boundary tests.
"""
import contextlib
import math

import numpy as np

import instseg_eval_ref as R


def dilation(H, W, ratio=0.02):
    return max(int(round(ratio * math.sqrt(H ** 2 + W ** 2))), 1)


def erode(m, d):
    """E of one (H, W) mask: the (2d+1)^2 window sums of the mask zero-padded by d equal (2d+1)^2."""
    m = np.asarray(m) != 0
    H, W = m.shape
    k = 2 * d + 1
    p = np.zeros((H + k, W + k), np.int64)
    p[d + 1:d + 1 + H, d + 1:d + 1 + W] = m
    S = p.cumsum(0).cumsum(1)
    return (S[k:, k:] - S[:-k, k:] - S[k:, :-k] + S[:-k, :-k]) == k * k


def erode_by_shifts(m, d):
    """The same E as the AND of the (2d+1)^2 shifted copies of the zero-padded mask."""
    m = np.asarray(m) != 0
    H, W = m.shape
    p = np.zeros((H + 2 * d, W + 2 * d), bool)
    p[d:d + H, d:d + W] = m
    out = np.ones((H, W), bool)
    for dy in range(2 * d + 1):
        for dx in range(2 * d + 1):
            out &= p[dy:dy + H, dx:dx + W]
    return out


def boundary(m, d):
    m = np.asarray(m) != 0
    return m & ~erode(m, d)


def boundaries(masks, d):
    masks = np.asarray(masks)
    if len(masks) == 0:
        return np.zeros(masks.shape, bool)
    return np.stack([boundary(m, d) for m in masks])


def _counts(a, b):
    hw = int(np.prod(a.shape[1:]))
    a = a.reshape(len(a), hw).astype(np.int64)
    b = b.reshape(len(b), hw).astype(np.int64)
    return a @ b.T, a.sum(1), b.sum(1)


def boundary_counts(mask_a, mask_b, d=None, ratio=0.02):
    """(inter (P,G), area_a (P,), area_b (G,)) int64 of the two sets' boundaries."""
    mask_a, mask_b = np.asarray(mask_a), np.asarray(mask_b)
    if d is None:
        d = dilation(mask_a.shape[1], mask_a.shape[2], ratio)
    return _counts(boundaries(mask_a, d), boundaries(mask_b, d))


def iou_of_counts(inter, area_a, area_b):
    union = area_a[:, None] + area_b[None, :] - inter
    iou = np.zeros(inter.shape, np.float64)
    nz = union != 0
    iou[nz] = inter[nz] / union[nz]
    return iou


def boundary_iou(mask_a, mask_b, d=None, ratio=0.02):
    return iou_of_counts(*boundary_counts(mask_a, mask_b, d, ratio))


def min_iou(mask_a, mask_b, ratio=0.02):
    """VOC table: min(mask IoU, boundary IoU), float64 (P, G)."""
    mask_a, mask_b = np.asarray(mask_a) != 0, np.asarray(mask_b) != 0
    return np.minimum(iou_of_counts(*_counts(mask_a, mask_b)), boundary_iou(mask_a, mask_b, None, ratio))


@contextlib.contextmanager
def _boundary_tables(ratio):
    """instseg_eval_ref with its two IoU functions replaced by the min tables; the matching and
    accumulation code of that module runs unchanged."""
    seg_iou, mask_iou = R._seg_iou, R.mask_iou

    def seg_min(dts, gts):
        out = seg_iou(dts, gts)
        if len(dts) == 0 or len(gts) == 0:
            return out
        H, W = dts[0]['m'].shape
        d = dilation(H, W, ratio)
        bd = [dict(x, m=boundary(x['m'], d)) for x in dts]
        bg = [dict(x, m=boundary(x['m'], d)) for x in gts]
        return np.minimum(out, seg_iou(bd, bg))

    def mask_min(a, b):
        if len(a) == 0 or len(b) == 0:
            return mask_iou(a, b)
        return min_iou(a, b, ratio)

    R._seg_iou, R.mask_iou = seg_min, mask_min
    try:
        yield
    finally:
        R._seg_iou, R.mask_iou = seg_iou, mask_iou


def coco_eval(pred_masks, pred_labels, pred_scores, gt_masks, gt_labels, gt_crowdeds=None,
              gt_areas=None, ratio=0.02):
    """(precision, recall, cat_ids) of Boundary AP; areas stay the masks'."""
    with _boundary_tables(ratio):
        return R.coco_eval(pred_masks, pred_labels, pred_scores, gt_masks, gt_labels, gt_crowdeds,
                           gt_areas)


def voc_prec_rec(pred_masks, pred_labels, pred_scores, gt_masks, gt_labels, gt_difficults=None,
                 iou_thresh=0.5, ratio=0.02):
    with _boundary_tables(ratio):
        return R.voc_prec_rec(pred_masks, pred_labels, pred_scores, gt_masks, gt_labels,
                              gt_difficults, iou_thresh)


def all_counts(pred_masks, gt_masks, ratio=0.02):
    """Per image: (mask counts, boundary counts), for the host matching code."""
    masks = R.coco_counts(pred_masks, gt_masks)
    bounds = [boundary_counts(pm, gm, None, ratio) if len(pm) and len(gm) else
              _counts(boundaries(pm, dilation(*pm.shape[1:], ratio)),
                      boundaries(gm, dilation(*gm.shape[1:], ratio)))
              for pm, gm in zip(pred_masks, gt_masks)]
    return masks, bounds


# ---------------------------------------------------------------- the kernel's test masks
KERNEL_CASES = [(1, 1, 1), (5, 64, 1), (7, 63, 2), (9, 65, 3), (40, 129, 5), (70, 130, 31),
                (70, 200, 63), (70, 200, 64), (70, 200, 65), (66, 130, 70), (3, 200, 100),
                (130, 70, 29)]
N_KERNEL_MASKS = 37


def blob(rng, H, W):
    """A random union of a few rectangles and discs, with a little salt and pepper."""
    m = np.zeros((H, W), bool)
    yy, xx = np.mgrid[:H, :W]
    for _ in range(rng.randint(1, 4)):
        cy, cx, r = rng.randint(0, H), rng.randint(0, W), rng.randint(1, max(H, W) // 2 + 2)
        if rng.randint(2):
            m |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        else:
            m |= (abs(yy - cy) <= r) & (abs(xx - cx) <= 2 * r)
    m ^= rng.uniform(size=(H, W)) < 0.01
    return m


def _bar(H, W, axis, start, width):
    m = np.zeros((H, W), bool)
    if axis == 0:
        m[max(start, 0):max(start + width, 0), :] = True
    else:
        m[:, max(start, 0):max(start + width, 0)] = True
    return m


def kernel_masks(H, W, d):
    """The N_KERNEL_MASKS masks of one kernel case: all ones, all zeros, one pixel, a one-pixel
    hole, a checkerboard, bars of width d, 2d, 2d+1, 2d+2 mid-image and on the four borders, blobs
    straddling the word boundaries at x = 63/64 and 127/128, random blobs."""
    rng = np.random.RandomState(H * 100003 + W * 101 + d)
    out = [np.ones((H, W), bool), np.zeros((H, W), bool)]
    single = np.zeros((H, W), bool)
    single[H // 2, W // 2] = True
    hole = np.ones((H, W), bool)
    hole[H // 2, W // 2] = False
    yy, xx = np.mgrid[:H, :W]
    out += [single, hole, (yy + xx) % 2 == 0]
    for width in (d, 2 * d, 2 * d + 1, 2 * d + 2):          # bars mid-image, both directions
        out.append(_bar(H, W, 0, max((H - width) // 2, 0), width))
        out.append(_bar(H, W, 1, max((W - width) // 2, 0), width))
    out += [_bar(H, W, 0, 0, 2 * d + 2), _bar(H, W, 0, H - 2 * d - 2, 2 * d + 2),   # on the borders
            _bar(H, W, 1, 0, 2 * d + 2), _bar(H, W, 1, W - 2 * d - 2, 2 * d + 2)]
    for x in (63, 127):                                      # blobs straddling a word boundary
        m = np.zeros((H, W), bool)
        m[H // 4:H - H // 4 + 1, max(x - d - 3, 0):x + d + 5] = True
        out.append(m)
    while len(out) < N_KERNEL_MASKS:
        out.append(blob(rng, H, W))
    return np.stack(out[:N_KERNEL_MASKS])


def packbits(bits):
    """np.packbits(bits, axis=-1, bitorder='little') over rows zero-padded to whole words."""
    N, H, W = bits.shape
    Wq = (W + 63) // 64
    padded = np.zeros((N, H, Wq * 64), np.uint8)
    padded[:, :, :W] = bits
    return np.packbits(padded, axis=-1, bitorder='little').view('<i8').reshape(N, H, Wq)


# ------------------------------------------------------------------------- the crafted set
SEED = 0            # 0 < boundary map < segm map on the reference: about 0.027 < 0.28 (0..4 all do)
SIZE = (96, 160)    # d = 4
N_CLASS = 3


def _shape(kind, cy, cx, r, H, W):
    yy, xx = np.mgrid[:H, :W]
    if kind == 0:
        return (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    return (abs(yy - cy) <= r) & (abs(xx - cx) <= int(r * 1.3))


def crafted_set(seed=SEED, n_img=6):
    """6 images of 96x160 and 3 classes: 1-4 ground-truth discs / rectangles of radius 6-39 each
    (about 20 % crowds, some cut by the border), 0-2 predictions per ground truth shifted by up to
    +-4 px and resized by up to +-3 px (about 10 % with a wrong label), 0-2 stray false positives.
    Returns a dict of per-image lists: pred_masks (uint8), pred_labels, pred_scores (float32),
    gt_masks (uint8), gt_labels, gt_crowdeds, gt_areas (float32), gt_difficults (bool)."""
    rng = np.random.RandomState(seed)
    H, W = SIZE
    out = dict(pred_masks=[], pred_labels=[], pred_scores=[], gt_masks=[], gt_labels=[],
               gt_crowdeds=[], gt_areas=[], gt_difficults=[])
    for _ in range(n_img):
        gm, gl, gc, pm, pl = [], [], [], [], []
        for _g in range(rng.randint(1, 5)):
            kind, r = rng.randint(0, 2), rng.randint(6, 40)
            cy, cx = rng.randint(0, H), rng.randint(0, W)     # centres anywhere: some are cut
            m = _shape(kind, cy, cx, r, H, W)
            if not m.any():
                continue
            label = rng.randint(0, N_CLASS)
            gm.append(m)
            gl.append(label)
            gc.append(int(rng.uniform() < 0.2))
            for _p in range(rng.randint(0, 3)):
                p = _shape(kind, cy + rng.randint(-4, 5), cx + rng.randint(-4, 5),
                           max(r + rng.randint(-3, 4), 1), H, W)
                if not p.any():
                    continue
                pm.append(p)
                pl.append(label if rng.uniform() >= 0.1 else (label + 1) % N_CLASS)
        for _f in range(rng.randint(0, 3)):
            p = _shape(rng.randint(0, 2), rng.randint(0, H), rng.randint(0, W), rng.randint(6, 40), H, W)
            if p.any():
                pm.append(p)
                pl.append(rng.randint(0, N_CLASS))
        gm = np.array(gm, np.uint8).reshape(-1, H, W)
        pm = np.array(pm, np.uint8).reshape(-1, H, W)
        out['gt_masks'].append(gm)
        out['gt_labels'].append(np.array(gl, np.int32))
        out['gt_crowdeds'].append(np.array(gc, np.int32))
        out['gt_difficults'].append(np.array(gc, bool))
        out['gt_areas'].append(gm.reshape(len(gm), -1).sum(1).astype(np.float32))
        out['pred_masks'].append(pm)
        out['pred_labels'].append(np.array(pl, np.int32))
        out['pred_scores'].append(rng.uniform(0.05, 1., len(pl)).astype(np.float32))
    return out


def coco_maps(data, crowds=True, ratio=0.02):
    """(segm map, boundary map) of the crafted set on the reference alone (IoU .50:.95)."""
    key = 'map/iou=0.50:0.95/area=all/maxDets=100'
    args = (data['pred_masks'], data['pred_labels'], data['pred_scores'], data['gt_masks'],
            data['gt_labels'])
    extra = (data['gt_crowdeds'], data['gt_areas']) if crowds else ()
    p, r, _ = R.coco_eval(*(args + extra))
    segm = R.coco_summary(p, r)[key]
    p, r, _ = coco_eval(*(args + extra), ratio=ratio)
    return segm, R.coco_summary(p, r)[key]
