"""NumPy reference of the box IoU conventions of detection evaluation and the inputs the
detection tests share: pycocotools' bbIou in float64, chainercv's +1 VOC IoU through
``utils.bbox.bbox_iou``, filled-rectangle rasters of integer-cornered boxes, and the box sets.
Written from the published algorithms; shares no code with utils/evaluations/boxes.py or the
kernels."""
import numpy as np

from chainer_mask_rcnn_amd.utils.bbox import bbox_iou


def bb_iou(dt, gt, crowd=None):
    """maskApi.c bbIou: (D, 4) and (G, 4) float64 (x, y, w, h) -> (D, G) float64, one pair at a
    time in the C code's operation order."""
    dt = np.asarray(dt, np.float64).reshape(-1, 4)
    gt = np.asarray(gt, np.float64).reshape(-1, 4)
    crowd = np.zeros(len(gt), bool) if crowd is None else np.asarray(crowd).astype(bool)
    out = np.zeros((len(dt), len(gt)), np.float64)
    for d in range(len(dt)):
        dx, dy, dw, dh = dt[d]
        da = dw * dh
        for g in range(len(gt)):
            gx, gy, gw, gh = gt[g]
            ga = gw * gh
            w = np.minimum(dx + dw, gx + gw) - np.maximum(dx, gx)
            if w <= 0:
                continue
            h = np.minimum(dy + dh, gy + gh) - np.maximum(dy, gy)
            if h <= 0:
                continue
            i = w * h
            u = da if crowd[g] else da + ga - i
            with np.errstate(divide='ignore', invalid='ignore'):
                out[d, g] = i / u
    return out


PLUS_ONE = np.array([0, 0, 1, 1], np.float32)


def voc_iou(a, b):
    """chainercv eval_detection_voc's IoU: ``bbox[:, 2:] += 1`` on both sets, then bbox_iou;
    (y1, x1, y2, x2) float32 -> (P, G) float32."""
    a = np.asarray(a, np.float32).reshape(-1, 4)
    b = np.asarray(b, np.float32).reshape(-1, 4)
    with np.errstate(divide='ignore', invalid='ignore'):
        return bbox_iou(a + PLUS_ONE, b + PLUS_ONE)


def xywh64(bbox):
    """(y1, x1, y2, x2) float32 -> float64 (x, y, w, h), the subtraction in float64."""
    b = np.asarray(bbox, np.float32).reshape(-1, 4).astype(np.float64)
    return np.stack([b[:, 1], b[:, 0], b[:, 3] - b[:, 1], b[:, 2] - b[:, 0]], axis=1)


def rasters(bbox, H, W, inclusive=False):
    """(N, H, W) bool filled rectangles of integer-cornered (y1, x1, y2, x2) boxes:
    ``[y1:y2, x1:x2]``, or ``[y1:y2+1, x1:x2+1]`` with ``inclusive`` (the VOC +1 convention)."""
    bbox = np.asarray(bbox).reshape(-1, 4)
    out = np.zeros((len(bbox), H, W), bool)
    e = 1 if inclusive else 0
    for n, (y1, x1, y2, x2) in enumerate(bbox.astype(np.int64)):
        assert 0 <= y1 and 0 <= x1 and y2 + e <= H and x2 + e <= W
        out[n, y1:y2 + e, x1:x2 + e] = True
    return out


def counts(pred_masks, gt_masks):
    """(inter, pred_area, gt_area) int64 per image from full boolean masks."""
    out = []
    for pm, gm in zip(pred_masks, gt_masks):
        hw = int(np.prod(pm.shape[1:]))
        pm = pm.reshape(len(pm), hw).astype(np.int64)
        gm = gm.reshape(len(gm), hw).astype(np.int64)
        out.append((pm @ gm.T, pm.sum(1), gm.sum(1)))
    return out


def integer_boxes(rng, n, H, W, min_side=0):
    """n integer-cornered float32 (y1, x1, y2, x2) boxes inside an (H, W) image, y2 >= y1 + min_side
    and x2 >= x1 + min_side (so zero-width boxes occur with min_side 0), the inclusive raster
    still inside the image."""
    y1 = rng.randint(0, H - 1 - min_side, n)
    x1 = rng.randint(0, W - 1 - min_side, n)
    y2 = np.array([rng.randint(a + min_side, H) for a in y1], np.int64).reshape(n)
    x2 = np.array([rng.randint(a + min_side, W) for a in x1], np.int64).reshape(n)
    return np.stack([y1, x1, y2, x2], 1).astype(np.float32).reshape(n, 4)


def integer_dataset(seed, n_img=36, H=40, W=40, n_class=4):
    """A few dozen images of integer-cornered detections and ground truth with labels, scores,
    crowd flags and annotation areas; about half the detections are jittered copies of a ground
    truth so that matches at every threshold occur.  Some images have no detections or no
    ground truth."""
    rng = np.random.RandomState(seed)
    data = dict(H=H, W=W, pred_bboxes=[], pred_labels=[], pred_scores=[], gt_bboxes=[],
                gt_labels=[], gt_crowdeds=[], gt_areas=[], gt_difficults=[])
    for i in range(n_img):
        G = 0 if i % 11 == 5 else rng.randint(1, 7)
        P = 0 if i % 13 == 7 else rng.randint(1, 12)
        gt = integer_boxes(rng, G, H - 1, W - 1, min_side=1)
        gl = rng.randint(0, n_class, G).astype(np.int32)
        pred = integer_boxes(rng, P, H - 1, W - 1)
        pl = rng.randint(0, n_class, P).astype(np.int32)
        for p in range(P):
            if G and rng.uniform() < 0.6:
                g = rng.randint(G)
                jit = rng.randint(-3, 4, 4)
                b = gt[g] + jit
                b[:2] = np.clip(b[:2], 0, [H - 2, W - 2])
                b[2:] = np.clip(b[2:], b[:2], [H - 2, W - 2])
                pred[p] = b
                pl[p] = gl[g]
        data['pred_bboxes'].append(pred.astype(np.float32))
        data['pred_labels'].append(pl)
        data['pred_scores'].append(rng.uniform(0.05, 1, P).astype(np.float32))
        data['gt_bboxes'].append(gt)
        data['gt_labels'].append(gl)
        data['gt_crowdeds'].append((rng.uniform(size=G) < 0.25).astype(np.int32))
        data['gt_difficults'].append(rng.uniform(size=G) < 0.2)
        # annotation areas that differ from the rectangles': some push a box out of its range
        data['gt_areas'].append((rng.uniform(0.5, 40., G)
                                 * (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])).astype(np.float32))
    return data


def ragged_kernel_batch(seed=0):
    """The kernel test's batch: per image (P, G) = (0, 3), (5, 0), (1, 1), (100, 7), (65, 64).
    (y1, x1, y2, x2) float32 boxes with y2 >= y1 and x2 >= x1: fractional corners, identical
    pairs, pairs sharing only an edge, nested pairs and zero-width boxes, and crowd flags on some
    columns.  Returns (boxes_a, boxes_b, crowd_b) per-image lists."""
    rng = np.random.RandomState(seed)
    shapes = [(0, 3), (5, 0), (1, 1), (100, 7), (65, 64)]

    def boxes(n):
        y1 = rng.uniform(0, 200, n)
        x1 = rng.uniform(0, 300, n)
        b = np.stack([y1, x1, y1 + rng.uniform(0, 120, n), x1 + rng.uniform(0, 150, n)], 1)
        whole = rng.uniform(size=n) < 0.3              # integer corners among fractional ones
        b[whole] = np.round(b[whole])
        return b.astype(np.float32).reshape(n, 4)

    A, Bs, C = [], [], []
    for P, G in shapes:
        a, b = boxes(P), boxes(G)
        if P and G:
            a[0] = b[0]                                # identical pair
        if P >= 8 and G >= 6:
            b[1] = [10, 20, 50, 60]
            a[1] = [10, 60, 50, 90]                    # shares only the edge x = 60 with b[1]
            a[2] = [50, 20, 70, 60]                    # shares only the edge y = 50 with b[1]
            a[3] = [20, 30, 40.5, 50.25]               # nested in b[1]
            b[2] = [5, 10, 80, 120]                    # b[1] (and a[3]) nested in b[2]
            a[4] = [12, 40, 45, 40]                    # zero width, inside b[1]
            b[3] = [30.5, 70, 30.5, 95]                # zero height
            a[5] = b[3]                                # identical zero-area pair
            a[6] = [0, 0, 0, 0]
            b[4] = [0, 0, 0, 0]                        # identical points at the origin
            a[7] = [10.25, 20.5, 50.75, 60.125]        # fractional, almost b[1]
        A.append(a)
        Bs.append(b)
        C.append((rng.uniform(size=G) < 0.3).astype(np.uint8))
    C[3] = np.array([0, 0, 0, 0, 0, 1, 1], np.uint8)   # the built pairs above stay regular
    assert [(len(a), len(b)) for a, b in zip(A, Bs)] == shapes
    assert C[4].any() and not C[4].all()
    return A, Bs, C
