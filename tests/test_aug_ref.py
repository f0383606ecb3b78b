"""NumPy statement of the two test-time augmentation rules of csrc/test_aug.hip
(include/mrcnn_hip.h: mrcnn_decode_cls_boxes_views, mrcnn_mask_aug_combine), in the arithmetic the
header gives: the un-mirror in fp32, the combine in double with one rounding to fp32 at the end."""
import numpy as np

HEURS = ('soft_avg', 'soft_max', 'logit_avg')


def unmirror_boxes(bbox, width):
    """x_min' = W - x_max, x_max' = W - x_min in fp32 on (..., 4) boxes (y_min, x_min, y_max,
    x_max): chainercv's flip_bbox(x_flip=True)."""
    bbox = np.asarray(bbox, np.float32)
    w = np.float32(width)
    out = bbox.copy()
    out[..., 1] = w - bbox[..., 3]
    out[..., 3] = w - bbox[..., 1]
    return out


def union_boxes(per_view, flips, width):
    """The union buffer: the views' decoded (R_v, n_class, 4) boxes one after another, mirrored
    views un-mirrored about ``width``."""
    return np.concatenate([unmirror_boxes(b, width) if f else np.asarray(b, np.float32)
                           for b, f in zip(per_view, flips)], axis=0)


def sigmoid_pair(l):
    """(sigmoid(l), sigmoid(-l)) in double through exp(-|l|)."""
    e = np.exp(-np.abs(l.astype(np.float64)))
    big, small = 1.0 / (1.0 + e), e / (1.0 + e)
    pos = l >= 0
    return np.where(pos, big, small), np.where(pos, small, big)


def mask_aug_combine(maps, flips, heur):
    """maps: V arrays (D, M, M, Kc) float32 NHWC logits; a view with flips[v] is read at column
    M-1-x.  Returns the combined (D, M, M, Kc) float32 logits."""
    assert heur in HEURS and 1 <= len(maps) == len(flips) <= 8
    views = [np.asarray(m, np.float32)[:, :, ::-1] if f else np.asarray(m, np.float32)
             for m, f in zip(maps, flips)]
    n = float(len(views))
    if heur == 'soft_max':
        out = views[0].copy()
        for l in views[1:]:
            out = np.where(l > out, l, out)
        return out
    if heur == 'logit_avg':
        acc = views[0].astype(np.float64)
        for l in views[1:]:
            acc = acc + l.astype(np.float64)
        return (acc / n).astype(np.float32)
    P, Q = sigmoid_pair(views[0])
    for l in views[1:]:
        p, q = sigmoid_pair(l)
        P, Q = P + p, Q + q
    with np.errstate(divide='ignore'):
        return (np.log(P / n) - np.log(Q / n)).astype(np.float32)


def soft_avg_analytic(logits):
    """logit(mean_v sigmoid(l_v)) of a 1-D array of logits by another route: log-sum-exp of the
    log-probabilities, log sigmoid(l) = -logaddexp(0, -l)."""
    l = np.asarray(logits, np.float64)
    log_p, log_q = -np.logaddexp(0.0, -l), -np.logaddexp(0.0, l)
    return np.logaddexp.reduce(log_p) - np.logaddexp.reduce(log_q)
