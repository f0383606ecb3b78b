"""NumPy statement of the two rules of csrc/soft_nms.hip (test infrastructure, not product code).

Soft-NMS over score-sorted boxes, as the sequential rule of include/mrcnn_hip.h:

    s = prob[:n] (fp32); every row alive
    repeat: i = the alive row with the largest s (ties: the lowest row)
            stop if none alive, or not (s[i] >= min_score), or `limit` picks were made
            emit i; alive[i] = False; for every alive j: s[j] = s[j] * w(iou(box_i, box_j))
    w hard: iou >= Nt ? 0 : 1;  linear: iou >= Nt ? 1 - iou : 1 (fp32);
    w gaussian: iou > 0 ? float32(exp(-(float64(iou) * float64(iou)) / float64(sigma))) : 1

The IoU is oracle.np_ref.non_maximum_suppression's own expression, in float32.  Box voting: each
kept row becomes the mean, weighted by the undecayed scores and summed in float64 in row order, of
the boxes with IoU >= vote_thresh.
"""
import numpy as np

f32 = np.float32
HARD, LINEAR, GAUSSIAN = 0, 1, 2
METHODS = {'hard': HARD, 'linear': LINEAR, 'gaussian': GAUSSIAN}


def iou_one_to_many(b, bbox):
    """np_ref.non_maximum_suppression's IoU of box b (4,) with every row of bbox (n, 4), fp32."""
    b = np.asarray(b, f32)
    bbox = np.asarray(bbox, f32)
    with np.errstate(invalid='ignore', divide='ignore'):
        tl = np.maximum(b[:2], bbox[:, :2])
        br = np.minimum(b[2:], bbox[:, 2:])
        area = np.prod(br - tl, axis=1) * (tl < br).all(axis=1)
        area_b = np.prod(b[2:] - b[:2])
        area_all = np.prod(bbox[:, 2:] - bbox[:, :2], axis=1)
        iou = area / (area_b + area_all - area)
    assert iou.dtype == f32
    return iou


def weights(iou, method, overlap_thresh, sigma):
    method = METHODS.get(method, method)
    one = np.ones_like(iou)
    with np.errstate(invalid='ignore'):
        if method == HARD:
            return np.where(iou >= f32(overlap_thresh), f32(0), one)
        if method == LINEAR:
            return np.where(iou >= f32(overlap_thresh), f32(1) - iou, one)
        assert method == GAUSSIAN
        i64 = iou.astype(np.float64)
        w = np.exp(-(i64 * i64) / np.float64(f32(sigma))).astype(f32)
        return np.where(iou > 0, w, one)


def _rel_gap(a, b):
    """(a - b) / a for a >= b >= 0."""
    a, b = float(a), float(b)
    return (a - b) / a if a > 0 else 0.


def soft_nms(bbox, prob, method, overlap_thresh=0.3, sigma=0.5, min_score=0.001, limit=0,
             with_margin=False, exact_undecayed=False):
    """bbox (n, 4), prob (n,) sorted descending.  Returns keep (rows in emission order, int32) and
    soft_prob (n,) float32: the score of every row when it was emitted, or when the loop ended.
    ``with_margin`` appends the pick margin: the smallest relative gap met between the best and
    the second-best alive score at a pick, and between a score compared with min_score (picked,
    or the one the loop stopped at) and min_score.  ``exact_undecayed`` leaves out of the margin
    every comparison in which no score has been decayed yet (weight 1 is no decay): those scores
    are the inputs' own bits in any implementation, so however close they are, ties included, the
    comparison cannot come out differently; only a decayed score carries a rounding."""
    bbox = np.ascontiguousarray(bbox, f32).reshape(-1, 4)
    s = np.array(prob, f32).reshape(-1)
    n = len(s)
    alive = np.ones(n, bool)
    decays = np.zeros(n, np.int64)                    # per row: weights other than 1 applied so far
    keep = []
    margin = np.inf
    ms = f32(min_score)
    while alive.any() and not (limit and len(keep) >= limit):
        live = np.where(alive)[0]
        i = live[np.argmax(s[live])]                  # first maximum: the lowest row
        if float(ms) > 0 and (decays[i] or not exact_undecayed):
            margin = min(margin, abs(float(s[i]) - float(ms)) / float(ms))
        if not (s[i] >= ms):
            break
        rest = live[live != i]
        if exact_undecayed and not decays[i]:
            rest = rest[decays[rest] > 0]
        if len(rest):
            margin = min(margin, _rel_gap(s[i], s[rest].max()))
        keep.append(i)
        alive[i] = False
        live = np.where(alive)[0]
        if len(live):
            w = weights(iou_one_to_many(bbox[i], bbox[live]), method, overlap_thresh, sigma)
            s[live] = s[live] * w
            decays[live] += w != 1
    keep = np.asarray(keep, np.int32)
    if with_margin:
        return keep, s, margin
    return keep, s


def soft_nms_batched(bbox, prob, counts, method, **kw):
    """bbox (G, n_max, 4), prob (G, n_max), counts (G,): per group (keep, soft_prob[:n])."""
    return [soft_nms(bbox[g, :counts[g]], prob[g, :counts[g]], method, **kw)
            for g in range(len(counts))]


def detectron_soft_nms(bbox, prob, method, overlap_thresh=0.3, sigma=0.5, min_score=0.001):
    """Detectron's cpu_soft_nms loop in its own form (swap the maximum to the front, decay what
    follows, swap rows that fall below min_score to the back and shrink), on this file's IoU and
    weights.  Returns the surviving original rows in order and their scores."""
    boxes = np.array(bbox, f32).reshape(-1, 4)
    s = np.array(prob, f32).reshape(-1)
    idx = np.arange(len(s))
    N = len(s)
    ms = f32(min_score)
    i = 0
    while i < N:
        m = i + int(np.argmax(s[i:N]))
        for a in (boxes, s, idx):
            a[[i, m]] = a[[m, i]]
        pos = i + 1
        while pos < N:
            w = weights(iou_one_to_many(boxes[i], boxes[pos:pos + 1]), method, overlap_thresh,
                        sigma)[0]
            s[pos] = s[pos] * w
            if s[pos] < ms:
                for a in (boxes, s, idx):
                    a[[pos, N - 1]] = a[[N - 1, pos]]
                N -= 1
                pos -= 1
            pos += 1
        i += 1
    return idx[:N].astype(np.int32), s[:N].copy()


def box_vote(bbox, prob, keep, vote_thresh=0.8):
    """bbox (n, 4), prob (n,) undecayed, keep rows -> voted (len(keep), 4) float32."""
    bbox = np.ascontiguousarray(bbox, f32).reshape(-1, 4)
    prob = np.asarray(prob, f32).reshape(-1)
    out = np.empty((len(keep), 4), f32)
    for q, k in enumerate(keep):
        with np.errstate(invalid='ignore'):
            hit = np.where(iou_one_to_many(bbox[k], bbox) >= f32(vote_thresh))[0]
        acc = np.zeros(4, np.float64)
        wsum = np.float64(0)
        for j in hit:                                  # row order: one fixed float64 sum
            w = np.float64(prob[j])
            acc += w * bbox[j].astype(np.float64)
            wsum += w
        out[q] = (acc / wsum).astype(f32) if wsum != 0 else bbox[k]
    return out


def suppress(raw_cls_bbox, raw_prob, n_class, method=None, soft_nms_thresh=0.3, sigma=0.5,
             min_score=0.001, bbox_vote_thresh=None, nms_thresh=0.5, score_thresh=0.05,
             with_picks=False, with_margin=False):
    """oracle.np_infer.suppress with its NMS call replaced: the same per-class `prob > thresh`
    filter and stable descending sort, then Soft-NMS (or hard NMS when ``method`` is None) and
    the vote.  Returns bbox, label, score packed class after class, in emission order
    (``with_picks``: also d, the number of picks made in its class before each row's;
    ``with_margin``: also the smallest pick margin of any class, comparisons between undecayed
    scores left out, last)."""
    from oracle import np_ref
    bbox, label, score, picks, margin = [], [], [], [], np.inf
    for l in range(1, n_class):
        cls_bbox_l = raw_cls_bbox.reshape((-1, n_class, 4))[:, l, :]
        prob_l = raw_prob[:, l]
        sel = prob_l > score_thresh
        cls_bbox_l, prob_l = cls_bbox_l[sel].astype(f32), prob_l[sel].astype(f32)
        order = np_ref.stable_argsort_desc(prob_l)
        cls_bbox_l, prob_l = cls_bbox_l[order], prob_l[order]
        if method is None:
            keep, soft, m = soft_nms(cls_bbox_l, prob_l, HARD, overlap_thresh=nms_thresh,
                                     with_margin=True, exact_undecayed=True)
        else:
            keep, soft, m = soft_nms(cls_bbox_l, prob_l, method, soft_nms_thresh, sigma, min_score,
                                     with_margin=True, exact_undecayed=True)
        margin = min(margin, m)
        boxes = cls_bbox_l[keep] if bbox_vote_thresh is None else box_vote(
            cls_bbox_l, prob_l, keep, bbox_vote_thresh)
        bbox.append(boxes.reshape(-1, 4))
        label.append(np.full((len(keep),), l - 1))
        score.append(soft[keep])
        picks.append(np.arange(len(keep)))
    out = (np.concatenate(bbox, axis=0).astype(f32), np.concatenate(label).astype(np.int32),
           np.concatenate(score).astype(f32))
    if with_picks:
        out = out + (np.concatenate(picks),)
    return out + (margin,) if with_margin else out

