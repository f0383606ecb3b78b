"""Host half of the instance-segmentation evaluations: matching and accumulation from
per-image intersection counts.  No masks are touched here — each image is described by

    inter (P, G) intersection pixel counts, pred_area (P,), gt_area (G,) pixel counts

(what ``masks.mask_counts`` / the evaluators' device path return), plus labels, scores and
flags.  The CPU tests feed counts computed with NumPy; everything that decides a number lives
in this file.

The box entry points (``voc_prec_rec_from_ious``, ``coco_evaluate_from_ious``) take per-image
IoU tables instead (boxes.py makes them on the device) and run the same loops.

* VOC: ``voc_prec_rec_from_counts`` restates ``calc_instseg_voc_prec_rec``
  (chainer_mask_rcnn/utils/evaluations/eval_instance_segmentation_voc.py) with its order rules.
* COCO: ``coco_evaluate_from_counts`` restates pycocotools' COCOeval ``evaluate`` /
  ``evaluateImg`` / ``accumulate`` for iouType 'segm' as the reference drives it, and
  ``summarize`` the reference's ``_summarize``.  Not pinned against pycocotools itself (it
  cannot be installed here): DESIGN.md section 9.
"""
from collections import defaultdict

import numpy as np

from .masks import iou_from_counts


# --------------------------------------------------------------------------------------- VOC
def voc_prec_rec_from_counts(counts, pred_labels, pred_scores, gt_labels, gt_difficults=None,
                             iou_thresh=0.5):
    """calc_instseg_voc_prec_rec with the masks replaced by per-image counts
    ``(inter, pred_area, gt_area)``."""
    return _voc_prec_rec(counts, lambda c: iou_from_counts(*c), pred_labels, pred_scores,
                         gt_labels, gt_difficults, iou_thresh)


def voc_prec_rec_from_ious(ious, pred_labels, pred_scores, gt_labels, gt_difficults=None,
                           iou_thresh=0.5):
    """chainercv's calc_detection_voc_prec_rec with the boxes replaced by per-image (P, G) IoU
    tables (``boxes.queue_box_ious(..., 'voc')``: float32, the +1 convention applied).  The
    matching is the one ``voc_prec_rec_from_counts`` runs."""
    return _voc_prec_rec(ious, np.asarray, pred_labels, pred_scores, gt_labels, gt_difficults,
                         iou_thresh)


def voc_prec_rec_from_boundary_counts(counts, boundary_counts, pred_labels, pred_scores,
                                      gt_labels, gt_difficults=None, iou_thresh=0.5):
    """The VOC matching on min(mask IoU, boundary IoU) (Boundary AP): ``counts`` and
    ``boundary_counts`` are the per-image ``(inter, pred_area, gt_area)`` of the masks and of
    their boundaries."""
    counts, boundary_counts = list(counts), list(boundary_counts)
    if len(counts) != len(boundary_counts):
        raise ValueError('Length of input iterables need to be same.')
    tables = [np.minimum(iou_from_counts(*c), iou_from_counts(*b))
              for c, b in zip(counts, boundary_counts)]
    return _voc_prec_rec(tables, np.asarray, pred_labels, pred_scores, gt_labels, gt_difficults,
                         iou_thresh)


def _voc_prec_rec(tables, iou_of, pred_labels, pred_scores, gt_labels, gt_difficults, iou_thresh):
    """The VOC matching and accumulation; ``iou_of(tables[i])`` is image i's (P, G) IoU."""
    counts, pred_labels, pred_scores, gt_labels = (
        list(tables), list(pred_labels), list(pred_scores), list(gt_labels))
    n = len(counts)
    gt_difficults = [None] * n if gt_difficults is None else list(gt_difficults)
    if not (len(pred_labels) == len(pred_scores) == len(gt_labels) == len(gt_difficults) == n):
        raise ValueError('Length of input iterables need to be same.')

    n_pos = defaultdict(int)
    score = defaultdict(list)
    match = defaultdict(list)

    for table, pred_label, pred_score, gt_label, gt_difficult in zip(
            counts, pred_labels, pred_scores, gt_labels, gt_difficults):
        pred_label = np.asarray(pred_label)
        pred_score = np.asarray(pred_score)
        gt_label = np.asarray(gt_label)
        if gt_difficult is None:
            gt_difficult = np.zeros(len(gt_label), dtype=bool)
        gt_difficult = np.asarray(gt_difficult)
        iou_all = iou_of(table)

        for l in np.unique(np.concatenate((pred_label, gt_label)).astype(int)):
            pred_keep_l = pred_label == l
            pred_score_l = pred_score[pred_keep_l]
            # sort by score: NumPy's default (unstable) kind, called as the reference calls it,
            # so that tied scores resolve identically
            order = pred_score_l.argsort()[::-1]
            pred_index_l = np.flatnonzero(pred_keep_l)[order]
            pred_score_l = pred_score_l[order]

            gt_keep_l = gt_label == l
            gt_index_l = np.flatnonzero(gt_keep_l)
            gt_difficult_l = gt_difficult[gt_keep_l]

            n_pos[l] += np.logical_not(gt_difficult_l).sum()
            score[l].extend(pred_score_l)

            if len(pred_index_l) == 0:
                continue
            if len(gt_index_l) == 0:
                match[l].extend((0,) * len(pred_index_l))
                continue

            iou = iou_all[pred_index_l][:, gt_index_l]
            gt_index = iou.argmax(axis=1)
            # -1 if there is no matching ground truth
            gt_index[iou.max(axis=1) < iou_thresh] = -1
            del iou

            selec = np.zeros(len(gt_index_l), dtype=bool)
            for gt_idx in gt_index:
                if gt_idx >= 0:
                    if gt_difficult_l[gt_idx]:
                        match[l].append(-1)
                    else:
                        if not selec[gt_idx]:
                            match[l].append(1)
                        else:
                            match[l].append(0)
                    selec[gt_idx] = True
                else:
                    match[l].append(0)

    n_fg_class = max(n_pos.keys()) + 1
    prec = [None] * n_fg_class
    rec = [None] * n_fg_class

    for l in n_pos.keys():
        score_l = np.array(score[l])
        match_l = np.array(match[l], dtype=np.int8)

        order = score_l.argsort()[::-1]
        match_l = match_l[order]

        tp = np.cumsum(match_l == 1)
        fp = np.cumsum(match_l == 0)

        # an element of fp + tp equal to 0 gives NaN precision
        prec[l] = tp / (fp + tp)
        # n_pos[l] == 0: rec[l] stays None
        if n_pos[l] > 0:
            rec[l] = tp / n_pos[l]

    return prec, rec


def calc_detection_voc_ap(prec, rec, use_07_metric=False):
    """chainercv.evaluations.calc_detection_voc_ap: per-class average precision from the
    precision / recall lists; NaN for a class whose prec or rec is None.
    ``use_07_metric``: the 11-point metric of VOC2007; otherwise the area under the
    monotone (envelope) precision-recall curve."""
    n_fg_class = len(prec)
    ap = np.empty(n_fg_class)
    for l in range(n_fg_class):
        if prec[l] is None or rec[l] is None:
            ap[l] = np.nan
            continue

        if use_07_metric:
            ap[l] = 0
            for t in np.arange(0., 1.1, 0.1):
                if np.sum(rec[l] >= t) == 0:
                    p = 0
                else:
                    p = np.max(np.nan_to_num(prec[l])[rec[l] >= t])
                ap[l] += p / 11
        else:
            # sentinels at both ends, then the precision envelope
            mpre = np.concatenate(([0], np.nan_to_num(prec[l]), [0]))
            mrec = np.concatenate(([0], rec[l], [1]))
            mpre = np.maximum.accumulate(mpre[::-1])[::-1]
            # sum of (delta recall) * precision where the recall changes
            i = np.where(mrec[1:] != mrec[:-1])[0]
            ap[l] = np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])
    return ap


# -------------------------------------------------------------------------------------- COCO
AREA_RANGES = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_RANGE_LABELS = ['all', 'small', 'medium', 'large']


def coco_params():
    """pycocotools.cocoeval.Params(iouType='segm') defaults."""
    return {
        'iouThrs': np.linspace(.5, .95, 10),          # [8] == 0.8999999999999999
        'recThrs': np.linspace(.0, 1.00, 101),
        'maxDets': [1, 10, 100],
        'areaRng': [list(r) for r in AREA_RANGES],
        'areaRngLbl': list(AREA_RANGE_LABELS),
    }


def _coco_ious(inter, dt_area, gt_area_px, gt_crowd):
    """maskUtils.iou(dt, gt, iscrowd): inter / union, union = dt area for a crowd gt; 0 where
    the masks do not intersect (rleIou only computes pairs whose boxes overlap)."""
    inter = np.asarray(inter, np.int64)
    union = np.where(np.asarray(gt_crowd, bool)[None, :], np.asarray(dt_area, np.int64)[:, None],
                     np.asarray(dt_area, np.int64)[:, None] + np.asarray(gt_area_px, np.int64)[None, :]
                     - inter)
    iou = np.zeros(inter.shape, np.float64)
    nz = inter > 0
    iou[nz] = inter[nz] / union[nz]
    return iou


def _evaluate_img(ious, dt_scores, dt_area, gt_crowd, gt_area, a_rng, max_det, iou_thrs):
    """COCOeval.evaluateImg for one (image, category, area range).  ``ious`` (D, G) rows are
    the detections already sorted by score (mergesort) and truncated to maxDets[-1]; columns the
    ground truth in annotation order."""
    G, D_all = len(gt_crowd), len(dt_scores)
    if G == 0 and D_all == 0:
        return None
    gt_ignore = np.array([bool(c) or (a < a_rng[0] or a > a_rng[1])
                          for c, a in zip(gt_crowd, gt_area)], dtype=bool).reshape(-1)
    gtind = np.argsort(gt_ignore.astype(np.int64), kind='mergesort')
    gt_ig = gt_ignore[gtind]
    iscrowd = np.asarray(gt_crowd, bool)[gtind]
    D = min(D_all, max_det)
    ious = ious[:D][:, gtind] if ious.size else ious
    T = len(iou_thrs)
    gtm = np.zeros((T, G), dtype=bool)
    dtm = np.zeros((T, D), dtype=bool)
    dt_ig = np.zeros((T, D), dtype=bool)
    if ious.size:
        for tind, t in enumerate(iou_thrs):
            for dind in range(D):
                iou = min([t, 1 - 1e-10])
                m = -1
                for gind in range(G):
                    # already matched and not a crowd: skip
                    if gtm[tind, gind] and not iscrowd[gind]:
                        continue
                    # matched to a regular gt and reached the ignored ones: stop
                    if m > -1 and not gt_ig[m] and gt_ig[gind]:
                        break
                    if ious[dind, gind] < iou:
                        continue
                    iou = ious[dind, gind]
                    m = gind
                if m == -1:
                    continue
                dt_ig[tind, dind] = gt_ig[m]
                dtm[tind, dind] = True
                gtm[tind, m] = True
    # unmatched detections outside the area range are ignored
    a = np.array([ar < a_rng[0] or ar > a_rng[1] for ar in dt_area[:D]], dtype=bool).reshape(1, D)
    dt_ig = np.logical_or(dt_ig, np.logical_and(~dtm, np.repeat(a, T, 0)))
    return {'dtMatches': dtm, 'dtScores': np.asarray(dt_scores[:D]), 'gtIgnore': gt_ig,
            'dtIgnore': dt_ig}


def _count_image(table, n_dt, n_gt):
    """Image record of the count form: ``(ious(d_idx, g_idx, crowd), dt_area, gt_area)``."""
    inter, pred_area, gt_area_px = table
    inter = np.asarray(inter, np.int64).reshape(n_dt, n_gt)
    pred_area = np.asarray(pred_area, np.int64)
    gt_area_px = np.asarray(gt_area_px, np.int64)

    def ious(d_idx, g_idx, gc):
        return _coco_ious(inter[d_idx][:, g_idx], pred_area[d_idx], gt_area_px[g_idx], gc[g_idx])
    return ious, pred_area, gt_area_px


def _iou_image(table, n_dt, n_gt):
    """Image record of the IoU form: the table already holds bbIou with the crowd rule."""
    iou, dt_area, gt_area = table
    iou = np.asarray(iou, np.float64).reshape(n_dt, n_gt)

    def ious(d_idx, g_idx, gc):
        return iou[d_idx][:, g_idx]
    return ious, np.asarray(dt_area, np.float64).ravel(), np.asarray(gt_area, np.float64).ravel()


def _boundary_image(table, n_dt, n_gt):
    """Image record of the boundary form: ``table`` = (mask counts, boundary counts); the lookup
    is min(mask IoU, boundary IoU), the crowd rule applied to each before the min; the areas are
    the masks'."""
    mask_ious, pred_area, gt_area_px = _count_image(table[0], n_dt, n_gt)
    boundary_ious, _, _ = _count_image(table[1], n_dt, n_gt)

    def ious(d_idx, g_idx, gc):
        return np.minimum(mask_ious(d_idx, g_idx, gc), boundary_ious(d_idx, g_idx, gc))
    return ious, pred_area, gt_area_px


def coco_evaluate_from_boundary_counts(counts, boundary_counts, pred_labels, pred_scores,
                                       gt_labels, gt_crowdeds=None, gt_areas=None):
    """COCOeval(gt, dt, 'boundary').evaluate() + accumulate() of the boundary-iou-api: the
    loops of ``coco_evaluate_from_counts`` on min(mask IoU, boundary IoU).  ``boundary_counts``
    are the per-image ``(inter, pred_area, gt_area_px)`` of the masks' boundaries; area ranges
    use the masks' areas, as for 'segm'."""
    counts, boundary_counts = list(counts), list(boundary_counts)
    if len(counts) != len(boundary_counts):
        raise ValueError('Length of input iterables need to be same.')
    return _coco_evaluate(list(zip(counts, boundary_counts)), _boundary_image, pred_labels,
                          pred_scores, gt_labels, gt_crowdeds, gt_areas)


def coco_evaluate_from_counts(counts, pred_labels, pred_scores, gt_labels, gt_crowdeds=None,
                              gt_areas=None):
    """COCOeval(gt, dt, 'segm').evaluate() + accumulate() as eval_instseg_coco sets them up,
    from per-image counts ``(inter, pred_area, gt_area_px)``.

    Returns the ``coco_eval`` dict: ``precision`` (T,R,K,A,M), ``recall`` (T,K,A,M) with -1
    where undefined, and ``params`` (iouThrs, recThrs, maxDets, areaRng, areaRngLbl, catIds,
    imgIds).  ``gt_areas`` (if given) decides the gt area range, as the annotation's 'area';
    otherwise the pixel count does.  A detection's area is its pixel count."""
    return _coco_evaluate(counts, _count_image, pred_labels, pred_scores, gt_labels, gt_crowdeds,
                          gt_areas)


def coco_evaluate_from_ious(tables, pred_labels, pred_scores, gt_labels, gt_crowdeds=None,
                            gt_areas=None):
    """COCOeval(gt, dt, 'bbox').evaluate() + accumulate() from per-image
    ``(iou (P,G), dt_area (P,), gt_box_area (G,))``: the float64 bbIou tables with the crowd rule
    applied (``boxes.queue_box_ious(..., 'coco', crowd_b)``) and the boxes' ``w*h``.  A
    detection's area is its box's ``w*h`` (what ``loadRes`` sets for bbox results); a ground
    truth's is ``gt_areas`` if given, else its box's.  Same loops and return value as
    ``coco_evaluate_from_counts``."""
    return _coco_evaluate(tables, _iou_image, pred_labels, pred_scores, gt_labels, gt_crowdeds,
                          gt_areas)


def _coco_evaluate(tables, image_of, pred_labels, pred_scores, gt_labels, gt_crowdeds, gt_areas):
    """COCOeval's evaluate() + accumulate(); ``image_of(tables[i], P, G)`` gives image i's IoU
    lookup, detection areas and default ground-truth areas."""
    counts, pred_labels, pred_scores, gt_labels = (
        list(tables), list(pred_labels), list(pred_scores), list(gt_labels))
    n_img = len(counts)
    gt_crowdeds = [None] * n_img if gt_crowdeds is None else list(gt_crowdeds)
    gt_areas = [None] * n_img if gt_areas is None else list(gt_areas)
    if not (len(pred_labels) == len(pred_scores) == len(gt_labels) == len(gt_crowdeds)
            == len(gt_areas) == n_img):
        raise ValueError('Length of input iterables need to be same.')
    p = coco_params()
    cat_ids = sorted(set(int(l) for ls in pred_labels + gt_labels for l in np.asarray(ls).ravel()))
    iou_thrs, rec_thrs, max_dets = p['iouThrs'], p['recThrs'], p['maxDets']
    T, R, K, A, M = len(iou_thrs), len(rec_thrs), len(cat_ids), len(p['areaRng']), len(max_dets)

    # evalImgs[k][a][i]
    eval_imgs = [[[None] * n_img for _ in range(A)] for _ in range(K)]
    for i, (table, pl, ps, gl, gc, ga) in enumerate(zip(
            counts, pred_labels, pred_scores, gt_labels, gt_crowdeds, gt_areas)):
        pl, ps, gl = np.asarray(pl).ravel(), np.asarray(ps).ravel(), np.asarray(gl).ravel()
        ious_of, pred_area, gt_area_px = image_of(table, len(pl), len(gl))
        gc = np.zeros(len(gl), bool) if gc is None else np.asarray(gc).astype(bool).ravel()
        # the annotation 'area' of a gt: the given one, else its pixel count (its box's w*h)
        ga = gt_area_px if ga is None else np.asarray(ga).ravel()
        for k, cat in enumerate(cat_ids):
            d_idx = np.flatnonzero(pl == cat)
            g_idx = np.flatnonzero(gl == cat)
            if len(d_idx) == 0 and len(g_idx) == 0:
                continue
            # computeIoU: detections by descending score (mergesort), first maxDets[-1]
            d_idx = d_idx[np.argsort(-ps[d_idx], kind='mergesort')][:max_dets[-1]]
            if len(d_idx) and len(g_idx):
                ious = ious_of(d_idx, g_idx, gc)
            else:
                ious = np.zeros((0, 0))
            for a, a_rng in enumerate(p['areaRng']):
                eval_imgs[k][a][i] = _evaluate_img(
                    ious, ps[d_idx], pred_area[d_idx], gc[g_idx], ga[g_idx], a_rng,
                    max_dets[-1], iou_thrs)

    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    for k in range(K):
        for a in range(A):
            for m, max_det in enumerate(max_dets):
                E = [e for e in eval_imgs[k][a] if e is not None]
                if len(E) == 0:
                    continue
                dt_scores = np.concatenate([e['dtScores'][0:max_det] for e in E])
                # mergesort: the order pycocotools (and its Matlab original) use
                inds = np.argsort(-dt_scores, kind='mergesort')
                dtm = np.concatenate([e['dtMatches'][:, 0:max_det] for e in E], axis=1)[:, inds]
                dt_ig = np.concatenate([e['dtIgnore'][:, 0:max_det] for e in E], axis=1)[:, inds]
                gt_ig = np.concatenate([e['gtIgnore'] for e in E])
                npig = np.count_nonzero(gt_ig == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dt_ig))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=np.float64)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=np.float64)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    for j in range(nd - 1, 0, -1):
                        if pr[j] > pr[j - 1]:
                            pr[j - 1] = pr[j]
                    for ri, pi in enumerate(np.searchsorted(rc, rec_thrs, side='left')):
                        if pi >= nd:
                            break
                        q[ri] = pr[pi]
                    precision[t, :, k, a, m] = q
    params = dict(p, catIds=cat_ids, imgIds=list(range(1, n_img + 1)))
    return {'precision': precision, 'recall': recall, 'params': params}


COCO_SETTINGS = [
    # key, ap, iou_thresh, area_range, max_detection
    ('ap/iou=0.50:0.95/area=all/maxDets=100', True, None, 'all', 100),
    ('ap/iou=0.50/area=all/maxDets=100', True, 0.5, 'all', 100),
    ('ap/iou=0.75/area=all/maxDets=100', True, 0.75, 'all', 100),
    ('ap/iou=0.50:0.95/area=small/maxDets=100', True, None, 'small', 100),
    ('ap/iou=0.50:0.95/area=medium/maxDets=100', True, None, 'medium', 100),
    ('ap/iou=0.50:0.95/area=large/maxDets=100', True, None, 'large', 100),
    ('ar/iou=0.50:0.95/area=all/maxDets=1', False, None, 'all', 1),
    ('ar/iou=0.50:0.95/area=all/maxDets=10', False, None, 'all', 10),
    ('ar/iou=0.50:0.95/area=all/maxDets=100', False, None, 'all', 100),
    ('ar/iou=0.50:0.95/area=small/maxDets=100', False, None, 'small', 100),
    ('ar/iou=0.50:0.95/area=medium/maxDets=100', False, None, 'medium', 100),
    ('ar/iou=0.50:0.95/area=large/maxDets=100', False, None, 'large', 100),
]


def summarize(prec, rec, iou_threshs, area_ranges, max_detection_list, ap=True,
              iou_thresh=None, area_range='all', max_detection=100):
    """The reference's ``_summarize``: per-class values (float32, NaN where undefined) over the
    K axis of ``prec`` / ``rec``, and their NaN-mean."""
    a_idx = area_ranges.index(area_range)
    m_idx = max_detection_list.index(max_detection)
    if ap:
        s = prec.copy()  # (T, R, K, A, M)
        if iou_thresh is not None:
            s = s[iou_thresh == iou_threshs]
        s = s[:, :, :, a_idx, m_idx]
    else:
        s = rec.copy()  # (T, K, A, M)
        if iou_thresh is not None:
            s = s[iou_thresh == iou_threshs]
        s = s[:, :, a_idx, m_idx]

    s[s == -1] = np.nan
    s = s.reshape((-1, s.shape[-1]))
    valid_classes = np.any(np.logical_not(np.isnan(s)), axis=0)
    class_s = np.nan * np.ones(len(valid_classes), dtype=np.float32)
    class_s[valid_classes] = np.nanmean(s[:, valid_classes], axis=0)

    if not np.any(valid_classes):
        mean_s = np.nan
    else:
        mean_s = np.nanmean(class_s)
    return class_s, mean_s


def coco_results(coco_eval):
    """eval_instseg_coco's result dict from a ``coco_evaluate_from_counts`` (or ``_from_ious``)
    result."""
    p = coco_eval['params']
    results = {'coco_eval': coco_eval}
    for key, ap, iou_thresh, area_range, max_detection in COCO_SETTINGS:
        metrics, mean_metric = summarize(
            coco_eval['precision'], coco_eval['recall'], p['iouThrs'], p['areaRngLbl'],
            p['maxDets'], ap=ap, iou_thresh=iou_thresh, area_range=area_range,
            max_detection=max_detection)
        results[key] = metrics
        results['m' + key] = mean_metric
    return results
