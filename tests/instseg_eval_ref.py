"""Independent NumPy restatement of the instance-segmentation evaluations on plain full-image
boolean masks: the reference's VOC algorithm (calc_instseg_voc_prec_rec + chainercv's
calc_detection_voc_ap) and pycocotools' COCOeval (segm: evaluate / evaluateImg / accumulate)
plus the reference's _summarize.  Written from the published algorithms, annotation dicts and
all, without sharing code with chainer_mask_rcnn_amd.utils.evaluations."""
from collections import defaultdict

import numpy as np


# ------------------------------------------------------------------------------------- VOC
def mask_iou(a, b):
    iou = np.zeros((len(a), len(b)), np.float64)
    for i, ma in enumerate(a):
        for j, mb in enumerate(b):
            inter = np.logical_and(ma, mb).sum()
            union = np.logical_or(ma, mb).sum()
            iou[i, j] = 0. if union == 0 else 1.0 * inter / union
    return iou


def voc_prec_rec(pred_masks, pred_labels, pred_scores, gt_masks, gt_labels, gt_difficults=None,
                 iou_thresh=0.5):
    n_pos, score, match = defaultdict(int), defaultdict(list), defaultdict(list)
    if gt_difficults is None:
        gt_difficults = [None] * len(gt_labels)
    for pm, pl, ps, gm, gl, gd in zip(pred_masks, pred_labels, pred_scores, gt_masks, gt_labels,
                                      gt_difficults):
        gd = np.zeros(len(gl), bool) if gd is None else np.asarray(gd, bool)
        for l in np.unique(np.concatenate((pl, gl)).astype(int)):
            ps_l = ps[pl == l]
            order = ps_l.argsort()[::-1]
            pm_l = pm[pl == l][order]
            gm_l, gd_l = gm[gl == l], gd[gl == l]
            n_pos[l] += int((~gd_l).sum())
            score[l].extend(ps_l[order])
            if len(pm_l) == 0:
                continue
            if len(gm_l) == 0:
                match[l] += [0] * len(pm_l)
                continue
            iou = mask_iou(pm_l, gm_l)
            best = iou.argmax(axis=1)
            best[iou.max(axis=1) < iou_thresh] = -1
            taken = np.zeros(len(gm_l), bool)
            for g in best:
                if g < 0:
                    match[l].append(0)
                    continue
                match[l].append(-1 if gd_l[g] else (0 if taken[g] else 1))
                taken[g] = True
    n = max(n_pos) + 1
    prec, rec = [None] * n, [None] * n
    for l in n_pos:
        m = np.array(match[l], np.int8)[np.array(score[l]).argsort()[::-1]]
        tp, fp = np.cumsum(m == 1), np.cumsum(m == 0)
        prec[l] = tp / (fp + tp)
        if n_pos[l] > 0:
            rec[l] = tp / n_pos[l]
    return prec, rec


def voc_ap(prec, rec, use_07_metric=False):
    ap = np.empty(len(prec))
    for l in range(len(prec)):
        if prec[l] is None or rec[l] is None:
            ap[l] = np.nan
        elif use_07_metric:
            ap[l] = 0
            for t in np.arange(0., 1.1, 0.1):
                sel = rec[l] >= t
                ap[l] += (np.max(np.nan_to_num(prec[l])[sel]) if sel.any() else 0) / 11
        else:
            mpre = np.concatenate(([0], np.nan_to_num(prec[l]), [0]))
            mrec = np.concatenate(([0], rec[l], [1]))
            for i in range(len(mpre) - 2, -1, -1):
                mpre[i] = max(mpre[i], mpre[i + 1])
            i = np.where(mrec[1:] != mrec[:-1])[0]
            ap[l] = np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])
    return ap


# ------------------------------------------------------------------------------------ COCO
IOU_THRS = np.linspace(.5, .95, 10)
REC_THRS = np.linspace(.0, 1.00, 101)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
AREA_LBL = ['all', 'small', 'medium', 'large']


def _seg_iou(dts, gts):
    """maskUtils.iou on full masks: crowd gt -> inter / area(dt)."""
    out = np.zeros((len(dts), len(gts)))
    for i, d in enumerate(dts):
        for j, g in enumerate(gts):
            inter = int(np.logical_and(d['m'], g['m']).sum())
            if inter == 0:
                continue
            u = int(d['m'].sum()) if g['iscrowd'] else int(np.logical_or(d['m'], g['m']).sum())
            out[i, j] = inter / u
    return out


def coco_eval(pred_masks, pred_labels, pred_scores, gt_masks, gt_labels, gt_crowdeds=None,
              gt_areas=None):
    n_img = len(gt_masks)
    dts, gts = defaultdict(list), defaultdict(list)
    cats = set()
    aid = 0
    for i in range(n_img):
        for m, l, s in zip(pred_masks[i], pred_labels[i], pred_scores[i]):
            aid += 1
            dts[i + 1, int(l)].append(dict(id=aid, m=m.astype(bool), score=s, area=int(m.astype(bool).sum()),
                                           iscrowd=0))
            cats.add(int(l))
    aid = 0
    for i in range(n_img):
        for j, (m, l) in enumerate(zip(gt_masks[i], gt_labels[i])):
            aid += 1
            crowd = 0 if gt_crowdeds is None else int(gt_crowdeds[i][j])
            area = int(m.astype(bool).sum()) if gt_areas is None else gt_areas[i][j]
            gts[i + 1, int(l)].append(dict(id=aid, m=m.astype(bool), area=area, iscrowd=crowd,
                                           ignore=crowd))
            cats.add(int(l))
    cat_ids, img_ids = sorted(cats), list(range(1, n_img + 1))
    ious = {}
    for img in img_ids:
        for c in cat_ids:
            g, d = gts[img, c], dts[img, c]
            if not g and not d:
                ious[img, c] = []
                continue
            d = [d[k] for k in np.argsort([-x['score'] for x in d], kind='mergesort')][:MAX_DETS[-1]]
            ious[img, c] = _seg_iou(d, g) if (d and g) else []

    def evaluate_img(img, c, a_rng, max_det):
        gt, dt = gts[img, c], dts[img, c]
        if not gt and not dt:
            return None
        for g in gt:
            g['_ignore'] = 1 if (g['ignore'] or g['area'] < a_rng[0] or g['area'] > a_rng[1]) else 0
        gtind = np.argsort([g['_ignore'] for g in gt], kind='mergesort')
        gt = [gt[k] for k in gtind]
        dtind = np.argsort([-d['score'] for d in dt], kind='mergesort')
        dt = [dt[k] for k in dtind[0:max_det]]
        iscrowd = [int(o['iscrowd']) for o in gt]
        iou_ = ious[img, c][:, gtind] if len(ious[img, c]) > 0 else ious[img, c]
        T, G, D = len(IOU_THRS), len(gt), len(dt)
        gtm, dtm = np.zeros((T, G)), np.zeros((T, D))
        gt_ig = np.array([g['_ignore'] for g in gt])
        dt_ig = np.zeros((T, D))
        if not len(iou_) == 0:
            for tind, t in enumerate(IOU_THRS):
                for dind, d in enumerate(dt):
                    iou = min([t, 1 - 1e-10])
                    m = -1
                    for gind, g in enumerate(gt):
                        if gtm[tind, gind] > 0 and not iscrowd[gind]:
                            continue
                        if m > -1 and gt_ig[m] == 0 and gt_ig[gind] == 1:
                            break
                        if iou_[dind, gind] < iou:
                            continue
                        iou = iou_[dind, gind]
                        m = gind
                    if m == -1:
                        continue
                    dt_ig[tind, dind] = gt_ig[m]
                    dtm[tind, dind] = gt[m]['id']
                    gtm[tind, m] = d['id']
        a = np.array([d['area'] < a_rng[0] or d['area'] > a_rng[1] for d in dt]).reshape((1, len(dt)))
        dt_ig = np.logical_or(dt_ig, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
        return dict(dtMatches=dtm, dtScores=[d['score'] for d in dt], gtIgnore=gt_ig, dtIgnore=dt_ig)

    evals = [evaluate_img(img, c, a, MAX_DETS[-1]) for c in cat_ids for a in AREA_RNG
             for img in img_ids]
    T, R, K, A, M = len(IOU_THRS), len(REC_THRS), len(cat_ids), len(AREA_RNG), len(MAX_DETS)
    precision, recall = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M))
    I0, A0 = len(img_ids), len(AREA_RNG)
    for k in range(K):
        for a in range(A):
            for m, max_det in enumerate(MAX_DETS):
                E = [evals[k * A0 * I0 + a * I0 + i] for i in range(I0)]
                E = [e for e in E if e is not None]
                if not E:
                    continue
                scores = np.concatenate([e['dtScores'][0:max_det] for e in E])
                inds = np.argsort(-scores, kind='mergesort')
                dtm = np.concatenate([e['dtMatches'][:, 0:max_det] for e in E], axis=1)[:, inds]
                dt_ig = np.concatenate([e['dtIgnore'][:, 0:max_det] for e in E], axis=1)[:, inds]
                gt_ig = np.concatenate([e['gtIgnore'] for e in E])
                npig = np.count_nonzero(gt_ig == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dt_ig))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
                tp_sum = np.cumsum(tps, axis=1).astype(float)
                fp_sum = np.cumsum(fps, axis=1).astype(float)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    nd = len(tp)
                    rc = tp / npig
                    pr = (tp / (fp + tp + np.spacing(1))).tolist()
                    q = [0.] * R
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    try:
                        for ri, pi in enumerate(np.searchsorted(rc, REC_THRS, side='left')):
                            q[ri] = pr[pi]
                    except IndexError:
                        pass
                    precision[t, :, k, a, m] = np.array(q)
    return precision, recall, cat_ids


SETTINGS = {
    'ap/iou=0.50:0.95/area=all/maxDets=100': (True, None, 'all', 100),
    'ap/iou=0.50/area=all/maxDets=100': (True, 0.5, 'all', 100),
    'ap/iou=0.75/area=all/maxDets=100': (True, 0.75, 'all', 100),
    'ap/iou=0.50:0.95/area=small/maxDets=100': (True, None, 'small', 100),
    'ap/iou=0.50:0.95/area=medium/maxDets=100': (True, None, 'medium', 100),
    'ap/iou=0.50:0.95/area=large/maxDets=100': (True, None, 'large', 100),
    'ar/iou=0.50:0.95/area=all/maxDets=1': (False, None, 'all', 1),
    'ar/iou=0.50:0.95/area=all/maxDets=10': (False, None, 'all', 10),
    'ar/iou=0.50:0.95/area=all/maxDets=100': (False, None, 'all', 100),
    'ar/iou=0.50:0.95/area=small/maxDets=100': (False, None, 'small', 100),
    'ar/iou=0.50:0.95/area=medium/maxDets=100': (False, None, 'medium', 100),
    'ar/iou=0.50:0.95/area=large/maxDets=100': (False, None, 'large', 100),
}


def coco_summary(precision, recall):
    out = {}
    for key, (ap, thr, area, max_det) in SETTINGS.items():
        a, m = AREA_LBL.index(area), MAX_DETS.index(max_det)
        s = (precision if ap else recall).copy()
        if thr is not None:
            s = s[thr == IOU_THRS]
        s = s[:, :, :, a, m] if ap else s[:, :, a, m]
        s[s == -1] = np.nan
        s = s.reshape((-1, s.shape[-1]))
        valid = np.any(~np.isnan(s), axis=0)
        cls = np.full(len(valid), np.nan, np.float32)
        cls[valid] = np.nanmean(s[:, valid], axis=0)
        out[key] = cls
        out['m' + key] = np.nanmean(cls) if valid.any() else np.nan
    return out


def coco_counts(pred_masks, gt_masks):
    """(inter, pred_area, gt_area) per image from full masks, for the host matching code."""
    out = []
    for pm, gm in zip(pred_masks, gt_masks):
        hw = int(np.prod(pm.shape[1:]))
        pm = pm.reshape(len(pm), hw).astype(bool).astype(np.int64)
        gm = gm.reshape(len(gm), hw).astype(bool).astype(np.int64)
        out.append((pm @ gm.T, pm.sum(1), gm.sum(1)))
    return out
