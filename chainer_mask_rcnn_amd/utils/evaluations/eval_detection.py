"""utils.eval_detection_voc / eval_detection_coco — chainercv's box-AP evaluations
(chainercv/evaluations/eval_detection_voc.py, eval_detection_coco.py) with their names and
argument orders, without chainercv or pycocotools: every IoU table of the call is made on the
device in one launch (boxes.py), the matching and accumulation are the loops the mask evaluations
run (matching.py).  Boxes are (y1, x1, y2, x2) float32, host arrays or device tensors."""
import numpy as np

from . import boxes as B
from . import matching
from .records import Readback


def voc_box_tables(pred_bboxes, gt_bboxes):
    """Per-image float32 (P, G) IoU tables in the VOC convention (+1 on the max corners)."""
    readback = Readback()
    readback.add_split(*B.queue_box_ious(pred_bboxes, gt_bboxes, 'voc'))
    return readback.fetch()


def coco_box_tables(pred_xywh, gt_xywh, gt_crowdeds=None):
    """Per-image ``(iou, dt_area, gt_box_area)`` for ``matching.coco_evaluate_from_ious`` from
    float64 (x, y, w, h) boxes: bbIou tables from the device, areas ``w*h``."""
    pred_xywh, gt_xywh = list(pred_xywh), list(gt_xywh)
    readback = Readback()
    readback.add_split(*B.queue_box_ious(pred_xywh, gt_xywh, 'coco', crowd_b=gt_crowdeds))
    return [(t, box_areas(d), box_areas(g))
            for t, d, g in zip(readback.fetch(), pred_xywh, gt_xywh)]


def box_areas(xywh):
    """``w*h`` float64 of (N, 4) (x, y, w, h) float64 boxes: the 'area' pycocotools' loadRes gives
    a bbox detection."""
    b = np.asarray(xywh, np.float64).reshape(-1, 4)
    return b[:, 2] * b[:, 3]


def eval_detection_voc(pred_bboxes, pred_labels, pred_scores, gt_bboxes, gt_labels,
                       gt_difficults=None, iou_thresh=0.5, use_07_metric=False):
    """{'ap': per-class box AP (NaN for absent classes), 'map': their NaN-mean}."""
    pred_bboxes, gt_bboxes = list(pred_bboxes), list(gt_bboxes)
    prec, rec = matching.voc_prec_rec_from_ious(
        voc_box_tables(pred_bboxes, gt_bboxes), pred_labels, pred_scores, gt_labels,
        gt_difficults, iou_thresh=iou_thresh)
    ap = matching.calc_detection_voc_ap(prec, rec, use_07_metric=use_07_metric)
    return {'ap': ap, 'map': np.nanmean(ap)}


def eval_detection_coco(pred_bboxes, pred_labels, pred_scores, gt_bboxes, gt_labels,
                        gt_areas=None, gt_crowdeds=None):
    """The key set of ``eval_instseg_coco`` (``ap/...``, ``map/...``, ``ar/...``, ``mar/...``,
    ``coco_eval``) for boxes.  ``gt_areas`` decides a ground truth's area range when given,
    otherwise its box's ``w*h`` does."""
    gt_crowdeds = None if gt_crowdeds is None else list(gt_crowdeds)
    tables = coco_box_tables([B.to_xywh64(b) for b in pred_bboxes],
                             [B.to_xywh64(b) for b in gt_bboxes], gt_crowdeds)
    return matching.coco_results(matching.coco_evaluate_from_ious(
        tables, pred_labels, pred_scores, gt_labels, gt_crowdeds, gt_areas))
