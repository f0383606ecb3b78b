"""utils.eval_instseg_voc / calc_instseg_voc_prec_rec / mask_iou — the reference's
chainer_mask_rcnn/utils/evaluations/eval_instance_segmentation_voc.py with the mask
intersections counted on the device (masks.py) and the matching in matching.py."""
import numpy as np

from .eval_instance_segmentation_coco import check_iou_type
from .masks import mask_and_boundary_counts, mask_counts, mask_iou  # noqa: F401
from .matching import (calc_detection_voc_ap, voc_prec_rec_from_boundary_counts,
                       voc_prec_rec_from_counts)


def calc_instseg_voc_prec_rec(pred_masks, pred_labels, pred_scores, gt_masks, gt_labels,
                              gt_difficults=None, iou_thresh=0.5, iou_type='segm',
                              dilation_ratio=0.02):
    """Per-class precision and recall lists as the reference computes them: ``prec[l]`` is
    None for a class in neither predictions nor ground truth, ``rec[l]`` is None for a class
    without non-difficult ground truth.  ``iou_type='boundary'`` matches on min(mask IoU,
    boundary IoU), the boundaries cut at ``dilation_ratio`` of the image diagonal."""
    check_iou_type(iou_type)
    if iou_type == 'boundary':
        both = [mask_and_boundary_counts(pm, gm, dilation_ratio)
                for pm, gm in zip(pred_masks, gt_masks)]
        return voc_prec_rec_from_boundary_counts(
            [m for m, _ in both], [b for _, b in both], pred_labels, pred_scores, gt_labels,
            gt_difficults, iou_thresh=iou_thresh)
    counts = [mask_counts(pm, gm) for pm, gm in zip(pred_masks, gt_masks)]
    return voc_prec_rec_from_counts(counts, pred_labels, pred_scores, gt_labels, gt_difficults,
                                    iou_thresh=iou_thresh)


def eval_instseg_voc(pred_masks, pred_labels, pred_scores, gt_masks, gt_labels,
                     gt_difficults=None, iou_thresh=0.5, use_07_metric=False, iou_type='segm',
                     dilation_ratio=0.02):
    """{'ap': per-class AP (NaN for absent classes), 'map': their NaN-mean}."""
    prec, rec = calc_instseg_voc_prec_rec(pred_masks, pred_labels, pred_scores, gt_masks,
                                          gt_labels, gt_difficults, iou_thresh=iou_thresh,
                                          iou_type=iou_type, dilation_ratio=dilation_ratio)
    ap = calc_detection_voc_ap(prec, rec, use_07_metric=use_07_metric)
    return {'ap': ap, 'map': np.nanmean(ap)}
