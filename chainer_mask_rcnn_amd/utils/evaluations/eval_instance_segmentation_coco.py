"""utils.eval_instseg_coco — the reference's
chainer_mask_rcnn/utils/evaluations/eval_instance_segmentation_coco.py without pycocotools:
the mask intersections are counted on the device (masks.py), COCOeval's segm matching and
accumulation and the reference's ``_summarize`` are restated in matching.py."""
from .masks import mask_and_boundary_counts, mask_counts
from .matching import (coco_evaluate_from_boundary_counts, coco_evaluate_from_counts,
                       coco_results)


def check_iou_type(iou_type):
    if iou_type not in ('segm', 'boundary'):
        raise ValueError("iou_type must be 'segm' or 'boundary', got %r" % (iou_type,))


def eval_instseg_coco(pred_masks, pred_labels, pred_scores, gt_masks, gt_labels,
                      gt_crowdeds=None, gt_areas=None, iou_type='segm', dilation_ratio=0.02):
    """Returns the reference's keys: ``ap/...``, ``map/...``, ``ar/...``, ``mar/...`` for the
    twelve COCO settings, and ``coco_eval``: a dict with ``precision`` (T,R,K,A,M),
    ``recall`` (T,K,A,M) and ``params`` (K = the sorted labels present).

    ``iou_type='boundary'``: Boundary AP, the same evaluation on min(mask IoU, boundary IoU)
    with the boundaries cut at ``dilation_ratio`` of the image diagonal (masks.py)."""
    check_iou_type(iou_type)
    if iou_type == 'boundary':
        both = [mask_and_boundary_counts(pm, gm, dilation_ratio)
                for pm, gm in zip(pred_masks, gt_masks)]
        return coco_results(coco_evaluate_from_boundary_counts(
            [m for m, _ in both], [b for _, b in both], pred_labels, pred_scores, gt_labels,
            gt_crowdeds, gt_areas))
    counts = [mask_counts(pm, gm) for pm, gm in zip(pred_masks, gt_masks)]
    return coco_results(coco_evaluate_from_counts(counts, pred_labels, pred_scores, gt_labels,
                                                  gt_crowdeds, gt_areas))
