"""utils.eval_instseg_coco — the reference's
chainer_mask_rcnn/utils/evaluations/eval_instance_segmentation_coco.py without pycocotools:
the mask intersections are counted on the device (masks.py), COCOeval's segm matching and
accumulation and the reference's ``_summarize`` are restated in matching.py."""
from .masks import mask_counts
from .matching import coco_evaluate_from_counts, coco_results


def eval_instseg_coco(pred_masks, pred_labels, pred_scores, gt_masks, gt_labels,
                      gt_crowdeds=None, gt_areas=None):
    """Returns the reference's keys: ``ap/...``, ``map/...``, ``ar/...``, ``mar/...`` for the
    twelve COCO settings, and ``coco_eval``: a dict with ``precision`` (T,R,K,A,M),
    ``recall`` (T,K,A,M) and ``params`` (K = the sorted labels present)."""
    counts = [mask_counts(pm, gm) for pm, gm in zip(pred_masks, gt_masks)]
    return coco_results(coco_evaluate_from_counts(counts, pred_labels, pred_scores, gt_labels,
                                                  gt_crowdeds, gt_areas))
