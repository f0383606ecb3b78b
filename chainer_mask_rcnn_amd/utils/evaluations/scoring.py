"""From ``EvalRecords`` to the evaluators' report keys: one loop over the IoU types, each row of
a table naming the matching entry point (matching.py), the tables it reads and its key prefix."""
import numpy as np

from . import matching

# IoU type -> (VOC entry point, COCO entry point, the records' tables it reads, key prefix)
SCORERS = {
    'segm': (matching.voc_prec_rec_from_counts, matching.coco_evaluate_from_counts,
             ('segm',), ''),
    'bbox': (matching.voc_prec_rec_from_ious, matching.coco_evaluate_from_ious,
             ('bbox',), 'bbox/'),
    'boundary': (matching.voc_prec_rec_from_boundary_counts,
                 matching.coco_evaluate_from_boundary_counts, ('segm', 'boundary'), 'boundary/'),
}


def voc_report(ap, label_names=None):
    report = {'map': np.nanmean(ap)}
    if label_names is not None:
        for l, label_name in enumerate(label_names):
            report['ap/{:s}'.format(label_name)] = ap[l] if l < len(ap) else np.nan
    return report


def coco_report(result, label_names=None):
    report = {
        'map': result['map/iou=0.50:0.95/area=all/maxDets=100'],
        'map@0.5': result['map/iou=0.50/area=all/maxDets=100'],
        'map@0.75': result['map/iou=0.75/area=all/maxDets=100'],
    }
    if label_names is not None:
        per_class = result['ap/iou=0.50:0.95/area=all/maxDets=100']
        k_of = {int(c): k for k, c in enumerate(result['coco_eval']['params']['catIds'])}
        for l, label_name in enumerate(label_names):
            k = k_of.get(l)
            report['ap/{:s}'.format(label_name)] = per_class[k] if k is not None else np.nan
    return report


def score_voc(records, iou_types, use_07_metric=False, label_names=None):
    """``map`` and ``ap/<name>`` per IoU type, under its prefix ('', 'bbox/', 'boundary/')."""
    report = {}
    for t in iou_types:
        entry, _, reads, prefix = SCORERS[t]
        prec, rec = entry(*[records.tables[k] for k in reads], records.pred_labels,
                          records.pred_scores, records.gt_labels, records.gt_difficults)
        ap = matching.calc_detection_voc_ap(prec, rec, use_07_metric=use_07_metric)
        report.update((prefix + k, v) for k, v in voc_report(ap, label_names).items())
    return report


def score_coco(records, iou_types, label_names=None):
    """``map``, ``map@0.5``, ``map@0.75`` and ``ap/<name>`` per IoU type, under its prefix."""
    report = {}
    for t in iou_types:
        _, entry, reads, prefix = SCORERS[t]
        result = matching.coco_results(entry(
            *[records.tables[k] for k in reads], records.pred_labels, records.pred_scores,
            records.gt_labels, records.gt_crowdeds, records.gt_areas))
        report.update((prefix + k, v) for k, v in coco_report(result, label_names).items())
    return report
