"""InstanceSegmentationVOCEvaluator / InstanceSegmentationCOCOEvaluator — the reference's
chainer_mask_rcnn/extensions/instance_segmentation_{voc,coco}_evaluator.py.

``evaluate()`` returns the observation dict chainer's reporter builds for ``name='validation'``
(``validation/main/map``, ...).  Predicted masks never leave the device: per batch,
``predict_images(masks_to_host=False)`` -> packed paste -> intersections
against the uploaded and packed ground truth, all queued before one read-back of the counts
and areas.  Boxes, labels and scores come back as ``predict_images`` returns them (with the
model's test-time augmentation, if it has any configured).  Matching
and accumulation run on the host from those counts (utils/evaluations/matching.py).

``iou_types=('segm', 'bbox')`` adds box AP under ``validation/main/bbox/...``: the batch's box IoU
tables (predicted boxes against the examples' ``bbox`` field) are made in one more launch
(utils/evaluations/boxes.py), queued before the same single read-back, and scored by the same
matching loops — the VOC evaluator as chainercv's ``eval_detection_voc`` would (float32, +1 on the
max corners), the COCO evaluator as pycocotools' iouType 'bbox' would (float64 x, y, w, h, crowd
rule).  The ground-truth boxes are whatever the dataset puts in the example, which is what
chainercv's detection evaluators are fed: for this project's COCO dataset that is the mask's tight
box, not the annotation's ``bbox``.  ``('bbox',)`` alone skips the paste,
pack and intersect work and reports only the ``bbox/`` keys.

``'boundary'`` in ``iou_types`` adds Boundary AP (Cheng et al., CVPR 2021) under
``validation/main/boundary/...``: the boundaries of the packed predictions and ground truth are cut
on the device (``masks.boundary_packed``, erosion distance ``boundary_dilation_ratio`` of the image
diagonal), intersected by the same kernel and carried in the same read-back; the matching runs on
min(mask IoU, boundary IoU).  The masks are pasted, packed and intersected
for it even without ``'segm'``.
"""
import copy

import numpy as np
import torch

from ..utils.evaluations import boxes as B
from ..utils.evaluations import eval_detection as D
from ..utils.evaluations import masks as M
from ..utils.evaluations import matching
from ..utils.evaluations import rle


def _batches(iterator):
    """Batches of examples from a chainer-style iterator (``reset()``: iterated once after a
    reset), an iterator exposing ``dataset`` and ``batch_size`` (the dataset in order, once), or
    any iterable of batches."""
    if hasattr(iterator, 'reset'):
        iterator.reset()
        for batch in iterator:
            yield batch
    elif hasattr(iterator, 'dataset') and hasattr(iterator, 'batch_size'):
        data, bs = iterator.dataset, int(iterator.batch_size)
        for i in range(0, len(data), bs):
            yield [data[j] for j in range(i, min(i + bs, len(data)))]
    else:
        # a one-shot iterator (e.g. a generator) is consumed as it is; a container is copied
        for batch in (iterator if iter(iterator) is iterator else copy.copy(iterator)):
            yield batch


class _InstanceSegmentationEvaluator(object):

    name = 'validation'
    results_sink = None
    box_convention = None     # 'voc' | 'coco': boxes.queue_box_ious' convention

    IOU_TYPES = ('segm', 'bbox', 'boundary')

    def __init__(self, iterator, target, label_names=None, iou_types=('segm',),
                 boundary_dilation_ratio=0.02):
        self.iterator = iterator
        self.target = target
        self.label_names = label_names
        iou_types = (iou_types,) if isinstance(iou_types, str) else tuple(iou_types)
        if not iou_types or any(t not in self.IOU_TYPES for t in iou_types):
            raise ValueError("iou_types: a non-empty subset of %r, got %r"
                             % (self.IOU_TYPES, iou_types))
        self.iou_types = iou_types
        self.boundary_dilation_ratio = boundary_dilation_ratio

    def __call__(self, trainer=None):
        return self.evaluate()

    def _observation(self, report):
        return {'%s/main/%s' % (self.name, k): v for k, v in report.items()}

    def _queue_box_ious(self, bboxes, batch, dev):
        """The batch's box IoU tables, queued: (flat device tensor, shapes, per-image areas)."""
        gt_boxes = [ex[1] for ex in batch]
        if self.box_convention == 'voc':
            iou, shapes = B.queue_box_ious(bboxes, gt_boxes, 'voc', device=dev)
            return iou, shapes, None
        pred, gt = [B.to_xywh64(b) for b in bboxes], [B.to_xywh64(b) for b in gt_boxes]
        crowd = [ex[4] for ex in batch] if len(batch[0]) == 6 else None
        iou, shapes = B.queue_box_ious(pred, gt, 'coco', crowd_b=crowd, device=dev)
        return iou, shapes, [(D.box_areas(p), D.box_areas(g)) for p, g in zip(pred, gt)]

    def collect(self):
        """Run the model over the iterator.  Returns (counts, pred_labels, pred_scores,
        ground-truth tuples): counts[i] = (inter (P,G), pred_area (P,), gt_area (G,)) host int64
        arrays; gt tuple = the example's entries after the image (bbox, label, mask, ...).

        With ``'bbox'`` in ``iou_types`` a fifth list follows, the images' box IoU records: the
        float32 (P, G) table (VOC evaluator) or ``(iou float64 (P,G), dt_area (P,), gt_box_area
        (G,))`` (COCO evaluator).  Without ``'segm'`` every counts[i] is None.

        With ``'boundary'`` in ``iou_types`` six lists come back: the fifth as above (every
        box_ious[i] None without ``'bbox'``), the sixth the boundaries' counts, boundary_counts[i] =
        (inter (P,G), pred boundary area (P,), gt boundary area (G,)); counts[i] is then always
        filled, as the matching takes the minimum of the two IoUs."""
        target = self.target
        sink = self.results_sink
        bbox, boundary = 'bbox' in self.iou_types, 'boundary' in self.iou_types
        segm = 'segm' in self.iou_types or boundary      # the masks are needed
        n_seen = 0
        counts, pred_labels, pred_scores, gts, box_ious = [], [], [], [], []
        boundary_counts = []
        for batch in _batches(self.iterator):
            batch = list(batch)
            if not batch:
                continue
            for ex in batch:
                if len(ex) not in (4, 5, 6):
                    raise ValueError('expected (img, bbox, label, mask[, difficult | crowd, area]) '
                                     'examples, got a %d-tuple' % len(ex))
            bboxes, roi_masks, labels, scores, sizes = target.predict_images(
                [ex[0] for ex in batch], masks_to_host=False)
            dev = roi_masks[0].device
            queued, encodes = [], []
            for j, ex in enumerate(batch if segm else ()):
                gt_mask = ex[3]
                H, W = sizes[j]
                if tuple(gt_mask.shape[1:]) != (H, W):
                    raise ValueError('ground-truth masks of shape %s for an image of size %s'
                                     % (tuple(gt_mask.shape), (H, W)))
                pred = M.paste_packed(roi_masks[j], labels[j], bboxes[j], (H, W))
                gt = M.pack_masks(gt_mask, device=dev)
                if boundary:
                    queued.append(M.queue_mask_and_boundary_counts(
                        pred, gt, (H, W), self.boundary_dilation_ratio))
                else:
                    queued.append((M.queue_intersections(pred, gt, W), pred[1], gt[1]))
                if sink is not None:          # the packed masks just intersected, encoded
                    encodes.append(rle.queue_encode(pred[0], pred[1], pred[2], (H, W)))
            parts = [t.reshape(-1).to(torch.int64) for q in queued for t in q]
            if bbox:
                # the IoU bit patterns ride at the end of the int64 buffer (a float32 pattern
                # widened from int32, a float64 one reinterpreted): exact both ways
                iou_d, shapes, areas = self._queue_box_ious(bboxes, batch, dev)
                parts.append(iou_d.view(torch.int32).to(torch.int64)
                             if iou_d.dtype == torch.float32 else iou_d.view(torch.int64))
            # one read-back for the whole batch
            flat = torch.cat(parts)
            host = flat.cpu().numpy()
            if sink is not None:              # the batch's strings: one more small read-back
                all_segs = rle.fetch_encoded(encodes) if segm else [None] * len(batch)
                for j, segs in enumerate(all_segs):
                    sink(n_seen + j, bboxes[j], labels[j], scores[j], segs)
            n_seen += len(batch)
            o = 0
            for j, (l, s, ex) in enumerate(zip(labels, scores, batch)):
                if segm:
                    P, G = queued[j][0].shape
                    c_inter = host[o:o + P * G].reshape(P, G)
                    o += P * G
                    c_pa = host[o:o + P]
                    o += P
                    c_ga = host[o:o + G]
                    o += G
                    counts.append((c_inter, c_pa, c_ga))
                    if boundary:
                        triple, o = M.take_counts(host, o, P, G)
                        boundary_counts.append(triple)
                else:
                    counts.append(None)
                pred_labels.append(l)
                pred_scores.append(s)
                gts.append(tuple(ex[1:]))
            if bbox:
                tail = host[o:]
                tail = (tail.astype(np.int32).view(np.float32) if self.box_convention == 'voc'
                        else tail.view(np.float64))
                tables = B.split_tables(tail, shapes)
                box_ious.extend(tables if areas is None else
                                [(t,) + a for t, a in zip(tables, areas)])
            else:
                box_ious.extend([None] * len(batch))
        if boundary:
            return counts, pred_labels, pred_scores, gts, box_ious, boundary_counts
        if bbox:
            return counts, pred_labels, pred_scores, gts, box_ious
        return counts, pred_labels, pred_scores, gts

    def _prefixed(self, report, prefix='bbox/'):
        return {prefix + k: v for k, v in report.items()}

    def _check_records(self, box_ious, boundary_counts=None):
        if 'bbox' in self.iou_types and (box_ious is None or any(b is None for b in box_ious)):
            raise ValueError("iou_types has 'bbox' but the records carry no box IoU tables")
        if 'boundary' in self.iou_types and boundary_counts is None:
            raise ValueError("iou_types has 'boundary' but the records carry no boundary counts")


class InstanceSegmentationVOCEvaluator(_InstanceSegmentationEvaluator):
    """``validation/main/map`` and, with ``label_names``, ``validation/main/ap/<name>``
    (class l's AP is ``ap[l]``; NaN for a class that never occurs).  With ``'bbox'`` in
    ``iou_types``: ``validation/main/bbox/map`` and ``bbox/ap/<name>``, chainercv's
    ``eval_detection_voc`` of the predicted boxes against the examples' boxes."""

    box_convention = 'voc'

    def __init__(self, iterator, target, use_07_metric=False, label_names=None,
                 iou_types=('segm',), boundary_dilation_ratio=0.02):
        super(InstanceSegmentationVOCEvaluator, self).__init__(
            iterator, target, label_names, iou_types, boundary_dilation_ratio)
        self.use_07_metric = use_07_metric

    def evaluate(self):
        return self.evaluate_collected(*self.collect())

    def evaluate_collected(self, counts, pred_labels, pred_scores, gts, box_ious=None,
                           boundary_counts=None):
        """The host half of ``evaluate``: matching and AP from ``collect()``'s records."""
        self._check_records(box_ious, boundary_counts)
        gt_labels = [g[1] for g in gts]
        gt_difficults = None
        if gts and len(gts[0]) == 4:
            gt_difficults = [g[3] for g in gts]
        report = {}
        if 'segm' in self.iou_types:
            prec, rec = matching.voc_prec_rec_from_counts(counts, pred_labels, pred_scores,
                                                          gt_labels, gt_difficults)
            ap = matching.calc_detection_voc_ap(prec, rec, use_07_metric=self.use_07_metric)
            report.update(voc_report(ap, self.label_names))
        if 'bbox' in self.iou_types:
            prec, rec = matching.voc_prec_rec_from_ious(box_ious, pred_labels, pred_scores,
                                                        gt_labels, gt_difficults)
            ap = matching.calc_detection_voc_ap(prec, rec, use_07_metric=self.use_07_metric)
            report.update(self._prefixed(voc_report(ap, self.label_names)))
        if 'boundary' in self.iou_types:
            prec, rec = matching.voc_prec_rec_from_boundary_counts(
                counts, boundary_counts, pred_labels, pred_scores, gt_labels, gt_difficults)
            ap = matching.calc_detection_voc_ap(prec, rec, use_07_metric=self.use_07_metric)
            report.update(self._prefixed(voc_report(ap, self.label_names), 'boundary/'))
        return self._observation(report)


class InstanceSegmentationCOCOEvaluator(_InstanceSegmentationEvaluator):
    """``validation/main/map`` (IoU .50:.95), ``map@0.5``, ``map@0.75`` and, with
    ``label_names``, ``ap/<name>`` keyed by the real label (the reference indexes the K axis,
    the sorted labels present, by label: DESIGN.md section 9).

    ``results_sink`` (optional, off by default): a callable ``sink(i, bboxes, labels, scores,
    segmentations)`` called for the i-th evaluated image with its detections and their masks as
    COCO compressed RLE (``utils.evaluations.coco_results.ResultsWriter`` writes a results
    file).  The packed masks that are intersected are the ones encoded, on the device; only the
    strings come back, in one more read-back per batch.  With ``iou_types=('bbox',)`` alone, which
    pastes no masks, the sink gets ``segmentations=None`` (bbox-only entries); with ``'boundary'``
    it still gets the masks, never the boundaries.

    With ``'bbox'`` in ``iou_types``: ``validation/main/bbox/map``, ``bbox/map@0.5``,
    ``bbox/map@0.75`` and ``bbox/ap/<name>``: pycocotools' iouType 'bbox' on the predicted boxes
    against the examples' boxes (the mask's tight box for this project's COCO dataset), crowds and
    areas as for the masks."""

    box_convention = 'coco'

    def __init__(self, iterator, target, label_names=None, results_sink=None,
                 iou_types=('segm',), boundary_dilation_ratio=0.02):
        super(InstanceSegmentationCOCOEvaluator, self).__init__(
            iterator, target, label_names, iou_types, boundary_dilation_ratio)
        self.results_sink = results_sink

    def evaluate(self):
        return self.evaluate_collected(*self.collect())

    def evaluate_collected(self, counts, pred_labels, pred_scores, gts, box_ious=None,
                           boundary_counts=None):
        """The host half of ``evaluate``: matching and AP from ``collect()``'s records."""
        self._check_records(box_ious, boundary_counts)
        gt_labels = [g[1] for g in gts]
        gt_crowdeds = gt_areas = None
        if gts and len(gts[0]) == 5:
            gt_crowdeds = [g[3] for g in gts]
            gt_areas = [g[4] for g in gts]
        report = {}
        if 'segm' in self.iou_types:
            result = matching.coco_results(matching.coco_evaluate_from_counts(
                counts, pred_labels, pred_scores, gt_labels, gt_crowdeds, gt_areas))
            report.update(coco_report(result, self.label_names))
        if 'bbox' in self.iou_types:
            result = matching.coco_results(matching.coco_evaluate_from_ious(
                box_ious, pred_labels, pred_scores, gt_labels, gt_crowdeds, gt_areas))
            report.update(self._prefixed(coco_report(result, self.label_names)))
        if 'boundary' in self.iou_types:
            result = matching.coco_results(matching.coco_evaluate_from_boundary_counts(
                counts, boundary_counts, pred_labels, pred_scores, gt_labels, gt_crowdeds,
                gt_areas))
            report.update(self._prefixed(coco_report(result, self.label_names), 'boundary/'))
        return self._observation(report)


def strip_records(counts, pred_labels, pred_scores, gts, box_ious=None, boundary_counts=None):
    """``collect()``'s records without what the host matching never reads: each ground-truth
    tuple keeps its length and its labels (and difficult / crowd / area) but loses the boxes and
    masks, which are by far the largest part.  The box IoU records and the boundary counts, when
    present, stay whole."""
    gts = [(None, g[1], None) + tuple(g[3:]) for g in gts]
    out = (list(counts), list(pred_labels), list(pred_scores), gts)
    if boundary_counts is not None:
        box_ious = [None] * len(gts) if box_ious is None else box_ious
        return out + (list(box_ious), list(boundary_counts))
    return out if box_ious is None else out + (list(box_ious),)


def merge_records(per_rank):
    """Concatenate the ranks' records (each ``(counts, pred_labels, pred_scores, gts[,
    box_ious[, boundary_counts]])``) in rank order, which is the test set's order when rank i holds the i-th
    contiguous shard."""
    per_rank = list(per_rank)
    widths = set(len(r) for r in per_rank)
    if len(widths) > 1:
        raise ValueError('records with and without box IoU tables or boundary counts cannot be '
                         'merged')
    merged = tuple([] for _ in range(widths.pop() if widths else 4))
    for records in per_rank:
        for out, part in zip(merged, records):
            out.extend(part)
    return merged


def gather_records(records, group=None):
    """Every rank's stripped records, merged in rank order, on every rank.  They travel on the
    control plane (pickled into uint8 CPU tensors over gloo, parallel.all_gather_bytes)."""
    from .. import parallel
    return merge_records(parallel.all_gather_object_cpu(strip_records(*records), group))


class _MultiNodeEvaluator(object):
    """See create_multi_node_evaluator."""

    def __init__(self, evaluator, group=None):
        self.evaluator, self.group = evaluator, group

    def __getattr__(self, name):
        return getattr(self.evaluator, name)

    def __call__(self, trainer=None):
        return self.evaluate()

    def evaluate(self):
        records = gather_records(self.evaluator.collect(), self.group)
        return self.evaluator.evaluate_collected(*records)


def create_multi_node_evaluator(evaluator, group=None):
    """chainermn.create_multi_node_evaluator's role for the instance-segmentation evaluators, with
    an exact result: each rank runs ``collect()`` (the device part) on its own test shard, the
    stripped records of all ranks are gathered in rank order and every rank runs the unchanged
    host matching over all of them.  Every rank gets the same observation, the one a single
    evaluator produces over the concatenated shards (chainermn averages the ranks' observations
    instead, which is not the test set's mAP).  Batching pads images, so a prediction depends on
    the images of its batch: the statement holds exactly when the test batches are the same,
    e.g. with batch size 1."""
    return _MultiNodeEvaluator(evaluator, group)


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
