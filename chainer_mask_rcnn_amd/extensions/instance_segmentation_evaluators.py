"""InstanceSegmentationVOCEvaluator / InstanceSegmentationCOCOEvaluator — the reference's
chainer_mask_rcnn/extensions/instance_segmentation_{voc,coco}_evaluator.py.

``evaluate()`` returns the observation dict chainer's reporter builds for ``name='validation'``
(``validation/main/map``, ...).  Predicted masks never leave the device: per batch,
``predict_images(masks_to_host=False)`` -> packed paste -> intersections
against the uploaded and packed ground truth, all queued before one read-back of the counts
and areas.  Boxes, labels and scores come back as ``predict_images`` returns them (with the
model's test-time augmentation, if it has any configured).  ``collect()`` returns it all as one
``EvalRecords`` (utils/evaluations/records.py), which ``evaluate_collected()`` takes and the ranks
exchange; the host scores its tables (utils/evaluations/scoring.py, matching.py).

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

from ..utils.evaluations import boxes as B
from ..utils.evaluations import eval_detection as D
from ..utils.evaluations import masks as M
from ..utils.evaluations import rle
from ..utils.evaluations.records import EvalRecords, Readback
from ..utils.evaluations.scoring import coco_report, score_coco, score_voc, voc_report  # noqa: F401


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
    flag_names = ()           # the EvalRecords flag lists this evaluator's examples may carry

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

    def _queue_box_ious(self, readback, bboxes, batch, dev):
        """Queue the batch's box IoU tables: (their ``fetch()`` slice, per-image areas or None)."""
        gt_boxes = [ex[1] for ex in batch]
        if self.box_convention == 'voc':
            return readback.add_split(*B.queue_box_ious(bboxes, gt_boxes, 'voc', device=dev)), None
        pred, gt = [B.to_xywh64(b) for b in bboxes], [B.to_xywh64(b) for b in gt_boxes]
        crowd = [ex[4] for ex in batch] if len(batch[0]) == 6 else None
        slots = readback.add_split(*B.queue_box_ious(pred, gt, 'coco', crowd_b=crowd, device=dev))
        return slots, [(D.box_areas(p), D.box_areas(g)) for p, g in zip(pred, gt)]

    def collect(self):
        """Run the model over the iterator: the device half of ``evaluate``.  Returns the
        ``EvalRecords`` of the images seen, with the tables ``iou_types`` asks for ('boundary'
        brings 'segm' with it: the matching takes the minimum of the two IoUs)."""
        target = self.target
        sink = self.results_sink
        bbox, boundary = 'bbox' in self.iou_types, 'boundary' in self.iou_types
        segm = 'segm' in self.iou_types or boundary      # the masks are needed
        n_seen = 0
        records = EvalRecords(tables={k: [] for k, on in (
            ('segm', segm), ('bbox', bbox), ('boundary', boundary)) if on})
        flags = []
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
            readback, slots, encodes = Readback(), [], []
            for j, ex in enumerate(batch if segm else ()):
                gt_mask = ex[3]
                H, W = sizes[j]
                if tuple(gt_mask.shape[1:]) != (H, W):
                    raise ValueError('ground-truth masks of shape %s for an image of size %s'
                                     % (tuple(gt_mask.shape), (H, W)))
                pred = M.paste_packed(roi_masks[j], labels[j], bboxes[j], (H, W))
                gt = M.pack_masks(gt_mask, device=dev)
                slots.append(M.queue_counts(readback, pred, gt, (H, W), boundary,
                                            self.boundary_dilation_ratio))
                if sink is not None:          # the packed masks just intersected, encoded
                    encodes.append(rle.queue_encode(pred[0], pred[1], pred[2], (H, W)))
            if bbox:
                box_slots, areas = self._queue_box_ious(readback, bboxes, batch, dev)
            host = readback.fetch()           # one read-back for the whole batch
            if sink is not None:              # the batch's strings: one more small read-back
                all_segs = rle.fetch_encoded(encodes) if segm else [None] * len(batch)
                for j, segs in enumerate(all_segs):
                    sink(n_seen + j, bboxes[j], labels[j], scores[j], segs)
            n_seen += len(batch)
            for image in slots:
                for k, s in zip(('segm', 'boundary'), image):
                    records.tables[k].append(tuple(host[s]))
            if bbox:
                tables = host[box_slots]
                records.tables['bbox'].extend(tables if areas is None else
                                              [(t,) + a for t, a in zip(tables, areas)])
            records.pred_labels.extend(labels)
            records.pred_scores.extend(scores)
            records.gt_labels.extend(ex[2] for ex in batch)
            # this evaluator's flags, from the examples that carry exactly them
            flags.extend(ex[4:] for ex in batch if len(ex) == 4 + len(self.flag_names))
        if len(flags) not in (0, n_seen):
            raise ValueError('%d of %d examples carry %s' % (len(flags), n_seen, self.flag_names))
        for i, name in enumerate(self.flag_names if flags else ()):
            setattr(records, name, [f[i] for f in flags])
        return records

    def evaluate(self):
        return self.evaluate_collected(self.collect())

    def evaluate_collected(self, records):
        """The host half of ``evaluate``: matching and AP from ``collect()``'s records."""
        records.require(self.iou_types)
        return {'%s/main/%s' % (self.name, k): v for k, v in self._score(records).items()}


class InstanceSegmentationVOCEvaluator(_InstanceSegmentationEvaluator):
    """``validation/main/map`` and, with ``label_names``, ``validation/main/ap/<name>``
    (class l's AP is ``ap[l]``; NaN for a class that never occurs).  With ``'bbox'`` in
    ``iou_types``: ``validation/main/bbox/map`` and ``bbox/ap/<name>``, chainercv's
    ``eval_detection_voc`` of the predicted boxes against the examples' boxes."""

    box_convention = 'voc'
    flag_names = ('gt_difficults',)           # taken from 5-tuple examples

    def __init__(self, iterator, target, use_07_metric=False, label_names=None,
                 iou_types=('segm',), boundary_dilation_ratio=0.02):
        super(InstanceSegmentationVOCEvaluator, self).__init__(
            iterator, target, label_names, iou_types, boundary_dilation_ratio)
        self.use_07_metric = use_07_metric

    def _score(self, records):
        return score_voc(records, self.iou_types, self.use_07_metric, self.label_names)


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
    flag_names = ('gt_crowdeds', 'gt_areas')  # taken from 6-tuple examples

    def __init__(self, iterator, target, label_names=None, results_sink=None,
                 iou_types=('segm',), boundary_dilation_ratio=0.02):
        super(InstanceSegmentationCOCOEvaluator, self).__init__(
            iterator, target, label_names, iou_types, boundary_dilation_ratio)
        self.results_sink = results_sink

    def _score(self, records):
        return score_coco(records, self.iou_types, self.label_names)


def gather_records(records, group=None):
    """Every rank's records, merged in rank order, on every rank.  They travel on the control
    plane (pickled into uint8 CPU tensors over gloo, parallel.all_gather_bytes)."""
    from .. import parallel
    return EvalRecords.merge(parallel.all_gather_object_cpu(records, group))


class _MultiNodeEvaluator(object):
    """See create_multi_node_evaluator."""

    def __init__(self, evaluator, group=None):
        self.evaluator, self.group = evaluator, group

    def __getattr__(self, name):
        return getattr(self.evaluator, name)

    def __call__(self, trainer=None):
        return self.evaluate()

    def evaluate(self):
        return self.evaluator.evaluate_collected(
            gather_records(self.evaluator.collect(), self.group))


def create_multi_node_evaluator(evaluator, group=None):
    """chainermn.create_multi_node_evaluator's role for the instance-segmentation evaluators, with
    an exact result: each rank runs ``collect()`` (the device part) on its own test shard, the
    records of all ranks are gathered in rank order and every rank runs the unchanged
    host matching over all of them.  Every rank gets the same observation, the one a single
    evaluator produces over the concatenated shards (chainermn averages the ranks' observations
    instead, which is not the test set's mAP).  Batching pads images, so a prediction depends on
    the images of its batch: the statement holds exactly when the test batches are the same,
    e.g. with batch size 1."""
    return _MultiNodeEvaluator(evaluator, group)
