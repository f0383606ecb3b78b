"""COCO results files: writing predictions in COCO's results format and scoring such a file.

A results file is a JSON list of ``{"image_id", "category_id", "bbox", "score",
"segmentation": {"size": [H, W], "counts": str}}``: the format of COCO's evaluation server
(test-dev has no public annotations, so this file is the only way to its mask AP) and of
pycocotools' ``COCO.loadRes``.  The segmentations are COCO's compressed RLE, encoded on the device
from the packed masks (rle.py); ``eval_coco_results`` decodes them on the device and scores them
with the same host matching as the in-memory evaluator, so a file written from a model scores
exactly what ``InstanceSegmentationCOCOEvaluator.evaluate()`` reports for it.

The detection track's file has the same entries without ``segmentation``: ``results_entries`` /
``ResultsWriter`` write it when given ``segmentations=None``, and ``eval_coco_results(...,
iou_type='bbox')`` scores the ``bbox`` fields of either kind of file (device bbIou tables,
boxes.py; the same matching) to the evaluator's ``bbox/`` keys.
"""
import json
from collections import OrderedDict

import numpy as np

from . import boxes as B
from . import eval_detection as D
from . import masks as M
from . import rle as R
from .records import EvalRecords, Readback
from .scoring import SCORERS, score_coco


def results_entries(img_id, bboxes, labels, scores, segmentations, class_id_to_cat_id):
    """The results entries of one image: ``bboxes`` (D, 4) (y1, x1, y2, x2) in original-image
    pixels -> ``bbox`` [x1, y1, x2 - x1, y2 - y1]; ``labels`` (D,) class ids -> the dataset's
    ``category_id``; ``scores`` (D,) float32 -> Python floats (exact); ``segmentations`` the
    compressed RLE dicts, or None for bbox-only entries (the detection track's format).  Entries
    keep the detections' order."""
    bboxes = np.asarray(bboxes, np.float32).reshape(-1, 4)
    labels = np.asarray(labels).ravel()
    scores = np.asarray(scores, np.float32).ravel()
    if segmentations is None:
        if not (len(bboxes) == len(labels) == len(scores)):
            raise ValueError('%d boxes, %d labels and %d scores'
                             % (len(bboxes), len(labels), len(scores)))
        segmentations = [None] * len(bboxes)
    if not (len(bboxes) == len(labels) == len(scores) == len(segmentations)):
        raise ValueError('%d boxes, %d labels, %d scores and %d segmentations'
                         % (len(bboxes), len(labels), len(scores), len(segmentations)))
    out = []
    for (y1, x1, y2, x2), l, s, seg in zip(bboxes.astype(np.float64), labels, scores,
                                           segmentations):
        out.append({'image_id': int(img_id), 'category_id': int(class_id_to_cat_id[int(l)]),
                    'bbox': [float(x1), float(y1), float(x2 - x1), float(y2 - y1)],
                    'score': float(s)})
        if seg is not None:
            out[-1]['segmentation'] = {'size': [int(v) for v in seg['size']],
                                       'counts': seg['counts']}
    return out


class ResultsWriter(object):
    """Streams a results file: ``writer(i, bboxes, labels, scores, segmentations)`` appends the
    entries of the i-th image of ``img_ids`` (the evaluators' results sink), ``write(entries)``
    appends ready entries.  Only the current image's entries are held in memory."""

    def __init__(self, path, img_ids=None, class_id_to_cat_id=None):
        self.path, self.img_ids, self.class_id_to_cat_id = path, img_ids, class_id_to_cat_id
        self.n_entries, self.image_ids = 0, []
        self._f = open(path, 'w')
        self._f.write('[')

    def __call__(self, i, bboxes, labels, scores, segmentations):
        img_id = self.img_ids[i]
        self.image_ids.append(img_id)
        self.write(results_entries(img_id, bboxes, labels, scores, segmentations,
                                   self.class_id_to_cat_id))

    def write(self, entries):
        for e in entries:
            self._f.write((',\n' if self.n_entries else '\n') + json.dumps(e))
            self.n_entries += 1

    def close(self):
        if self._f is not None:
            self._f.write('\n]\n')
            self._f.close()
            self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _check_bbox(k, e):
    b = e['bbox']
    if (not isinstance(b, (list, tuple)) or len(b) != 4
            or not all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in b)):
        raise ValueError('results entry %d: bbox must be [x, y, w, h] numbers' % k)


def _load(results, dataset, iou_type='segm'):
    """load_results with each entry's position in the file: image_id -> [(k, entry), ...]."""
    if iou_type not in ('segm', 'bbox', 'boundary'):
        raise ValueError("iou_type must be 'segm', 'bbox' or 'boundary', got %r" % (iou_type,))
    needed = ('image_id', 'category_id', 'score') + (
        ('bbox',) if iou_type == 'bbox' else ('segmentation',))
    if isinstance(results, str):
        with open(results) as f:
            results = json.load(f)
    if not isinstance(results, list):
        raise ValueError('a results file is a JSON list of entries, got %s'
                         % type(results).__name__)
    grouped = OrderedDict()
    for k, e in enumerate(results):
        if not isinstance(e, dict):
            raise ValueError('results entry %d is not an object' % k)
        for key in needed:
            if key not in e:
                raise ValueError('results entry %d has no %r' % (k, key))
        img_id = e['image_id']
        if img_id not in dataset.img_sizes:
            raise ValueError('results entry %d: unknown image_id %r' % (k, img_id))
        if e['category_id'] not in dataset.cat_id_to_class_id:
            raise ValueError('results entry %d: unknown category_id %r' % (k, e['category_id']))
        if iou_type == 'bbox':                        # the segmentation, if any, is not read
            _check_bbox(k, e)
            grouped.setdefault(img_id, []).append((k, e))
            continue
        seg = e['segmentation']
        if isinstance(seg, list):
            raise ValueError('results entry %d: polygon segmentations are not supported; '
                             'segm results are RLE {"size", "counts"}' % k)
        if not isinstance(seg, dict) or 'counts' not in seg or 'size' not in seg:
            raise ValueError('results entry %d: segmentation must be {"size", "counts"}' % k)
        counts = seg['counts']
        if not isinstance(counts, (str, list)):
            raise ValueError('results entry %d: counts must be a string or a list' % k)
        try:
            size = tuple(int(v) for v in seg['size'])
        except (TypeError, ValueError):
            size = None
        if size != dataset.img_sizes[img_id]:
            raise ValueError('results entry %d: segmentation size %r, image %r is %r'
                             % (k, seg['size'], img_id, list(dataset.img_sizes[img_id])))
        grouped.setdefault(img_id, []).append((k, e))
    return grouped


def load_results(results, dataset, iou_type='segm'):
    """A results file (path) or list of entries -> OrderedDict image_id -> entries, in file
    order, validated against ``dataset`` (a COCOInstanceSegmentationDataset): every image id and
    category id must be the annotation file's, every segmentation a compressed string or a count
    list of the image's size.  ``bbox`` is optional (Detectron's segmentation results have
    none); polygons are refused, as pycocotools' ``loadRes`` refuses them for segm results.
    With ``iou_type='bbox'`` an entry needs ``bbox`` ([x, y, w, h] numbers) instead and need not
    have a ``segmentation``; ``'boundary'`` reads what ``'segm'`` reads."""
    return OrderedDict((i, [e for _, e in v])
                       for i, v in _load(results, dataset, iou_type).items())


def eval_coco_results(results, dataset, limit=None, label_names=None, iou_type='segm',
                      dilation_ratio=0.02):
    """Score a results file (path or list of entries) against ``dataset`` (a
    COCOInstanceSegmentationDataset; its images in order, the first ``limit`` when given; an
    image without entries has no detections).  Each image's segmentations are decoded in one
    device call and intersected with its packed ground truth; the counts feed
    ``matching.coco_evaluate_from_counts``.  Returns the keys of
    ``InstanceSegmentationCOCOEvaluator.evaluate()`` (``validation/main/map``, ...).

    ``iou_type='bbox'``: the entries' ``bbox`` fields are scored against the boxes of
    ``dataset.get_annotations(i)`` (the masks' tight boxes) instead, and the evaluator's
    ``validation/main/bbox/...`` keys come back; the entries need no ``segmentation``.

    ``iou_type='boundary'``: the decoded segmentations and the ground truth are scored by Boundary
    AP (boundaries cut on the device at ``dilation_ratio`` of the image diagonal, matching on
    min(mask IoU, boundary IoU)) and the evaluator's ``validation/main/boundary/...`` keys come
    back."""
    grouped = _load(results, dataset, iou_type)
    n = len(dataset) if not limit else min(int(limit), len(dataset))
    bbox, boundary = iou_type == 'bbox', iou_type == 'boundary'
    dev = None if bbox else M._device()
    records = EvalRecords(tables={k: [] for k in SCORERS[iou_type][2]})
    pred_boxes, gt_boxes, flags = [], [], []
    for i in range(n):
        img_id = dataset.img_ids[i]
        gt = dataset.get_annotations(i)
        entries = [e for _, e in grouped.get(img_id, [])]
        records.pred_labels.append(np.array([dataset.cat_id_to_class_id[e['category_id']]
                                             for e in entries], np.int32))
        records.pred_scores.append(np.array([e['score'] for e in entries], np.float32))
        records.gt_labels.append(gt[1])
        if len(gt) == 5:                              # as the evaluator: crowds and areas
            flags.append(gt[3:])
        if bbox:
            pred_boxes.append(np.array([e['bbox'] for e in entries], np.float64).reshape(-1, 4))
            gt_boxes.append(B.to_xywh64(gt[0]))
            continue
        size = dataset.img_sizes[img_id]
        job = R.queue_decode([e['segmentation'] for e in entries], size=size, device=dev)
        readback = Readback()
        status = readback.add(job.status)
        slots = M.queue_counts(readback, job.packed, M.pack_masks(gt[2], device=dev), size,
                               boundary, dilation_ratio)
        host = readback.fetch()
        R.check_decoded(host[status][0], ['results entry %d (image %r)' % (k, img_id)
                                          for k, _ in grouped.get(img_id, [])])
        for k, s in zip(('segm', 'boundary'), slots):
            records.tables[k].append(tuple(host[s]))
    if flags:
        records.gt_crowdeds, records.gt_areas = [f[0] for f in flags], [f[1] for f in flags]
    if bbox:                                          # one launch makes every image's table
        records.tables['bbox'] = D.coco_box_tables(pred_boxes, gt_boxes, records.gt_crowdeds)
    return {'validation/main/%s' % k: v
            for k, v in score_coco(records, (iou_type,), label_names).items()}
