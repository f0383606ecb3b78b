"""``EvalRecords``: what the evaluators' ``collect()`` returns, ``evaluate_collected()`` and
``scoring.score_voc`` / ``score_coco`` take and the ranks exchange.
``Readback``: the one copy that brings a batch's queued device results to the host."""
import math

import numpy as np
import torch

_NP = {torch.int32: np.int32, torch.int64: np.int64, torch.uint8: np.uint8,
       torch.float32: np.float32, torch.float64: np.float64}


class EvalRecords(object):
    """What the host matching reads, and no box, mask or image: per-image lists in the test
    set's order.

    * ``pred_labels``, ``pred_scores``, ``gt_labels``;
    * ``gt_difficults`` (VOC) or ``gt_crowdeds`` and ``gt_areas`` (COCO): each None as a whole
      when the examples carry none.  The evaluator that builds the record decides that;
    * ``tables``: IoU type -> per-image list.  ``'segm'`` and ``'boundary'``: ``(inter (P,G),
      pred_area (P,), gt_area (G,))`` host int64; ``'bbox'``: the float32 (P, G) IoU table (VOC) or
      ``(iou float64 (P,G), dt_area (P,), gt_box_area (G,))`` (COCO).  A key is there if and only
      if that table was produced."""

    LISTS = ('pred_labels', 'pred_scores', 'gt_labels')
    FLAGS = ('gt_difficults', 'gt_crowdeds', 'gt_areas')

    def __init__(self, pred_labels=(), pred_scores=(), gt_labels=(), gt_difficults=None,
                 gt_crowdeds=None, gt_areas=None, tables=None):
        self.pred_labels, self.pred_scores = list(pred_labels), list(pred_scores)
        self.gt_labels = list(gt_labels)
        self.gt_difficults, self.gt_crowdeds, self.gt_areas = (
            None if f is None else list(f) for f in (gt_difficults, gt_crowdeds, gt_areas))
        self.tables = {k: list(v) for k, v in (tables or {}).items()}
        lists = [getattr(self, k) for k in self.LISTS + self.FLAGS] + list(self.tables.values())
        if any(v is not None and len(v) != len(self) for v in lists):
            raise ValueError('per-image lists of different lengths')

    def __len__(self):
        return len(self.pred_labels)

    def require(self, iou_types):
        """Raise ValueError when a requested IoU type has no table ('boundary' also reads
        'segm': the matching takes the minimum of the two IoUs)."""
        what = {'segm': 'mask counts', 'bbox': 'box IoU tables', 'boundary': 'boundary counts'}
        for t in iou_types:
            for k in (('segm', 'boundary') if t == 'boundary' else (t,)):
                if k not in self.tables:
                    raise ValueError('iou_types has %r but the records carry no %s' % (t, what[k]))

    @classmethod
    def merge(cls, parts):
        """The parts concatenated in order: the test set's order when part i holds the i-th
        contiguous shard.  No parts give an empty record."""
        parts = list(parts)
        keys = set(frozenset(p.tables) for p in parts)
        if len(keys) > 1:
            raise ValueError('records with different tables cannot be merged: %s'
                             % sorted(sorted(k) for k in keys))
        out = cls(tables={k: [] for k in (keys.pop() if keys else ())})
        for name in cls.FLAGS:
            # a part without images never saw an example, so it cannot disagree
            present = set(getattr(p, name) is not None for p in parts if len(p))
            if len(present) > 1:
                raise ValueError('records with and without %s cannot be merged' % name)
            setattr(out, name, [] if True in present else None)
        for p in parts:
            for name in cls.LISTS + cls.FLAGS:
                if getattr(out, name) is not None and getattr(p, name) is not None:
                    getattr(out, name).extend(getattr(p, name))
            for k, v in p.tables.items():
                out.tables[k].extend(v)
        return out


class Readback(object):
    """Queue device (or host) tensors, then bring them all to the host in one copy, each as its
    own bytes in one uint8 buffer.  ``add`` / ``add_split`` return the slice of ``fetch()``'s list
    their arrays will stand at.  Integer tensors (int32, int64, uint8) arrive as int64 arrays,
    float32 / float64 tensors with their exact bits, all with their shapes (zero sizes too)."""

    def __init__(self):
        self._parts = []        # (tensor, shapes of the arrays cut from it)
        self._n = 0

    def _queue(self, tensor, shapes):
        if tensor.dtype not in _NP:
            raise TypeError('Readback carries %s, got %s' % (sorted(map(str, _NP)), tensor.dtype))
        self._parts.append((tensor, shapes))
        n0, self._n = self._n, self._n + len(shapes)
        return slice(n0, self._n)

    def add(self, *tensors):
        """Queue tensors, each to come back as one array of its own shape."""
        n0 = self._n
        for t in tensors:
            self._queue(t, [tuple(t.shape)])
        return slice(n0, self._n)

    def add_split(self, flat, shapes):
        """Queue one flat tensor that holds row-major arrays of ``shapes`` one after another
        (``boxes.queue_box_ious``' result), to come back as those arrays."""
        shapes = [tuple(int(v) for v in s) for s in shapes]
        if flat.dim() != 1 or flat.numel() != sum(math.prod(s) for s in shapes):
            raise ValueError('a flat tensor of %s elements for shapes %s'
                             % (tuple(flat.shape), shapes))
        return self._queue(flat, shapes)

    def fetch(self):
        """The one read-back: the list of host arrays, in the order they were queued."""
        if not self._parts:
            return []
        # the widest element types first: every part then starts at a multiple of its element
        # size, so the typed host views below are aligned without padding
        order = sorted(range(len(self._parts)), key=lambda i: -self._parts[i][0].element_size())
        flat = torch.cat([self._parts[i][0].contiguous().reshape(-1).view(torch.uint8)
                          for i in order])
        host = flat.cpu().numpy()
        out, o = [None] * len(self._parts), 0
        for i in order:
            tensor, shapes = self._parts[i]
            nbytes = tensor.numel() * tensor.element_size()
            a = host[o:o + nbytes].view(_NP[tensor.dtype])
            o += nbytes
            if a.dtype.kind in 'iu':
                a = a.astype(np.int64, copy=False)
            arrays, e = [], 0
            for s in shapes:
                arrays.append(a[e:e + math.prod(s)].reshape(s))
                e += math.prod(s)
            out[i] = arrays
        return [a for arrays in out for a in arrays]
