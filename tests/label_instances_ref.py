"""Independent NumPy restatement of the reference's label2instance_boxes and
instance_boxes2label (chainer_mask_rcnn/utils/geometry.py), pinned to
tests/golden/label_instances.npz by tests/test_label_instances_cpu.py.

Vectorised rather than a per-instance loop: instance ranks from np.unique(return_inverse),
per-(instance, class) counts from np.bincount, the first row-major position of each pair
from np.minimum.at; the majority class is the largest count, ties to the smallest first
position (the reference's Counter insertion order)."""
import numpy as np


def label2instance_boxes(ins, cls, return_masks=False):
    ins = np.asarray(ins, np.int64)
    cls = np.asarray(cls, np.int64)
    H, W = ins.shape
    flat_i, flat_c = ins.ravel(), cls.ravel()
    sel = np.flatnonzero(flat_i != -1)
    ids, inv = np.unique(flat_i[sel], return_inverse=True)
    n = len(ids)
    if n == 0:
        out = (np.zeros(0, np.int32), np.zeros((0, 4), np.int32))
        return out + (np.zeros((0, H, W), bool),) if return_masks else out
    cvals, cinv = np.unique(flat_c[sel], return_inverse=True)
    nc = len(cvals)
    key = inv * nc + cinv
    count = np.bincount(key, minlength=n * nc).reshape(n, nc)
    first = np.full(n * nc, np.iinfo(np.int64).max)
    np.minimum.at(first, key, sel)
    first = first.reshape(n, nc)
    best = np.array([np.lexsort((first[i], -count[i]))[0] for i in range(n)])
    classes = cvals[best].astype(np.int32)
    ys, xs = sel // W, sel % W
    boxes = np.zeros((n, 4), np.int32)
    for k, (fn, col, off) in enumerate(((np.minimum, ys, 0), (np.minimum, xs, 0),
                                        (np.maximum, ys, 1), (np.maximum, xs, 1))):
        init = np.iinfo(np.int64).max if fn is np.minimum else -1
        acc = np.full(n, init)
        fn.at(acc, inv, col)
        boxes[:, k] = acc + off
    if not return_masks:
        return classes, boxes
    rank = -np.ones(H * W, np.int64)
    rank[sel] = inv
    masks = rank.reshape(1, H, W) == np.arange(n).reshape(n, 1, 1)
    return classes, boxes, masks


def instance_boxes2label(labels, bboxes, masks, scores=None):
    masks = np.asarray(masks, bool)
    labels = np.asarray(labels)
    N, H, W = masks.shape
    order = np.argsort(scores) if scores is not None else np.arange(N)
    lbl_ins = -np.ones((H, W), np.int32)
    lbl_cls = np.zeros((H, W), np.int32)
    if N:
        painted = masks[order]
        covered = painted.any(0)
        last = N - 1 - np.argmax(painted[::-1], axis=0)
        lbl_ins[covered] = last[covered]
        lbl_cls[covered] = labels[order][last[covered]]
    return lbl_ins, lbl_cls


def voc_preprocess(raw_ins, raw_cls):
    """The datasets' int32 conversion of the PNG / .mat label pair."""
    ins = np.asarray(raw_ins).astype(np.int32)
    cls = np.asarray(raw_cls).astype(np.int32)
    cls[cls == 255] = -1
    ins[ins == 255] = -1
    ins[np.isin(cls, [-1, 0])] = -1
    return ins, cls
