"""utils/geometry.py of the reference (chainer_mask_rcnn/utils/geometry.py): instance label
images <-> per-instance classes, boxes and masks, and the box / mask overlaps.

``label2instance_boxes`` and ``instance_boxes2label`` run on the device (csrc/instance_labels.hip,
contract in include/mrcnn_hip.h, "Instance label images"); there is no host fallback.  Host
NumPy input gives NumPy output with the reference's dtypes, device tensor input gives device
tensors.  A conversion synchronises twice: once to size the outputs, once to read the classes
(for the reference's assertion) together with the boxes.

uint8 label images follow the VOC PNG convention: 255 reads as -1 ("void"), so decoded palette
indices can be passed as they are.  int32 (and the other integer dtypes, widened to int32)
are taken at face value.
"""
import numpy as np
import torch

from .. import _lib
from .evaluations.masks import mask_counts

LABEL_WINDOW = 1 << 24   # MRCNN_LABEL_WINDOW: value span per image, and the table size limit
_WINDOW_WORDS = LABEL_WINDOW // 32


def _device():
    return torch.device('cuda', torch.cuda.current_device())


def _as_device_label(lbl, dev):
    """(H, W) label image -> contiguous device int32 or uint8 tensor."""
    if isinstance(lbl, torch.Tensor):
        t = lbl.to(dev) if lbl.device != dev else lbl
        if t.dtype == torch.bool:
            t = t.view(torch.uint8)
        elif t.dtype in (torch.int8, torch.int16):
            t = t.to(torch.int32)
        elif t.dtype not in (torch.uint8, torch.int32):
            raise TypeError('label images on the device must be int32 or uint8 (got %s)' % t.dtype)
        return t.contiguous()
    a = np.asarray(lbl)
    if a.dtype == np.bool_:
        a = a.view(np.uint8)
    elif a.dtype not in (np.uint8, np.int32):
        if a.dtype.kind not in 'iu':
            raise TypeError('label images must have an integer dtype (got %s)' % a.dtype)
        if a.size and (a.min() < np.iinfo(np.int32).min or a.max() > np.iinfo(np.int32).max):
            raise ValueError('label values must fit in int32')
        a = a.astype(np.int32)
    if not a.flags.writeable:          # e.g. np.asarray of a PIL image: torch wants writable memory
        a = a.copy()
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def label_instances(label_instance, label_class, return_masks=False, mask_by_class=False):
    """Device half of ``label2instance_boxes``: (ids (n,), classes (n,), boxes (n, 4),
    masks (n, H, W) bool or None) as device int32 tensors.  Classes are reported as computed,
    -1 / 0 included."""
    flat, n, masks = _convert(label_instance, label_class, return_masks, mask_by_class)
    return flat[:n], flat[n:2 * n], flat[2 * n:].view(n, 4), masks


def _convert(label_instance, label_class, return_masks, mask_by_class):
    """-> (flat (6n,) int32 device tensor = ids, classes, boxes; n; masks or None)."""
    if tuple(label_instance.shape) != tuple(label_class.shape) or len(label_instance.shape) != 2:
        raise ValueError('label_instance and label_class must be (H, W) images of one shape, got '
                         '%s and %s' % (tuple(label_instance.shape), tuple(label_class.shape)))
    dev = next((t.device for t in (label_instance, label_class)
                if isinstance(t, torch.Tensor) and t.is_cuda), None) or _device()
    ins = _as_device_label(label_instance, dev)
    cls = _as_device_label(label_class, dev)
    _lib.require_device(ins, cls)
    H, W = ins.shape
    empty = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
    no_masks = torch.zeros((0, H, W), dtype=torch.bool, device=dev) if return_masks else None
    if H == 0 or W == 0:
        return empty(0), 0, no_masks
    ws = _lib.workspace(4 * 4 * _WINDOW_WORDS, dev, tag='label_instances')
    # the prototypes name 32-bit words: typed views of the byte workspace
    bitmaps = ws[:8 * _WINDOW_WORDS].view(torch.int32)
    prefix = ws[8 * _WINDOW_WORDS:16 * _WINDOW_WORDS].view(torch.int32)
    meta = empty(6)
    args = (_lib.ptr(ins), ins.element_size(), _lib.ptr(cls), cls.element_size(), H, W,
            int(bool(mask_by_class)))
    _lib.call('mrcnn_label_scan', *args, _lib.ptr(meta), _lib.ptr(bitmaps), _lib.ptr(prefix),
              _lib.stream_ptr())
    ins_min, ins_max, cls_min, cls_max, n, ncls = (int(v) for v in meta.cpu())   # sync 1
    if n == 0:
        return empty(0), 0, no_masks
    span_ins, span_cls = ins_max - ins_min + 1, cls_max - cls_min + 1
    if span_ins > LABEL_WINDOW:
        raise ValueError('instance ids span %d values (%d..%d); the device conversion handles '
                         'a span of at most 2^24' % (span_ins, ins_min, ins_max))
    if span_cls > LABEL_WINDOW:
        raise ValueError('class values under instances span %d values (%d..%d); the device '
                         'conversion handles a span of at most 2^24' % (span_cls, cls_min, cls_max))
    if n * ncls > LABEL_WINDOW:
        raise ValueError('%d instances x %d distinct classes exceed the 2^24-entry instance x '
                         'class table of the device conversion' % (n, ncls))
    out = empty(6 * n)      # ids, classes, boxes: one buffer, read back in one copy
    table = empty(2 * n * ncls + ncls)
    masks = torch.empty((n, H, W), dtype=torch.uint8, device=dev) if return_masks else None
    _lib.call('mrcnn_label_instances', *args, _lib.ptr(meta), _lib.ptr(bitmaps), _lib.ptr(prefix),
              span_ins, span_cls, n, ncls, _lib.ptr(table), _lib.ptr(out[:n]),
              _lib.ptr(out[n:2 * n]), _lib.ptr(out[2 * n:]), _lib.ptr(masks), _lib.stream_ptr())
    # meta and table are released on return: the caching allocator hands their blocks only to
    # work queued after these kernels on this stream (as in utils/evaluations/masks.py)
    return out, n, masks.view(torch.bool) if masks is not None else None


def label2instance_boxes(label_instance, label_class, return_masks=False, mask_by_class=False):
    """Convert instance label to boxes (the reference's ``label2instance_boxes``).

    label_instance, label_class: (H, W) label images (host arrays or device tensors).
    Returns instance_classes (n,) int32, boxes (n, 4) int32 (y1, x1, y2, x2) and, with
    ``return_masks``, masks (n, H, W) bool, one per distinct instance value other than -1 in
    ascending order.  The class of an instance is its majority class; among classes of equal
    count the one whose first pixel (row-major) comes first wins.  With ``mask_by_class`` pixels
    of class -1 or 0 belong to no instance (the datasets' preprocessing).  Raises
    ``AssertionError`` when an instance's class is -1 or 0, as the reference does, and
    ``ValueError`` beyond the 2^24 limits of include/mrcnn_hip.h.
    """
    host = not (isinstance(label_instance, torch.Tensor) and label_instance.is_cuda)
    out, n, masks = _convert(label_instance, label_class, return_masks, mask_by_class)
    flat = out.cpu().numpy()                                                      # sync 2
    bad = np.isin(flat[n:2 * n], (-1, 0))
    assert not bad.any(), 'majority class -1 or 0 for instance id(s) %s' % (flat[:n][bad],)
    if host:
        classes, boxes = flat[n:2 * n].copy(), flat[2 * n:].reshape(n, 4).copy()
        if return_masks:
            masks = masks.cpu().numpy()
    else:
        classes, boxes = out[n:2 * n], out[2 * n:].view(n, 4)
    if return_masks:
        return classes, boxes, masks
    return classes, boxes


def instance_boxes2label(labels, bboxes, masks, scores=None):
    """Paint instance masks into (lbl_ins, lbl_cls) (H, W) int32 label images (the reference's
    ``instance_boxes2label``): -1 / 0 where no mask covers a pixel, else the last covering mask
    in painting order wins.  The painting order is ascending ``np.argsort(scores)`` when scores
    are given (computed on the host exactly as the reference does), else the given order;
    lbl_ins holds the position in that order.  masks: (N, H, W) bool; every label must be > 0.
    ``bboxes`` is accepted for the reference's signature and not used."""
    host = not (isinstance(masks, torch.Tensor) and masks.is_cuda)
    lab = labels.cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
    order = None
    if scores is not None:
        sc = scores.cpu().numpy() if isinstance(scores, torch.Tensor) else np.asarray(scores)
        order = np.argsort(sc)
    if masks.dtype not in (bool, np.bool_, torch.bool):
        raise AssertionError('masks must be bool, got %s' % (masks.dtype,))
    N, H, W = masks.shape
    assert N == 0 or (lab[:N] > 0).all()   # instance must be foreground
    dev = masks.device if not host else _device()
    m = masks if not host else torch.from_numpy(np.ascontiguousarray(masks))
    m = m.to(dev).contiguous().view(torch.uint8)
    lbl_ins = torch.empty((H, W), dtype=torch.int32, device=dev)
    lbl_cls = torch.empty((H, W), dtype=torch.int32, device=dev)
    if H and W:
        lab_d = torch.from_numpy(np.ascontiguousarray(lab[:N], np.int32)).to(dev)
        order_d = (torch.from_numpy(order.astype(np.int32)).to(dev) if order is not None else None)
        _lib.call('mrcnn_instances_to_label', _lib.ptr(m), _lib.ptr(order_d), _lib.ptr(lab_d), N,
                  H, W, _lib.ptr(lbl_ins), _lib.ptr(lbl_cls), _lib.stream_ptr())
    if host:
        return lbl_ins.cpu().numpy(), lbl_cls.cpu().numpy()
    return lbl_ins, lbl_cls


def mask_to_bbox(mask):
    """(y1, x1, y2, x2) half-open box of the nonzero pixels of an (H, W) mask; ``ValueError``
    for an empty mask, as the reference's ``argwhere(...).min(0)``."""
    if isinstance(mask, torch.Tensor) and mask.is_cuda:
        lbl = torch.where(mask != 0, 0, 255).to(torch.uint8)
    else:
        lbl = np.where(np.asarray(mask) != 0, 0, 255).astype(np.uint8)
    _, _, boxes, _ = label_instances(lbl, lbl)
    b = boxes.cpu().numpy()
    if len(b) == 0:
        raise ValueError('zero-size array to reduction operation minimum which has no identity')
    return tuple(int(v) for v in b[0])


def get_bbox_overlap(bbox1, bbox2):
    """IoU of two (y1, x1, y2, x2) boxes (the reference's formula, in its operation order)."""
    y11, x11, y12, x12 = bbox1
    y21, x21, y22, x22 = bbox2
    w1, h1 = x12 - x11, y12 - y11
    w2, h2 = x22 - x21, y22 - y21
    intersect = (max(0, min(x12, x22) - max(x11, x21)) *
                 max(0, min(y12, y22) - max(y11, y21)))
    union = w1 * h1 + w2 * h2 - intersect
    return 1.0 * intersect / union


def get_mask_overlap(mask1, mask2, half_if_nounion=False):
    """IoU of two (H, W) masks (nonzero = foreground) from the device counts of
    ``evaluations.masks.mask_counts``; 0.5 (``half_if_nounion``) or 0 when both are empty."""
    inter, a1, a2 = mask_counts(mask1[None], mask2[None])
    intersect = int(inter[0, 0])
    union = int(a1[0]) + int(a2[0]) - intersect
    if union == 0:
        return 0.5 if half_if_nounion else 0.
    return 1.0 * intersect / union
