"""Box IoU tables on the device (include/mrcnn_hip.h, "Box IoU for evaluation").

``queue_box_ious`` makes the (P_i, G_i) IoU tables of a whole batch of images in one launch, in
one of two conventions:

* ``'voc'``: (y1, x1, y2, x2) float32 with chainercv's ``bbox[:, 2:] += 1`` — bit for bit
  ``utils.bbox.bbox_iou(a + [0, 0, 1, 1], b + [0, 0, 1, 1])``;
* ``'coco'``: (x, y, w, h) float64 with crowd flags — pycocotools' ``bbIou``.

Nothing here synchronises; ``records.Readback.add_split`` brings the flat result to the host as
the per-image tables.  There is no host fallback: a device is required.
"""
import numpy as np
import torch

from ... import _lib
from .masks import _device

CONVENTIONS = {'voc': (np.float32, torch.float32, 'mrcnn_box_iou_voc'),
               'coco': (np.float64, torch.float64, 'mrcnn_box_iou_coco')}


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def to_xywh64(bbox):
    """(N, 4) (y1, x1, y2, x2) float32 boxes -> float64 ``[x1, y1, x2 - x1, y2 - y1]``, the
    subtraction in float64: the numbers ``coco_results.results_entries`` writes as ``bbox``."""
    b = _host(bbox).astype(np.float32).reshape(-1, 4).astype(np.float64)
    return np.stack([b[:, 1], b[:, 0], b[:, 3] - b[:, 1], b[:, 2] - b[:, 0]], axis=1)


def _concat_upload(per_image, np_dtype, t_dtype, width, dev):
    """Per-image host arrays or device tensors -> one contiguous device tensor (sum, width) (or
    (sum,) for width 0) and the int32 prefix offsets."""
    off = np.zeros(len(per_image) + 1, np.int64)
    if any(isinstance(a, torch.Tensor) and a.is_cuda for a in per_image):
        parts = [(a if isinstance(a, torch.Tensor) else torch.from_numpy(
            np.ascontiguousarray(np.asarray(a, np_dtype)))).to(dev).to(t_dtype).reshape(
                (-1, width) if width else (-1,)) for a in per_image]
        flat = torch.cat(parts).contiguous() if parts else torch.empty(
            (0, width) if width else (0,), dtype=t_dtype, device=dev)
        off[1:] = np.cumsum([len(p) for p in parts])
    else:
        parts = [_host(a).astype(np_dtype).reshape((-1, width) if width else (-1,))
                 for a in per_image]
        host = np.concatenate(parts) if parts else np.zeros((0, width) if width else (0,),
                                                            np_dtype)
        off[1:] = np.cumsum([len(p) for p in parts])
        flat = torch.from_numpy(np.ascontiguousarray(host)).to(dev)
    if off[-1] >= 2 ** 31:
        raise ValueError('%d boxes in one call: the offsets are int32' % off[-1])
    return flat, off


def queue_box_ious(boxes_a, boxes_b, convention, crowd_b=None, device=None):
    """The IoU tables of a batch of images, queued on the current stream (not synchronised).

    ``boxes_a`` / ``boxes_b``: per-image lists of (P_i, 4) / (G_i, 4) boxes (host arrays or device
    tensors) in the convention's own format — ``'voc'``: (y1, x1, y2, x2) float32; ``'coco'``:
    (x, y, w, h) float64 (``to_xywh64``).  ``crowd_b``: per-image (G_i,) flags, ``'coco'`` only.
    Returns ``(iou, shapes)``: the flat device tensor (float32 / float64) holding the images'
    row-major tables one after another, and the list of their ``(P_i, G_i)``."""
    if convention not in CONVENTIONS:
        raise ValueError("convention must be 'voc' or 'coco', got %r" % (convention,))
    np_dtype, t_dtype, entry = CONVENTIONS[convention]
    boxes_a, boxes_b = list(boxes_a), list(boxes_b)
    if len(boxes_a) != len(boxes_b):
        raise ValueError('%d images of detections, %d of ground truth' % (len(boxes_a), len(boxes_b)))
    if crowd_b is not None and convention != 'coco':
        raise ValueError("crowd flags belong to the 'coco' convention")
    dev = torch.device(device) if device is not None else _device()
    a, a_off = _concat_upload(boxes_a, np_dtype, t_dtype, 4, dev)
    b, b_off = _concat_upload(boxes_b, np_dtype, t_dtype, 4, dev)
    _lib.require_device(a, b)
    n_img = len(boxes_a)
    shapes = [(int(a_off[i + 1] - a_off[i]), int(b_off[i + 1] - b_off[i])) for i in range(n_img)]
    out_off = np.zeros(n_img + 1, np.int64)
    out_off[1:] = np.cumsum([p * g for p, g in shapes])
    total = int(out_off[-1])
    iou = torch.empty((total,), dtype=t_dtype, device=dev)
    if total == 0:
        return iou, shapes
    off_d = torch.from_numpy(out_off).to(dev)
    a_off_d = torch.from_numpy(a_off.astype(np.int32)).to(dev)
    b_off_d = torch.from_numpy(b_off.astype(np.int32)).to(dev)
    args = [_lib.ptr(a), _lib.ptr(b)]
    crowd = None
    if convention == 'coco':
        if crowd_b is not None:
            crowd_b = [np.zeros(g, np.uint8) if c is None else c
                       for c, (_, g) in zip(list(crowd_b), shapes)]
            crowd, c_off = _concat_upload(
                [(_host(c) != 0).astype(np.uint8) for c in crowd_b], np.uint8, torch.uint8, 0, dev)
            if not np.array_equal(c_off, b_off):
                raise ValueError('crowd flags do not match the ground-truth boxes')
        args.append(_lib.ptr(crowd))
    _lib.call(entry, *(args + [_lib.ptr(a_off_d), _lib.ptr(b_off_d), _lib.ptr(off_d), n_img,
                               int(a_off[-1]), int(b_off[-1]), total, _lib.ptr(iou),
                               _lib.stream_ptr()]))
    # a, b, the offsets and the flags: the caching allocator keeps their blocks for the queued
    # kernel (same stream), as in masks.paste_packed
    return iou, shapes

