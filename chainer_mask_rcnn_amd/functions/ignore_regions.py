"""Ignore regions of the train step (include/mrcnn_hip.h
``mrcnn_mask_union_pack`` / ``mrcnn_box_coverage``, csrc/ignore_regions.hip): a region that training
must neither reward nor punish — a COCO ``iscrowd`` annotation — as one bit plane of the
network-size image, and how many of its pixels each anchor and each proposal covers.  The two
integers per box come back to the host, where ``ignored_from_counts`` is the rule."""
import numpy as np
import torch

from .. import _lib


def _plane(t, fn, arg):
    t = _lib.dense(t, torch.int64, fn, arg)
    if t.dim() != 2:
        raise ValueError('%s: %s must be an int64 (H, Wq) tensor, got %s' % (fn, arg, tuple(t.shape)))
    return t


def union_plane(masks_u8, base=None):
    """The union of ``masks_u8`` (G, H, W) uint8 — a byte other than 0 counts as set — as a bit
    plane: an int64 device tensor (H, ceil(W / 64)) in the packed-mask format, carried as
    ``upload_packed_masks`` carries its words (torch has no arithmetic on uint64).  With ``base``
    (such a plane of the same image) the result is ``base & ~union``: the plane with these masks
    cut out of it.  ``G`` may be 0: an empty plane, or a copy of ``base``.  Current stream.  The
    returned tensor carries W as the Python attribute ``_mrcnn_width`` (read by
    ``MaskRCNNTrainChain``; an attribute of this tensor object only, not of views or copies)."""
    _lib.require_device(masks_u8, base)
    masks_u8 = _lib.dense(masks_u8, torch.uint8, 'union_plane', 'masks_u8')
    if masks_u8.dim() != 3 or masks_u8.shape[1] <= 0 or masks_u8.shape[2] <= 0:
        raise ValueError('union_plane: masks_u8 must be a uint8 (G, H, W) tensor with H, W > 0, got %s'
                         % (tuple(masks_u8.shape),))
    G, H, W = (int(v) for v in masks_u8.shape)
    Wq = (W + 63) // 64
    dev = masks_u8.device
    if base is not None:
        base = _plane(base, 'union_plane', 'base')
        if tuple(base.shape) != (H, Wq) or base.device != dev:
            raise ValueError('union_plane: base must be a (%d, %d) plane on %s, got %s on %s'
                             % (H, Wq, dev, tuple(base.shape), base.device))
    plane = torch.empty((H, Wq), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.call('mrcnn_mask_union_pack', _lib.ptr(masks_u8) if G else None, G, H, W,
                  _lib.ptr(base), _lib.ptr(plane), _lib.stream_ptr())
    plane._mrcnn_width = W      # the pixel width, which the word count alone does not give
    return plane


def box_coverage(plane, width, boxes):
    """``(covered, area)`` per box as an int32 device tensor (n, 2): ``boxes`` (n, 4) float32
    ``(y1, x1, y2, x2)`` are rounded half to even and clipped to the plane's ``H`` rows and
    ``width`` columns; ``area`` is the pixel count of that rectangle, ``covered`` the number of set
    bits of ``plane`` inside it.  A box with a non-finite coordinate gives (0, 0).  ``plane``: int64
    (H, ceil(width / 64)) as ``union_plane`` returns it.  n == 0 launches nothing.  Current stream."""
    _lib.require_device(plane, boxes)
    plane = _plane(plane, 'box_coverage', 'plane')
    boxes = _lib.dense(boxes, torch.float32, 'box_coverage', 'boxes')
    width = int(width)
    H, Wq = (int(v) for v in plane.shape)
    if H <= 0 or width <= 0 or Wq != (width + 63) // 64:
        raise ValueError('box_coverage: plane must be (H, ceil(width / 64)) with H, width > 0; %d words '
                         'per row do not hold %d pixels' % (Wq, width))
    if boxes.dim() != 2 or boxes.shape[1] != 4:
        raise ValueError('box_coverage: boxes must be a float32 (n, 4) tensor, got %s' % (tuple(boxes.shape),))
    if boxes.device != plane.device:
        raise ValueError('box_coverage: plane and boxes must be on one device')
    n = int(boxes.shape[0])
    out = torch.empty((n, 2), dtype=torch.int32, device=plane.device)
    if n:
        with torch.cuda.device(plane.device):
            _lib.call('mrcnn_box_coverage', _lib.ptr(plane), H, width, _lib.ptr(boxes), n, _lib.ptr(out),
                      _lib.stream_ptr())
    return out


def ignored_from_counts(counts, thresh):
    """The rule, on the host: ``counts`` (n, 2) integers ``(covered, area)`` -> (n,) bool, true
    where the ignore region covers MORE than ``thresh`` of a box of nonzero area (strictly more, as
    Detectron's ``TRAIN.CROWD_FILTER_THRESH`` test)."""
    counts = np.asarray(counts)
    covered, area = counts[:, 0], counts[:, 1]
    return (area > 0) & (covered.astype(np.float64) > np.float64(thresh) * area)
