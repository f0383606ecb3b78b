"""Test-time augmentation on the device (csrc/test_aug.hip): the views' candidates decoded into one
union in the image frame, and the views' mask maps combined into one (include/mrcnn_hip.h)."""
import ctypes

import torch

from .. import _lib
from ._layout import empty_nhwc, nhwc


def mask_aug_heur(heur):
    """'soft_avg' / 'soft_max' / 'logit_avg' -> the MRCNN_MASK_AUG_* integer."""
    if heur not in _lib.MASK_AUG_HEURS:
        raise ValueError('mask_aug_heur must be one of %s, got %r'
                         % (sorted(_lib.MASK_AUG_HEURS), heur))
    return _lib.MASK_AUG_HEURS[heur]


def decode_cls_boxes_views(views, n_class, mean, std, size):
    """One image's union of candidates.  ``views``: at most 8 tuples (roi (R_v,4), cls_loc
    (R_v, 4*n_class) device float32, scale, flip_x); ``mean`` / ``std``: the 4 loc-normalisation
    values; ``size``: the image's original (H, W).  Returns cls_bbox (sum R_v, n_class, 4) in the
    image frame, view after view: each row as mrcnn_decode_cls_boxes gives it, un-mirrored about W
    for a mirrored view."""
    if len(views) > _lib.TEST_AUG_MAX_VIEWS:
        raise ValueError('at most %d views, got %d' % (_lib.TEST_AUG_MAX_VIEWS, len(views)))
    recs = (_lib.TestAugView * max(len(views), 1))()
    keep, total, dev = [], 0, None
    for v, (roi, loc, scale, flip) in enumerate(views):
        _lib.require_device(roi, loc)
        R = roi.shape[0]
        if roi.dtype != torch.float32 or tuple(roi.shape) != (R, 4):
            raise ValueError('view %d: roi must be float32 (R, 4), got %s %s'
                             % (v, roi.dtype, tuple(roi.shape)))
        if loc.dtype != torch.float32 or tuple(loc.shape) != (R, 4 * n_class):
            raise ValueError('view %d: cls_loc must be float32 (%d, %d), got %s %s'
                             % (v, R, 4 * n_class, loc.dtype, tuple(loc.shape)))
        roi = _lib.dense(roi, torch.float32, 'decode_cls_boxes_views', 'roi', align=True)
        if R and (loc.stride(1) != 1 or loc.stride(0) < loc.shape[1]):
            loc = loc.contiguous()
        keep.append((roi, loc))
        recs[v] = _lib.TestAugView(_lib.addr(roi, 'roi') if R else None, _lib.addr(loc, 'cls_loc') if R else None,
                                   loc.stride(0) if R else 4 * n_class, R, float(scale),
                                   int(bool(flip)))
        total += R
        dev = roi.device
    if dev is None:
        raise ValueError('decode_cls_boxes_views needs at least one view')
    cls_bbox = torch.empty((total, n_class, 4), dtype=torch.float32, device=dev)
    mean4 = (ctypes.c_double * 4)(*[float(m) for m in mean])
    std4 = (ctypes.c_double * 4)(*[float(s) for s in std])
    _lib.call('mrcnn_decode_cls_boxes_views', recs, len(views), n_class, mean4, std4,
              float(size[0]), float(size[1]), _lib.ptr(cls_bbox), _lib.stream_ptr())
    return cls_bbox


def mask_aug_combine(maps, flips, heur='soft_avg'):
    """The views' mask-head outputs for the same boxes, (D, Kc, M, M) logits each as the head
    returns them, combined into one map of that shape by Detectron's MASK_AUG.HEUR rule ``heur``;
    view v is read mirrored left-right where ``flips[v]``."""
    heur = mask_aug_heur(heur)
    V = len(maps)
    if not 1 <= V <= _lib.TEST_AUG_MAX_VIEWS or len(flips) != V:
        raise ValueError('1 to %d maps with one flip flag each, got %d and %d'
                         % (_lib.TEST_AUG_MAX_VIEWS, V, len(flips)))
    _lib.require_device(*maps)
    shape = tuple(maps[0].shape)
    for m in maps:
        if m.dtype != torch.float32 or m.dim() != 4 or tuple(m.shape) != shape \
                or m.shape[2] != m.shape[3]:
            raise ValueError('maps must be float32 (D, Kc, M, M) of one shape, got %s %s'
                             % (m.dtype, tuple(m.shape)))
    D, Kc, M, _ = shape
    out = empty_nhwc(shape, maps[0].device)
    if D == 0:
        return out
    maps = [nhwc(m, torch.float32, 'mask_aug_combine', 'maps') for m in maps]
    ptrs = (_lib.c_vp * V)(*[_lib.addr(m, 'maps') for m in maps])
    flags = (ctypes.c_int32 * V)(*[int(bool(f)) for f in flips])
    _lib.call('mrcnn_mask_aug_combine', ptrs, flags, V, D, M, Kc, heur, _lib.ptr(out),
              _lib.stream_ptr())
    return out
