"""Thin wrappers over the device half of the target creators (include/mrcnn_hip.h "Target
creators: the device half")."""
import ctypes

import torch

from .. import _lib


def bbox_iou_argmax(boxes_a, boxes_b, want_matrix=False):
    """chainercv ``bbox_iou(a, b)`` reduced per row of ``a``: (max_iou (na,) f32, argmax (na,)
    i32[, iou (na,g), col_max (g,)]).  No rows and ``want_matrix``: ValueError, as NumPy's max of
    an empty column (the library writes no col_max then)."""
    _lib.require_device(boxes_a, boxes_b)
    boxes_a = _lib.dense(boxes_a, torch.float32, 'bbox_iou_argmax', 'boxes_a')
    boxes_b = _lib.dense(boxes_b, torch.float32, 'bbox_iou_argmax', 'boxes_b')
    na, g = boxes_a.shape[0], boxes_b.shape[0]
    if want_matrix and na == 0:
        raise ValueError('bbox_iou_argmax: column maxima of an IoU matrix without rows')
    dev = boxes_a.device
    best = torch.empty((na,), dtype=torch.float32, device=dev)
    arg = torch.empty((na,), dtype=torch.int32, device=dev)
    iou = col = None
    if want_matrix:
        iou = torch.empty((na, g), dtype=torch.float32, device=dev)
        col = torch.empty((g,), dtype=torch.float32, device=dev)
    _lib.call('mrcnn_bbox_iou_argmax', _lib.ptr(boxes_a), na, _lib.ptr(boxes_b), g, _lib.ptr(iou),
              _lib.ptr(best), _lib.ptr(arg), _lib.ptr(col), _lib.stream_ptr())
    return (best, arg, iou, col) if want_matrix else (best, arg)


def anchor_labels(iou, max_iou, gt_max, neg_iou_thresh, pos_iou_thresh):
    _lib.require_device(iou, max_iou, gt_max)
    iou = _lib.dense(iou, torch.float32, 'anchor_labels', 'iou')
    max_iou = _lib.dense(max_iou, torch.float32, 'anchor_labels', 'max_iou')
    gt_max = _lib.dense(gt_max, torch.float32, 'anchor_labels', 'gt_max')
    na, g = iou.shape
    label = torch.empty((na,), dtype=torch.int32, device=iou.device)
    _lib.call('mrcnn_anchor_labels', _lib.ptr(iou), _lib.ptr(max_iou), _lib.ptr(gt_max), na, g,
              float(neg_iou_thresh), float(pos_iou_thresh), _lib.ptr(label), _lib.stream_ptr())
    return label


def anchor_targets_finish(anchor_inside, inside_index, label_inside, argmax, bbox, disabled, n_anchor):
    fn = 'anchor_targets_finish'
    _lib.require_device(anchor_inside, inside_index, label_inside, argmax, bbox, disabled)
    anchor_inside = _lib.dense(anchor_inside, torch.float32, fn, 'anchor_inside')
    inside_index = _lib.dense(inside_index, torch.int32, fn, 'inside_index')
    label_inside = _lib.dense(label_inside, torch.int32, fn, 'label_inside')
    argmax = _lib.dense(argmax, torch.int32, fn, 'argmax')
    bbox = _lib.dense(bbox, torch.float32, fn, 'bbox')
    if disabled is not None:
        disabled = _lib.dense(disabled, torch.int32, fn, 'disabled')
    dev = anchor_inside.device
    loc = torch.empty((n_anchor, 4), dtype=torch.float32, device=dev)
    label = torch.empty((n_anchor,), dtype=torch.int32, device=dev)
    n_dis = 0 if disabled is None else int(disabled.numel())
    _lib.call('mrcnn_anchor_targets_finish', _lib.ptr(anchor_inside), _lib.ptr(inside_index),
              _lib.ptr(label_inside), _lib.ptr(argmax), _lib.ptr(bbox), int(anchor_inside.shape[0]),
              _lib.ptr(disabled) if n_dis else None, n_dis, int(n_anchor), _lib.ptr(loc),
              _lib.ptr(label), _lib.stream_ptr())
    return loc, label


def proposal_targets_gather(cand, bbox, gt_label, assigned, chosen, n_fg, mean, std):
    fn = 'proposal_targets_gather'
    _lib.require_device(cand, bbox, gt_label, assigned, chosen)
    cand = _lib.dense(cand, torch.float32, fn, 'cand', align=True)    # rows read as one float4
    bbox = _lib.dense(bbox, torch.float32, fn, 'bbox')
    gt_label = _lib.dense(gt_label, torch.int32, fn, 'gt_label')
    assigned = _lib.dense(assigned, torch.int32, fn, 'assigned')
    chosen = _lib.dense(chosen, torch.int32, fn, 'chosen')
    dev = cand.device
    n = int(chosen.numel())
    sample_roi = torch.empty((n, 4), dtype=torch.float32, device=dev)
    loc = torch.empty((n, 4), dtype=torch.float32, device=dev)
    label = torch.empty((n,), dtype=torch.int32, device=dev)
    gt_index = torch.empty((n,), dtype=torch.int32, device=dev)
    m = (_lib.c_f32 * 4)(*[float(v) for v in mean])
    s = (_lib.c_f32 * 4)(*[float(v) for v in std])
    _lib.call('mrcnn_proposal_targets_gather', _lib.ptr(cand), _lib.ptr(bbox), _lib.ptr(gt_label),
              _lib.ptr(assigned), _lib.ptr(chosen), n, int(n_fg), m, s, _lib.ptr(sample_roi),
              _lib.ptr(loc), _lib.ptr(label), _lib.ptr(gt_index), _lib.stream_ptr())
    return sample_roi, loc, label, gt_index


def mask_targets(masks_u8, sample_roi, gt_index, n_fg, mask_size, n=None):
    """masks_u8 (G,H,W) uint8 device -> (n, M, M) int32 {-1,0,1}.  ``n`` defaults to the rows of
    ``sample_roi``; a caller that holds only the ``n_fg`` foreground rows (the library reads no
    others) passes the full row count."""
    _lib.require_device(masks_u8, sample_roi, gt_index)
    masks_u8 = _lib.dense(masks_u8, torch.uint8, 'mask_targets', 'masks_u8')
    sample_roi = _lib.dense(sample_roi, torch.float32, 'mask_targets', 'sample_roi')
    gt_index = _lib.dense(gt_index, torch.int32, 'mask_targets', 'gt_index')
    G, H, W = masks_u8.shape
    n = int(sample_roi.shape[0]) if n is None else int(n)
    assert int(n_fg) <= min(n, int(sample_roi.shape[0]), int(gt_index.shape[0]))
    out = torch.empty((n, mask_size, mask_size), dtype=torch.int32, device=sample_roi.device)
    _lib.call('mrcnn_mask_targets', _lib.ptr(masks_u8), G, H, W, _lib.ptr(sample_roi),
              _lib.ptr(gt_index), n, int(n_fg), int(mask_size), _lib.ptr(out), _lib.stream_ptr())
    return out
