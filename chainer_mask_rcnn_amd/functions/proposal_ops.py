"""Device-side box ops behind the proposal / detection path.

``non_maximum_suppression`` mirrors chainercv's function of the same name (the
reference imports it at /root/reference/chainer_mask_rcnn/models/mask_rcnn.py:39
and uses it at :193-194; ProposalCreator calls it internally).  The other
functions are thin wrappers over the C ABI used by ``ProposalCreator``.
"""
import torch

from .. import _lib


def decode_clip(anchor, loc, img_size, min_size=0., out=None):
    """loc2bbox + clip (+ min-size validity). anchor, loc: (n,4) -> roi (n,4), valid (n,) uint8
    (``out`` = preallocated contiguous (roi, valid) to write into)."""
    _lib.require_device(anchor, loc)
    n = anchor.shape[0]
    anchor = _lib.dense(anchor, torch.float32, 'decode_clip', 'anchor', align=True)
    loc = _lib.dense(loc, torch.float32, 'decode_clip', 'loc', align=True)
    if out is not None:
        roi, valid = out
    else:
        roi = torch.empty((n, 4), dtype=torch.float32, device=loc.device)
        valid = torch.empty((n,), dtype=torch.uint8, device=loc.device)
    _lib.call('mrcnn_decode_clip', _lib.ptr(anchor), _lib.ptr(loc), _lib.ptr(roi),
              _lib.ptr(valid), n, float(img_size[0]), float(img_size[1]),
              float(min_size), _lib.stream_ptr())
    return roi, valid


def topk_desc_batched(score, k, valid=None):
    """Stable descending top-k of every row of score (G, n) (valid (G, n) uint8 or None).
    Returns (order int32 (G, k), n_out int32 (G,))."""
    _lib.require_device(score, valid)
    score = _lib.dense(score, torch.float32, 'topk_desc_batched', 'score')
    G, n = score.shape
    k = int(min(k, n)) if k > 0 else n
    order = torch.empty((G, max(k, 1)), dtype=torch.int32, device=score.device)
    n_out = torch.empty((G,), dtype=torch.int32, device=score.device)
    per = (_lib.load().mrcnn_topk_workspace_bytes(n) + 63) // 64 * 64
    ws = _lib.workspace(per * G, score.device, 'topk')
    if valid is not None:
        valid = _lib.dense(valid, torch.uint8, 'topk_desc_batched', 'valid')
    _lib.call('mrcnn_topk_desc_batched', _lib.ptr(score), _lib.ptr(valid), G, n, k,
              _lib.ptr(order), _lib.ptr(n_out), _lib.ptr(ws), _lib.stream_ptr())
    return order, n_out


def topk_desc(score, k, valid=None):
    """Stable descending top-k. Returns (order int32 (k,), n_out int32 device scalar)."""
    _lib.require_device(score, valid)
    score = _lib.dense(score, torch.float32, 'topk_desc', 'score')
    if valid is not None:
        valid = _lib.dense(valid, torch.uint8, 'topk_desc', 'valid')
    n = score.numel()
    k = int(min(k, n)) if k > 0 else n
    order = torch.empty((max(k, 1),), dtype=torch.int32, device=score.device)
    n_out = torch.empty((1,), dtype=torch.int32, device=score.device)
    ws = _lib.workspace(_lib.load().mrcnn_topk_workspace_bytes(n), score.device, 'topk')
    _lib.call('mrcnn_topk_desc', _lib.ptr(score), _lib.ptr(valid), n, k,
              _lib.ptr(order), _lib.ptr(n_out), _lib.ptr(ws), _lib.stream_ptr())
    return order[:k], n_out


def gather_rows(src, idx, n_dev=None):
    """dst[j] = src[idx[j]] for j < n_dev (zero rows after)."""
    _lib.require_device(src, idx, n_dev)
    src = _lib.dense(src, torch.float32, 'gather_rows', 'src')
    idx = _lib.dense(idx, torch.int32, 'gather_rows', 'idx')
    if n_dev is not None:
        n_dev = _lib.dense(n_dev, torch.int32, 'gather_rows', 'n_dev')
    cols = src.shape[1]
    n_max = idx.numel()
    dst = torch.empty((n_max, cols), dtype=torch.float32, device=src.device)
    _lib.call('mrcnn_gather_rows', _lib.ptr(src), _lib.ptr(idx), _lib.ptr(n_dev),
              n_max, cols, _lib.ptr(dst), _lib.stream_ptr())
    return dst


def nms_sorted(bbox, thresh, n_dev=None, limit=0):
    """NMS over score-sorted boxes. Returns (keep int32 (n_max,), n_keep int32 device scalar)."""
    _lib.require_device(bbox, n_dev)
    bbox = _lib.dense(bbox, torch.float32, 'nms_sorted', 'bbox', align=True)
    if n_dev is not None:
        n_dev = _lib.dense(n_dev, torch.int32, 'nms_sorted', 'n_dev')
    n_max = bbox.shape[0]
    keep = torch.empty((max(n_max, 1),), dtype=torch.int32, device=bbox.device)
    n_keep = torch.empty((1,), dtype=torch.int32, device=bbox.device)
    ws = _lib.workspace(_lib.load().mrcnn_nms_workspace_bytes(n_max, 1), bbox.device, 'nms')
    _lib.call('mrcnn_nms_sorted', _lib.ptr(bbox), _lib.ptr(n_dev), n_max, float(thresh),
              int(limit or 0), _lib.ptr(keep), _lib.ptr(n_keep), _lib.ptr(ws),
              _lib.stream_ptr())
    return keep, n_keep


def nms_sorted_batched(bbox, n_dev, thresh, limit=0):
    """bbox (G, n_max, 4) sorted per group, n_dev (G,) int32. Returns keep (G,n_max), n_keep (G,)."""
    _lib.require_device(bbox, n_dev)
    bbox = _lib.dense(bbox, torch.float32, 'nms_sorted_batched', 'bbox', align=True)
    n_dev = _lib.dense(n_dev, torch.int32, 'nms_sorted_batched', 'n_dev')
    G, n_max = bbox.shape[0], bbox.shape[1]
    keep = torch.empty((G, max(n_max, 1)), dtype=torch.int32, device=bbox.device)
    n_keep = torch.empty((G,), dtype=torch.int32, device=bbox.device)
    ws = _lib.workspace(_lib.load().mrcnn_nms_workspace_bytes(n_max, G), bbox.device, 'nms')
    _lib.call('mrcnn_nms_sorted_batched', _lib.ptr(bbox), _lib.ptr(n_dev), G, n_max,
              float(thresh), int(limit or 0), _lib.ptr(keep), _lib.ptr(n_keep),
              _lib.ptr(ws), _lib.stream_ptr())
    return keep, n_keep


SOFT_NMS_METHODS = {'hard': 0, 'linear': 1, 'gaussian': 2}      # MRCNN_SOFT_NMS_*


def soft_nms_method(method):
    """'hard' / 'linear' / 'gaussian' (or the MRCNN_SOFT_NMS_* integer) -> the integer."""
    if method in SOFT_NMS_METHODS:
        return SOFT_NMS_METHODS[method]
    if isinstance(method, int) and not isinstance(method, bool) and method in SOFT_NMS_METHODS.values():
        return method
    raise ValueError("soft_nms: method must be one of %s, got %r"
                     % (sorted(SOFT_NMS_METHODS), method))


def _require_array(name, t, dtype, shape, align=False):
    """The C ABI reads raw pointers: a wrong dtype or shape would read out of bounds.  ``align``: the
    operand holds box rows, read as one float4 — a view that starts off a 16-byte boundary is copied."""
    if t.dtype != dtype or tuple(t.shape) != tuple(shape):
        raise ValueError('%s must be %s of shape %s, got %s %s'
                         % (name, dtype, tuple(shape), t.dtype, tuple(t.shape)))
    return _lib.dense(t, dtype, name, name, align=align)


def soft_nms_sorted_batched(bbox, prob, n_dev, method, overlap_thresh=0.3, sigma=0.5,
                            min_score=0.001, limit=0):
    """Soft-NMS (Detectron's cpu_soft_nms) over boxes sorted per group: bbox (G, n_max, 4), prob
    (G, n_max), n_dev (G,) int32.  Returns keep (G, n_max) = rows in emission order, n_keep (G,)
    and soft_prob (G, n_max) = the decayed score of every row."""
    _lib.require_device(bbox, prob, n_dev)
    method = soft_nms_method(method)
    if bbox.dim() != 3 or bbox.shape[2] != 4:
        raise ValueError('bbox must be (G, n_max, 4), got %s' % (tuple(bbox.shape),))
    G, n_max = bbox.shape[0], bbox.shape[1]
    bbox = _require_array('bbox', bbox, torch.float32, (G, n_max, 4), align=True)
    prob = _require_array('prob', prob, torch.float32, (G, n_max))
    n_dev = _require_array('n_dev', n_dev, torch.int32, (G,))
    keep = torch.empty((G, max(n_max, 1)), dtype=torch.int32, device=bbox.device)
    n_keep = torch.empty((G,), dtype=torch.int32, device=bbox.device)
    soft_prob = torch.empty((G, max(n_max, 1)), dtype=torch.float32, device=bbox.device)
    _lib.call('mrcnn_soft_nms_sorted_batched', _lib.ptr(bbox), _lib.ptr(prob), _lib.ptr(n_dev), G,
              n_max, method, float(overlap_thresh), float(sigma), float(min_score), int(limit or 0),
              _lib.ptr(keep), _lib.ptr(n_keep), _lib.ptr(soft_prob), _lib.stream_ptr())
    return keep, n_keep, soft_prob


def box_vote(bbox, prob, n_dev, keep, n_keep, vote_thresh=0.8):
    """Bounding-box voting (Detectron's box_voting, scoring method ID): every kept row becomes the
    mean, weighted by the undecayed ``prob``, of its group's boxes with IoU >= vote_thresh.
    Returns voted (G, n_max, 4), written at the kept rows only."""
    _lib.require_device(bbox, prob, n_dev, keep, n_keep)
    if bbox.dim() != 3 or bbox.shape[2] != 4:
        raise ValueError('bbox must be (G, n_max, 4), got %s' % (tuple(bbox.shape),))
    G, n_max = bbox.shape[0], bbox.shape[1]
    bbox = _require_array('bbox', bbox, torch.float32, (G, n_max, 4), align=True)
    prob = _require_array('prob', prob, torch.float32, (G, n_max))
    n_dev = _require_array('n_dev', n_dev, torch.int32, (G,))
    keep = _require_array('keep', keep, torch.int32, (G, max(n_max, 1)))
    n_keep = _require_array('n_keep', n_keep, torch.int32, (G,))
    voted = torch.empty((G, max(n_max, 1), 4), dtype=torch.float32, device=bbox.device)
    _lib.call('mrcnn_box_vote', _lib.ptr(bbox), _lib.ptr(prob), _lib.ptr(n_dev), _lib.ptr(keep),
              _lib.ptr(n_keep), G, n_max, float(vote_thresh), _lib.ptr(voted), _lib.stream_ptr())
    return voted


def non_maximum_suppression(bbox, thresh, score=None, limit=None):
    """Suppress bounding boxes according to their IoUs (chainercv semantics).

    bbox: (R, 4) float32 device tensor (y_min, x_min, y_max, x_max).  Returns an
    int32 device tensor of selected indices, sorted by descending score when
    ``score`` is given (ties: lower index first).
    """
    _lib.require_device(bbox)
    if bbox.shape[0] == 0:
        return torch.zeros((0,), dtype=torch.int32, device=bbox.device)
    order = None
    if score is not None:
        order, _ = topk_desc(score, bbox.shape[0])
        bbox = gather_rows(bbox, order)
    keep, n_keep = nms_sorted(bbox, thresh, None, limit or 0)
    keep = keep[:int(n_keep.item())]
    if order is not None:
        keep = order[keep.long()]
    return keep


def soft_nms(bbox, score, method='linear', overlap_thresh=0.3, sigma=0.5, min_score=0.001,
             limit=None):
    """Soft-NMS of one set of boxes (Detectron's ``soft_nms``; Bodla et al. 2017).

    bbox: (R, 4) float32 device tensor (y_min, x_min, y_max, x_max), score: (R,) finite and
    non-negative.  Returns (indices, new_scores): int32 indices into the caller's order, in
    emission order (non-increasing decayed score; ties: lower index first), and their decayed
    float32 scores.
    """
    _lib.require_device(bbox, score)
    method = soft_nms_method(method)
    if bbox.dim() != 2 or bbox.shape[1] != 4 or tuple(score.shape) != (bbox.shape[0],):
        raise ValueError('bbox must be (R, 4) and score (R,), got %s and %s'
                         % (tuple(bbox.shape), tuple(score.shape)))
    R = bbox.shape[0]
    if R == 0:
        return (torch.zeros((0,), dtype=torch.int32, device=bbox.device),
                torch.zeros((0,), dtype=torch.float32, device=bbox.device))
    # the kernels read float32: other floating types are converted, not reinterpreted
    bbox, score = bbox.to(torch.float32), score.to(torch.float32)
    order, _ = topk_desc(score, R)
    sorted_bbox = gather_rows(bbox, order)
    sorted_score = gather_rows(score.reshape(R, 1), order).reshape(R)
    n_dev = torch.full((1,), R, dtype=torch.int32, device=bbox.device)
    keep, n_keep, soft_prob = soft_nms_sorted_batched(
        sorted_bbox[None], sorted_score[None], n_dev, method, overlap_thresh, sigma, min_score,
        limit or 0)
    keep = keep[0, :int(n_keep.item())].long()
    return order[keep], soft_prob[0][keep]
