"""Packed instance masks on the device (format: include/mrcnn_hip.h, "Packed masks").

``pack_masks`` / ``paste_packed`` produce (packed, area, extent) device tensors and
``queue_intersections`` the (P, G) int32 intersection counts of two packed sets; nothing here
synchronises.  ``mask_iou`` is the reference's ``mask_iou`` (utils/evaluations/
eval_instance_segmentation_voc.py) on top of them: the counts come from the device, the float64
IoU is formed on the host.  There is no host fallback: a device is required.
"""
import math

import numpy as np
import torch

from ... import _lib
from .records import Readback


def _device():
    return torch.device('cuda', torch.cuda.current_device())


def _as_device_masks(masks, dev):
    """(N, H, W) host array or device tensor -> contiguous device uint8 or int32 tensor whose
    nonzero elements are foreground."""
    if isinstance(masks, torch.Tensor):
        t = masks.to(dev) if masks.device != dev else masks
        if t.dtype == torch.bool:
            t = t.view(torch.uint8)
        elif t.dtype not in (torch.uint8, torch.int32):
            t = (t != 0).to(torch.uint8)
        return t.contiguous()
    a = np.asarray(masks)
    if a.dtype == np.bool_:
        a = a.view(np.uint8)
    elif a.dtype not in (np.uint8, np.int32):
        a = (a != 0).view(np.uint8)
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev, non_blocking=False)


def packed_words(W):
    return (int(W) + 63) // 64


def pack_masks(masks, device=None):
    """(N, H, W) uint8 / bool / int32 masks (host array or device tensor) -> (packed (N,H,Wq)
    int64 bit pattern, area (N,) int32, extent (N,4) int32) device tensors.

    Ground truth that never was a dense stack is taken as it is: a ``datasets.PolygonMasks`` is
    drawn on the device from its vertices (``functions.rasterize_polygons``), a host
    ``datasets.PackedMasks`` is uploaded as its words, with areas and extents counted on the host."""
    from ...datasets.packed_masks import PackedMasks, packed_metadata
    from ...datasets.polygon_masks import PolygonMasks
    if isinstance(masks, PolygonMasks):
        from ...functions.polygons import rasterize_polygons
        return rasterize_polygons(masks, device=device if device is not None else _device())[:3]
    if isinstance(masks, PackedMasks):
        dev = torch.device(device) if device is not None else _device()
        area, extent, _ = packed_metadata(masks.words, masks.width)
        return (torch.from_numpy(masks.words.view(np.int64)).to(dev), torch.from_numpy(area).to(dev),
                torch.from_numpy(extent).to(dev))
    dev = torch.device(device) if device is not None else (
        masks.device if isinstance(masks, torch.Tensor) and masks.is_cuda else _device())
    m = _as_device_masks(masks, dev)
    _lib.require_device(m)
    if m.dim() != 3:
        raise ValueError('pack_masks expects (N, H, W) masks, got shape %s' % (tuple(m.shape),))
    N, H, W = m.shape
    packed = torch.empty((N, H, packed_words(W)), dtype=torch.int64, device=dev)
    area = torch.empty((N,), dtype=torch.int32, device=dev)
    extent = torch.empty((N, 4), dtype=torch.int32, device=dev)
    if N == 0 or H == 0 or W == 0:
        area.zero_()
        extent.zero_()
    else:
        _lib.call('mrcnn_mask_pack', _lib.ptr(m), m.element_size(), N, H, W, _lib.ptr(packed),
                  _lib.ptr(area), _lib.ptr(extent), _lib.stream_ptr())
    return packed, area, extent


def paste_packed(roi_mask_logits, label, bbox, size):
    """``MaskRCNN._to_masks`` for one image in the packed format: roi_mask_logits is the
    (D, n_fg, M, M) device tensor of ``predict_prepared(masks_to_host=False)``, label (D,) and
    bbox (D, 4) the host detections, size (H, W).  Returns (packed, area, extent)."""
    from ...functions._layout import nhwc
    H, W = int(size[0]), int(size[1])
    D = len(bbox)
    dev = roi_mask_logits.device
    packed = torch.empty((D, H, packed_words(W)), dtype=torch.int64, device=dev)
    area = torch.empty((D,), dtype=torch.int32, device=dev)
    extent = torch.empty((D, 4), dtype=torch.int32, device=dev)
    if D == 0:
        return packed, area, extent
    _lib.require_device(roi_mask_logits)
    logits = nhwc(roi_mask_logits, torch.float32, 'paste_packed', 'roi_mask_logits')
    label_d = torch.tensor(np.asarray(label, np.int32), device=dev)
    bbox_d = torch.tensor(np.asarray(bbox, np.float32), device=dev)
    _lib.call('mrcnn_paste_masks_packed', _lib.ptr(logits), _lib.ptr(label_d), _lib.ptr(bbox_d),
              D, logits.shape[2], logits.shape[1], H, W, _lib.ptr(packed), _lib.ptr(area),
              _lib.ptr(extent), _lib.stream_ptr())
    # label_d / bbox_d: the caching allocator keeps their blocks for the queued kernel (same
    # stream), as in MaskRCNN._to_masks
    return packed, area, extent


def queue_intersections(a, b, W):
    """inter (P, G) int32 device tensor = |A_p & B_g| for packed sets a = (packed, area, extent)
    and b of an image of width W (queued, not synchronised)."""
    pa, _, ea = a
    pb, _, eb = b
    P, H = pa.shape[0], pa.shape[1]
    G = pb.shape[0]
    if pb.shape[1:] != pa.shape[1:] or pa.shape[2] != packed_words(W):
        raise ValueError('packed mask sets of different image sizes: %s vs %s'
                         % (tuple(pa.shape[1:]), tuple(pb.shape[1:])))
    inter = torch.zeros((P, G), dtype=torch.int32, device=pa.device)
    if P and G and H:
        _lib.require_device(pa, ea, pb, eb)
        pa, pb = (_lib.dense(t, torch.int64, 'queue_intersections', 'packed') for t in (pa, pb))
        ea, eb = (_lib.dense(t, torch.int32, 'queue_intersections', 'extent') for t in (ea, eb))
        _lib.call('mrcnn_mask_intersect', _lib.ptr(pa), _lib.ptr(ea), P, _lib.ptr(pb),
                  _lib.ptr(eb), G, H, int(W), _lib.ptr(inter), _lib.stream_ptr())
    return inter


def queue_counts(readback, a, b, size, boundary=False, dilation_ratio=0.02, dilation=None):
    """One image's step of every evaluation: for packed sets a (predictions) and b (ground truth)
    of an image of ``size`` (H, W), queue (inter (P,G), area_a (P,), area_b (G,)) onto
    ``readback`` and, with ``boundary``, the same triple of the two sets' boundaries.  Returns
    the triples' slices of ``readback.fetch()``: [masks] or [masks, boundaries]."""
    W = int(size[1])
    slots = [readback.add(queue_intersections(a, b, W), a[1], b[1])]
    if boundary:
        ba = boundary_packed(a, size, dilation_ratio, dilation)
        bb = boundary_packed(b, size, dilation_ratio, dilation)
        slots.append(readback.add(queue_intersections(ba, bb, W), ba[1], bb[1]))
    return slots


def _counts(mask_a, mask_b, boundary, dilation_ratio=0.02, dilation=None):
    if tuple(mask_a.shape[1:]) != tuple(mask_b.shape[1:]):
        raise ValueError('mask sets of different image sizes: %s vs %s'
                         % (tuple(mask_a.shape[1:]), tuple(mask_b.shape[1:])))
    a = pack_masks(mask_a)
    b = pack_masks(mask_b, device=a[0].device)
    readback = Readback()
    slots = queue_counts(readback, a, b, mask_a.shape[1:], boundary, dilation_ratio, dilation)
    host = readback.fetch()
    return [tuple(host[s]) for s in slots]


def mask_counts(mask_a, mask_b):
    """(inter (P,G), area_a (P,), area_b (G,)) as host int64 arrays for two mask sets of the
    same image size (host arrays or device tensors)."""
    return _counts(mask_a, mask_b, False)[0]


def iou_from_counts(inter, area_a, area_b):
    """float64 (P, G): inter / (a + b - inter), 0 where the union is 0 — the reference's
    ``1.0 * intersect / union`` of get_mask_overlap, value for value."""
    inter = np.asarray(inter, dtype=np.int64)
    union = np.asarray(area_a, np.int64)[:, None] + np.asarray(area_b, np.int64)[None, :] - inter
    iou = np.zeros(inter.shape, dtype=np.float64)
    nz = union != 0
    iou[nz] = inter[nz] / union[nz]
    return iou


def mask_iou(mask_a, mask_b):
    """utils.mask_iou: float64 (P, G) IoU of two (N, H, W) mask sets."""
    if tuple(mask_a.shape[1:]) != tuple(mask_b.shape[1:]):
        raise ValueError
    return iou_from_counts(*mask_counts(mask_a, mask_b))


# ---------------------------------------------------------------------------- Boundary IoU
# Cheng et al., "Boundary IoU: Improving Object-Centric Image Segmentation Evaluation" (CVPR
# 2021) as the boundary-iou-api computes it: the boundary of a mask is what an erosion by the
# (2d+1) x (2d+1) square removes, with the outside of the image as background (DESIGN.md
# section 22).  The erosion runs on the packed words (csrc/mask_boundary.hip).
def boundary_dilation(size, dilation_ratio=0.02):
    """The erosion distance d in pixels for an image of ``size`` (H, W): the image diagonal times
    ``dilation_ratio``, rounded (Python's ``round``), at least 1."""
    H, W = int(size[0]), int(size[1])
    return max(int(round(dilation_ratio * math.sqrt(H ** 2 + W ** 2))), 1)


def boundary_packed(packed_set, size, dilation_ratio=0.02, dilation=None):
    """The boundary set ``(packed, area, extent)`` of a packed set of an image of ``size`` (H, W)
    (queued, not synchronised).  ``dilation`` gives d directly instead of ``dilation_ratio``.
    The boundary set shares the input's extent tensor: a mask's outermost pixels are always
    boundary."""
    packed, _, extent = packed_set
    H, W = int(size[0]), int(size[1])
    N = packed.shape[0]
    if tuple(packed.shape[1:]) != (H, packed_words(W)):
        raise ValueError('packed masks of shape %s for an image of size %s'
                         % (tuple(packed.shape), (H, W)))
    d = boundary_dilation((H, W), dilation_ratio) if dilation is None else int(dilation)
    if d < 1:
        raise ValueError('dilation must be >= 1, got %d' % d)
    _lib.require_device(packed, extent)
    dev = packed.device
    out = torch.empty(tuple(packed.shape), dtype=torch.int64, device=dev)
    area = torch.empty((N,), dtype=torch.int32, device=dev)
    if N == 0 or H == 0 or W == 0:
        out.zero_()
        area.zero_()
        return out, area, extent
    packed = _lib.dense(packed, torch.int64, 'boundary_packed', 'packed')
    extent = _lib.dense(extent, torch.int32, 'boundary_packed', 'extent')
    nbytes = _lib.load().mrcnn_mask_boundary_workspace_bytes(N, H, W)
    ws = _lib.workspace(nbytes, dev, tag='mask_boundary')
    _lib.call('mrcnn_mask_boundary', _lib.ptr(packed), _lib.ptr(extent), N, H, W, d,
              _lib.ptr(out), _lib.ptr(area), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    return out, area, extent


def mask_to_boundary(masks, dilation_ratio=0.02, dilation=None):
    """boundary_iou.utils.boundary_utils.mask_to_boundary for a set: (N, H, W) masks -> (N, H, W)
    uint8 {0, 1} boundaries (a host array for a host array, a device tensor for a device
    tensor).  Pack, boundary and unpack all run on the device."""
    packed = pack_masks(masks)
    N, H, W = packed[0].shape[0], int(masks.shape[1]), int(masks.shape[2])
    out = torch.empty((N, H, W), dtype=torch.uint8, device=packed[0].device)
    if N and H and W:
        b = boundary_packed(packed, (H, W), dilation_ratio, dilation)
        _lib.call('mrcnn_mask_unpack', _lib.ptr(b[0]), N, H, W, _lib.ptr(out), _lib.stream_ptr())
    return out if isinstance(masks, torch.Tensor) else out.cpu().numpy()


def mask_and_boundary_counts(mask_a, mask_b, dilation_ratio=0.02, dilation=None):
    """``(mask_counts, boundary_counts)`` of two mask sets of the same image size from one
    read-back: each ``(inter (P,G), area_a (P,), area_b (G,))`` host int64."""
    return tuple(_counts(mask_a, mask_b, True, dilation_ratio, dilation))


def boundary_counts(mask_a, mask_b, dilation_ratio=0.02, dilation=None):
    """``mask_counts`` of the two sets' boundaries: (inter (P,G), area_a (P,), area_b (G,))."""
    return mask_and_boundary_counts(mask_a, mask_b, dilation_ratio, dilation)[1]


def boundary_iou(mask_a, mask_b, dilation_ratio=0.02, dilation=None):
    """float64 (P, G) Boundary IoU of two (N, H, W) mask sets: |B_a & B_b| / |B_a | B_b|, 0 where
    the boundaries do not meet.  The pure measure; Boundary AP matches on min(mask IoU, this)."""
    return iou_from_counts(*boundary_counts(mask_a, mask_b, dilation_ratio, dilation))
