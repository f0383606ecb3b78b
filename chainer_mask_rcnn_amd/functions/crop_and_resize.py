"""Crop-and-resize RoI features on MI355X — drop-in for the reference's
``chainer_mask_rcnn.functions.crop_and_resize`` (functions/crop_and_resize.py:7-41), the
``--pooling-func resize`` of examples/train_common.py:143-144.

Tensors are PyTorch-ROCm tensors with the reference's logical NCHW shapes (physically
channels-last); the arithmetic is the HIP kernel behind ``mrcnn_crop_resize_fwd / _bwd_ws``.
"""
import torch

from . import _roi_extractor as _re


def _output_rows(rois):
    """Output row of every RoI: its position in the stable sort by batch index (the reference
    collects the outputs per image and concatenates them in image order)."""
    R = rois.shape[0]
    perm = torch.sort(rois[:, 0].to(torch.int64), stable=True).indices
    rows = torch.empty(R, dtype=torch.int32, device=rois.device)
    rows[perm] = torch.arange(R, dtype=torch.int32, device=rois.device)
    return rows


# mrcnn_crop_resize_fwd(x, rois, out_rows, y, N .. bin_stride, spatial_scale, order, stream),
# mrcnn_crop_resize_bwd_ws(gy, rois, out_rows, gx, N .. bin_stride, spatial_scale, ws, ws_bytes, stream)
_EXT = _re.Extractor('crop_and_resize', 'mrcnn_crop_resize_fwd', 'mrcnn_crop_resize_bwd_workspace_bytes',
                     'mrcnn_crop_resize_bwd_ws', 'crop_resize_bwd', fwd_ptrs=('x', 'rois', 'extra', 'y'),
                     bwd_ptrs=('gy', 'rois', 'extra', 'gx'),
                     extra=lambda rois, shape: _output_rows(rois) if shape[0] > 0 else None)
_CropAndResizeFn = _EXT.function('_CropAndResizeFn')


class CropAndResize(object):

    """Crop-and-resize RoI feature transformation (reference: crop_and_resize.py:7-41)."""

    def __init__(self, outh, outw, spatial_scale, bin_stride=1, order=None):
        self.spatial_scale = _re.check_args(outh, outw, spatial_scale, bin_stride)
        self.outh, self.outw = outh, outw
        self.bin_stride = bin_stride
        self.order = order

    def __call__(self, x, rois):
        _re.check_inputs('CropAndResize', x, rois)
        return _CropAndResizeFn.apply(x, rois, self.outh, self.outw, self.spatial_scale,
                                      self.bin_stride, self.order)


def crop_and_resize(x, rois, outh, outw, spatial_scale, axes='xy', bin_stride=1, order=None):
    """ROI feature transformation by crop-and-resize.

    x: (N, C, H, W) float32; rois: (R, 5) float32 rows ``(batch_index, x1, y1, x2, y2)``
    (``axes='xy'``) or ``(batch_index, y1, x1, y2, x2)`` (``axes='yx'``).  Returns (R, C, outh,
    outw) float32, channels-last.  No gradient w.r.t. ``rois``.

    The crop is ``x[b, :, y1':y2', x1':x2']`` with ``x1' = round(x1 * s)`` (float64, half to even
    as Python's ``round``), ``x2' = max(round(x2 * s), x1' + 1)`` and a slice's truncation at the
    map edge; the resize is ``F.resize_images`` (bilinear, aligned corners: sample positions
    ``linspace(0, crop - 1, out)`` in float64, taps ``clip(floor(v), 0, crop - 2)`` and ``+ 1``,
    weights rounded once to fp32, the four-tap sum in fp32).  The backward is the adjoint of the
    taps.

    Output rows follow the reference's order: the RoIs stably sorted by batch index (it
    concatenates the outputs per image), which is the input order whenever the RoIs are grouped
    by image.

    Extensions where the reference is ill-defined: the crop start is clamped into
    ``[0, H - 1]`` / ``[0, W - 1]`` (the reference wraps a negative start and fails on a start
    past the map), and an image without RoIs is allowed (the reference's ``vstack([])`` raises).
    ``bin_stride``: exactly ``crop_and_resize(...)[:, :, ::s, ::s]``.  ``order``: an int32 device
    permutation of the RoI rows, the sequence in which they are processed; the result does not
    depend on it.
    """
    rois = _re.swap_axes(rois, axes)
    return CropAndResize(outh, outw, spatial_scale, bin_stride, order)(x, rois)
