"""Fast R-CNN RoI max pooling on MI355X — the reference's ``--pooling-func pooling``
(examples/train_common.py:141-142: ``cmr.functions.roi_pooling_2d``, which the reference
references but never exports; chainer's ``F.roi_pooling_2d``).

Tensors are PyTorch-ROCm tensors with the reference's logical NCHW shapes (physically
channels-last); the arithmetic is the HIP kernel behind ``mrcnn_roi_pool_fwd / _bwd_ws``.
"""
import torch

from . import _roi_extractor as _re
from ._layout import empty_nhwc

# the backward needs the argmax (R, C, oh, ow) int32 of every output element
# mrcnn_roi_pool_fwd(x, rois, y, argmax, N .. bin_stride, spatial_scale, order, stream),
# mrcnn_roi_pool_bwd_ws(gy, argmax, rois, gx, N .. bin_stride, spatial_scale, ws, ws_bytes, stream)
_EXT = _re.Extractor('roi_pooling_2d', 'mrcnn_roi_pool_fwd', 'mrcnn_roi_pool_bwd_workspace_bytes',
                     'mrcnn_roi_pool_bwd_ws', 'roi_pool_bwd', fwd_ptrs=('x', 'rois', 'y', 'extra'),
                     bwd_ptrs=('gy', 'extra', 'rois', 'gx'),
                     extra=lambda rois, shape: empty_nhwc(shape, rois.device, torch.int32))
_ROIPooling2DFn = _EXT.function('_ROIPooling2DFn')


class ROIPooling2D(object):

    """RoI max pooling over a set of 2d planes (chainer's ``ROIPooling2D``)."""

    def __init__(self, outh, outw, spatial_scale, bin_stride=1, order=None):
        self.spatial_scale = _re.check_args(outh, outw, spatial_scale, bin_stride)
        self.outh, self.outw = outh, outw
        self.bin_stride = bin_stride
        self.order = order

    def __call__(self, x, rois):
        _re.check_inputs('ROIPooling2D', x, rois)
        return _ROIPooling2DFn.apply(x, rois, self.outh, self.outw, self.spatial_scale,
                                     self.bin_stride, self.order)


def roi_pooling_2d(x, rois, outh, outw, spatial_scale, axes='xy', bin_stride=1, order=None):
    """Spatial Region of Interest (ROI) max pooling (Fast R-CNN; chainer ``F.roi_pooling_2d``).

    x: (N, C, H, W) float32; rois: (R, 5) float32 rows ``(batch_index, x1, y1, x2, y2)``
    (``axes='xy'``) or ``(batch_index, y1, x1, y2, x2)`` (``axes='yx'``).  Returns (R, C, outh,
    outw) float32, channels-last.  No gradient w.r.t. ``rois``.

    Semantics of chainer's GPU kernel, all in fp32: ``start = roundf(x1 * s)`` (half away from
    zero; chainer's CPU path rounds half to even and differs on ties), RoI size
    ``max(end - start + 1, 1)``, bin ``[floor(p * bin), ceil((p + 1) * bin)) + start`` clamped to
    the map; the first maximum in row-major scan order from an initial ``-1e37``, 0 for an empty
    bin.  The backward sends each output gradient to its argmax pixel, summed in (RoI, bin row,
    bin column) order.

    ``bin_stride`` (extension): exactly ``roi_pooling_2d(...)[:, :, ::s, ::s]``.  ``order``
    (extension): an int32 device permutation of the RoI rows, the sequence in which they are
    processed; the result does not depend on it.
    """
    rois = _re.swap_axes(rois, axes)
    return ROIPooling2D(outh, outw, spatial_scale, bin_stride, order)(x, rois)
