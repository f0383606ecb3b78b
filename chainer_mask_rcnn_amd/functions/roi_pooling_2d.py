"""Fast R-CNN RoI max pooling on MI355X — the reference's ``--pooling-func pooling``
(examples/train_common.py:141-142: ``cmr.functions.roi_pooling_2d``, which the reference
references but never exports; chainer's ``F.roi_pooling_2d``).

Tensors are PyTorch-ROCm tensors with the reference's logical NCHW shapes (physically
channels-last); the arithmetic is the HIP kernel behind ``mrcnn_roi_pool_fwd / _bwd_ws``.
"""
import importlib

import torch

from .. import _lib
from ._layout import nhwc, empty_nhwc

# the module (the package's ``roi_align_2d`` attribute is the function): its VALIDATE_ORDER switch
_roi_align = importlib.import_module(__package__ + '.roi_align_2d')


def _check_order(order, R, device, name):
    """``order`` of the extractors: as ``roi_align_2d``'s (and checked as a permutation when
    ``roi_align_2d.VALIDATE_ORDER`` is set)."""
    if order is None:
        return
    if not (order.dtype == torch.int32 and order.is_contiguous() and order.device == device
            and tuple(order.shape) == (R,)):
        raise TypeError('{}: order must be a contiguous int32 device tensor of shape (R,) — a '
                        'permutation of the RoI rows'.format(name))
    if _roi_align.VALIDATE_ORDER and R > 0 and not torch.equal(
            torch.sort(order.long())[0], torch.arange(R, device=order.device)):
        raise ValueError('{}: order is not a permutation of 0..R-1'.format(name))


class _ROIPooling2DFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, rois, outh, outw, spatial_scale, bin_stride=1, order=None):
        _lib.require_device(x, rois)
        x = nhwc(x)
        rois = rois.contiguous()
        N, C, H, W = x.shape
        R = rois.shape[0]
        oh = (outh + bin_stride - 1) // bin_stride
        ow = (outw + bin_stride - 1) // bin_stride
        y = empty_nhwc((R, C, oh, ow), x.device)
        argmax = empty_nhwc((R, C, oh, ow), x.device, torch.int32)
        _check_order(order, R, x.device, 'roi_pooling_2d')
        _lib.call('mrcnn_roi_pool_fwd', _lib.ptr(x), _lib.ptr(rois), _lib.ptr(y), _lib.ptr(argmax),
                  N, H, W, C, R, outh, outw, bin_stride, spatial_scale,
                  _lib.ptr(order) if order is not None and R > 0 else None, _lib.stream_ptr())
        ctx.save_for_backward(rois, argmax)
        ctx.x_shape = (N, C, H, W)
        ctx.args = (outh, outw, spatial_scale, bin_stride)
        return y

    @staticmethod
    def backward(ctx, gy):
        rois, argmax = ctx.saved_tensors
        N, C, H, W = ctx.x_shape
        outh, outw, spatial_scale, bin_stride = ctx.args
        gy = nhwc(gy)
        gx = empty_nhwc((N, C, H, W), gy.device)
        R = rois.shape[0]
        nbytes = _lib.load().mrcnn_roi_pool_bwd_workspace_bytes(N, H, W, R, outh, outw, bin_stride)
        ws = _lib.workspace(nbytes, gy.device, 'roi_pool_bwd')
        _lib.call('mrcnn_roi_pool_bwd_ws', _lib.ptr(gy), _lib.ptr(argmax), _lib.ptr(rois),
                  _lib.ptr(gx), N, H, W, C, R, outh, outw, bin_stride, spatial_scale,
                  _lib.ptr(ws), int(ws.numel() * ws.element_size()), _lib.stream_ptr())
        # no gradient w.r.t. rois
        return gx, None, None, None, None, None, None


def _check_args(name, outh, outw, spatial_scale, bin_stride):
    for arg, value in (('outh', outh), ('outw', outw), ('bin_stride', bin_stride)):
        if not (isinstance(value, int) and not isinstance(value, bool) and value >= 1):
            raise TypeError('{} must be positive integer: {}, {}'.format(arg, type(value), value))
    if isinstance(spatial_scale, int) and not isinstance(spatial_scale, bool):
        spatial_scale = float(spatial_scale)
    elif not isinstance(spatial_scale, float):
        raise TypeError('spatial_scale must be float: {}'.format(type(spatial_scale)))
    return spatial_scale


def _check_inputs(name, x, rois):
    if not (x.dtype == torch.float32 and x.dim() == 4 and rois.dtype == torch.float32
            and rois.dim() == 2 and rois.shape[1] == 5):
        raise TypeError('{} expects x: float32 (N,C,H,W), rois: float32 (R,5); got {} {} and {} {}'
                        .format(name, x.dtype, tuple(x.shape), rois.dtype, tuple(rois.shape)))


class ROIPooling2D(object):

    """RoI max pooling over a set of 2d planes (chainer's ``ROIPooling2D``)."""

    def __init__(self, outh, outw, spatial_scale, bin_stride=1, order=None):
        self.spatial_scale = _check_args('ROIPooling2D', outh, outw, spatial_scale, bin_stride)
        self.outh, self.outw = outh, outw
        self.bin_stride = bin_stride
        self.order = order

    def __call__(self, x, rois):
        _check_inputs('ROIPooling2D', x, rois)
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
    if axes not in ['xy', 'yx']:
        raise ValueError('Unsupported axes: {}'.format(axes))
    if axes == 'yx':
        rois = rois[:, [0, 2, 1, 4, 3]]
    return ROIPooling2D(outh, outw, spatial_scale, bin_stride, order)(x, rois)
