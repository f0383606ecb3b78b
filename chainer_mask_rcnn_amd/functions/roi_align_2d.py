"""ROIAlign on MI355X — drop-in for the reference's
``chainer_mask_rcnn.functions.roi_align_2d`` / ``ROIAlign2D``
(/root/reference/chainer_mask_rcnn/functions/roi_align_2d.py:25-60, :527-560).

Same names, argument meaning and error behaviour; tensors are PyTorch-ROCm
tensors with the reference's logical NCHW shapes (physically channels-last),
arithmetic is the hand-written HIP kernel behind ``mrcnn_roi_align_fwd/bwd``.
"""
import collections

from . import _roi_extractor as _re


# Pixel-owner backward (no atomics, fixed summation order); False = atomic gather form.
DETERMINISTIC_BACKWARD = True

# mrcnn_roi_align_fwd_ex(x, rois, y, N .. bin_stride, spatial_scale, sampling_ratio, order, stream),
# mrcnn_roi_align_bwd_ws(gy, rois, gx, N .. bin_stride, spatial_scale, sampling_ratio, ws, ws_bytes, stream)
_EXT = _re.Extractor('roi_align_2d', 'mrcnn_roi_align_fwd_ex', 'mrcnn_roi_align_bwd_workspace_bytes',
                     'mrcnn_roi_align_bwd_ws', 'roi_align_bwd', scalars=('sampling_ratio',),
                     wants_ws=lambda: DETERMINISTIC_BACKWARD)
# apply(x, rois, outh, outw, spatial_scale, sampling_ratio, bin_stride=1, order=None); only rois
# are retained (roi_align_2d.py:62-63 retain_inputs((1,))), no gradient w.r.t. them (:389, :524)
_ROIAlign2DFn = _EXT.function('_ROIAlign2DFn')


def roi_align_backward(gy, rois, map_shape, outh, outw, bin_stride, spatial_scale, sampling_ratio,
                       deterministic=True):
    """ROIAlign's adjoint: gy (R, C, oh, ow) -> the (N, C, H, W) = ``map_shape`` gradient of the
    map, for contiguous ``(batch, x1, y1, x2, y2)`` rois; pixel-owner form (no atomics) unless
    ``deterministic`` is False."""
    return _EXT.backward(gy, rois, None, map_shape, outh, outw, spatial_scale, (sampling_ratio,),
                         bin_stride, use_ws=deterministic)


class ROIAlign2D(object):

    """ROI align over a set of 2d planes (reference: roi_align_2d.py:25-47)."""

    def __init__(self, outh, outw, spatial_scale, sampling_ratio=0, bin_stride=1, order=None):
        self.bin_stride = int(bin_stride)
        self.order = order
        for arg, value in (('outh', outh), ('outw', outw),
                           ('sampling_ratio', sampling_ratio)):
            if not (isinstance(value, int) and not isinstance(value, bool)
                    and value >= 0):
                raise TypeError(
                    '{} must be positive integer: {}, {}'
                    .format(arg, type(value), value))
        if isinstance(spatial_scale, int):
            spatial_scale = float(spatial_scale)
        elif not isinstance(spatial_scale, float):
            raise TypeError(
                'spatial_scale must be float: {}'.format(type(spatial_scale)))
        self.outh, self.outw = outh, outw
        self.spatial_scale = spatial_scale
        self.sampling_ratio = sampling_ratio

    def check_type_forward(self, x, rois):
        # roi_align_2d.py:49-59
        _re.check_inputs('ROIAlign2D', x, rois)

    def __call__(self, x, rois):
        self.check_type_forward(x, rois)
        return _ROIAlign2DFn.apply(x, rois, self.outh, self.outw,
                                   self.spatial_scale, self.sampling_ratio, self.bin_stride,
                                   self.order)


# ``ResNetRoIHead.forward(hints=)``, device tensors: (R, 5) float32 rows (batch, x1, y1, x2, y2), (R,) int32
# processing order (``spatial_order``), (R,) int32 row -> position among ``mask_rows`` (-1 elsewhere)
RoiHints = collections.namedtuple('RoiHints', 'rois5 order mask_slot', defaults=(None, None, None))


def spatial_order(rois_yx, roi_indices, spatial_scale, band=6.0):
    """Processing order for ``roi_align_2d(..., order=)`` from HOST arrays: RoIs sorted by
    (image, band of ``band`` feature rows of the box centre, x centre).  ``rois_yx`` (R, 4) rows
    ``(y_min, x_min, y_max, x_max)``, ``roi_indices`` (R,).  Returns int32 (R,) NumPy."""
    import numpy as np
    rois_yx = np.asarray(rois_yx, np.float32).reshape(-1, 4)
    yc = (rois_yx[:, 0] + rois_yx[:, 2]) * (0.5 * spatial_scale)
    xc = (rois_yx[:, 1] + rois_yx[:, 3]) * (0.5 * spatial_scale)
    return np.lexsort((xc, np.floor(yc / band), np.asarray(roi_indices))).astype(np.int32)


def roi_align_2d(x, rois, outh, outw, spatial_scale, sampling_ratio=0, axes='xy',
                 bin_stride=1, order=None):
    """Spatial Region of Interest (ROI) align function.

    x: (N, C, H, W) float32; rois: (R, 5) float32 rows
    ``(batch_index, x_min, y_min, x_max, y_max)`` (``axes='xy'``) or
    ``(batch_index, y_min, x_min, y_max, x_max)`` (``axes='yx'``).
    Returns (R, C, outh, outw).  Reference: roi_align_2d.py:527-560.

    ``bin_stride`` (extension, default 1 = reference behaviour): produce only every
    ``bin_stride``-th bin in each direction, i.e. exactly ``roi_align_2d(...)[:, :, ::s, ::s]``.

    ``order`` (extension, default None): int32 device permutation of the RoI rows — the sequence
    in which the forward kernel PROCESSES them (``spatial_order``); the result does not depend on it.
    """
    rois = _re.swap_axes(rois, axes)
    return ROIAlign2D(outh, outw, spatial_scale, sampling_ratio, bin_stride, order)(x, rois)
