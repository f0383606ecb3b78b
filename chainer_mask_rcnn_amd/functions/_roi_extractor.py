"""The contract of the three RoI feature extractors (``roi_align_2d``, ``roi_pooling_2d``,
``crop_and_resize``), stated once: float32 ``x`` (N, C, H, W) stored channels-last, ``rois`` (R, 5)
rows ``(batch_index, x1, y1, x2, y2)``, the result (R, C, outh, outw) — or every ``bin_stride``-th
bin of it —, an optional processing ``order``, and a backward that owns every pixel of the map's
gradient and takes its tables from a cached workspace.  No gradient w.r.t. ``rois``.
"""
import torch

from .. import _lib
from ._layout import nhwc, empty_nhwc


# debug / test switch: check that ``order`` is a permutation of 0..R-1 (one device sort + a read-back)
VALIDATE_ORDER = False


def out_size(n, bin_stride):
    """Bins produced along an axis of ``n`` bins: every ``bin_stride``-th one."""
    return (n + bin_stride - 1) // bin_stride


def swap_axes(rois, axes):
    """The (R, 5) RoIs as ``(batch_index, x1, y1, x2, y2)`` rows, from ``axes`` 'xy' or 'yx'."""
    if axes not in ['xy', 'yx']:
        raise ValueError('Unsupported axes: {}'.format(axes))
    return rois[:, [0, 2, 1, 4, 3]] if axes == 'yx' else rois


def check_args(outh, outw, spatial_scale, bin_stride):
    """Constructor arguments of the pooling and crop-and-resize classes; returns ``spatial_scale``
    as a float."""
    for arg, value in (('outh', outh), ('outw', outw), ('bin_stride', bin_stride)):
        if not (isinstance(value, int) and not isinstance(value, bool) and value >= 1):
            raise TypeError('{} must be positive integer: {}, {}'.format(arg, type(value), value))
    if isinstance(spatial_scale, int) and not isinstance(spatial_scale, bool):
        spatial_scale = float(spatial_scale)
    elif not isinstance(spatial_scale, float):
        raise TypeError('spatial_scale must be float: {}'.format(type(spatial_scale)))
    return spatial_scale


def check_inputs(name, x, rois):
    if not (x.dtype == torch.float32 and x.dim() == 4 and rois.dtype == torch.float32
            and rois.dim() == 2 and rois.shape[1] == 5):
        raise TypeError('{} expects x: float32 (N,C,H,W), rois: float32 (R,5); got {} {} and {} {}'
                        .format(name, x.dtype, tuple(x.shape), rois.dtype, tuple(rois.shape)))


def check_order(order, R, device, name):
    """``order``: None, or a contiguous int32 device permutation of the RoI rows (checked as one
    when ``VALIDATE_ORDER`` is set)."""
    if order is None:
        return
    if not (order.dtype == torch.int32 and order.is_contiguous() and order.device == device
            and tuple(order.shape) == (R,)):
        raise TypeError('{}: order must be a contiguous int32 device tensor of shape (R,) — a '
                        'permutation of the RoI rows'.format(name))
    if VALIDATE_ORDER and R > 0 and not torch.equal(
            torch.sort(order.long())[0], torch.arange(R, device=order.device)):
        raise ValueError('{}: order is not a permutation of 0..R-1 (a duplicate leaves output rows '
                         'unwritten, an out-of-range value reads past rois)'.format(name))


class Extractor(object):
    """What one extractor adds to the contract: its three C entry points (``fwd``, ``ws_query``,
    ``bwd``) with the order of their leading pointers (``fwd_ptrs`` / ``bwd_ptrs``: names among
    x, gy, rois, y, gx, extra), the names of the scalars that follow ``spatial_scale`` in both
    calls (``scalars``), the tensor it keeps for the backward besides the RoIs
    (``extra(rois, out_shape)``, or None) and the tag of its cached workspace.  ``wants_ws()``
    False runs the backward without a workspace (ROIAlign's atomic forms)."""

    def __init__(self, name, fwd, ws_query, bwd, ws_tag, fwd_ptrs=('x', 'rois', 'y'),
                 bwd_ptrs=('gy', 'rois', 'gx'), scalars=(), extra=None, wants_ws=lambda: True):
        self.name, self.fwd, self.ws_query, self.bwd, self.ws_tag = name, fwd, ws_query, bwd, ws_tag
        self.fwd_ptrs, self.bwd_ptrs, self.scalars = fwd_ptrs, bwd_ptrs, scalars
        self.extra, self.wants_ws = extra, wants_ws

    def forward(self, x, rois, outh, outw, spatial_scale, scalars, bin_stride, order):
        """-> (y, rois as passed to the kernel, extra)"""
        _lib.require_device(x, rois)
        x = nhwc(x, torch.float32, self.name)
        rois = _lib.dense(rois, torch.float32, self.name, 'rois')
        N, C, H, W = x.shape
        R = rois.shape[0]
        shape = (R, C, out_size(outh, bin_stride), out_size(outw, bin_stride))
        t = dict(x=x, rois=rois, y=empty_nhwc(shape, x.device))
        t['extra'] = self.extra(rois, shape) if self.extra is not None else None
        check_order(order, R, x.device, self.name)
        _lib.call(self.fwd, *[_lib.ptr(t[k]) for k in self.fwd_ptrs], N, H, W, C, R, outh, outw,
                  bin_stride, spatial_scale, *scalars,
                  _lib.ptr(order) if order is not None and R > 0 else None, _lib.stream_ptr())
        return t['y'], rois, t['extra']

    def backward(self, gy, rois, extra, map_shape, outh, outw, spatial_scale, scalars, bin_stride,
                 use_ws=True):
        """The gradient of the (N, C, H, W) map from ``gy`` (R, C, oh, ow)."""
        N, C, H, W = map_shape
        R = rois.shape[0]
        gy = nhwc(gy, torch.float32, self.name, 'gy')
        t = dict(gy=gy, rois=rois, extra=extra, gx=empty_nhwc(map_shape, gy.device))
        ws = None
        if use_ws:
            nbytes = getattr(_lib.load(), self.ws_query)(N, H, W, R, outh, outw, bin_stride)
            ws = _lib.workspace(nbytes, gy.device, self.ws_tag)
        _lib.call(self.bwd, *[_lib.ptr(t[k]) for k in self.bwd_ptrs], N, H, W, C, R, outh, outw,
                  bin_stride, spatial_scale, *scalars, _lib.ptr(ws),
                  int(ws.numel() * ws.element_size()) if ws is not None else 0, _lib.stream_ptr())
        return t['gx']

    def function(self, cls_name):
        """The extractor's autograd node, a class named ``cls_name``: ``apply(x, rois, outh, outw,
        spatial_scale, *scalars, bin_stride=1, order=None)``.  Only the RoIs (and ``extra``) are
        retained, not ``x``."""
        ext = self
        n = len(self.scalars)

        def tail(bin_stride=1, order=None):
            return bin_stride, order

        class Fn(torch.autograd.Function):

            @staticmethod
            def forward(ctx, x, rois, outh, outw, spatial_scale, *rest):
                bin_stride, order = tail(*rest[n:])
                y, rois, extra = ext.forward(x, rois, outh, outw, spatial_scale, rest[:n],
                                             bin_stride, order)
                ctx.save_for_backward(rois, extra)
                ctx.x_shape = tuple(x.shape)
                ctx.args = (outh, outw, spatial_scale, rest[:n], bin_stride)
                ctx.n_inputs = 5 + len(rest)
                return y

            @staticmethod
            def backward(ctx, gy):
                rois, extra = ctx.saved_tensors
                gx = ext.backward(gy, rois, extra, ctx.x_shape, *ctx.args, use_ws=ext.wants_ws())
                return (gx,) + (None,) * (ctx.n_inputs - 1)

        Fn.__name__ = Fn.__qualname__ = cls_name
        return Fn
