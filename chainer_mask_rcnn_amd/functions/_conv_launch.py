"""The launches of the convolution family: one Python function per entry point of libmrcnn_hip.so.

What a function here decides is how ONE launch is spelled — the epilogue flags, the scratch, the
output tensor (allocated here), which of two entry points computes the same thing — and nothing
else: no knob, no autograd, no module state.  Who owns a weight gradient is functions/_wgrad.py,
which route a layer takes is functions/conv.py, the fused stage is functions/stage.py; each of them
imports only the modules named before it.

``_lib`` is always called through the module (``_lib.call``, ``_lib.ptr``, ...): tests replace those
attributes.
"""
import ctypes

import torch

from .. import _lib
from .._lib import ConvDesc, EPI_BIAS, EPI_AFFINE, EPI_RESIDUAL, EPI_RELU, EPI_ACCUM, EPI_EXACT_SIGNS
from ._layout import nhwc, empty_nhwc
from ._roi_extractor import out_size
from .roi_align_2d import roi_align_backward


def conv_out_size(size, k, s, p):
    return (size + 2 * p - k) // s + 1


def make_desc(x_shape, w_shape, stride, pad):
    N, C, H, W = x_shape
    if len(w_shape) == 2:            # L.Linear weight (out, in) == 1x1 filter
        w_shape = (w_shape[0], w_shape[1], 1, 1)
    K, Cw, R, S = w_shape
    if Cw != C:
        raise ValueError('conv: input has %d channels, filter expects %d' % (C, Cw))
    return ConvDesc(N, H, W, C, K, R, S, stride, pad,
                    conv_out_size(H, R, stride, pad), conv_out_size(W, S, stride, pad))


def ctx_desc(d):
    return ctypes.byref(d)


def _colsum(g2d_ptr, M, C, out, device):
    ws = _lib.workspace(_lib.load().mrcnn_colsum_workspace_bytes(C), device, 'colsum')
    _lib.call('mrcnn_colsum', g2d_ptr, _lib.ptr(out), M, C, _lib.ptr(ws), _lib.stream_ptr())


def split_ws(device):
    """Scratch for the split-K leftover launches of small-M forward / dgrad GEMMs (cached per
    device and stream-ordered: safe because every user runs on the compute stream)."""
    return _lib.workspace(_lib.load().mrcnn_conv2d_split_workspace_bytes(), device, 'conv-split')


def epilogue_bwd(gy, y=None, scale=None):
    """g = gy * (y > 0) * scale[c] on NHWC tensors (any of y/scale may be None)."""
    _lib.require_device(gy, y, scale)
    gy = nhwc(gy, torch.float32, 'epilogue_bwd', 'gy')
    if y is not None:
        y = nhwc(y, torch.float32, 'epilogue_bwd', 'y')
    if scale is not None:
        scale = _lib.dense(scale, torch.float32, 'epilogue_bwd', 'scale', align=True)
    N, C = gy.shape[0], gy.shape[1]
    M = gy.numel() // C
    g = empty_nhwc(tuple(gy.shape), gy.device)
    _lib.call('mrcnn_epilogue_bwd', _lib.ptr(gy), _lib.ptr(y), _lib.ptr(scale), _lib.ptr(g),
              M, C, _lib.stream_ptr())
    return g


# ---- implicit-GEMM convolution: forward, data gradient, weight gradient ----------------------------

def _fwd_raw(x, Wc, d, scale=None, shift=None, residual=None, relu=False, bias=None):
    """y = relu?( affine?( conv(x, Wc) + bias? ) + residual? ) on prepared (NHWC / dense) operands."""
    flags = (EPI_BIAS if bias is not None else 0) | (EPI_AFFINE if scale is not None else 0) \
        | (EPI_RESIDUAL if residual is not None else 0) | (EPI_RELU if relu else 0)
    y = empty_nhwc((d.N, d.K, d.P, d.Q), x.device)
    _lib.call('mrcnn_conv2d_fwd', ctx_desc(d), _lib.ptr(x), _lib.ptr(Wc), _lib.ptr(bias), _lib.ptr(scale),
              _lib.ptr(shift), _lib.ptr(residual), _lib.ptr(y), flags, _lib.ptr(split_ws(x.device)),
              _lib.stream_ptr())
    return y


def _flip_transpose(Wc, d, row_scale, out):
    """``out`` = the filter ``Wc`` (d.K, d.R, d.S, d.C) flipped and transposed, rows scaled."""
    _lib.call('mrcnn_filter_flip_transpose', _lib.ptr(Wc), _lib.ptr(out), d.K, d.R, d.S, d.C,
              _lib.ptr(row_scale), _lib.stream_ptr())
    return out


def _flip_transpose_batched(jobs, device):
    """``_flip_transpose`` of every ``(Wc, d, row_scale)`` of ``jobs`` by ONE launch into one buffer;
    returns the flat transposed filters in the order of the jobs."""
    buf = torch.empty((sum(Wc.numel() for Wc, _, _ in jobs),), dtype=torch.float32, device=device)
    n = len(jobs)
    vp, ci = ctypes.c_void_p * n, ctypes.c_int * n
    w, wT, sc = vp(), vp(), vp()
    K, R, S, C = ci(), ci(), ci(), ci()
    out, off = [], 0
    for i, (Wc, d, scale) in enumerate(jobs):
        t = buf[off:off + Wc.numel()]
        off += Wc.numel()
        out.append(t)
        w[i], wT[i] = _lib.addr(Wc, 'w'), _lib.addr(t, 'wT')
        sc[i] = _lib.addr(scale, 'row_scale')
        K[i], R[i], S[i], C[i] = d.K, d.R, d.S, d.C
    _lib.call('mrcnn_filter_flip_transpose_batched', n, w, wT, K, R, S, C, sc, _lib.stream_ptr())
    return out


# Data gradients in forward form on the flipped, transposed filter: stride-1 square filters, and
# the strided 1x1 / pad 0 ones (res3.a / res4.a conv1 and conv4: dense gather of gy, rows scattered
# to the strided pixels of a zero-filled gx).  Split-operand kernels; the K-strided form that the
# other filters take runs on fp32 MFMA.
def _uses_transposed_dgrad(d):
    if d.stride == 1:
        return d.R == d.S
    return d.R == 1 and d.S == 1 and d.pad == 0


def _dgrad_raw(d, g, Wc, res_g=None, res_y=None, out=None, accum=False,
               out_mask_y=None, out_scale=None, fold_scale=None, wT=None):
    """gx = dgrad(g) with the fused pieces of include/mrcnn_hip.h "Extended backward entry
    points": producer-side ``out_mask_y`` / ``out_scale``, shortcut gradient ``res_g`` (masked
    by ``res_y`` if given).  ``fold_scale`` is a per-output-channel scale of the incoming
    gradient folded into the transposed filter (forward form only)."""
    gx = out if out is not None else empty_nhwc((d.N, d.C, d.H, d.W), g.device)
    if _uses_transposed_dgrad(d):
        # forward-form dgrad on the flipped, transposed filter; ``wT`` = already built (with
        # fold_scale applied), else rebuilt here (it moves 2 x the filter bytes)
        if wT is None:
            wT = _flip_transpose(Wc, d, fold_scale,
                                 _lib.workspace(4 * d.K * d.R * d.S * d.C, g.device,
                                                'wT').view(torch.float32))
        entry, filt = 'mrcnn_conv2d_dgrad_wt', wT
    elif fold_scale is not None:
        raise ValueError('dgrad: fold_scale needs the forward form (stride-1 square filters or '
                         '1x1 / pad 0), got %dx%d / stride %d / pad %d' % (d.R, d.S, d.stride, d.pad))
    else:
        entry, filt = 'mrcnn_conv2d_dgrad_ex', Wc
    _lib.call(entry, ctx_desc(d), _lib.ptr(g), _lib.ptr(filt), _lib.ptr(gx),
              EPI_ACCUM if accum else 0, _lib.ptr(res_g), _lib.ptr(res_y), _lib.ptr(out_mask_y),
              _lib.ptr(out_scale), _lib.ptr(split_ws(g.device)), _lib.stream_ptr())
    return gx


def _launch_wgrad(d, x, g, gW, row_scale=None, ex=True):
    """The implicit-GEMM weight gradient into the buffer ``gW``, on the current stream.  ``ex``
    False: the plain entry point (no ``row_scale``)."""
    ws = _lib.workspace(_lib.load().mrcnn_conv2d_wgrad_workspace_bytes(ctx_desc(d)), g.device, 'wgrad')
    tail = (_lib.ptr(row_scale), _lib.stream_ptr()) if ex else (_lib.stream_ptr(),)
    _lib.call('mrcnn_conv2d_wgrad_ex' if ex else 'mrcnn_conv2d_wgrad', ctx_desc(d), _lib.ptr(x),
              _lib.ptr(g), _lib.ptr(gW), _lib.ptr(ws), *tail)


# ---- row-sparse backward of a 3x3 convolution (include/mrcnn_hip.h "row-sparse backward") ----------

def _sparse3x3_gather(d, x, g, rows, n):
    """(patches (n, 9 C), g_rows (n, K)): the 3x3 input patches around, and the gradient rows at,
    the ``n`` map positions ``rows``."""
    patches = torch.empty((n, 9 * d.C), dtype=torch.float32, device=g.device)
    g_rows = torch.empty((n, d.K), dtype=torch.float32, device=g.device)
    _lib.call('mrcnn_sparse3x3_gather', _lib.ptr(x), _lib.ptr(g), _lib.ptr(rows), n,
              d.N, d.H, d.W, d.C, d.K, _lib.ptr(patches), _lib.ptr(g_rows), _lib.stream_ptr())
    return patches, g_rows


def _sparse3x3_scatter(d, gp, lookup):
    """gx (N, C, H, W) from the (rows, 3, 3, C) patch gradients ``gp``."""
    gx = empty_nhwc((d.N, d.C, d.H, d.W), gp.device)
    _lib.call('mrcnn_sparse3x3_scatter', _lib.ptr(gp), _lib.ptr(lookup), d.N, d.H, d.W,
              d.C, _lib.ptr(gx), _lib.stream_ptr())
    return gx


# ---- the stem and the 2x2 / stride 2 deconvolution ----------------------------------------------------

def _stem_fwd(x4, w784, b, scale, shift):
    """relu(affine?(conv7x7/2 pad 3 (x4) + b?)) of the dense (N, H, W, 4) image ``x4``."""
    N, H, W_, four = x4.shape
    assert four == 4
    K = w784.shape[0]
    P, Q = conv_out_size(H, 7, 2, 3), conv_out_size(W_, 7, 2, 3)
    y = empty_nhwc((N, K, P, Q), x4.device)
    flags = EPI_RELU | (EPI_BIAS if b is not None else 0) | \
        (EPI_AFFINE if scale is not None else 0)
    _lib.call('mrcnn_conv_stem_fwd', _lib.ptr(x4), _lib.ptr(w784), _lib.ptr(b),
              _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(y), N, H, W_, K, flags,
              _lib.stream_ptr())
    return y


def _deconv_fwd(x, Wc, b, dims, relu, forward_form):
    """y = relu?(deconv2x2s2(x, Wc) + b?); ``dims`` = (N, H, W, C, K) of the input map and the
    filter.  ``forward_form``: as a forward-form GEMM on the transposed filter (4K, C) — both
    operands K-contiguous: the split-operand kernels — instead of the K-strided form (fp32 MFMA)."""
    N, H, Wd, C, K = dims
    y = empty_nhwc((N, K, 2 * H, 2 * Wd), x.device)
    flags = (EPI_BIAS if b is not None else 0) | (EPI_RELU if relu else 0)
    if forward_form:
        wT = _lib.workspace(4 * C * 4 * K, x.device, 'deconv-wT').view(torch.float32)
        # (the (C, 2, 2, K) filter read as C rows of a 1x1 filter over 4K channels)
        _flip_transpose(Wc, ConvDesc(N, H, Wd, 4 * K, C, 1, 1, 1, 0, H, Wd), None, wT)
        _lib.call('mrcnn_deconv2x2s2_fwd_wt', _lib.ptr(x), _lib.ptr(wT), _lib.ptr(b), _lib.ptr(y),
                  N, H, Wd, C, K, flags, _lib.stream_ptr())
    else:
        _lib.call('mrcnn_deconv2x2s2_fwd', _lib.ptr(x), _lib.ptr(Wc), _lib.ptr(b), _lib.ptr(y),
                  N, H, Wd, C, K, flags, _lib.stream_ptr())
    return y


def _deconv_dgrad(g, Wc, dims):
    N, H, Wd, C, K = dims
    gx = empty_nhwc((N, C, H, Wd), g.device)
    _lib.call('mrcnn_deconv2x2s2_dgrad', _lib.ptr(g), _lib.ptr(Wc), _lib.ptr(gx),
              N, H, Wd, C, K, _lib.stream_ptr())
    return gx


def _deconv_wgrad_into(x, g, gW, dims):
    N, H, Wd, C, K = dims
    ws = _lib.workspace(_lib.load().mrcnn_deconv2x2s2_wgrad_workspace_bytes(N, H, Wd, C, K),
                        g.device, 'wgrad')
    _lib.call('mrcnn_deconv2x2s2_wgrad', _lib.ptr(x), _lib.ptr(g), _lib.ptr(gW),
              N, H, Wd, C, K, _lib.ptr(ws), _lib.stream_ptr())


# ---- Winograd F(4x4,3x3) (csrc/conv_winograd.h) -------------------------------------------------------

def _wino_ws(d, device):
    return _lib.workspace(_lib.load().mrcnn_conv3x3_wino_workspace_bytes(ctx_desc(d)), device, 'wino')


def _wino_filter(d, Wc):
    """The transformed filter of ``Wc``, for ``_wino_fwd_raw(u=)``."""
    u = torch.empty((_lib.load().mrcnn_conv3x3_wino_u_bytes(ctx_desc(d)) // 4,),
                    dtype=torch.float32, device=Wc.device)
    _lib.call('mrcnn_conv3x3_wino_filter', ctx_desc(d), _lib.ptr(Wc), _lib.ptr(u), _lib.stream_ptr())
    return u


def _wino_fwd_raw(x, Wc, d, scale, shift, relu, keep_v=False, u=None, exact_signs=False):
    """y = relu?(affine?(conv3x3(x))) — ``scale`` None with a ``shift``: plain bias — and, with
    ``keep_v``, the transformed input (36, tiles, C) for the weight gradient.  ``u``: the filter
    already transformed (``_wino_filter``), None = transformed by this launch.  ``exact_signs``:
    outputs within the Winograd rounding bound of zero are recomputed directly
    (MRCNN_EPI_EXACT_SIGNS)."""
    flags = (EPI_AFFINE if scale is not None else (EPI_BIAS if shift is not None else 0)) \
        | (EPI_RELU if relu else 0) | (EPI_EXACT_SIGNS if exact_signs else 0)
    y = empty_nhwc((d.N, d.K, d.P, d.Q), x.device)
    v = None
    if keep_v:
        v = torch.empty((_lib.load().mrcnn_conv3x3_wino_v_bytes(ctx_desc(d)) // 4,),
                        dtype=torch.float32, device=x.device)
    _lib.call('mrcnn_conv3x3_wino_fwd', ctx_desc(d), _lib.ptr(x), _lib.ptr(Wc), _lib.ptr(u),
              _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(y), flags, _lib.ptr(v),
              _lib.ptr(_wino_ws(d, x.device)), _lib.stream_ptr())
    return y, v


def wino_dgrad(d, g, Wc, fold_scale=None, out_scale=None, out_mask_y=None):
    gx = empty_nhwc((d.N, d.C, d.H, d.W), g.device)
    _lib.call('mrcnn_conv3x3_wino_dgrad', ctx_desc(d), _lib.ptr(g), _lib.ptr(Wc),
              _lib.ptr(fold_scale), _lib.ptr(gx), _lib.ptr(out_scale), _lib.ptr(out_mask_y),
              _lib.ptr(_wino_ws(d, g.device)), _lib.stream_ptr())
    return gx


def wino_wgrad_into(d, x, v, g, gW, row_scale=None):
    """gW = backward-filter from ``g`` and exactly one of ``x`` (raw input) / ``v`` (the
    transformed input a forward with ``keep_v`` returned)."""
    _lib.call('mrcnn_conv3x3_wino_wgrad', ctx_desc(d), _lib.ptr(x), _lib.ptr(v), _lib.ptr(g),
              _lib.ptr(gW), _lib.ptr(row_scale), _lib.ptr(_wino_ws(d, g.device)),
              _lib.stream_ptr())


# ---- ROIAlign inside the fused stage, and the RoI head's tail ------------------------------------------

class RoiSpec(object):
    """What ``building_block(..., roi=)`` needs to pool inside the stage node: ``rois`` (R, 5) float32
    device rows (batch, x1, y1, x2, y2), the pooled size ``outh`` x ``outw`` of the FULL bin grid,
    ``bin_stride`` (the stride of block a's 1x1 convolutions: only those bins are produced) and the
    optional processing ``order`` (functions.roi_align_2d.spatial_order)."""

    def __init__(self, rois, outh, outw, spatial_scale, bin_stride=1, order=None, sampling_ratio=0,
                 proj=None):
        # ``proj`` (inference only): the two projections of the map, ``projected_map(...)``, when the
        # caller pools several RoI sets from one map (MaskRCNN.predict_prepared: one head call per image)
        self.proj = proj
        _lib.require_device(rois, order)
        self.rois = _lib.dense(rois, torch.float32, 'RoiSpec', 'rois')
        if order is not None:
            order = _lib.dense(order, torch.int32, 'RoiSpec', 'order')
        self.outh, self.outw = int(outh), int(outw)
        self.spatial_scale = float(spatial_scale)
        self.bin_stride = int(bin_stride)
        self.order = order
        self.sampling_ratio = int(sampling_ratio)

    @property
    def out_hw(self):
        return out_size(self.outh, self.bin_stride), out_size(self.outw, self.bin_stride)


def _roi_pool_affine(z, roi, scale, shift, relu):
    """relu?(roi_align(z) * scale + shift) for an NHWC map ``z`` (N, C, H, W logical)."""
    N, C, H, W = z.shape
    R = roi.rois.shape[0]
    oh, ow = roi.out_hw
    y = empty_nhwc((R, C, oh, ow), z.device)
    order = roi.order if R > 0 else None
    _lib.call('mrcnn_roi_align_fwd_affine', _lib.ptr(z), _lib.ptr(roi.rois), _lib.ptr(y), N, H, W, C, R,
              roi.outh, roi.outw, roi.bin_stride, roi.spatial_scale, roi.sampling_ratio,
              _lib.ptr(order) if order is not None else None, _lib.ptr(scale), _lib.ptr(shift),
              1 if relu else 0, _lib.stream_ptr())
    return y


def _roi_pool_bwd(g, roi, map_shape):
    """ROIAlign's adjoint: g (R, C, oh, ow) -> (N, C, H, W), pixel-owner form (no atomics)."""
    return roi_align_backward(g, roi.rois, map_shape, roi.outh, roi.outw, roi.bin_stride,
                              roi.spatial_scale, roi.sampling_ratio)


def _avgpool_fwd(h):
    """(R, C) means of the NHWC maps ``h`` (R, C, H, W) over their positions."""
    R, C = h.shape[0], h.shape[1]
    pooled = torch.empty((R, C), dtype=torch.float32, device=h.device)
    _lib.call('mrcnn_avgpool_fwd', _lib.ptr(h), _lib.ptr(pooled), R, h.shape[2] * h.shape[3],
              C, _lib.stream_ptr())
    return pooled


def _head_tail_bwd(gp, gr, slot, y):
    """The gradient of ``(average_pooling(y), y[rows])`` w.r.t. y, through y's ReLU, in one pass:
    ``gp`` (R, C) the pooled gradient, ``gr`` the gradient of the selected rows (or None) and
    ``slot`` the int32 table row -> position among them."""
    R, C, H, W = y.shape
    gm = empty_nhwc((R, C, H, W), y.device)
    _lib.call('mrcnn_head_tail_bwd', _lib.ptr(gp), _lib.ptr(gr),
              _lib.ptr(slot) if gr is not None else None, _lib.ptr(y),
              _lib.ptr(gm), R, H * W, C, _lib.stream_ptr())
    return gm
