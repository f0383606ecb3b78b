"""Convolution / deconvolution / linear ops on the fp32-MFMA implicit-GEMM kernel.

Host-side mirror of chainer's ``L.Convolution2D`` (+ the ``AffineChannel2D``,
residual add and ReLU that follow it inside chainer's Bottleneck blocks),
``L.Deconvolution2D(k=2, s=2)`` and ``L.Linear`` as the reference uses them
(/root/reference/chainer_mask_rcnn/models/region_proposal_network.py:75-80,
models/mask_rcnn_resnet.py:131-143).  Tensors carry the
reference's logical shapes — x (N,C,H,W), conv W (out,in,kh,kw), deconv W
(in,out,kh,kw), linear W (out,in) — stored channels-last, which is exactly the
NHWC / KRSC layout the HIP kernels consume.
"""
import collections
import ctypes
import os as _os

import torch

from .. import _lib
from .._lib import ConvDesc, EPI_BIAS, EPI_AFFINE, EPI_RESIDUAL, EPI_RELU, EPI_ACCUM, EPI_EXACT_SIGNS
from ..streams import join_wgrad_stream, wgrad_stream
from ._layout import nhwc, empty_nhwc
from ._roi_extractor import out_size
from .roi_align_2d import roi_align_backward


def _direct_grad(p):
    """Claim the right to WRITE ``p``'s gradient in place: true for an arena-backed parameter
    (optimizers.ParamArena) whose arena view is intact and that has not received a gradient yet
    in this step.  Otherwise the caller returns a fresh tensor and autograd accumulates it."""
    arena = getattr(p, '_arena', None)
    if arena is None:
        return False
    if arena.claim(p):
        return True
    join_wgrad_stream(p.device)      # an earlier in-place write may still be queued there
    return False


def _grad_target(p):
    """The gradient-ownership rule in one place: ``(buffer, result)`` for parameter ``p`` — the
    buffer the producing kernel writes (not adds) p's gradient into and what the autograd node
    returns for p: ``(p.grad, None)`` when the arena slot could be claimed, else the same fresh
    tensor twice (autograd accumulates it)."""
    if _direct_grad(p):
        return p.grad, None
    g = empty_nhwc(tuple(p.shape), p.device) if p.dim() == 4 else \
        torch.empty(tuple(p.shape), dtype=torch.float32, device=p.device)
    return g, g


def _bias_grad(b, g, M):
    """Bias gradient = column sum of the (M, len(b)) gradient ``g``; returns what autograd gets."""
    gb, result = _grad_target(b)
    _colsum(_lib.ptr(g), M, b.shape[0], gb, g.device)
    return result


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


# Test hook: when set to a list, every ReLU output this module produces (fused conv epilogues, the
# three activations of each bottleneck of a fused stage, the deconvolution) is appended as
# (kind, tensor) in call order — tests/test_gpu_model.py reads the ReLU DECISIONS of the HIP path
# from it.  None (default): nothing is recorded or kept alive.
RELU_TAP = None


# ---- row-sparse backward of a 3x3 convolution (include/mrcnn_hip.h "row-sparse backward") -------
# The RPN's losses ignore every anchor but the <= 256 sampled ones per image, so the gradient
# reaching conv1's output is exactly zero outside their map positions; the train chain, which
# builds the anchor targets on the host, hands the positions to the RPN in a ``SparseRows``.
SPARSE_CONV_BACKWARD = True


class SparseRows(object):
    """Positions of a (N, H, W) map outside which the gradient arriving at a convolution's output
    is EXACTLY zero: ``rows`` int32 device tensor of sorted indices into N*H*W, ``lookup`` int32
    device tensor (N*H*W) position -> index into rows or -1, ``n`` = len(rows) (host int).
    One-shot and owned by ONE forward: the producer makes a new object per forward (the conv node
    records it), the backward that uses it clears it.  ``valid_for`` is the backward's guard: a hint
    whose tables do not describe the node's own (N, H, W) map is ignored (dense backward)."""

    def __init__(self):
        self.clear()

    def clear(self):
        self.rows = self.lookup = None
        self.n = 0

    def set(self, rows, lookup, n):
        self.rows, self.lookup, self.n = rows, lookup, int(n)

    def valid_for(self, d, device):
        """True when the tables can drive the row-sparse backward of a convolution with output
        map (d.N, d.P, d.Q) on ``device`` (shape / dtype / device checks only: no read-back)."""
        r, l = self.rows, self.lookup
        if r is None or l is None or self.n <= 0:
            return False
        size = d.N * d.P * d.Q
        return (r.dtype == torch.int32 and l.dtype == torch.int32 and r.device == device and
                l.device == device and r.is_contiguous() and l.is_contiguous() and
                r.numel() == self.n and self.n <= size and l.numel() == size)

    @staticmethod
    def host_tables(positions, size):
        """(rows int32 sorted unique, lookup int32 (size,)) NumPy arrays from map positions."""
        import numpy as np
        rows = np.unique(np.asarray(positions, np.int64)).astype(np.int32)
        lookup = np.full((int(size),), -1, np.int32)
        lookup[rows] = np.arange(len(rows), dtype=np.int32)
        return rows, lookup


def _check_grad_rows(d, stride, pad, scale, residual):
    """A convolution given ``grad_rows`` must be able to use it: 3x3 / stride 1 / pad 1, no affine,
    no residual (the row-sparse backward is the 1x1 problem on gathered 3x3 patches)."""
    if (d.R, d.S) != (3, 3):
        why = 'the filter is %dx%d, not 3x3' % (d.R, d.S)
    elif stride != 1:
        why = 'stride is %d, not 1' % stride
    elif pad != 1:
        why = 'pad is %d, not 1' % pad
    elif scale is not None:
        why = 'it has an affine scale'
    elif residual is not None:
        why = 'it has a residual'
    else:
        return
    raise ValueError('conv2d: grad_rows needs a 3x3 / stride 1 / pad 1 convolution without scale '
                     'or residual, but %s' % why)


def _sparse3x3_backward(ctx, d, x, Wc, g, hint, need_x, need_w, need_b):
    """Backward of a 3x3 / stride 1 / pad 1 convolution whose output gradient ``g`` (already through
    ReLU) is zero outside ``hint.rows``: the 1x1 problem (N = rows, C = 9 C_in) on gathered patches."""
    dev, n = g.device, hint.n
    patches = torch.empty((n, 9 * d.C), dtype=torch.float32, device=dev)
    g_rows = torch.empty((n, d.K), dtype=torch.float32, device=dev)
    _lib.call('mrcnn_sparse3x3_gather', _lib.ptr(x), _lib.ptr(g), _lib.ptr(hint.rows), n,
              d.N, d.H, d.W, d.C, d.K, _lib.ptr(patches), _lib.ptr(g_rows), _lib.stream_ptr())
    d1 = ConvDesc(n, 1, 1, 9 * d.C, d.K, 1, 1, 1, 0, 1, 1)
    gx = gW = gb = None
    if need_w:
        gW = _wgrad(d1, patches, g_rows, ctx.W_param)
    if need_x:
        gp = _dgrad_raw(d1, g_rows, Wc)          # (rows, 3, 3, C) patch gradients
        gx = empty_nhwc((d.N, d.C, d.H, d.W), dev)
        _lib.call('mrcnn_sparse3x3_scatter', _lib.ptr(gp), _lib.ptr(hint.lookup), d.N, d.H, d.W,
                  d.C, _lib.ptr(gx), _lib.stream_ptr())
    if need_b:
        gb = _bias_grad(ctx.b_param, g_rows, n)
    return gx, gW, gb


class _Conv2dFn(torch.autograd.Function):
    """y = relu?( affine?( conv(x, W) + b? ) + residual? )"""

    @staticmethod
    def forward(ctx, x, W, b, scale, shift, residual, stride, pad, relu, records_graph, grad_rows):
        # ``records_graph``: torch.is_grad_enabled() at the call (in here grad mode is always off and
        # ctx.needs_input_grad reports the inputs' requires_grad flags even under torch.no_grad())
        _lib.require_device(x, W, b, scale, shift, residual)
        x = nhwc(x, torch.float32, 'conv2d')
        Wc = nhwc(W, torch.float32, 'conv2d', 'W') if W.dim() == 4 else \
            _lib.dense(W, torch.float32, 'conv2d', 'W', align=True)
        b_param = b
        b, scale, shift = (v if v is None else _lib.dense(v, torch.float32, 'conv2d', name, align=True)
                           for name, v in (('b', b), ('scale', scale), ('shift', shift)))
        d = make_desc(x.shape, W.shape, stride, pad)
        if grad_rows is not None:
            _check_grad_rows(d, stride, pad, scale, residual)
        flags = 0
        if b is not None:
            flags |= EPI_BIAS
        if scale is not None:
            flags |= EPI_AFFINE
        if residual is not None:
            residual = nhwc(residual, torch.float32, 'conv2d', 'residual')
            flags |= EPI_RESIDUAL
        if relu:
            flags |= EPI_RELU
        ctx.wino = uses_winograd(d) and residual is None and (b is None or scale is None)
        if ctx.wino and _wino_forward('conv2d', records_graph and any(ctx.needs_input_grad)):
            y, _ = wino_fwd(x, Wc, d, scale, shift if scale is not None else b, relu,
                            cache_for=None if records_graph else W,
                            exact_signs=relu and records_graph)
        else:
            y = empty_nhwc((d.N, d.K, d.P, d.Q), x.device)
            _lib.call('mrcnn_conv2d_fwd', ctx_desc(d), _lib.ptr(x), _lib.ptr(Wc), _lib.ptr(b),
                      _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(residual), _lib.ptr(y), flags,
                      _lib.ptr(split_ws(x.device)), _lib.stream_ptr())
        ctx.d = d
        ctx.relu = relu
        ctx.has_bias = b is not None
        ctx.has_res = residual is not None
        ctx.sparse_hint = grad_rows
        ctx.W_param = W
        ctx.b_param = b_param
        ctx.save_for_backward(x, Wc, scale, y if relu else None)
        if RELU_TAP is not None and relu:
            RELU_TAP.append(('conv', y))
        return y

    @staticmethod
    def backward(ctx, gy):
        x, Wc, scale, y = ctx.saved_tensors
        d = ctx.d
        gy = nhwc(gy, torch.float32, 'conv2d', 'gy')
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], \
            ctx.has_bias and ctx.needs_input_grad[2]
        # through ReLU, then through the affine scale
        gr = epilogue_bwd(gy, y, None) if ctx.relu else gy
        g = epilogue_bwd(gr, None, scale) if scale is not None else gr
        gx = gW = gb = None
        hint = ctx.sparse_hint
        if hint is not None and SPARSE_CONV_BACKWARD and hint.valid_for(d, gy.device):
            gx, gW, gb = _sparse3x3_backward(ctx, d, x, Wc, g, hint, need_x, need_w, need_b)
            hint.clear()
            return gx, gW, gb, None, None, None, None, None, None, None, None
        if need_w:
            if ctx.wino:
                gW = _wgrad(d, x, g, ctx.W_param, wino=True)
            else:
                # the plain entry point, and NOT through the defer queue (MomentumSGD.step raises
                # for a deferred parameter whose gradient came this way)
                gWt, gW = _grad_target(ctx.W_param)
                _launch_wgrad(d, x, g, gWt, ex=False)
        if need_x:
            gx = wino_dgrad(d, g, Wc) if ctx.wino else _dgrad_raw(d, g, Wc)
        if need_b:
            gb = _bias_grad(ctx.b_param, g, d.N * d.P * d.Q)
        gres = gr if ctx.has_res and ctx.needs_input_grad[5] else None
        return gx, gW, gb, None, None, gres, None, None, None, None, None


def conv2d(x, W, b=None, stride=1, pad=0, scale=None, shift=None, residual=None, relu=False,
           grad_rows=None):
    """Fused convolution: ``relu(affine(conv(x,W)+b) + residual)`` with each stage optional.

    ``scale``/``shift`` are the AffineChannel2D ``W``/``b`` (frozen: no gradient is
    produced for them — the reference computes but never uses it,
    examples/train_common.py:188-190).  ``grad_rows``: a ``SparseRows`` (filled before backward) the
    backward of a 3x3 / stride 1 / pad 1 convolution may take its rows from; ValueError for a
    convolution that cannot use it.
    """
    return _Conv2dFn.apply(x, W, b, scale, shift, residual, stride, pad, relu,
                           torch.is_grad_enabled(), grad_rows)


class _StemFn(torch.autograd.Function):
    """conv1 7x7/2 pad 3 + bias + affine + ReLU, forward only (frozen stem)."""

    @staticmethod
    def forward(ctx, x4, w784, b, scale, shift):
        _lib.require_device(x4, w784, b, scale, shift)
        x4 = _lib.dense(x4, torch.float32, 'stem_conv', 'x4', align=True)
        w784 = _lib.dense(w784, torch.float32, 'stem_conv', 'w784', align=True)
        b, scale, shift = (v if v is None else _lib.dense(v, torch.float32, 'stem_conv', name, align=True)
                           for name, v in (('b', b), ('scale', scale), ('shift', shift)))
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

    @staticmethod
    def backward(ctx, gy):
        raise _lib.MrcnnHipError(
            'the ResNet stem is frozen (unchain_backward at res2, '
            'models/resnet_extractor.py:86-87): no backward is implemented')


def stem_conv(x4, w784, b, scale, shift):
    return _StemFn.apply(x4, w784, b, scale, shift)


# The deconvolution's forward as a forward-form GEMM on the transposed filter (split-operand kernels)
# instead of the K-strided data-gradient form (fp32 MFMA): see mrcnn_deconv2x2s2_fwd_wt.
DECONV_FORWARD_FORM = True


class _Deconv2x2Fn(torch.autograd.Function):
    """L.Deconvolution2D(in, out, 2, stride=2) (+ bias, + ReLU)."""

    @staticmethod
    def forward(ctx, x, W, b, relu):
        _lib.require_device(x, W, b)
        x = nhwc(x, torch.float32, 'deconv2x2s2')
        Wc = nhwc(W, torch.float32, 'deconv2x2s2', 'W')     # logical (C, K, 2, 2) -> physical (C, 2, 2, K)
        b_param = b
        if b is not None:
            b = _lib.dense(b, torch.float32, 'deconv2x2s2', 'b', align=True)
        N, C, H, Wd = x.shape
        K = W.shape[1]
        if tuple(W.shape) != (C, K, 2, 2):
            raise ValueError('deconv: filter must be (in, out, 2, 2), got %s' % (tuple(W.shape),))
        y = empty_nhwc((N, K, 2 * H, 2 * Wd), x.device)
        flags = (EPI_BIAS if b is not None else 0) | (EPI_RELU if relu else 0)
        if DECONV_FORWARD_FORM and GEMM_ARITHMETIC in SPLIT_GEMM_ARITHMETICS:
            # forward form on the transposed filter (4K, C): both operands K-contiguous -> the
            # split-operand kernels; the K-strided form below runs on fp32 MFMA
            wT = _lib.workspace(4 * C * 4 * K, x.device, 'deconv-wT').view(torch.float32)
            _lib.call('mrcnn_filter_flip_transpose', _lib.ptr(Wc), _lib.ptr(wT), C, 1, 1, 4 * K, None,
                      _lib.stream_ptr())
            _lib.call('mrcnn_deconv2x2s2_fwd_wt', _lib.ptr(x), _lib.ptr(wT), _lib.ptr(b), _lib.ptr(y),
                      N, H, Wd, C, K, flags, _lib.stream_ptr())
        else:
            _lib.call('mrcnn_deconv2x2s2_fwd', _lib.ptr(x), _lib.ptr(Wc), _lib.ptr(b), _lib.ptr(y),
                      N, H, Wd, C, K, flags, _lib.stream_ptr())
        ctx.dims = (N, H, Wd, C, K)
        ctx.relu = relu
        ctx.W_param, ctx.b_param = W, b_param
        ctx.save_for_backward(x, Wc, y if relu else None)
        if RELU_TAP is not None and relu:
            RELU_TAP.append(('deconv', y))
        return y

    @staticmethod
    def backward(ctx, gy):
        x, Wc, y = ctx.saved_tensors
        N, H, Wd, C, K = ctx.dims
        gy = nhwc(gy, torch.float32, 'deconv2x2s2', 'gy')
        g = epilogue_bwd(gy, y, None) if ctx.relu else gy
        gx = gW = gb = None
        if ctx.needs_input_grad[0]:
            gx = empty_nhwc((N, C, H, Wd), gy.device)
            _lib.call('mrcnn_deconv2x2s2_dgrad', _lib.ptr(g), _lib.ptr(Wc), _lib.ptr(gx),
                      N, H, Wd, C, K, _lib.stream_ptr())
        if ctx.needs_input_grad[1]:
            gWt, gW = _grad_target(ctx.W_param)
            ws = _lib.workspace(
                _lib.load().mrcnn_deconv2x2s2_wgrad_workspace_bytes(N, H, Wd, C, K),
                gy.device, 'wgrad')
            _lib.call('mrcnn_deconv2x2s2_wgrad', _lib.ptr(x), _lib.ptr(g), _lib.ptr(gWt),
                      N, H, Wd, C, K, _lib.ptr(ws), _lib.stream_ptr())
        if ctx.b_param is not None and ctx.needs_input_grad[2]:
            gb = _bias_grad(ctx.b_param, g, N * 4 * H * Wd)
        return gx, gW, gb, None


def deconv2x2s2(x, W, b=None, relu=False):
    return _Deconv2x2Fn.apply(x, W, b, relu)


def linear(x, W, b=None):
    """L.Linear: y = x.reshape(N,-1) @ W.T + b, as a 1x1 convolution on (N,C,1,1)."""
    n = x.shape[0]
    x4 = x.reshape(n, -1, 1, 1)
    y = conv2d(x4, W, b)
    return y.reshape(n, W.shape[0])


# ---- raw GEMM launches of the fused stage (_StageFn below) -------------------------------------

def _fwd_raw(x, Wc, d, scale, shift, residual, relu):
    flags = (EPI_AFFINE if scale is not None else 0) | (EPI_RESIDUAL if residual is not None else 0) \
        | (EPI_RELU if relu else 0)
    y = empty_nhwc((d.N, d.K, d.P, d.Q), x.device)
    _lib.call('mrcnn_conv2d_fwd', ctx_desc(d), _lib.ptr(x), _lib.ptr(Wc), None, _lib.ptr(scale),
              _lib.ptr(shift), _lib.ptr(residual), _lib.ptr(y), flags, _lib.ptr(split_ws(x.device)),
              _lib.stream_ptr())
    return y


def _flip_transpose(Wc, d, row_scale, out):
    _lib.call('mrcnn_filter_flip_transpose', _lib.ptr(Wc), _lib.ptr(out), d.K, d.R, d.S, d.C,
              _lib.ptr(row_scale), _lib.stream_ptr())
    return out


def _stage_transposes(blocks, device):
    """Flipped / transposed filters of every stride-1 convolution of a stage, built by ONE
    launch into one buffer.  ``blocks``: one ``_StageBlock`` per bottleneck (the affine scales
    s3 / s4 are folded into conv3 / conv4).  Returns a dict {'1','2','3','4'} -> flat tensor
    per block."""
    jobs = []
    for bi, b in enumerate(blocks):
        for key, W, d, sc in (('1', b.W1, b.d1, None), ('2', b.W2, b.d2, None),
                              ('3', b.W3, b.d3, b.s3), ('4', b.W4, b.d4, b.s4)):
            if W is not None and _uses_transposed_dgrad(d) and not uses_winograd(d):
                jobs.append((bi, key, nhwc(W), d, sc))
    out = [dict() for _ in blocks]
    if not jobs:
        return out
    total = sum(j[2].numel() for j in jobs)
    buf = torch.empty((total,), dtype=torch.float32, device=device)
    n = len(jobs)
    vp, ci = ctypes.c_void_p * n, ctypes.c_int * n
    w, wT, sc = vp(), vp(), vp()
    K, R, S, C = ci(), ci(), ci(), ci()
    off = 0
    for i, (bi, key, Wc, d, scale) in enumerate(jobs):
        t = buf[off:off + Wc.numel()]
        off += Wc.numel()
        out[bi][key] = t
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
        _lib.call('mrcnn_conv2d_dgrad_wt', ctx_desc(d), _lib.ptr(g), _lib.ptr(wT), _lib.ptr(gx),
                  EPI_ACCUM if accum else 0, _lib.ptr(res_g), _lib.ptr(res_y), _lib.ptr(out_mask_y),
                  _lib.ptr(out_scale), _lib.ptr(split_ws(g.device)), _lib.stream_ptr())
        return gx
    if fold_scale is not None:
        raise ValueError('dgrad: fold_scale needs the forward form (stride-1 square filters or '
                         '1x1 / pad 0), got %dx%d / stride %d / pad %d' % (d.R, d.S, d.stride, d.pad))
    _lib.call('mrcnn_conv2d_dgrad_ex', ctx_desc(d), _lib.ptr(g), _lib.ptr(Wc), _lib.ptr(gx),
              EPI_ACCUM if accum else 0, _lib.ptr(res_g), _lib.ptr(res_y), _lib.ptr(out_mask_y),
              _lib.ptr(out_scale), _lib.ptr(split_ws(g.device)), _lib.stream_ptr())
    return gx


# ---- Winograd F(4x4,3x3) path (csrc/conv_winograd.h) ------------------------------------------
# The RoI head's 3x3 convolutions run on ~1000 maps of 7x7: padded to 8x8 that is four 4x4
# output tiles per map, 144 multiply-adds per (map, c, k) instead of the direct form's 441.
# Selected for 3x3 / stride 1 / pad 1 layers over many small maps; the backbone's large maps keep
# the implicit-GEMM kernel.  fp32 throughout; error 3.4e-6 of the tensor scale (direct: 3.5e-7),
# parity tolerance 1e-4.
USE_WINOGRAD = True
# Which layers: 3x3 / stride 1 / pad 1 with enough work per frequency plane for the 36 batched
# GEMMs to fill the GPU — the RoI head's res5 (1024 maps of 7x7, 512 -> 512), the RPN's conv1
# (1024 -> 1024) and, at inference batch sizes, res4 (256 -> 256).  Narrow layers (C < 256) and
# the two-image res4 maps of a train step stay on the implicit-GEMM kernel: their GEMMs would
# be 2-8 K slices deep and the transform passes would cost what the MFMAs save.
WINOGRAD_MIN_CHANNELS = int(_os.environ.get('MRCNN_WINO_MIN_CH', 256))
WINOGRAD_MIN_WORK = int(_os.environ.get('MRCNN_WINO_MIN_WORK', 1 << 27))          # tiles x C x K
# Which passes take the Winograd route.  Backward-data and backward-filter always do: their
# extra rounding (3e-6 of the gradient tensor's scale) is invisible next to the fp32 floor of
# the whole-graph gradients (tools/grad_floor.py: the per-layer errors against the float64 graph
# are the same with and without).  The FORWARD of a recorded (training) graph is decided per
# layer kind, by the same measurement on the random-init R-101 of tests/test_gpu_model.py:
#   * F.conv2d layers (the RPN's conv1) take it: worst layer 3.6e-4 of entries beyond 1e-4 of
#     the tensor scale, max 5.6e-4 — the same figures as with the direct forward;
#   * the fused stages (res5 in the RoI head) do NOT.  The forward difference itself is benign
#     (Winograd vs direct output: rms 9e-7, max 3e-6 of the output scale at every head layer of
#     both test nets, activations max/rms 7-11: tools/exp/head_activation_stats.py), but it is
#     ten times the direct kernel's rounding, and every ReLU DOWNSTREAM of the layer (conv3 +
#     shortcut, the next blocks) sees it: ten times as many decisions of units sitting at zero
#     flip.  On the R-101 instance one such flip behind res5.b1.conv2 carries enough gradient
#     that 69 of the 512 rows of head.res5.b1.conv{1,2}.W (and a few rows of most backbone
#     layers) moved beyond 1e-4 of the tensor scale — 0.2 % of the entries where the parity
#     test allows 0.1 %.  (R-50, and the same R-101 with res5's residual branches damped like
#     res4's, pass with the forward routed: it is a lottery, lost once.)
# A routed forward inside a recorded graph asks for MRCNN_EPI_EXACT_SIGNS: outputs within the
# propagated rounding bound of zero (5 in 10^5) are recomputed as direct dot products, so the
# layer's OWN ReLU decisions agree with float64 at least as often as the direct kernel's
# (0-1 disagreements per 25 M outputs, direct kernel 4-6, plain Winograd 12-22:
# tools/exp/wino_signs.py).  That settles the RPN's conv1, behind whose ReLU there is only a 1x1
# convolution and the losses; it cannot help the ReLUs further down a fused stage.
# Without a graph (inference) every routed layer's forward takes it: only the per-op tolerance
# applies there and it holds with a 30x margin.
WINOGRAD_TRAIN_FORWARD = True         # False / 'conv2d' / 'stage' / True (both; default since round 3)


def uses_winograd(d):
    if not (USE_WINOGRAD and d.R == 3 and d.S == 3 and d.stride == 1 and d.pad == 1):
        return False
    # 'bf16x1': the direct kernel at one product per tap (9 units of matrix work per output) beats the
    # Winograd GEMMs, which always run six (36 / 16 x 6 = 13.5), and is the arithmetic asked for
    if GEMM_ARITHMETIC == 'bf16x1':
        return False
    tiles = d.N * ((d.H + 3) // 4) * ((d.W + 3) // 4)
    return min(d.C, d.K) >= WINOGRAD_MIN_CHANNELS and tiles * d.C * d.K >= WINOGRAD_MIN_WORK


def _wino_forward(kind, training):
    """Does the FORWARD of a routed layer (``uses_winograd``) take the Winograd route?  ``kind``:
    'conv2d' (F.conv2d) or 'stage' (a fused stage's conv2); ``training``: the call records a graph
    (see WINOGRAD_TRAIN_FORWARD above; without one every routed forward takes it)."""
    return WINOGRAD_TRAIN_FORWARD in (True, kind) or not training


def _wino_ws(d, device):
    return _lib.workspace(_lib.load().mrcnn_conv3x3_wino_workspace_bytes(ctx_desc(d)), device, 'wino')


# Transformed filters of inference calls, keyed by the filter tensor: valid while the tensor has
# not been written (torch bumps ``_version`` on every in-place update, the optimizer's included).
_wino_u_cache = {}


# ---- arithmetic of the convolution GEMMs ----------------------------------------------------
# 'split_bf16x3' (default since round 4): every fp32 operand element is split EXACTLY into three
# bf16 values (8 + 8 + 8 significand bits) while it is staged, and a K step runs six bf16 MFMAs
# (hi*hi, hi*mid, mid*hi, mid*mid, hi*lo, lo*hi) with fp32 accumulation; the three dropped cross
# terms (mid*lo, lo*mid, lo*lo) are <= 2^-24 of a product each, <= 2^-23 in total — the size of ONE
# fp32 rounding — so the result carries the error of an fp32 GEMM (tests/test_gpu_split_bf16.py measures it against float64 next to the fp32-MFMA
# kernels': smaller on every case) at 2.7x the matrix-pipe rate (gfx950 has no TF32 / xf32 and its
# fp32 MFMA runs at 1/16 of the bf16 rate).  Covers the forward-form kernels (forward, stride-1 data
# gradient, the Winograd per-frequency GEMMs) and the 128x128 weight gradient; the strided data
# gradient, the position-major and the 64x64 weight gradient stay on fp32 MFMA.
# 'fp32': v_mfma_f32_32x32x2_f32 everywhere (the default up to round 3; bench.py reports it as
# `fp32_mfma`).
# 'split_bf16x2' / 'bf16x1': the same kernels staging two planes / one plane and issuing three
# products / one product per K step ("split_planes" knob; csrc/conv_gemm_kernel.h, NP): reduced
# precision on request — 16-bit-class operands (tighter than the TF32 the reference's cuDNN uses by
# default) and plain bf16 operands.  Same launch plan, same K order, fp32 accumulation and storage.
DEFAULT_GEMM_ARITHMETIC = 'split_bf16x3'
GEMM_ARITHMETIC = DEFAULT_GEMM_ARITHMETIC
# name -> (split_bf16, split_planes) of mrcnn_set_tuning
GEMM_ARITHMETICS = {'fp32': (0, 3), 'split_bf16x3': (3, 3), 'split_bf16x2': (3, 2), 'bf16x1': (3, 1)}
SPLIT_GEMM_ARITHMETICS = ('split_bf16x3', 'split_bf16x2', 'bf16x1')     # the split-operand kernel family


def set_gemm_arithmetic(kind):
    """Select 'split_bf16x3' (default) or 'fp32' for the convolution GEMM kernels (process-wide).

    Operand range of 'split_bf16x3' (bf16 has fp32's exponent range, so nothing is rescaled):
    * finite elements up to bf16's largest value (3.3895e38; |x| <= 0.99 FLT_MAX is safe) split
      exactly, whatever mix of magnitudes a K row or a tile holds (per element, no shared exponent);
    * an element that is NaN, +-inf or finite but beyond that value (it rounds to +-inf in bf16)
      makes EVERY output that reads it NaN — fp32 multiplication would give +-inf for the
      infinities; outputs that do not read it are unaffected;
    * parts of an element below 2^-126 may be flushed to zero: the error of an element's
      representation is < 3 x 2^-126 in absolute terms (relative to elements below ~1e-33 that is
      more than an fp32 rounding).
    Asserted by tests/test_gpu_split_bf16.py (device) and tests/test_split_arithmetic_cpu.py (model).

    'split_bf16x2' and 'bf16x1' run the same kernels on fewer planes of the same split
    (x = hi + mid + lo; hi = bf16(x), mid = bf16(x - hi)), fp32 accumulation and fp32 storage as ever:
    * 'split_bf16x2' multiplies hi + mid of each operand (16 significand bits) as hi*hi + hi*mid +
      mid*hi: an error of about 3 x 2^-16 of sum |a||b| per output, half the matrix-pipe work;
    * 'bf16x1' multiplies hi of each operand (8 significand bits), the single bf16 product of mixed
      precision: about 2^-7 of sum |a||b| per output, one sixth of the matrix-pipe work.
    Epilogue operands (bias, scale, shift, residual, masks) are never rounded.  Kernels that run fp32
    MFMA under 'split_bf16x3' (strided data gradient, position-major and 64x64 weight gradient) do
    so under every name.  The Winograd route (``uses_winograd``) always runs three planes — its
    transforms amplify operand rounding; it stays on under 'split_bf16x2' and is switched OFF
    under 'bf16x1', where the direct 3x3 kernel at one product per tap is both cheaper and the
    arithmetic that was asked for.  (The library knob alone, ``MRCNN_TUNE=split_planes=1``, does
    not change the route: routed layers then still run Winograd on three planes.)
    Operand range: the finite ranges and the flushing of 'split_bf16x3' apply (one or two parts
    instead of three).  A NaN operand gives NaN.  An infinite operand, or a finite one beyond
    3.3895e38, gives NaN under 'split_bf16x2' (mid = inf - inf) as under 'split_bf16x3', but under
    'bf16x1' hi = +-inf is the only plane and the outputs that read it are +-inf as in IEEE
    multiplication (NaN where it meets a zero or an infinity of the other sign).  Asserted by
    tests/test_gpu_arithmetic_ladder.py."""
    global GEMM_ARITHMETIC
    if kind not in GEMM_ARITHMETICS:
        raise ValueError('gemm arithmetic must be one of %s, got %r' % (', '.join(map(repr, GEMM_ARITHMETICS)), kind))
    split_bf16, planes = GEMM_ARITHMETICS[kind]
    _lib.load()                                     # (a library that cannot be loaded changes nothing)
    _lib.set_tuning('split_planes', planes)
    _lib.set_tuning('split_bf16', split_bf16)
    GEMM_ARITHMETIC = kind
    _wino_u_cache.clear()                           # the route may change with the name: no stale filters


def weights_changed():
    """Public invalidation call: parameters were written outside torch's version tracking — the
    SGD kernel updates the flat arena through a raw pointer; user code that writes through
    ``p.data`` (``p.data.copy_``, ``np.copyto`` on a mapped array, ``load_state_dict(assign=
    True)``) does not bump ``_version`` either.  Drops every cached transformed filter; the
    serializers call it, and so must any other out-of-band writer."""
    _wino_u_cache.clear()
    _proj_cache.clear()


# The cache has no cross-stream ordering: an entry is produced and read on the caller's current
# stream and freed by ``weights_changed`` (every SGD step).  Work queued on a SIDE stream (the
# frozen-prefix prefetch of models/resnet_extractor.py) therefore bypasses it.
_WINO_CACHE_BYPASS = 0


class no_filter_cache(object):
    """``with no_filter_cache(): ...`` — Winograd convolutions inside transform their filter per call
    instead of reading / filling the per-parameter cache (for work on a stream other than the one
    the cache's entries live on)."""

    def __enter__(self):
        global _WINO_CACHE_BYPASS
        _WINO_CACHE_BYPASS += 1

    def __exit__(self, *exc):
        global _WINO_CACHE_BYPASS
        _WINO_CACHE_BYPASS -= 1
        return False


def _cached_filter_transform(W, Wc, d):
    key = id(W)
    hit = _wino_u_cache.get(key)
    # identity + version + storage address: ``p.data = t`` / ``assign=True`` loads swap the
    # storage without touching the version counter
    if hit is not None and hit[0] is W and hit[1] == W._version and hit[3] == W.data_ptr() \
            and hit[2].device == Wc.device:
        return hit[2]
    u = torch.empty((_lib.load().mrcnn_conv3x3_wino_u_bytes(ctx_desc(d)) // 4,),
                    dtype=torch.float32, device=Wc.device)
    _lib.call('mrcnn_conv3x3_wino_filter', ctx_desc(d), _lib.ptr(Wc), _lib.ptr(u), _lib.stream_ptr())
    _wino_u_cache[key] = (W, W._version, u, W.data_ptr())
    return u


def wino_fwd(x, Wc, d, scale, shift, relu, keep_v=False, cache_for=None, exact_signs=False):
    """y = relu?(affine?(conv3x3(x))) — ``scale`` None with a ``shift``: plain bias — and, with
    ``keep_v``, the transformed input (36, tiles, C) for the weight gradient.  ``cache_for``: the
    parameter tensor ``Wc`` was taken from; its transformed filter is then built once and reused
    until the parameter is written (inference).  ``exact_signs``: outputs within the Winograd
    rounding bound of zero are recomputed directly (MRCNN_EPI_EXACT_SIGNS)."""
    flags = (EPI_AFFINE if scale is not None else (EPI_BIAS if shift is not None else 0)) \
        | (EPI_RELU if relu else 0) | (EPI_EXACT_SIGNS if exact_signs else 0)
    y = empty_nhwc((d.N, d.K, d.P, d.Q), x.device)
    v = None
    if keep_v:
        v = torch.empty((_lib.load().mrcnn_conv3x3_wino_v_bytes(ctx_desc(d)) // 4,),
                        dtype=torch.float32, device=x.device)
    u = _cached_filter_transform(cache_for, Wc, d) \
        if cache_for is not None and not _WINO_CACHE_BYPASS else None
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


# ---- weight-gradient side stream -----------------------------------------------------------
# dgrad and wgrad of a convolution are independent given the incoming gradient.  The wgrad
# launches of a bottleneck go to a second HIP stream so that their workgroups fill the CUs
# that the tail round of the concurrently running dgrad leaves idle (and vice versa): with
# 128x128 tiles and 512 resident workgroups a single kernel wastes up to a round at its end.
# (The stream itself: streams.wgrad_stream.)


# ---- weight gradients deferred into the next step's proposal window --------------------------
# Between the RPN convolution and the RoI head of a train step the GPU is nearly idle: the
# proposal kernels (top-k, NMS scan: two workgroups) run, then the host samples the RoIs
# (~2 ms together).  The RoI head's weights are not read before that window has passed, so the
# weight gradients of some head layers — and the SGD update of exactly those parameters — can be
# held back at the end of a step and run INSIDE the next step's window on a second stream, where
# they cost nothing (optimizers.MomentumSGD.defer_weight_gradients; same gradients, same update,
# applied before the parameter is read again: results are bit-identical).
class WgradJob(object):
    """One weight gradient: ``gW`` = backward-filter of descriptor ``d`` from the input ``x`` and
    the output gradient ``g`` (rows scaled by ``row_scale`` if given).  ``wino``: on the Winograd
    route, from the raw input ``x`` or the forward's kept transform ``v`` (the other is None)."""

    def __init__(self, d, x, g, gW, row_scale=None, wino=False, v=None):
        self.d, self.x, self.g, self.gW = d, x, g, gW
        self.row_scale, self.wino, self.v = row_scale, wino, v

    def launch(self):
        """On the current stream (``_lib.workspace`` keys the scratch on it: two streams never
        share a buffer)."""
        if self.wino:
            wino_wgrad_into(self.d, self.x, self.v, self.g, self.gW, self.row_scale)
        else:
            _launch_wgrad(self.d, self.x, self.g, self.gW, self.row_scale)

    def tensors(self):
        """The operands a held-back job keeps alive."""
        return [t for t in (self.x, self.g, self.gW, self.row_scale, self.v) if t is not None]


class DeferQueue(object):
    """``jobs``: one ``WgradJob`` per held-back weight gradient of the parameters ``params``.
    MomentumSGD.update hangs one on the parameter arena (``ParamArena.defer``) around backward."""

    def __init__(self, params):
        self.ids = set(id(p) for p in params)
        self.jobs = []

    def grad_ptrs(self):
        """Addresses of the gradient buffers the held-back jobs will write."""
        return set(j.gW.data_ptr() for j in self.jobs)


def run_deferred_wgrads(jobs):
    """Launch the held-back weight gradients on the current stream (the caller selects it)."""
    for job in jobs:
        job.launch()


def _launch_wgrad(d, x, g, gW, row_scale=None, ex=True):
    """The implicit-GEMM weight gradient into the buffer ``gW``, on the current stream.  ``ex``
    False: the plain entry point (no ``row_scale``)."""
    ws = _lib.workspace(_lib.load().mrcnn_conv2d_wgrad_workspace_bytes(ctx_desc(d)), g.device, 'wgrad')
    tail = (_lib.ptr(row_scale), _lib.stream_ptr()) if ex else (_lib.stream_ptr(),)
    _lib.call('mrcnn_conv2d_wgrad_ex' if ex else 'mrcnn_conv2d_wgrad', ctx_desc(d), _lib.ptr(x),
              _lib.ptr(g), _lib.ptr(gW), _lib.ptr(ws), *tail)


def _wgrad(d, x, g, W, side=None, row_scale=None, wino=False, v=None):
    """Weight gradient of parameter ``W``; returns the tensor autograd should see for W (None when
    written in place or held back in the defer queue).  ``wino`` / ``v``: see ``WgradJob``.  With
    ``side`` (a stream) the launch is queued there, ordered after everything queued so far on the
    current stream; only arena-backed (direct) gradients may use it."""
    gW, result = _grad_target(W)
    job = WgradJob(d, x, g, gW, row_scale, wino, v)
    direct = result is None
    # (direct: the arena slot was claimed, so the arena exists and answers the rest of the question)
    defer = W._arena.defer if direct else None
    if defer is not None and id(W) in defer.ids:
        defer.jobs.append(job)
    elif direct and side is not None:
        side.wait_stream(torch.cuda.current_stream(g.device))
        for t in (x, g):
            t.record_stream(side)
        with torch.cuda.stream(side):
            job.launch()
    else:
        job.launch()
    return result


# ---------------------------------------------------------------------------------------
# Whole-stage op: chainer BuildingBlock (BottleneckA + n x BottleneckB) as ONE autograd node.
# Forward = 3 (4) fused implicit-GEMM launches per block; backward = 3 (4) dgrad + 3 (4) wgrad
# launches per block and nothing else: every gradient tensor inside the stage is written ALREADY
# multiplied by the ReLU mask (and affine scale) of the conv that consumes it — in the epilogue
# of the dgrad that produces it — and the identity-shortcut gradient is added there too, so none
# of the stage's backward GEMMs stages a mask: they all run the 168-register kernels, three
# workgroups per CU.  Only the gradient entering the stage from autograd takes one elementwise
# masking pass.
# ---------------------------------------------------------------------------------------
# Weight gradients of the backbone's small-M layers (<= 40 000 output pixels: res3 / res4) are
# queued on a second HIP stream: such a launch has only 2-4 workgroups per CU, so the wgrad and
# the next dgrad share the GPU (same-box A/B: 54.4 -> 54.0 ms per step).  For the large res5
# launches the same trick measured no overlap (round 1: 68.9 vs 68.1 ms per step).
SMALL_WGRAD_MAX_PIXELS = int(_os.environ.get('MRCNN_SIDE_WGRAD_MAX_PIXELS', 40000))


# ---- pooling AFTER res5.a's 1x1 projections ("projected pooling") --------------------------------
# The RoI head applies ROIAlign to the C4 feature map and then res5 (models/mask_rcnn_resnet.py:
# 168-176), whose first block reads the pooled map only through two 1x1 convolutions (conv1 and the
# shortcut conv4, each followed by AffineChannel2D).  ROIAlign is linear over positions per channel
# with no constant term, a bias-free 1x1 convolution is linear over channels per position: they
# commute exactly,
#     bn(conv1x1(roi_align(x))) == bn(roi_align(conv1x1(x))),
# so both projections run on the N*H*W map pixels (2 x 51 x 84 = 8 568 at the C2 shape) instead of
# the R*7*7 pooled ones (50 176), and ROIAlign pools their 512- / 2048-channel outputs with the
# affine (+ ReLU) in its epilogue.  Backward likewise: ROIAlign's adjoint first, then data and
# weight gradient of the projections on the map.  Same sums in a different order (fp32 rounding
# only); PROJECTED_POOLING = False restores the reference order.
PROJECTED_POOLING = _os.environ.get('MRCNN_PROJECTED_POOLING', '1') != '0'


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


# The projections of one feature map, kept while the SAME map is pooled again without a graph
# (inference runs the head once per image and once per mask group on one batch's map): the map
# tensor itself is held so that its identity cannot be recycled; ``weights_changed`` drops the entry.
_proj_cache = {}


def projected_map(x, W1, W4):
    """(conv1x1(x, W1), conv1x1(x, W4)) of an NHWC map, bias-free and without epilogue — the inputs
    ``RoiSpec(proj=)`` takes.  Cached per (map, filters) while autograd is off."""
    _lib.require_device(x, W1, W4)
    x = nhwc(x, torch.float32, 'projected_map')
    key = (id(x), x._version, x.data_ptr(), tuple(x.shape), id(W1), W1._version, W1.data_ptr(),
           id(W4), W4._version, W4.data_ptr())
    hit = _proj_cache.get('entry')
    if hit is not None and hit[0] == key:
        return hit[2], hit[3]
    d1 = make_desc(x.shape, W1.shape, 1, 0)
    d4 = make_desc(x.shape, W4.shape, 1, 0)
    z1 = _fwd_raw(x, nhwc(W1, torch.float32, 'projected_map', 'W1'), d1, None, None, None, False)
    z4 = _fwd_raw(x, nhwc(W4, torch.float32, 'projected_map', 'W4'), d4, None, None, None, False)
    _proj_cache['entry'] = (key, x, z1, z4)
    return z1, z4


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


def _pool_bwd_alone(side, device):
    """The compute stream waits for the weight-gradient side stream before a pixel-owner ROIAlign
    backward inside a stage.  Round 6 finding (tests/test_gpu_model.py::test_training_is_bit_
    reproducible_run_to_run on the small test model, whose RoI head is small enough to use the side
    stream): with the weight-gradient GEMM of the SAME block running on the side stream — it reads the
    gradient tensor the ROIAlign backward reads, written by the data-gradient GEMM just before — a
    launch now and then lost ONE list entry's contribution in ONE component of 16 lanes (a handful
    of gx elements, different from run to run; captured and analysed on the host: inputs and tables
    identical, the sum short of exactly one term).  The same two kernels side by side in isolation
    (900 launches, the captured tensors included) never did; neither kernel uses scratch; four
    plain v_fma_f32 instead of the packed FMAs change nothing.  Two measures, either of which removes
    it on its own (each 8 of 8 runs clean): the pooled backward of a block is queued BEFORE that
    block's weight gradients go to the side stream (no second reader of its input is in flight), and
    the streams are serialised here.  Costs nothing at full size (the head's weight gradients do not
    use the side stream there), ~20 us in the small configurations that do.  Root cause not found."""
    if side is not None:
        torch.cuda.current_stream(device).wait_stream(side)


class _StageBlock(object):
    """One bottleneck of a stage node, built once by ``_StageFn.forward``: the filters W1..W4 with
    their affine vectors s* / b* (conv4's are None without a projection shortcut), the
    descriptors d1..d4 (d4 None likewise) and ``i1..i4``, the index of each filter among
    ``forward``'s inputs — that of its flag in ``needs_input_grad`` and of its gradient in what
    ``backward`` returns."""

    def __init__(self, params, at, has_proj):
        """From forward's flat ``params``, this block's starting at ``params[at]``."""
        self.n_params = 12 if has_proj else 9
        (self.W1, self.s1, self.b1, self.W2, self.s2, self.b2,
         self.W3, self.s3, self.b3) = params[at:at + 9]
        self.W4, self.s4, self.b4 = params[at + 9:at + 12] if has_proj else (None, None, None)
        for name in ('W1', 'W2', 'W3', 'W4', 's1', 'b1', 's2', 'b2', 's3', 'b3', 's4', 'b4'):
            t = getattr(self, name)
            if t is None:
                continue
            if t.dtype != torch.float32:
                raise TypeError('building_block: %s must be %s, got %s' % (name, torch.float32, t.dtype))
            if name[0] != 'W':      # (the filters go through nhwc() where they are read)
                setattr(self, name, _lib.dense(t, torch.float32, 'building_block', name, align=True))
        w1 = _StageFn.FIXED_INPUTS + at
        self.i1, self.i2, self.i3, self.i4 = w1, w1 + 3, w1 + 6, w1 + 9
        self.d1 = self.d2 = self.d3 = self.d4 = None


# The activations of one bottleneck that backward reads: its input and its three ReLU outputs.
_StageActs = collections.namedtuple('_StageActs', 'x h1 h2 y')


def _save_stage(ctx, x, acts, wino_v):
    """Saved tensors of a stage node: the input, (h1, h2, y) per block, then the kept Winograd
    input transforms (``wino_v[i]`` of block i, or None)."""
    ctx.wino_slots = [i for i, v in enumerate(wino_v) if v is not None]
    ctx.save_for_backward(x, *([t for a in acts for t in a] + [wino_v[i] for i in ctx.wino_slots]))


def _saved_stage(ctx):
    """Inverse of ``_save_stage``: ([_StageActs per block], {block index: kept transform})."""
    saved = ctx.saved_tensors
    acts, xin = [], saved[0]
    for i in range(len(ctx.blocks)):
        acts.append(_StageActs(xin, *saved[1 + 3 * i:4 + 3 * i]))
        xin = acts[-1].y
    return acts, dict(zip(ctx.wino_slots, saved[1 + 3 * len(acts):]))


class _StageFn(torch.autograd.Function):

    # inputs of forward in front of *params (x .. records_graph): a change of the signature below
    # changes this number, and nothing else
    FIXED_INPUTS = 8

    @staticmethod
    def forward(ctx, x, strides, proj, poll, tail_rows, tail_slot, roi, records_graph, *params):
        """``roi`` (a ``RoiSpec`` or None): with it ``x`` is the FEATURE MAP and block 0 (which must
        have a projection shortcut) runs its two 1x1 convolutions on the map and pools their outputs
        (projected pooling, see above) — the stage then equals ``stage(roi_align(x, roi))``.
        ``strides[i]`` / ``proj[i]``: conv1(/conv4) stride and has-projection flag of block
        i; ``poll``: optional callable invoked during backward at the stage's entry and after
        every block's weight gradients have been queued (parallel.DataParallelGradSync launches
        the gradient buckets that are complete); ``tail_rows``: None, or an int64 index tensor —
        the node then returns ``(average_pooling(y) (N,C,1,1), y[tail_rows])`` instead of the
        stage output y (the RoI head's two consumers of res5, models/mask_rcnn_resnet.py:186-195),
        and its backward forms the gradient entering the last block from both in ONE pass,
        ReLU mask included (``mrcnn_head_tail_bwd``); ``tail_slot``: the int32 table row -> position
        among ``tail_rows`` (-1 elsewhere), None = built here; ``records_graph``: torch.is_grad_enabled()
        at the call (in here grad mode is always off and ctx.needs_input_grad reports the inputs'
        requires_grad flags even under torch.no_grad()); ``params``: per block
        W1,s1,b1,W2,s2,b2,W3,s3,b3 (+ W4,s4,b4 when proj[i])."""
        assert len(ctx.needs_input_grad) == _StageFn.FIXED_INPUTS + len(params)
        _lib.require_device(x, tail_rows, tail_slot, *params)
        x = nhwc(x, torch.float32, 'building_block')
        if tail_rows is not None and tail_rows.dtype != torch.int64:
            raise TypeError('building_block: tail_rows must be %s, got %s' % (torch.int64, tail_rows.dtype))
        if tail_slot is not None:
            tail_slot = _lib.dense(tail_slot, torch.int32, 'building_block', 'tail_slot')
        ng = ctx.needs_input_grad
        training = records_graph and any(ng)
        blocks, at = [], 0
        for pj in proj:
            blocks.append(_StageBlock(params, at, pj))
            at += blocks[-1].n_params
        if roi is not None:
            if roi.proj is not None and training:
                raise ValueError('RoiSpec(proj=) is for graph-free calls (the projections would be '
                                 'outside the recorded graph)')
            a = blocks[0]
            if not (a.W4 is not None and strides[0] == 1 and a.W1.shape[2] == 1 and a.W4.shape[2] == 1):
                raise ValueError('projected pooling needs a first block with 1x1 conv1 / conv4 at stride 1 '
                                 '(the RoI bins of the stride are selected by RoiSpec.bin_stride)')
        acts, wino_v = [], []
        h = x
        for b, stride in zip(blocks, strides):
            pooled_here = roi is not None and b is blocks[0]
            b.d1 = make_desc(h.shape, b.W1.shape, stride, 0)
            if pooled_here:
                # conv1 on the map, then pooled with bn1 + ReLU in ROIAlign's epilogue
                z1 = roi.proj[0] if roi.proj is not None else _fwd_raw(h, nhwc(b.W1), b.d1, None, None, None, False)
                h1 = _roi_pool_affine(z1, roi, b.s1, b.b1, True)
                del z1
            else:
                h1 = _fwd_raw(h, nhwc(b.W1), b.d1, b.s1, b.b1, None, True)
            b.d2 = make_desc(h1.shape, b.W2.shape, 1, 1)
            v2 = None
            if uses_winograd(b.d2) and _wino_forward('stage', training):
                # (with a weight gradient to come, the transformed input is kept for it)
                h2, v2 = wino_fwd(h1, nhwc(b.W2), b.d2, b.s2, b.b2, True,
                                  keep_v=training and bool(ng[b.i2]),
                                  cache_for=None if training else b.W2,
                                  exact_signs=training)
            else:
                h2 = _fwd_raw(h1, nhwc(b.W2), b.d2, b.s2, b.b2, None, True)
            if b.W4 is None:
                shortcut = h
            else:
                b.d4 = make_desc(h.shape, b.W4.shape, stride, 0)
                if pooled_here:
                    z4 = roi.proj[1] if roi.proj is not None else _fwd_raw(h, nhwc(b.W4), b.d4, None, None, None, False)
                    shortcut = _roi_pool_affine(z4, roi, b.s4, b.b4, False)
                    del z4
                else:
                    shortcut = _fwd_raw(h, nhwc(b.W4), b.d4, b.s4, b.b4, None, False)
            b.d3 = make_desc(h2.shape, b.W3.shape, 1, 0)
            y = _fwd_raw(h2, nhwc(b.W3), b.d3, b.s3, b.b3, shortcut, True)
            if RELU_TAP is not None:
                RELU_TAP.append(('block', (h1, h2, y)))
            acts.append((h1, h2, y))
            wino_v.append(v2)
            h = y
        ctx.blocks = blocks
        ctx.poll = poll
        ctx.roi = roi
        _save_stage(ctx, x, acts, wino_v)
        ctx.tail = tail_rows is not None
        if ctx.tail:
            # the two consumers of the stage output, produced here so that backward receives
            # their gradients separately (h itself is not an output of the node)
            R_, C_ = h.shape[0], h.shape[1]
            pooled = torch.empty((R_, C_), dtype=torch.float32, device=h.device)
            _lib.call('mrcnn_avgpool_fwd', _lib.ptr(h), _lib.ptr(pooled), R_, h.shape[2] * h.shape[3],
                      C_, _lib.stream_ptr())
            sub = h.permute(0, 2, 3, 1).index_select(0, tail_rows).permute(0, 3, 1, 2)
            if tail_slot is None:
                tail_slot = torch.full((R_,), -1, dtype=torch.int32, device=h.device)
                tail_slot[tail_rows] = torch.arange(tail_rows.numel(), dtype=torch.int32, device=h.device)
            ctx.tail_slot = tail_slot
        if ctx.tail:
            return pooled.reshape(R_, C_, 1, 1), sub
        return h

    @staticmethod
    def backward(ctx, gy, g_rows=None):
        acts, wino_v = _saved_stage(ctx)
        blocks = ctx.blocks
        ng = ctx.needs_input_grad
        grads = [None] * len(ng)
        poll = ctx.poll
        if poll is not None:
            poll()                 # everything upstream of this stage has queued its gradients
        if not ctx.tail:
            gy = nhwc(gy)
        # small-M layers (backbone stages) leave CUs idle: their weight gradients go to a
        # second stream so that they can share the GPU with the next dgrad
        d_top = blocks[-1].d3
        dev_ = gy.device if gy is not None else g_rows.device
        side = wgrad_stream(dev_) if d_top.N * d_top.P * d_top.Q <= SMALL_WGRAD_MAX_PIXELS else None
        # all the stage's filter transposes in one launch (built during the forward on the side
        # stream instead, they measured no faster: 53.2 vs 53.0 ms per step)
        stage_wT = _stage_transposes(blocks, dev_)
        # gm: gradient w.r.t. the block output, already through that output's ReLU
        y_top = acts[-1].y
        if ctx.tail:
            R_, C_, Hh, Ww = y_top.shape
            if gy is None:
                gy = torch.zeros((R_, C_), dtype=torch.float32, device=dev_)
            gp = _lib.dense(gy.reshape(R_, C_), torch.float32, 'building_block', 'the pooled gradient',
                            align=True)
            gr = nhwc(g_rows) if g_rows is not None else None
            gm = empty_nhwc((R_, C_, Hh, Ww), dev_)
            _lib.call('mrcnn_head_tail_bwd', _lib.ptr(gp), _lib.ptr(gr),
                      _lib.ptr(ctx.tail_slot) if gr is not None else None, _lib.ptr(y_top),
                      _lib.ptr(gm), R_, Hh * Ww, C_, _lib.stream_ptr())
        else:
            gm = epilogue_bwd(gy, y_top, None)
        for i in range(len(blocks) - 1, -1, -1):
            b, wT = blocks[i], stage_wT[i]
            x, h1, h2, _ = acts[i]
            first = i == 0
            pooled_here = first and ctx.roi is not None
            need_w4 = b.W4 is not None and ng[b.i4]
            # what the gradient leaving this block must be masked with: the previous block's
            # output ReLU (= this block's input); the stage input belongs to someone else
            xm = None if first else x
            # the gradient the shortcut's conv4 reads: the block output's, or with pooling ...
            g4 = gm
            if pooled_here and (need_w4 or ng[0]):
                # ... that gradient back on the map (ROIAlign's adjoint commutes with the
                # per-channel scale s4, which stays folded into conv4's filter / gradient rows).
                # Queued BEFORE this block's weight gradients go to the side stream, and with the side
                # stream drained: see _pool_bwd_alone.
                _pool_bwd_alone(side, dev_)
                g4 = _roi_pool_bwd(gm, ctx.roi, (x.shape[0], b.d4.K, x.shape[2], x.shape[3]))
            if ng[b.i3]:
                grads[b.i3] = _wgrad(b.d3, h2, gm, b.W3, side, row_scale=b.s3)
            if need_w4:
                grads[b.i4] = _wgrad(b.d4, x, g4, b.W4, side, row_scale=b.s4)
            gh2 = _dgrad_raw(b.d3, gm, nhwc(b.W3), fold_scale=b.s3, out_mask_y=h2, out_scale=b.s2,
                             wT=wT.get('3'))
            if uses_winograd(b.d2):
                if ng[b.i2]:
                    v2 = wino_v.get(i)
                    grads[b.i2] = _wgrad(b.d2, h1 if v2 is None else None, gh2, b.W2, wino=True, v=v2)
                gh1 = wino_dgrad(b.d2, gh2, nhwc(b.W2), out_scale=b.s1, out_mask_y=h1)
            else:
                if ng[b.i2]:
                    grads[b.i2] = _wgrad(b.d2, h1, gh2, b.W2, side)
                gh1 = _dgrad_raw(b.d2, gh2, nhwc(b.W2), out_mask_y=h1, out_scale=b.s1, wT=wT.get('2'))
            if pooled_here and (ng[b.i1] or ng[0]):
                _pool_bwd_alone(side, dev_)
                gh1 = _roi_pool_bwd(gh1, ctx.roi, (x.shape[0], b.d1.K, x.shape[2], x.shape[3]))
            if ng[b.i1]:
                grads[b.i1] = _wgrad(b.d1, x, gh1, b.W1, side)
            if poll is not None:
                poll()             # this block's weight gradients are queued
            if first and not ng[0]:
                break
            if b.W4 is None:
                gm = _dgrad_raw(b.d1, gh1, nhwc(b.W1), res_g=gm, out_mask_y=xm, wT=wT.get('1'))
                continue
            # projection shortcut: both data gradients into one buffer; the input's ReLU mask is
            # fused into the second where conv1 has stride 1, else applied by a pass of its own
            fused = b.d1.stride == 1
            gx = _dgrad_raw(b.d1, gh1, nhwc(b.W1), wT=wT.get('1'))
            gm = _dgrad_raw(b.d4, g4, nhwc(b.W4), fold_scale=b.s4, out=gx, accum=True,
                            out_mask_y=xm if fused else None, wT=wT.get('4'))
            if xm is not None and not fused:
                gm = epilogue_bwd(gm, xm, None)
        if ng[0]:
            grads[0] = gm
        return tuple(grads)


def building_block(x, blocks, first_stride=None, poll=None, tail_rows=None, roi=None, tail_slot=None):
    """A chain of Bottleneck links (chainer BuildingBlock) as one fused autograd node.  With
    ``tail_rows`` (int64 row indices) it returns ``(average_pooling_2d(y, map size), y[tail_rows])``
    instead of y (``tail_slot``: their optional slot table) — see _StageFn.forward.  With ``roi``
    (a ``RoiSpec``) ``x`` is the feature map and the result is ``building_block(roi_align(x, roi), ...)`` (projected pooling)."""
    strides, proj, params = [], [], []
    for i, b in enumerate(blocks):
        strides.append(b.conv1.stride if not (i == 0 and first_stride is not None) else first_stride)
        proj.append(bool(b.projection))
        params += [b.conv1.W, b.bn1.W, b.bn1.b, b.conv2.W, b.bn2.W, b.bn2.b,
                   b.conv3.W, b.bn3.W, b.bn3.b]
        if b.projection:
            params += [b.conv4.W, b.bn4.W, b.bn4.b]
    return _StageFn.apply(x, tuple(strides), tuple(proj), poll, tail_rows, tail_slot, roi,
                          torch.is_grad_enabled(), *params)
