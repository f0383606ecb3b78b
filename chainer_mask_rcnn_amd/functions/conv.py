"""Convolution / deconvolution / linear ops on the fp32-MFMA implicit-GEMM kernel.

Host-side mirror of chainer's ``L.Convolution2D`` (+ the ``AffineChannel2D``,
residual add and ReLU that follow it inside chainer's Bottleneck blocks),
``L.Deconvolution2D(k=2, s=2)`` and ``L.Linear`` as the reference uses them
(the reference's models/region_proposal_network.py:75-80,
models/mask_rcnn_resnet.py:131-143).  Tensors carry the
reference's logical shapes — x (N,C,H,W), conv W (out,in,kh,kw), deconv W
(in,out,kh,kw), linear W (out,in) — stored channels-last, which is exactly the
NHWC / KRSC layout the HIP kernels consume.

This module decides WHICH ROUTE a layer takes — the knobs below, ``uses_winograd``, the caches
derived from weights with ``weights_changed`` — and holds the autograd nodes of the single layers.
The launches are functions/_conv_launch.py, gradient ownership is functions/_wgrad.py (both
re-exported here), the fused stage node is functions/stage.py, which reads the knobs from here.
Every knob is read at call time as an attribute of THIS module: tests, tools and the benchmark
assign them (``conv.WINOGRAD_MIN_WORK = ...``).
"""
import os as _os

import torch

from .. import _lib
from .._lib import ConvDesc
# (some of these names are not used below: tests, tools, the benchmark and the rest of the package
# reach them through this module)
from ._layout import nhwc, empty_nhwc                                           # noqa: F401
from ._conv_launch import (                                                     # noqa: F401
    make_desc, ctx_desc, split_ws, epilogue_bwd, _fwd_raw, _flip_transpose, _dgrad_raw,
    _launch_wgrad, _sparse3x3_gather, _sparse3x3_scatter, _stem_fwd, _deconv_fwd, _deconv_dgrad,
    _deconv_wgrad_into, _wino_ws, _wino_filter, _wino_fwd_raw, wino_dgrad, wino_wgrad_into,
    RoiSpec, _roi_pool_affine, _roi_pool_bwd)
from ._wgrad import _grad_target, _bias_grad, _wgrad, DeferQueue, run_deferred_wgrads   # noqa: F401


# Test hook: when set to a list, every ReLU output this module and functions/stage.py produce (fused
# conv epilogues, the three activations of each bottleneck of a fused stage, the deconvolution) is
# appended as (kind, tensor) in call order — tests/test_gpu_model.py reads the ReLU DECISIONS of
# the HIP path from it.  None (default): nothing is recorded or kept alive.
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
    n = hint.n
    patches, g_rows = _sparse3x3_gather(d, x, g, hint.rows, n)
    d1 = ConvDesc(n, 1, 1, 9 * d.C, d.K, 1, 1, 1, 0, 1, 1)
    gx = gW = gb = None
    if need_w:
        gW = _wgrad(d1, patches, g_rows, ctx.W_param)
    if need_x:
        gp = _dgrad_raw(d1, g_rows, Wc)          # (rows, 3, 3, C) patch gradients
        gx = _sparse3x3_scatter(d, gp, hint.lookup)
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
        if residual is not None:
            residual = nhwc(residual, torch.float32, 'conv2d', 'residual')
        ctx.wino = uses_winograd(d) and residual is None and (b is None or scale is None)
        if ctx.wino and _wino_forward('conv2d', records_graph and any(ctx.needs_input_grad)):
            y, _ = wino_fwd(x, Wc, d, scale, shift if scale is not None else b, relu,
                            cache_for=None if records_graph else W,
                            exact_signs=relu and records_graph)
        else:
            y = _fwd_raw(x, Wc, d, scale, shift, residual, relu, bias=b)
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
        return _stem_fwd(x4, w784, b, scale, shift)

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
        ctx.dims = (N, H, Wd, C, K)
        y = _deconv_fwd(x, Wc, b, ctx.dims, relu,
                        forward_form=DECONV_FORWARD_FORM and GEMM_ARITHMETIC in SPLIT_GEMM_ARITHMETICS)
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
            gx = _deconv_dgrad(g, Wc, ctx.dims)
        if ctx.needs_input_grad[1]:
            gWt, gW = _grad_target(ctx.W_param)
            _deconv_wgrad_into(x, g, gWt, ctx.dims)
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
    u = _wino_filter(d, Wc)
    _wino_u_cache[key] = (W, W._version, u, W.data_ptr())
    return u


def wino_fwd(x, Wc, d, scale, shift, relu, keep_v=False, cache_for=None, exact_signs=False):
    """``_conv_launch._wino_fwd_raw`` (which see) behind the filter cache.  ``cache_for``: the
    parameter tensor ``Wc`` was taken from; its transformed filter is then built once and reused
    until the parameter is written (inference)."""
    u = _cached_filter_transform(cache_for, Wc, d) \
        if cache_for is not None and not _WINO_CACHE_BYPASS else None
    return _wino_fwd_raw(x, Wc, d, scale, shift, relu, keep_v=keep_v, u=u, exact_signs=exact_signs)


# ---- knobs of the fused stage (functions/stage.py reads them from here) --------------------------
# Weight gradients of the backbone's small-M layers (<= 40 000 output pixels: res3 / res4) are
# queued on a second HIP stream: such a launch has only 2-4 workgroups per CU, so the wgrad and
# the next dgrad share the GPU (same-box A/B: 54.4 -> 54.0 ms per step).  For the large res5
# launches the same trick measured no overlap (round 1: 68.9 vs 68.1 ms per step).
SMALL_WGRAD_MAX_PIXELS = int(_os.environ.get('MRCNN_SIDE_WGRAD_MAX_PIXELS', 40000))

# Pooling AFTER res5.a's 1x1 projections ("projected pooling", described in functions/stage.py);
# False restores the reference order.
PROJECTED_POOLING = _os.environ.get('MRCNN_PROJECTED_POOLING', '1') != '0'


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
    z1 = _fwd_raw(x, nhwc(W1, torch.float32, 'projected_map', 'W1'), d1)
    z4 = _fwd_raw(x, nhwc(W4, torch.float32, 'projected_map', 'W4'), d4)
    _proj_cache['entry'] = (key, x, z1, z4)
    return z1, z4

