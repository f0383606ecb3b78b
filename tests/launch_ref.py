"""Launch checker: every call of a checked libmrcnn_hip.so entry point, compared with a float64
restatement of the same operation (include/mrcnn_hip.h, the comment next to each declaration).

``LaunchChecker.install(monkeypatch)`` wraps ``chainer_mask_rcnn_amd._lib.call`` — every library
call of ``functions/`` goes through it.  Per checked call: synchronise the device, copy the
operands out of the argument pointers (sizes from the descriptor / arguments; the output's prior
contents where the call accumulates into it), make the call, synchronise, copy the output, build
the reference in float64 with plain torch ops on the same device, compare, record, free.
Operands are read by address with a device-to-device copy, so the host pointer arrays of
mrcnn_filter_flip_transpose_batched are read like any other argument.

State carried between calls: the filter ``w`` behind a Winograd transform ``u``
(mrcnn_conv3x3_wino_filter), the input ``x`` behind a kept Winograd input transform ``v``, and
the ``w`` / ``row_scale`` behind a flipped, transposed filter ``wT``.  ``wT`` itself is compared
bit for bit; the data gradients on ``wT`` are referenced from ``w`` and ``row_scale``, so a wrong
transpose cannot cancel out.

The references themselves take and return float64 NCHW / row tensors and run on any device:
tests/test_launch_ref_cpu.py checks them against the NumPy oracle on the CPU.

Comparison (``ratio``): per element |got - ref| <= rel |ref| + floor max|ref| with the suite's
convolution bound rel = 1e-4, floor = 1e-5 (tests/test_gpu_conv.py); the recorded figure is the
worst |got - ref| / bound, a launch passes at <= 1.  Data movement and ops the header calls
same-order are compared bit for bit against an fp32 restatement (``exact``).  The losses have
bounds of their own, derived from the kernels' arithmetic in units of 2^-24 (``tol_ratio``, the
comment above ``sigmoid_ce``): a loss is one number summed over up to 2^24 terms, and the suite's
1e-4 would hide a lost element.

The device half of the target creators (csrc/targets.hip) produces integer decisions, so it is
checked in two layers (the comment above ``K_IOU``).  Arithmetic — the IoU matrix, its row and
column maxima, ``bbox2loc`` — against a float64 restatement under bounds derived from the kernels'
operation count, again in units of 2^-24: K_IOU = 16 relative for an IoU; for ``bbox2loc``
dy, dx:  u ((|src centre| + |dst centre| + (|src size| + |dst size|) / 2) / size + 3 |dy|),
dh, dw:  u (3 + |dh|), and the normalised target adds 2 u of itself; non-finite values must sit at
the reference's positions with its class and sign.  Decisions — argmax, labels, gathers, scatter
patterns, mask targets — exactly: as functions of the kernel's own fp32 values where those are
outputs, else against the NumPy fp32 restatement in the reference's operation order.  These
references are NumPy on the host (the arrays are small) and are pure functions of the operands and
outputs, so tests/test_launch_ref_cpu.py runs them on emulated kernels, right and wrong.
"""
import collections
import ctypes
import math

import numpy as np
import torch
import torch.nn.functional as F

from chainer_mask_rcnn_amd import _lib
from chainer_mask_rcnn_amd._lib import (EPI_ACCUM, EPI_AFFINE, EPI_BIAS, EPI_RELU,
                                        EPI_RESIDUAL)

F64 = torch.float64
REL, FLOOR = 1e-4, 1e-5


def _close(got, ref, rel=REL, floor=FLOOR):
    """The suite's parity bound on NumPy arrays (float64 reference)."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    scale = max(np.abs(ref).max(), 1e-6)
    excess = np.abs(got - ref) - (rel * np.abs(ref) + floor * scale)
    worst = excess.max()
    assert worst <= 0, 'element %s: got %.9g ref %.9g (scale %.3e)' % (
        np.unravel_index(excess.argmax(), excess.shape), got.flat[excess.argmax()],
        ref.flat[excess.argmax()], scale)


def ratio(got, ref, rel=REL, floor=FLOOR):
    """Worst |got - ref| / (rel |ref| + floor max|ref|) over the elements, float64 on ref's device
    (<= 1: within the bound).  Empty tensors give 0."""
    ref = ref.to(F64)
    got = got.to(device=ref.device, dtype=F64).reshape(ref.shape)
    if ref.numel() == 0:
        return 0.
    scale = max(float(ref.abs().max()), 1e-6)
    err = (got - ref).abs()
    if not bool(torch.isfinite(got).all()):
        return math.inf
    return float((err / (rel * ref.abs() + floor * scale)).max())


def exact(got, ref):
    """0 when bit-identical (fp32 restatement), inf otherwise."""
    return 0. if torch.equal(got.reshape(ref.shape), ref) else math.inf


def _same_bits(got, ref):
    """exact() on the bit patterns: untouched memory may hold NaNs."""
    return exact(got.view(torch.int32), ref.view(torch.int32))


# ---- float64 references (NCHW activations, KCRS filters, as chainer) ---------------------------

_CHUNK = 1 << 27      # elements of the largest temporary (1 GiB in float64)


def conv_fwd(x, w, stride=1, pad=0):
    """y (N,K,P,Q) = conv2d(x (N,C,H,W), w (K,C,R,S))."""
    N, C, H, W = x.shape
    K, _, R, S = w.shape
    P, Q = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
    wm = w.reshape(K, C * R * S)
    y = x.new_empty((N, K, P, Q))
    per = max(1, _CHUNK // max(1, C * R * S * P * Q))
    for n0 in range(0, N, per):
        xs = x[n0:n0 + per]
        if R == 1 and S == 1 and pad == 0:
            cols = xs[:, :, ::stride, ::stride].reshape(xs.shape[0], C, P * Q)
        else:
            cols = F.unfold(xs, (R, S), padding=pad, stride=stride)
        y[n0:n0 + per] = torch.matmul(wm, cols).view(-1, K, P, Q)
    return y


def conv_dgrad(gy, w, H, W, stride=1, pad=0):
    """gx (N,C,H,W): the adjoint of conv_fwd applied to gy (N,K,P,Q)."""
    N, K, P, Q = gy.shape
    _, C, R, S = w.shape
    wt = w.reshape(K, C * R * S).t()
    gx = gy.new_zeros((N, C, H, W))
    per = max(1, _CHUNK // max(1, C * R * S * P * Q))
    for n0 in range(0, N, per):
        cols = torch.matmul(wt, gy[n0:n0 + per].reshape(-1, K, P * Q))
        if R == 1 and S == 1 and pad == 0:
            gx[n0:n0 + per, :, ::stride, ::stride] = cols.view(-1, C, P, Q)
        else:
            gx[n0:n0 + per] = F.fold(cols, (H, W), (R, S), padding=pad, stride=stride)
    return gx


def conv_wgrad(x, gy, R, S, stride=1, pad=0):
    """gw (K,C,R,S) = sum over n, p, q of gy x-patch."""
    N, C, H, W = x.shape
    K, P, Q = gy.shape[1:]
    gw = x.new_zeros((K, C * R * S))
    per = max(1, _CHUNK // max(1, C * R * S * P * Q))
    for n0 in range(0, N, per):
        xs = x[n0:n0 + per]
        if R == 1 and S == 1 and pad == 0:
            cols = xs[:, :, ::stride, ::stride].reshape(xs.shape[0], C, P * Q)
        else:
            cols = F.unfold(xs, (R, S), padding=pad, stride=stride)
        g = gy[n0:n0 + per].reshape(-1, K, P * Q)
        gw += torch.einsum('nkl,ncl->kc', g, cols)
    return gw.view(K, C, R, S)


def _per_c(v, nd=4):
    return None if v is None else v.view((1, -1) + (1,) * (nd - 2))


def fwd_epilogue(y, flags, bias=None, scale=None, shift=None, residual=None):
    """MRCNN_EPI_*: bias, affine, residual, ReLU in the header's order (per-channel dim 1)."""
    if flags & EPI_BIAS:
        y = y + _per_c(bias, y.dim())
    if flags & EPI_AFFINE:
        y = y * _per_c(scale, y.dim()) + _per_c(shift, y.dim())
    if flags & EPI_RESIDUAL:
        y = y + residual
    if flags & EPI_RELU:
        y = y.clamp_min(0)
    return y


def dgrad_epilogue(acc, flags, prev=None, res_g=None, res_y=None, out_mask_y=None,
                   out_scale=None):
    """gx = (acc * out_scale[c] + res_g * (res_y > 0) [+ prev]) * (out_mask_y > 0)."""
    g = acc if out_scale is None else acc * _per_c(out_scale)
    if res_g is not None:
        g = g + (res_g if res_y is None else res_g * (res_y > 0))
    if flags & EPI_ACCUM:
        g = g + prev
    if out_mask_y is not None:
        g = g * (out_mask_y > 0)
    return g


def deconv_fwd(x, w):
    """Deconvolution2D(k=2, s=2): x (N,C,H,W), w (C,K,2,2) -> (N,K,2H,2W)."""
    N, C, H, W = x.shape
    K = w.shape[1]
    y = torch.einsum('nchw,ckab->nkhawb', x, w)
    return y.reshape(N, K, 2 * H, 2 * W)


def deconv_dgrad(gy, w):
    N, K, H2, W2 = gy.shape
    g = gy.view(N, K, H2 // 2, 2, W2 // 2, 2)
    return torch.einsum('nkhawb,ckab->nchw', g, w)


def deconv_wgrad(x, gy):
    N, K, H2, W2 = gy.shape
    g = gy.view(N, K, H2 // 2, 2, W2 // 2, 2)
    return torch.einsum('nchw,nkhawb->ckab', x, g)


def roi_tables(rois, H, W, PH, PW, spatial_scale, sampling_ratio, bin_stride=1):
    """Separable ROIAlign weights, geometry in fp32 exactly as the kernels (roi_align.hip: roi_geom,
    tap1d, sample position start + p * bin + (i + .5) * bin / grid), weights in float64:
    Ay (R, OH, H), Bx (R, OW, W) with y[r, oh, ow] = sum_hw Ay[r,oh,h] Bx[r,ow,w] x[b_r,h,w] /
    count_r.  Returns (batch index (R), Ay, Bx, count (R) float64)."""
    f = rois.to(torch.float32)
    s = torch.tensor(spatial_scale, dtype=torch.float32)
    batch = f[:, 0].long()

    def axis(lo_, hi_, n_bins, size):
        start = lo_ * s
        end = hi_ * s
        roi = torch.clamp_min(end - start, 1.)
        bin_ = roi / float(n_bins)
        if sampling_ratio > 0:
            grid = torch.full_like(roi, sampling_ratio, dtype=torch.int64)
        else:
            grid = torch.ceil(roi / float(n_bins)).long()
        G = int(grid.max()) if grid.numel() else 1
        p = torch.arange(0, n_bins, bin_stride, device=f.device)
        i = torch.arange(G, device=f.device)
        # (R, O, G) positions, left to right in fp32
        pos = (start[:, None, None] + p[None, :, None].float() * bin_[:, None, None]) \
            + (i[None, None, :].float() + .5) * bin_[:, None, None] / grid[:, None, None].float()
        use = (i[None, None, :] < grid[:, None, None]) & ~((pos < -1.) | (pos > float(size)))
        pc = torch.clamp_min(pos, 0.)
        lo = pc.long()
        edge = lo >= size - 1
        lo = torch.where(edge, torch.full_like(lo, size - 1), lo)
        hi = torch.where(edge, lo, lo + 1)
        pc = torch.where(edge, lo.float(), pc)
        wl = (pc - lo.float())                     # weight of hi, fp32 as tap1d
        wh = (1. - wl)                             # weight of lo
        A = torch.zeros((f.shape[0], p.numel(), size), dtype=F64, device=f.device)
        m = use.to(F64)
        A.scatter_add_(2, lo.clamp(0, size - 1).view(f.shape[0], p.numel(), -1),
                       (wh.to(F64) * m).view(f.shape[0], p.numel(), -1))
        A.scatter_add_(2, hi.clamp(0, size - 1).view(f.shape[0], p.numel(), -1),
                       (wl.to(F64) * m).view(f.shape[0], p.numel(), -1))
        return A, grid

    Ay, gh = axis(f[:, 2], f[:, 4], PH, H)
    Bx, gw = axis(f[:, 1], f[:, 3], PW, W)
    return batch, Ay, Bx, (gh * gw).to(F64)


def roi_align_fwd(x, rois, PH, PW, spatial_scale, sampling_ratio=0, bin_stride=1, chunk=64):
    """x (N,H,W,C) float64 -> y (R, OH, OW, C) float64 (NHWC, as the kernels)."""
    N, H, W, C = x.shape
    batch, Ay, Bx, count = roi_tables(rois, H, W, PH, PW, spatial_scale, sampling_ratio, bin_stride)
    R, OH, OW = Ay.shape[0], Ay.shape[1], Bx.shape[1]
    y = x.new_empty((R, OH, OW, C))
    for n in range(N):
        idx = torch.nonzero(batch == n).flatten()
        for i0 in range(0, idx.numel(), chunk):
            r = idx[i0:i0 + chunk]
            t = torch.matmul(Ay[r].reshape(-1, H), x[n].reshape(H, W * C)).view(-1, OH, W, C)
            y[r] = torch.einsum('rqw,rpwc->rpqc', Bx[r], t) / count[r].view(-1, 1, 1, 1)
    y[(batch < 0) | (batch >= N)] = 0
    return y


def roi_align_bwd(gy, rois, x_shape, spatial_scale, sampling_ratio=0, bin_stride=1, PH=None,
                  PW=None, chunk=64):
    """gy (R, OH, OW, C) float64 -> gx (N,H,W,C) float64: the adjoint of roi_align_fwd."""
    N, H, W, C = x_shape
    PH = PH if PH is not None else gy.shape[1] * bin_stride
    PW = PW if PW is not None else gy.shape[2] * bin_stride
    batch, Ay, Bx, count = roi_tables(rois, H, W, PH, PW, spatial_scale, sampling_ratio, bin_stride)
    gx = gy.new_zeros((N, H, W, C))
    for n in range(N):
        idx = torch.nonzero(batch == n).flatten()
        for i0 in range(0, idx.numel(), chunk):
            r = idx[i0:i0 + chunk]
            s = torch.einsum('rqw,rpqc->rpwc', Bx[r], gy[r] / count[r].view(-1, 1, 1, 1))
            gx[n] += torch.matmul(Ay[r].reshape(-1, H).t(), s.reshape(-1, W * C)).view(H, W, C)
    return gx


def sparse3x3_gather(x, g, rows):
    """fp32 restatement: patches (n,3,3,C) of x (N,H,W,C) around rows (indices into N*H*W), zero
    outside the map, and g_rows (n,K)."""
    N, H, W, C = x.shape
    n, hw = rows // (H * W), rows % (H * W)
    h, w = hw // W, hw % W
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    dy = torch.arange(3, device=x.device)
    patches = xp[n[:, None, None], h[:, None, None] + dy[None, :, None],
                 w[:, None, None] + dy[None, None, :]]
    return patches, g.reshape(-1, g.shape[-1])[rows]


def sparse3x3_scatter(g_patches, lookup, N, H, W, C):
    """gx (N,H,W,C): every pixel sums the patch gradients of the listed rows whose 3x3 window
    covers it (lookup: position -> row or -1)."""
    gx = g_patches.new_zeros((N, H + 2, W + 2, C))
    rows = torch.nonzero(lookup.view(-1) >= 0).flatten()
    r = lookup.view(-1)[rows].long()
    n, hw = rows // (H * W), rows % (H * W)
    h, w = hw // W, hw % W
    for dy in range(3):
        for dx in range(3):
            gx.index_put_((n, h + dy, w + dx), g_patches[r, dy, dx], accumulate=True)
    return gx[:, 1:H + 1, 1:W + 1]


def maxpool3x3s2p1(x):
    """fp32 restatement (NCHW): F.max_pooling_2d(x, 3, 2, 1, cover_all=True)."""
    return F.max_pool2d(x, 3, 2, 1, ceil_mode=True)


def sgd(p, g, v, lr, momentum, wd, grad_scale):
    """float64 update of sgd_momentum_wd: v' = m v - lr (g gs + wd p); p' = p + v'; and the
    per-element tolerance (4 fp32 ulps of the operands)."""
    v2 = momentum * v - lr * (g * grad_scale + wd * p)
    p2 = p + v2
    eps = 2. ** -23
    tv = 4 * eps * (abs(momentum) * v.abs() + abs(lr) * ((g * grad_scale).abs() + abs(wd) * p.abs()))
    tp = 4 * eps * (p.abs() + v2.abs()) + tv
    return p2, v2, tp, tv


# ---- losses (csrc/loss.hip) ------------------------------------------------------------------
#
# Bounds are in units of the fp32 unit roundoff u = 2^-24 (one correctly rounded operation has a
# relative error of at most u; a function documented to n ulp has at most 2 n u).  The device math
# library is built to the OpenCL full-profile limits expf <= 3 ulp, logf <= 3 ulp, log1pf <= 2 ulp
# (the HIP math API documentation lists tighter figures; the wider, guaranteed ones are used), and
# a / b is charged 1 ulp.  loss.hip is compiled without fast-math; FMA contraction only removes
# roundings.
#
# Every loss is  (sum of element terms) / count  reduced as: each thread adds its grid-stride
# elements in fp32 (`per_thread` adds), a 6-step fp32 butterfly over the 64 lanes, the four wave
# sums and the <= 256 partials in double (errors of 2^-53, not counted), one division in double
# and one rounding to fp32.  With every term of the sum bounded in magnitude by its share of
# S = sum |term|, the error of the normalised loss is at most
#     K_loss u S / count,     K_loss = K_el + per_thread + 6 + 1
# where K_el bounds the relative error of one element term.  This is a worst-case (linear) bound;
# the same reduction emulated on the CPU (tests/test_launch_ref_cpu.py) stays under 1 u at the
# project's sizes, and one dropped element of mean size is 130 u at the RPN's n = 128 520 and
# 83 u at the mask loss's 1024 x 196, so K_loss must stay under about 40 there (it is 22).
#
# Gradients are written per element as (f(x) - target) * (1 / count) with |f| <= 1, so their
# bound is absolute in units of 1 / count:  K_g u max(1, A_r) / count  (A_r = 1 unless noted).
U = 2. ** -24
ULP_EXP, ULP_LOG, ULP_LOG1P, ULP_DIV = 3, 3, 2, 1
# inv = 1.f / (float)count, then g * inv.  The conversion is exact below 2^24; above, its 1 u is
# inside the slack of charging a correctly rounded division a full ulp.
K_INV = 2 * ULP_DIV + 1

# sigmoid CE element  max(x, 0) - x t + log1pf(expf(-|x|)):  x * (t - (x >= 0)) is a product with
# -1, 0 or 1 (exact); e = expf(-|x|) carries 2 ULP_EXP u, which log1p passes on with a condition
# number e / ((1 + e) log1p(e)) <= 1, plus log1pf's own 2 ULP_LOG1P u; both summands are >= 0, so
# the final add costs 1 u of the element.
K_SCE_EL = 2 * ULP_EXP + 2 * ULP_LOG1P + 1
# sigmoid CE gradient (sigmoidf(x) - t) * inv,  sigmoidf = 1 / (1 + expf(-x)) <= 1: expf 2 ULP_EXP u
# (condition of 1 / (1 + e) in e is <= 1), the add 1 u, the division 2 ULP_DIV u, then - t (|result|
# <= 1) 1 u.  Absolute, because sigmoidf(20) - 1 is 0 in fp32 and -2e-9 in float64: the cancellation
# is the formula's own (chainer's float32 sigmoid has it too).
K_SCE_G = 2 * ULP_EXP + 1 + 2 * ULP_DIV + 1 + K_INV
# smooth L1 element: d = pred - gt 1 u of d.  |d| < 1 / sigma^2: (sigma^2 / 2) d d, d's error twice,
# two products, sigma * sigma: 5 u.  Otherwise |d| - 0.5 / sigma^2 >= |d| / 2: d's error doubles to
# 2 u, the constant's division 2 ULP_DIV u of a term no larger than the result, the subtraction
# 1 u, sigma * sigma 1 u: 6 u.  Value and gradient are continuous at the switch, so a branch taken
# differently in fp32 and float64 changes nothing beyond these roundings.
K_SL1_EL = 4 + 2 * ULP_DIV
# smooth L1 gradient: sigma^2 d (|.| < 1): d 1 u, sigma * sigma 1 u, the product 1 u; or +-1, 0.
K_SL1_G = 3 + K_INV


def flat_parts(n):
    """parts_for(n) of loss.hip: workgroups of the flat kernels' first pass."""
    return max(1, min(256, -(-int(n) // 1024)))


def row_parts(R):
    """First-pass workgroups of softmax CE (four rows, one per wave, per workgroup)."""
    return max(1, min(256, -(-int(R) // 4)))


def k_loss(k_el, per_thread):
    return k_el + per_thread + 6 + 1


def k_softmax_z(ncls):
    """Relative error of z = sum_k expf(x_k - m), in u: expf 2 ULP_EXP; the rounding of x_k - m is
    u |x_k - m| in the exponent, weighted by p_k it sums to at most u ln(ncls) (the mean of m - x_k
    under the softmax weights is the entropy minus ln z); ceil(ncls / 64) adds per lane and 6
    butterfly steps on non-negative terms."""
    return 2 * ULP_EXP + math.log(ncls) + -(-ncls // 64) + 6


def k_softmax_lse(ncls):
    """Absolute error of lse = m + logf(z) in u max(1, |lse|): z's relative error is an absolute
    error of log z; logf 2 ULP_LOG u of log z <= ln(ncls); the add 1 u of lse."""
    return k_softmax_z(ncls) + 2 * ULP_LOG * max(1., math.log(ncls)) + 1


def _tol_like(valid, value):
    return torch.where(valid, value, torch.zeros_like(value))


def tol_ratio(got, ref, tol):
    """Worst |got - ref| / tol over the elements (<= 1: within the bound).  Where tol is 0 the
    values must be equal.  NaN matches NaN; a value equal to the float64 reference rounded to
    fp32 always passes (a reference beyond FLT_MAX rounds to inf, and so must the kernel).  Any
    other non-finite value or difference gives inf.  Empty tensors give 0."""
    ref = ref.to(F64)
    got = got.to(device=ref.device, dtype=F64).reshape(ref.shape)
    if ref.numel() == 0:
        return 0.
    tol = torch.as_tensor(tol, dtype=F64, device=ref.device).expand(ref.shape)
    same = (got == ref) | (got == ref.float().to(F64)) | (torch.isnan(got) & torch.isnan(ref))
    err = (got - ref).abs()
    r = torch.where(same, torch.zeros_like(err), err / tol)
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    return float(r.max())


def _sce_terms(x, t):
    valid = t != -1
    tt = t.to(F64)
    el = x.clamp_min(0) - x * tt + torch.log1p(torch.exp(-x.abs()))
    el = torch.where(valid, el, torch.zeros_like(el))
    g = torch.where(valid, torch.sigmoid(x) - tt, torch.zeros_like(x))
    return valid, el, g


def sigmoid_ce(x, t):
    """F.sigmoid_cross_entropy(x, t): x float64 (any shape), t integer in {-1, 0, 1}, -1 ignored;
    loss = sum over the rest of  max(x, 0) - x t + log1p(exp(-|x|))  / max(count, 1),
    gx = (sigmoid(x) - t) / max(count, 1), 0 where ignored.
    Returns (loss, gx, loss_tol, gx_tol): the bounds of the module comment with K_el = K_SCE_EL,
    per_thread = ceil(n / (256 flat_parts(n))), K_g = K_SCE_G; gx_tol is 0 where t is ignored (the
    kernel writes an exact 0 there)."""
    valid, el, g = _sce_terms(x, t)
    n = x.numel()
    count = max(int(valid.sum()), 1)
    per_thread = -(-n // (256 * flat_parts(n)))
    S = el.sum()
    loss_tol = k_loss(K_SCE_EL, per_thread) * U * S / count
    g_tol = _tol_like(valid, torch.full_like(x, K_SCE_G * U / count))
    return S / count, g / count, loss_tol, g_tol


def mask_sigmoid_ce(x, label, t):
    """F.sigmoid_cross_entropy(x[arange(R), :, label - 1], t): x (R, HW, Kc) float64, label (R),
    t (R, HW).  The channel index label - 1 follows NumPy: a background row (label 0) selects
    channel Kc - 1.  gx (R, HW, Kc) is 0 outside the selected channel.  Bounds as sigmoid_ce with
    n = R HW; gx_tol is 0 wherever gx must be an exact 0."""
    R, HW, Kc = x.shape
    ch = torch.remainder(label.long() - 1, Kc)
    sel = torch.gather(x, 2, ch.view(R, 1, 1).expand(R, HW, 1)).squeeze(2)
    loss, g_sel, loss_tol, g_sel_tol = sigmoid_ce(sel, t)
    gx = torch.zeros_like(x)
    g_tol = torch.zeros_like(x)
    idx = ch.view(R, 1, 1).expand(R, HW, 1)
    gx.scatter_(2, idx, g_sel.unsqueeze(2))
    g_tol.scatter_(2, idx, g_sel_tol.unsqueeze(2))
    return loss, gx, loss_tol, g_tol


def _softmax_scale(x, lse):
    """max(1, A_r), A_r = max(|lse_r|, max_k |x_rk|) over the finite logits: the operands whose
    rounding enters expf's argument."""
    finite = torch.where(torch.isfinite(x), x.abs(), torch.zeros_like(x))
    return torch.maximum(lse.abs(), finite.max(1).values).clamp_min(1.)


def softmax_ce(x, t):
    """F.softmax_cross_entropy(x (R, ncls) float64, t (R) integer), ignore_label -1:
    loss = sum over valid rows of (lse_r - x[r, t_r]) / max(count, 1), lse = logsumexp,
    gx[r, k] = (exp(x_rk - lse_r) - [k == t_r]) / max(count, 1), rows of 0 where ignored.
    Loss bound: S = sum over valid rows of |lse_r| + |x[r, t_r]| (the two cancel for a confident
    row), K_el = k_softmax_lse(ncls) + 1 (the subtraction), per_thread = rows per wave
    = ceil(R / (4 row_parts(R))).  The part of lse's error that does not scale with |lse| (z's
    relative error, logf's error of log z) is charged to S as if |lse_r| + |x[r, t_r]| >= 1 on the
    average row, which holds for every input of the suite and the step (lse is near ln(ncls) for an
    untrained head) but not for rows whose target logit is dominant and exactly 0.
    Gradient bound: K_g u max(1, A_r) / count with A_r of _softmax_scale and
    K_g = 2 (x - lse rounds to u (|x| + |lse|) in expf's argument) + k_softmax_lse + 2 ULP_EXP
    + 1 (the subtraction) + K_INV; 0 on ignored rows."""
    R, ncls = x.shape
    valid = t != -1
    count = max(int(valid.sum()), 1)
    lse = torch.logsumexp(x, 1) if R else x.new_zeros((0,))
    tt = torch.where(valid, t, torch.zeros_like(t)).long()
    xt = torch.gather(x, 1, tt.view(R, 1)).squeeze(1) if R else x.new_zeros((0,))
    zero = torch.zeros_like(lse)
    loss = torch.where(valid, lse - xt, zero).sum() / count
    S = torch.where(valid, lse.abs() + xt.abs(), zero).sum()
    per_thread = -(-R // (4 * row_parts(R)))
    loss_tol = k_loss(k_softmax_lse(ncls) + 1, per_thread) * U * S / count
    p = torch.exp(x - lse.view(R, 1))
    onehot = torch.zeros_like(x)
    if R:
        onehot.scatter_(1, tt.view(R, 1), 1.)
    gx = torch.where(valid.view(R, 1), (p - onehot) / count, torch.zeros_like(x))
    k_g = 2 + k_softmax_lse(ncls) + 2 * ULP_EXP + 1 + K_INV
    g_tol = torch.where(valid, k_g * U * _softmax_scale(x, lse) / count, zero)
    g_tol = g_tol.view(R, 1).expand(R, ncls)
    return loss, gx, loss_tol, g_tol


def softmax(x):
    """F.softmax(x (R, ncls) float64, axis 1).  Returns (y, y_tol): expf(x - m) / z with
    K = 2 (x - m rounds to u (|x| + |m|) in expf's argument, y <= 1) + 2 ULP_EXP + k_softmax_z
    + 2 ULP_DIV, times u max(1, A_r)."""
    R, ncls = x.shape
    if R == 0:
        return x.clone(), x.clone()
    lse = torch.logsumexp(x, 1)
    y = torch.exp(x - lse.view(R, 1))
    k = 2 + 2 * ULP_EXP + k_softmax_z(ncls) + 2 * ULP_DIV
    return y, (k * U * _softmax_scale(x, lse)).view(R, 1).expand(R, ncls)


def smooth_l1(pred, cls, gt_loc, gt_label, sigma):
    """_fast_rcnn_loc_loss: pred (n, ld) float64, row r's 4-vector at columns 4 cls[r] .. + 4
    (0 .. 4 when cls is None), gt_loc (n, 4), gt_label (n).  With d = pred4 - gt_loc on rows of label > 0:
    element = (sigma^2 / 2) d^2 if |d| < 1 / sigma^2 else |d| - 0.5 / sigma^2, loss = sum / count,
    count = #(label >= 0) WITHOUT a guard: nothing counted gives 0 / 0 = NaN, as the original.
    gx (n, ld) = (sigma^2 d | sign(d)) / count in the selected columns of label > 0 rows, else 0.
    Bounds: K_el = K_SL1_EL, per_thread = 4 ceil(n / (256 flat_parts(n))), K_g = K_SL1_G; gx_tol
    is 0 wherever gx is an exact 0 (rows of label <= 0, columns outside the selection)."""
    n, ld = pred.shape
    s2 = float(sigma) ** 2
    c = torch.zeros((n,), dtype=torch.int64, device=pred.device) if cls is None else cls.long()
    cols = (4 * c).view(n, 1) + torch.arange(4, device=pred.device).view(1, 4)
    d = torch.gather(pred, 1, cols) - gt_loc if n else pred.new_zeros((0, 4))
    fg = (gt_label > 0).view(n, 1)
    a = d.abs()
    quad = a < 1. / s2
    el = torch.where(quad, (s2 / 2.) * d * d, a - 0.5 / s2)
    el = torch.where(fg, el, torch.zeros_like(el))
    g = torch.where(quad, s2 * d, torch.sign(d))
    count = (gt_label >= 0).sum().to(F64)
    S = el.sum()
    per_thread = 4 * -(-n // (256 * flat_parts(n)))
    loss_tol = k_loss(K_SL1_EL, per_thread) * U * S / count
    gx = torch.zeros_like(pred)
    g_tol = torch.zeros_like(pred)
    if n:
        gx.scatter_(1, cols, torch.where(fg, g / count, torch.zeros_like(g)))
        g_tol.scatter_(1, cols, torch.where(fg, (K_SL1_G * U / count).expand(n, 4),
                                            torch.zeros_like(g)))
    return S / count, gx, loss_tol, g_tol


# ---- target creators (csrc/targets.hip) ------------------------------------------------------
#
# NumPy on the host: each check_* takes the operands and the kernel's outputs as arrays and yields
# (ratio, what) like a LaunchChecker post().  Box coordinates are fp32 values, so every first
# difference (br - tl, y1 - y0) of exact inputs carries one rounding, 1 u relative.
#
# IoU = I / ((A + B) - I):  I, A, B are products of two such differences: 3 u each.  A + B: 4 u of
# A + B.  D = (A + B) - I:  4 u (A + B) + 3 u I + 1 u D in absolute terms; I <= min(A, B) gives
# A + B <= 2 D and I <= D, so D carries 12 u.  The division adds 1 u:  K_IOU = 3 + 12 + 1 = 16,
# relative to the IoU (an IoU of exactly 0 has I = 0 exactly and must be 0).  A row or column
# maximum is one of those values, so it is within 16 u of the float64 maximum.  0 / 0 (two
# zero-area boxes) is NaN in both.
K_IOU = 16
# bbox2loc (src -> dst), per axis with s = src size, c_s = src centre, d, c_d likewise:
#   s, d:  1 u.   c = lo + 0.5 s:  0.5 u |s| + 1 u |c| absolute (0.5 s is exact).
#   dy = (c_d - c_s) / max(s, eps):  numerator u (0.5 |s| + |c_s| + 0.5 |d| + |c_d| + |c_d - c_s|),
#     the divisor's 1 u and the division's 1 u:
#     tol_dy = u ((0.5 |s| + |c_s| + 0.5 |d| + |c_d|) / s + 3 |dy|)
#   dh = (float) log((double) (d / s)):  d / s carries 3 u, which the logarithm turns into 3 u
#     absolute; the double log is exact at this scale; the rounding to fp32 1 u of |dh|:
#     tol_dh = u (3 + |dh|).   d = 0 gives -inf, d < 0 NaN, in both.
#   normalised (x - mean) / std with fp32 mean, std:  tol_x / |std| + 2 u |result|.


def _np_tol(got, ref, tol):
    """tol_ratio on NumPy arrays; the bound counts only where the reference is finite."""
    ref = np.asarray(ref, np.float64)
    tol = np.where(np.isfinite(ref), np.broadcast_to(np.asarray(tol, np.float64), ref.shape), 0.)
    got = np.asarray(got)
    if got.shape != ref.shape:
        return math.inf
    return tol_ratio(torch.from_numpy(np.ascontiguousarray(got)), torch.from_numpy(ref),
                     torch.from_numpy(np.ascontiguousarray(tol)))


def _np_exact(got, ref):
    """0 when equal element for element (NaN equal to NaN, -0 to 0), inf otherwise."""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape:
        return math.inf
    if got.dtype.kind == 'f' or ref.dtype.kind == 'f':
        return 0. if np.array_equal(got, ref, equal_nan=True) else math.inf
    return 0. if np.array_equal(got, ref) else math.inf


def _np_bits(got, ref):
    """0 when the two arrays hold the same bytes."""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    same = got.shape == ref.shape and got.dtype == ref.dtype and got.tobytes() == ref.tobytes()
    return 0. if same else math.inf


def bbox_iou_f64(a, b):
    """chainercv bbox_iou in float64: (na, g)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.empty((len(a), len(b)))
    with np.errstate(invalid='ignore', divide='ignore'):
        area_b = np.prod(b[:, 2:] - b[:, :2], axis=1)
        for i0 in range(0, len(a), 8192):
            x = a[i0:i0 + 8192]
            tl = np.maximum(x[:, None, :2], b[None, :, :2])
            br = np.minimum(x[:, None, 2:], b[None, :, 2:])
            inter = np.prod(br - tl, axis=2) * (tl < br).all(axis=2)
            area_a = np.prod(x[:, 2:] - x[:, :2], axis=1)
            out[i0:i0 + 8192] = inter / (area_a[:, None] + area_b[None, :] - inter)
    return out


def bbox_iou_f32(a, b):
    """oracle.np_ref.bbox_iou (fp32, the reference's operation order), in row chunks."""
    from oracle import np_ref
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    with np.errstate(invalid='ignore', divide='ignore'):
        parts = [np_ref.bbox_iou(a[i0:i0 + 8192], b) for i0 in range(0, len(a), 8192)]
    return np.concatenate(parts, 0) if parts else np.empty((0, len(b)), np.float32)


def check_bbox_iou_argmax(a, b, max_iou, argmax, iou=None, col_max=None):
    """mrcnn_bbox_iou_argmax.  The matrix against float64 under K_IOU; max_iou / argmax / col_max as
    np.max / np.argmax (first index of the maximum, a NaN wins and propagates) of the kernel's own
    matrix when it is an output, else of the fp32 restatement; both maxima against float64."""
    na = len(a)
    if na == 0:
        return
    ref = bbox_iou_f64(a, b)
    if iou is not None:
        yield _np_tol(iou, ref, K_IOU * U * np.abs(ref)), 'iou vs float64'
    own = iou if iou is not None else bbox_iou_f32(a, b)
    yield _np_exact(max_iou, own.max(axis=1)), 'max_iou is the row maximum'
    yield _np_exact(argmax, own.argmax(axis=1).astype(np.int32)), 'argmax is its first index'
    m = ref.max(axis=1)
    yield _np_tol(max_iou, m, K_IOU * U * np.abs(m)), 'max_iou vs float64'
    if col_max is not None:
        yield _np_exact(col_max, own.max(axis=0)), 'col_max is the column maximum'
        m = ref.max(axis=0)
        yield _np_tol(col_max, m, K_IOU * U * np.abs(m)), 'col_max vs float64'


def anchor_labels_ref(iou, max_iou, gt_max, neg_iou_thresh, pos_iou_thresh):
    """chainercv AnchorTargetCreator._create_label before the draws, in its statement order, on
    fp32 values (the thresholds arrive as C floats)."""
    label = np.full((len(iou),), -1, np.int32)
    with np.errstate(invalid='ignore'):
        label[max_iou < np.float32(neg_iou_thresh)] = 0
        label[(iou == gt_max[None, :]).any(axis=1)] = 1
        label[max_iou >= np.float32(pos_iou_thresh)] = 1
    return label


def check_anchor_labels(iou, max_iou, gt_max, neg_iou_thresh, pos_iou_thresh, label):
    yield _np_exact(label, anchor_labels_ref(iou, max_iou, gt_max, neg_iou_thresh,
                                             pos_iou_thresh)), 'labels'


def bbox2loc_f64(src, dst):
    """chainercv bbox2loc in float64 and its bound (the comment above): (loc (n, 4), tol (n, 4))."""
    s, d = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    eps = float(np.finfo(np.float32).eps)
    loc, tol = np.empty((len(s), 4)), np.empty((len(s), 4))
    with np.errstate(invalid='ignore', divide='ignore'):
        for ax in (0, 1):
            ss, ds = s[:, 2 + ax] - s[:, ax], d[:, 2 + ax] - d[:, ax]
            cs, cd = s[:, ax] + 0.5 * ss, d[:, ax] + 0.5 * ds
            sc = np.maximum(ss, eps)
            dy = (cd - cs) / sc
            dh = np.log(ds / sc)
            loc[:, ax], loc[:, 2 + ax] = dy, dh
            tol[:, ax] = U * ((0.5 * np.abs(ss) + np.abs(cs) + 0.5 * np.abs(ds) + np.abs(cd)) / sc
                              + 3 * np.abs(dy))
            tol[:, 2 + ax] = U * (3 + np.abs(dh))
    return loc, tol


def check_anchor_targets_finish(anchor_inside, inside_index, label_inside_before, argmax, bbox,
                                disabled, n_anchor, label_inside_after, loc, label):
    """mrcnn_anchor_targets_finish: label_inside changed at exactly the disabled entries; label is
    -1 and loc +0 on every row inside_index does not name; the named rows carry label_inside and
    bbox2loc(anchor, bbox[argmax])."""
    expect_li = label_inside_before.copy()
    expect_li[disabled] = -1
    yield _np_exact(label_inside_after, expect_li), 'label_inside: exactly the disabled entries'
    expect = np.full((n_anchor,), -1, np.int32)
    expect[inside_index] = expect_li
    yield _np_exact(label, expect), 'label scatter'
    outside = np.ones((n_anchor,), bool)
    outside[inside_index] = False
    yield _np_bits(loc[outside], np.zeros((int(outside.sum()), 4), np.float32)), 'loc outside is 0'
    if len(inside_index):
        ref, tol = bbox2loc_f64(anchor_inside, bbox[argmax])
        yield _np_tol(loc[inside_index], ref, tol), 'loc vs float64'


def check_proposal_targets_gather(cand, bbox, gt_label, assigned, chosen, n_fg, mean, std,
                                  sample_roi, loc, label, gt_index):
    """mrcnn_proposal_targets_gather: sample_roi a bit-equal gather, gt_index = assigned[chosen],
    gt_roi_label = class + 1 on the first n_fg rows and 0 after, gt_roi_loc against float64."""
    a = assigned[chosen]
    yield _np_bits(sample_roi, cand[chosen]), 'sample_roi is cand[chosen]'
    yield _np_exact(gt_index, a), 'gt_index'
    expect = (gt_label[a] + 1).astype(np.int32)
    expect[n_fg:] = 0
    yield _np_exact(label, expect), 'gt_roi_label'
    ref, tol = bbox2loc_f64(cand[chosen], bbox[a])
    m = np.asarray(mean, np.float32).astype(np.float64)
    s = np.asarray(std, np.float32).astype(np.float64)
    out = (ref - m) / s
    yield _np_tol(loc, out, tol / np.abs(s) + 2 * U * np.abs(out)), 'gt_roi_loc vs float64'


def mask_targets_ref(masks, sample_roi, gt_index, n_fg, M):
    """The modelled project's construction (ProposalTargetCreator.__call__, as oracle/np_targets.py
    states it): integer box by np.round (half to even), Python slice of the ground-truth mask,
    one-hot of the crop, bilinear resize of each channel in fp32, argmax over the channels.  The
    resize is oracle.np_ref.resize_bilinear, the oracle's restatement of OpenCV's documented
    half-pixel INTER_LINEAR rule: cv2 itself is not available, so the rule stays pinned only to
    that restatement and to tests/golden/proposal_target_creator.npz.  A ground-truth mask is
    {0, 1} there; the kernel takes uint8 and reads any non-zero value as 1, so the crop is
    binarised first.  Sampled RoIs lie inside the image; a negative coordinate (where a Python
    slice would wrap) is outside the contract and is clamped to 0 here as in the kernel.  Rows
    >= n_fg are -1; an empty crop is all 0 (the documented deviation: the original raises)."""
    from oracle import np_ref
    n = len(sample_roi)
    out = -np.ones((n, M, M), np.int32)
    for i in range(n_fg):
        r = np.maximum(np.round(sample_roi[i]).astype(np.int32), 0)
        m = (masks[gt_index[i]][r[0]:r[2], r[1]:r[3]] != 0).astype(np.int32)
        if m.size == 0:
            out[i] = 0
            continue
        score = (np.arange(m.max() + 1) == m[..., None]).astype(np.float32)
        score = np.stack([np_ref.resize_bilinear(score[..., c], M, M)
                          for c in range(score.shape[2])], axis=2)
        out[i] = np.argmax(score, axis=2).astype(np.int32)
    return out


def check_mask_targets(masks, sample_roi, gt_index, n_fg, M, out):
    yield _np_exact(out, mask_targets_ref(masks, sample_roi, gt_index, n_fg, M)), 'mask targets'


# ---- reading operands by address -------------------------------------------------------------

_hip = None


def _hip_lib():
    """The HIP runtime torch has loaded (its path from /proc/self/maps)."""
    global _hip
    if _hip is None:
        path = None
        with open('/proc/self/maps') as f:
            for line in f:
                if 'libamdhip64.so' in line:
                    path = line.split()[-1]
                    break
        _hip = ctypes.CDLL(path or 'libamdhip64.so')
        _hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                        ctypes.c_int, ctypes.c_void_p]
        _hip.hipMemcpyAsync.restype = ctypes.c_int
    return _hip


def _addr(a):
    if a is None:
        return 0
    if isinstance(a, ctypes.c_void_p):
        return a.value or 0
    return int(a)


def read(addr, shape, dtype=torch.float32, device='cuda'):
    """A fresh tensor holding `shape` elements at device address `addr` (None for NULL)."""
    addr = _addr(addr)
    if not addr:
        return None
    t = torch.empty(tuple(int(s) for s in shape), dtype=dtype, device=device)
    if t.numel():
        # on the current torch stream, so that the torch ops that read `t` are ordered after the
        # copy (a device-to-device hipMemcpy may return before it completes, and the null stream
        # does not order a non-blocking side stream such as the deferred-gradient stream)
        rc = _hip_lib().hipMemcpyAsync(ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(addr),
                                       t.numel() * t.element_size(), 3,   # hipMemcpyDeviceToDevice
                                       ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream))
        if rc != 0:
            raise RuntimeError('hipMemcpyAsync from 0x%x failed (%d)' % (addr, rc))
    return t


def _nchw(t, N, H, W, C):
    """(N,H,W,C) fp32 buffer -> float64 NCHW."""
    return None if t is None else t.view(N, H, W, C).permute(0, 3, 1, 2).to(F64)


def _krsc(t, K, R, S, C):
    return None if t is None else t.view(K, R, S, C).permute(0, 3, 1, 2).to(F64)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _d(arg):
    """ctypes.byref(ConvDesc) -> the descriptor."""
    return arg._obj if hasattr(arg, '_obj') else arg.contents


# ---- entry points that need no reference here ---------------------------------------------------

# name -> the test that compares it bit-exactly or in float64 at realistic sizes (or: a query)
ALLOWED = {
    'mrcnn_nms_sorted': 'tests/test_gpu_proposal.py (vs the C oracle, exact keep lists)',
    'mrcnn_nms_sorted_batched': 'tests/test_gpu_proposal.py::test_nms_batched_structure_and_device_counts, '
                                '::test_nms_workspace_reuse (vs the C oracle, exact keep lists)',
    'mrcnn_topk_desc': 'tests/test_gpu_proposal.py',
    'mrcnn_topk_desc_batched': 'tests/test_gpu_proposal.py',
    'mrcnn_decode_clip': 'tests/test_gpu_proposal.py::test_decode_clip_min_size_validity, '
                         '::test_proposal_creator_default_min_size (boxes and valid bytes, bit for bit)',
    'mrcnn_gather_rows': 'tests/test_gpu_proposal.py',
    'mrcnn_detect_sort': 'tests/test_gpu_inference.py::test_suppress_edges_match_oracle',
    'mrcnn_detect_compact': 'tests/test_gpu_inference.py::test_suppress_edges_match_oracle',
    'mrcnn_decode_cls_boxes': 'tests/test_gpu_inference.py::test_decode_cls_boxes_mean_std_and_stride',
    'mrcnn_observe_accumulate': 'tests/test_gpu_trainer.py (loss observation)',
    'mrcnn_prepare_image': 'tests/test_gpu_inference.py (image preparation)',
    'mrcnn_paste_masks': 'tests/test_gpu_inference.py (mask pasting)',
    'mrcnn_paste_masks_packed': 'tests/test_gpu_mask_rle.py (mask pasting)',
    'mrcnn_mask_pack': 'tests/test_gpu_mask_rle.py',
}


class LaunchChecker:
    """Wraps _lib.call; see the module docstring.  ``stats[name] = [launches, worst ratio]``,
    ``fails`` lists (name, detail, ratio) of every launch over its bound, ``unchecked`` the entry
    points called that have neither a reference nor an ALLOWED entry, ``launches[name]`` the calls
    checked.  With ``only`` (a set of names) the other entry points are passed through unchecked;
    one that has neither a reference nor an ALLOWED entry is still reported."""

    def __init__(self, allowed=ALLOWED, only=None):
        self.allowed = allowed
        self.only = None if only is None else frozenset(only)
        self.launches = collections.Counter()
        self.stats = collections.OrderedDict()
        self.fails = []
        self.unchecked = collections.Counter()
        self.u_of = {}      # u address -> (w fp32 (K,3,3,C), desc fields)
        self.v_of = {}      # v address -> x fp32 (N,H,W,C)
        self.wt_of = {}     # wT address -> (w fp32 (K,R,S,C), row_scale fp32 or None)
        self._orig = None

    def install(self, monkeypatch):
        self._orig = _lib.call
        monkeypatch.setattr(_lib, 'call', self.call)

    # -- bookkeeping
    def _record(self, name, r, detail):
        st = self.stats.setdefault(name, [0, 0.])
        st[0] += 1
        st[1] = max(st[1], r)
        if not r <= 1.:
            self.fails.append((name, detail, r))

    def table(self):
        lines = ['%-40s %8s %12s' % ('entry point', 'launches', 'excess/bound')]
        for k, (n, r) in sorted(self.stats.items()):
            lines.append('%-40s %8d %12.4g' % (k, n, r))
        for k, n in sorted(self.unchecked.items()):
            lines.append('%-40s %8d %12s' % (k, n, 'UNCHECKED'))
        return '\n'.join(lines)

    def assert_clean(self):
        assert not self.unchecked, 'entry points without a reference: %s' % dict(self.unchecked)
        assert not self.fails, 'launches over the bound:\n' + '\n'.join(
            '%s %s: %.4g' % f for f in self.fails[:20])

    # -- the wrapper
    def call(self, name, *args):
        fn = getattr(self, '_' + name[len('mrcnn_'):], None)
        if fn is None:
            if name not in self.allowed:
                self.unchecked[name] += 1
            return self._orig(name, *args)
        if self.only is not None and name not in self.only:
            return self._orig(name, *args)
        self.launches[name] += 1
        torch.cuda.synchronize()
        post = fn(*args)                  # reads the operands, returns the checker of the outputs
        self._orig(name, *args)
        torch.cuda.synchronize()
        with torch.no_grad():
            for r, detail in post():
                self._record(name, r, detail)
        del post
        torch.cuda.synchronize()

    # ---- convolution family ------------------------------------------------------------------
    @staticmethod
    def _dims(d):
        return (d.N, d.H, d.W, d.C, d.K, d.R, d.S, d.stride, d.pad, d.P, d.Q)

    def _conv2d_fwd(self, dp, x, w, bias, scale, shift, residual, y, flags, split_ws, stream):
        d = _d(dp)
        N, H, W, C, K, R, S, st, pd, P, Q = self._dims(d)
        X = _nchw(read(x, (N, H, W, C)), N, H, W, C)
        Wt = _krsc(read(w, (K, R, S, C)), K, R, S, C)
        b, sc, sh = (read(p, (K,)) for p in (bias, scale, shift))
        res = _nchw(read(residual, (N, P, Q, K)), N, P, Q, K)

        def post():
            ref = fwd_epilogue(conv_fwd(X, Wt, st, pd), flags, *(None if t is None else t.to(F64)
                                                               for t in (b, sc, sh)), res)
            got = _nchw(read(y, (N, P, Q, K)), N, P, Q, K)
            yield ratio(got, ref), _desc_str(d, flags)
        return post

    def _dgrad_common(self, d, gy, wfull, row_scale, gx, flags, res_g, res_y, mask, oscale,
                      form):
        N, H, W, C, K, R, S, st, pd, P, Q = self._dims(d)
        G = _nchw(read(gy, (N, P, Q, K)), N, P, Q, K)
        prev = _nchw(read(gx, (N, H, W, C)), N, H, W, C) if flags & EPI_ACCUM else None
        rg = _nchw(read(res_g, (N, H, W, C)), N, H, W, C)
        ry = _nchw(read(res_y, (N, H, W, C)), N, H, W, C)
        my = _nchw(read(mask, (N, H, W, C)), N, H, W, C)
        os_ = read(oscale, (C,))

        def post():
            g = G if row_scale is None else G * _per_c(row_scale.to(F64))
            acc = conv_dgrad(g, wfull, H, W, st, pd)
            ref = dgrad_epilogue(acc, flags, prev, rg, ry, my, None if os_ is None else os_.to(F64))
            got = _nchw(read(gx, (N, H, W, C)), N, H, W, C)
            yield ratio(got, ref), form + ' ' + _desc_str(d, flags)
        return post

    def _conv2d_dgrad(self, dp, gy, w, gx, flags, stream):
        d = _d(dp)
        Wt = _krsc(read(w, (d.K, d.R, d.S, d.C)), d.K, d.R, d.S, d.C)
        return self._dgrad_common(d, gy, Wt, None, gx, flags, None, None, None, None, 'dgrad')

    def _conv2d_dgrad_ex(self, dp, gy, w, gx, flags, res_g, res_y, mask, oscale, split_ws, stream):
        d = _d(dp)
        Wt = _krsc(read(w, (d.K, d.R, d.S, d.C)), d.K, d.R, d.S, d.C)
        return self._dgrad_common(d, gy, Wt, None, gx, flags, res_g, res_y, mask, oscale,
                                  'dgrad_ex')

    def _conv2d_dgrad_wt(self, dp, gy, wT, gx, flags, res_g, res_y, mask, oscale, split_ws,
                         stream):
        d = _d(dp)
        src = self.wt_of.get(_addr(wT))
        if src is None:
            raise AssertionError('mrcnn_conv2d_dgrad_wt: wT at 0x%x was not built by a checked '
                                 'flip-transpose' % _addr(wT))
        w, rs = src
        Wt = _krsc(w, d.K, d.R, d.S, d.C)
        return self._dgrad_common(d, gy, Wt, rs, gx, flags, res_g, res_y, mask, oscale, 'dgrad_wt')

    def _wgrad_common(self, d, x, gy, gw, row_scale, form):
        N, H, W, C, K, R, S, st, pd, P, Q = self._dims(d)
        X = _nchw(read(x, (N, H, W, C)), N, H, W, C)
        G = _nchw(read(gy, (N, P, Q, K)), N, P, Q, K)
        rs = read(row_scale, (K,))

        def post():
            ref = conv_wgrad(X, G, R, S, st, pd)
            if rs is not None:
                ref = ref * rs.to(F64).view(-1, 1, 1, 1)
            got = _krsc(read(gw, (K, R, S, C)), K, R, S, C)
            yield ratio(got, ref), form + ' ' + _desc_str(d, 0)
        return post

    def _conv2d_wgrad(self, dp, x, gy, gw, ws, stream):
        return self._wgrad_common(_d(dp), x, gy, gw, None, 'wgrad')

    def _conv2d_wgrad_ex(self, dp, x, gy, gw, ws, row_scale, stream):
        return self._wgrad_common(_d(dp), x, gy, gw, row_scale, 'wgrad_ex')

    def _filter_flip_transpose(self, w, wT, K, R, S, C, row_scale, stream):
        return self._flip_jobs([(w, wT, K, R, S, C, row_scale)])

    def _filter_flip_transpose_batched(self, n, w, wT, K, R, S, C, row_scale, stream):
        return self._flip_jobs([(w[i], wT[i], K[i], R[i], S[i], C[i], row_scale[i])
                                for i in range(n)])

    def _flip_jobs(self, jobs):
        src = [(read(w, (K, R, S, C)), read(rs, (K,)), wT, (K, R, S, C)) for w, wT, K, R, S, C, rs
               in jobs]

        def post():
            for w, rs, wT, (K, R, S, C) in src:
                ref = w if rs is None else w * rs.view(-1, 1, 1, 1)
                ref = ref.flip(1, 2).permute(3, 1, 2, 0).contiguous()     # (C,R,S,K)
                self.wt_of[_addr(wT)] = (w, rs)
                yield exact(read(wT, (C, R, S, K)), ref), 'K%d R%d S%d C%d' % (K, R, S, C)
        return post

    # ---- Winograd ----------------------------------------------------------------------------
    def _conv3x3_wino_filter(self, dp, w, u, stream):
        d = _d(dp)
        W_ = read(w, (d.K, 3, 3, d.C))

        def post():
            self.u_of[_addr(u)] = W_
            return iter(())
        return post

    def _conv3x3_wino_fwd(self, dp, x, w, u, scale, shift, y, flags, v, ws, stream):
        d = _d(dp)
        N, H, W, C, K, R, S, st, pd, P, Q = self._dims(d)
        x32 = read(x, (N, H, W, C))
        w32 = read(w, (K, 3, 3, C))
        if w32 is None:
            w32 = self.u_of.get(_addr(u))
            if w32 is None:
                raise AssertionError('wino_fwd: u at 0x%x has no checked filter transform' % _addr(u))
        sc, sh = read(scale, (K,)), read(shift, (K,))

        def post():
            if _addr(v):
                self.v_of[_addr(v)] = x32
            X = _nchw(x32, N, H, W, C)
            ref = conv_fwd(X, _krsc(w32, K, 3, 3, C), 1, 1)
            f = flags & (EPI_AFFINE | EPI_BIAS | EPI_RELU)
            if f & EPI_BIAS:
                ref = fwd_epilogue(ref, f, bias=sh.to(F64))
            else:
                ref = fwd_epilogue(ref, f, scale=None if sc is None else sc.to(F64),
                                   shift=None if sh is None else sh.to(F64))
            got = _nchw(read(y, (N, P, Q, K)), N, P, Q, K)
            yield ratio(got, ref), 'wino_fwd ' + _desc_str(d, flags)
        return post

    def _conv3x3_wino_dgrad(self, dp, gy, w, w_row_scale, gx, out_scale, out_mask_y, ws, stream):
        d = _d(dp)
        Wt = _krsc(read(w, (d.K, 3, 3, d.C)), d.K, 3, 3, d.C)
        rs = read(w_row_scale, (d.K,))
        return self._dgrad_common(d, gy, Wt, rs, gx, 0, None, None, out_mask_y, out_scale,
                                  'wino_dgrad')

    def _conv3x3_wino_wgrad(self, dp, x, v, gy, gw, out_row_scale, ws, stream):
        d = _d(dp)
        if not _addr(x):
            src = self.v_of.get(_addr(v))
            if src is None:
                raise AssertionError('wino_wgrad: v at 0x%x has no checked forward' % _addr(v))
            x = ctypes.c_void_p(src.data_ptr())
            post = self._wgrad_common(d, x, gy, gw, out_row_scale, 'wino_wgrad(v)')
            return post
        return self._wgrad_common(d, x, gy, gw, out_row_scale, 'wino_wgrad(x)')

    # ---- stem and deconvolution --------------------------------------------------------------
    def _conv_stem_fwd(self, x4, w784, bias, scale, shift, y, N, H, W, K, flags, stream):
        X = read(x4, (N, H, W, 4))[..., :3].permute(0, 3, 1, 2).to(F64)
        Wt = read(w784, (K, 7, 8, 4))[:, :, :7, :3].permute(0, 3, 1, 2).to(F64)
        b, sc, sh = (read(p, (K,)) for p in (bias, scale, shift))
        P, Q = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1

        def post():
            ref = fwd_epilogue(conv_fwd(X, Wt, 2, 3), flags, *(None if t is None else t.to(F64)
                                                            for t in (b, sc, sh)))
            got = _nchw(read(y, (N, P, Q, K)), N, P, Q, K)
            yield ratio(got, ref), 'stem N%d H%d W%d K%d f%d' % (N, H, W, K, flags)
        return post

    def _deconv_common(self, x, w, bias, y, N, H, W, C, K, flags, form):
        X = _nchw(read(x, (N, H, W, C)), N, H, W, C)
        b = read(bias, (K,))

        def post():
            ref = fwd_epilogue(deconv_fwd(X, w.view(C, 2, 2, K).permute(0, 3, 1, 2).to(F64)),
                               flags, None if b is None else b.to(F64))
            got = _nchw(read(y, (N, 2 * H, 2 * W, K)), N, 2 * H, 2 * W, K)
            yield ratio(got, ref), '%s N%d H%d W%d C%d K%d f%d' % (form, N, H, W, C, K, flags)
        return post

    def _deconv2x2s2_fwd(self, x, w, bias, y, N, H, W, C, K, flags, stream):
        return self._deconv_common(x, read(w, (C, 2, 2, K)), bias, y, N, H, W, C, K, flags,
                                   'deconv_fwd')

    def _deconv2x2s2_fwd_wt(self, x, wT, bias, y, N, H, W, C, K, flags, stream):
        src = self.wt_of.get(_addr(wT))
        if src is None or src[1] is not None:
            raise AssertionError('deconv_fwd_wt: wT at 0x%x has no checked flip-transpose' % _addr(wT))
        return self._deconv_common(x, src[0], bias, y, N, H, W, C, K, flags, 'deconv_fwd_wt')

    def _deconv2x2s2_dgrad(self, gy, w, gx, N, H, W, C, K, stream):
        G = _nchw(read(gy, (N, 2 * H, 2 * W, K)), N, 2 * H, 2 * W, K)
        Wt = read(w, (C, 2, 2, K)).permute(0, 3, 1, 2).to(F64)

        def post():
            got = _nchw(read(gx, (N, H, W, C)), N, H, W, C)
            yield ratio(got, deconv_dgrad(G, Wt)), 'deconv_dgrad N%d H%d W%d C%d K%d' % (N, H, W, C, K)
        return post

    def _deconv2x2s2_wgrad(self, x, gy, gw, N, H, W, C, K, ws, stream):
        X = _nchw(read(x, (N, H, W, C)), N, H, W, C)
        G = _nchw(read(gy, (N, 2 * H, 2 * W, K)), N, 2 * H, 2 * W, K)

        def post():
            got = read(gw, (C, 2, 2, K)).permute(0, 3, 1, 2)
            yield ratio(got, deconv_wgrad(X, G)), 'deconv_wgrad N%d H%d W%d C%d K%d' % (N, H, W, C, K)
        return post

    # ---- row-sparse 3x3 backward ---------------------------------------------------------------
    def _sparse3x3_gather(self, x, g, rows, n_rows, N, H, W, C, K, patches, g_rows, stream):
        X = read(x, (N, H, W, C))
        G = read(g, (N, H, W, K))
        rw = read(rows, (n_rows,), torch.int32).long()

        def post():
            p_ref, g_ref = sparse3x3_gather(X, G, rw)
            yield exact(read(patches, (n_rows, 3, 3, C)), p_ref), 'patches n%d C%d' % (n_rows, C)
            yield exact(read(g_rows, (n_rows, K)), g_ref), 'g_rows n%d K%d' % (n_rows, K)
        return post

    def _sparse3x3_scatter(self, g_patches, lookup, N, H, W, C, gx, stream):
        lk = read(lookup, (N, H, W), torch.int32)
        n = int(lk.max()) + 1 if lk.numel() else 0
        gp = read(g_patches, (max(n, 0), 3, 3, C))

        def post():
            ref = sparse3x3_scatter(gp.to(F64), lk, N, H, W, C)
            yield ratio(read(gx, (N, H, W, C)), ref), 'scatter n%d N%d H%d W%d C%d' % (n, N, H, W, C)
        return post

    # ---- ROIAlign ------------------------------------------------------------------------------
    def _roi_fwd(self, x, rois, y, N, H, W, C, R, PH, PW, bs, ss, sr, scale=None, shift=None,
                 relu=0, form='roi_fwd_ex'):
        X = read(x, (N, H, W, C))
        ro = read(rois, (R, 5))
        sc, sh = read(scale, (C,)), read(shift, (C,))
        OH, OW = -(-PH // bs), -(-PW // bs)

        def post():
            ref = roi_align_fwd(X.to(F64), ro, PH, PW, ss, sr, bs)
            if sc is not None:
                ref = ref * sc.to(F64) + sh.to(F64)
                if relu:
                    ref = ref.clamp_min(0)
            yield ratio(read(y, (R, OH, OW, C)), ref), '%s N%d H%d W%d C%d R%d %dx%d/%d relu%d' % (
                form, N, H, W, C, R, PH, PW, bs, relu)
        return post

    def _roi_align_fwd_ex(self, x, rois, y, N, H, W, C, R, PH, PW, bs, ss, sr, order, stream):
        return self._roi_fwd(x, rois, y, N, H, W, C, R, PH, PW, bs, ss, sr)

    def _roi_align_fwd_affine(self, x, rois, y, N, H, W, C, R, PH, PW, bs, ss, sr, order, scale,
                              shift, relu, stream):
        return self._roi_fwd(x, rois, y, N, H, W, C, R, PH, PW, bs, ss, sr, scale, shift, relu,
                             'roi_fwd_affine')

    def _roi_align_bwd_ws(self, gy, rois, gx, N, H, W, C, R, PH, PW, bs, ss, sr, ws, ws_bytes,
                          stream):
        OH, OW = -(-PH // bs), -(-PW // bs)
        G = read(gy, (R, OH, OW, C))
        ro = read(rois, (R, 5))

        def post():
            ref = roi_align_bwd(G.to(F64), ro, (N, H, W, C), ss, sr, bs, PH, PW)
            yield ratio(read(gx, (N, H, W, C)), ref), 'roi_bwd_ws N%d H%d W%d C%d R%d %dx%d/%d' % (
                N, H, W, C, R, PH, PW, bs)
        return post

    # ---- elementwise, reductions, pools, optimiser -------------------------------------------
    def _epilogue_bwd(self, gy, y, scale, g, M, C, stream):
        G, Y, sc = read(gy, (M, C)), read(y, (M, C)), read(scale, (C,))

        def post():
            ref = G.to(F64)
            if Y is not None:
                ref = ref * (Y > 0)
            if sc is not None:
                ref = ref * sc.to(F64)
            yield ratio(read(g, (M, C)), ref), 'M%d C%d' % (M, C)
        return post

    def _colsum(self, g, out, M, C, ws, stream):
        G = read(g, (M, C))

        def post():
            yield ratio(read(out, (C,)), G.to(F64).sum(0)), 'M%d C%d' % (M, C)
        return post

    def _affine_fwd(self, x, w, b, y, M, C, stream):
        X, Wt, B = read(x, (M, C)), read(w, (C,)), read(b, (C,))

        def post():
            yield ratio(read(y, (M, C)), X.to(F64) * Wt.to(F64) + B.to(F64)), 'M%d C%d' % (M, C)
        return post

    def _affine_bwd(self, x, w, gy, gx, gW, gb, M, C, ws, stream):
        X, Wt, G = read(x, (M, C)), read(w, (C,)), read(gy, (M, C))

        def post():
            G64 = G.to(F64)
            yield ratio(read(gx, (M, C)), G64 * Wt.to(F64)), 'gx M%d C%d' % (M, C)
            if _addr(gW):
                yield ratio(read(gW, (C,)), (G64 * X.to(F64)).sum(0)), 'gW M%d C%d' % (M, C)
            if _addr(gb):
                yield ratio(read(gb, (C,)), G64.sum(0)), 'gb M%d C%d' % (M, C)
        return post

    def _maxpool3x3s2p1_fwd(self, x, y, N, H, W, C, P, Q, stream):
        X = read(x, (N, H, W, C))

        def post():
            ref = _nhwc(maxpool3x3s2p1(X.permute(0, 3, 1, 2)))
            yield exact(read(y, (N, P, Q, C)), ref.contiguous()), 'N%d H%d W%d C%d' % (N, H, W, C)
        return post

    def _avgpool_fwd(self, x, y, R, HW, C, stream):
        X = read(x, (R, HW, C))

        def post():
            yield ratio(read(y, (R, C)), X.to(F64).mean(1)), 'R%d HW%d C%d' % (R, HW, C)
        return post

    def _avgpool_bwd(self, gy, gx, R, HW, C, accumulate, stream):
        G = read(gy, (R, C))
        prev = read(gx, (R, HW, C)) if accumulate else None

        def post():
            ref = (G.to(F64) / HW)[:, None, :].expand(R, HW, C)
            if prev is not None:
                ref = ref + prev.to(F64)
            yield ratio(read(gx, (R, HW, C)), ref), 'R%d HW%d C%d acc%d' % (R, HW, C, accumulate)
        return post

    def _head_tail_bwd(self, g_pool, g_rows, slot, y, g, R, HW, C, stream):
        gp, Y = read(g_pool, (R, C)), read(y, (R, HW, C))
        sl = read(slot, (R,), torch.int32)
        gr = None
        if sl is not None and _addr(g_rows):
            nf = int(sl.max()) + 1 if R else 0
            gr = read(g_rows, (max(nf, 0), HW, C))

        def post():
            ref = (gp.to(F64) / HW)[:, None, :].expand(R, HW, C).clone()
            if gr is not None and gr.numel():
                on = sl >= 0
                ref[on] += gr.to(F64)[sl[on].long()]
            ref = ref * (Y > 0)
            yield ratio(read(g, (R, HW, C)), ref), 'R%d HW%d C%d' % (R, HW, C)
        return post

    def _sgd_momentum_wd_ex(self, p, g, v, n, lr, momentum, wd, grad_scale, zero_grad, stream):
        P0, G0, V0 = read(p, (n,)), read(g, (n,)), read(v, (n,))

        def post():
            p2, v2, tp, tv = sgd(P0.to(F64), G0.to(F64), V0.to(F64), lr, momentum, wd, grad_scale)
            for name, got, ref, tol in (('p', read(p, (n,)), p2, tp), ('v', read(v, (n,)), v2, tv)):
                err = (got.to(F64) - ref).abs()
                yield float((err / tol.clamp_min(1e-45)).max()) if n else 0., 'sgd %s n%d' % (name, n)
            if zero_grad:
                yield exact(read(g, (n,)), torch.zeros_like(G0)), 'sgd zero_grad n%d' % n
        return post

    # ---- losses ----------------------------------------------------------------------------------
    @staticmethod
    def _rows(addr, R, ncols, ld, dtype=torch.float32):
        """(R, ncols) view of the rows at `addr` with row stride ld, and the flat copy behind it."""
        if R == 0 or not _addr(addr):
            return torch.empty((R, ncols), dtype=dtype, device='cuda'), None
        flat = read(addr, ((R - 1) * ld + ncols,), dtype)
        return flat.as_strided((R, ncols), (ld, 1)), flat

    def _loss_post(self, loss, gx, ref, detail, got_gx):
        """The checks every loss shares: ref = (loss, gx, loss_tol, gx_tol) in float64."""
        l_ref, g_ref, l_tol, g_tol = ref
        yield tol_ratio(read(loss, ()), l_ref, l_tol), 'loss ' + detail
        if _addr(gx):
            yield tol_ratio(got_gx(), g_ref, g_tol), 'gx ' + detail

    def _sigmoid_ce(self, x, t, n, loss, gx, ws, stream):
        X = read(x, (n,)) if n else torch.empty((0,), device='cuda')
        T = read(t, (n,), dtype=torch.int32) if n else torch.empty((0,), dtype=torch.int32,
                                                                   device='cuda')

        def post():
            yield from self._loss_post(loss, gx, sigmoid_ce(X.to(F64), T), 'n%d' % n,
                                       lambda: read(gx, (n,)) if n else X)
        return post

    def _mask_sigmoid_ce(self, x, label, t, R, HW, Kc, loss, gx, ws, stream):
        def rd(a, shape, dtype=torch.float32):
            return read(a, shape, dtype) if R else torch.empty(shape, dtype=dtype, device='cuda')
        X, Lb, T = rd(x, (R, HW, Kc)), rd(label, (R,), torch.int32), rd(t, (R, HW), torch.int32)

        def post():
            yield from self._loss_post(loss, gx, mask_sigmoid_ce(X.to(F64), Lb, T),
                                       'R%d HW%d Kc%d' % (R, HW, Kc), lambda: rd(gx, (R, HW, Kc)))
        return post

    def _softmax_ce(self, x, ldx, t, R, ncls, loss, gx, ldg, ws, stream):
        X, _ = self._rows(x, R, ncls, ldx)
        T = read(t, (R,), dtype=torch.int32) if R else torch.empty((0,), dtype=torch.int32,
                                                                   device='cuda')
        _, before = self._rows(gx, R, ncls, ldg)
        detail = 'R%d ncls%d ldx%d ldg%d' % (R, ncls, ldx, ldg)

        def post():
            got, after = self._rows(gx, R, ncls, ldg)
            yield from self._loss_post(loss, gx, softmax_ce(X.to(F64), T), detail, lambda: got)
            if after is not None and ldg > ncls:
                before.as_strided((R, ncls), (ldg, 1)).copy_(got)
                yield _same_bits(after, before), 'gx padding untouched ' + detail
        return post

    def _softmax(self, x, ldx, y, ldy, R, ncls, stream):
        X, _ = self._rows(x, R, ncls, ldx)
        _, before = self._rows(y, R, ncls, ldy)
        detail = 'R%d ncls%d ldx%d ldy%d' % (R, ncls, ldx, ldy)

        def post():
            got, after = self._rows(y, R, ncls, ldy)
            ref, tol = softmax(X.to(F64))
            yield tol_ratio(got, ref, tol), 'y ' + detail
            if after is not None and ldy > ncls:
                before.as_strided((R, ncls), (ldy, 1)).copy_(got)
                yield _same_bits(after, before), 'y padding untouched ' + detail
        return post

    def _smooth_l1(self, pred, ld, cls, gt_loc, gt_label, n, sigma, loss, gx, ws, stream):
        def rd(a, shape, dtype=torch.float32):
            return read(a, shape, dtype) if n else torch.empty(shape, dtype=dtype, device='cuda')
        P, G, Lb = rd(pred, (n, ld)), rd(gt_loc, (n, 4)), rd(gt_label, (n,), torch.int32)
        C = rd(cls, (n,), torch.int32) if _addr(cls) else None
        before = rd(gx, (n, ld)) if _addr(gx) else None
        detail = 'n%d ld%d cls%d sigma%g' % (n, ld, C is not None, sigma)

        def post():
            ref = smooth_l1(P.to(F64), C, G.to(F64), Lb, sigma)
            after = rd(gx, (n, ld)) if before is not None else None
            yield from self._loss_post(loss, gx, ref, detail, lambda: after)
            if after is not None and n:
                # the kernel writes the selected 4-vector of every row and nothing else
                c = torch.zeros((n,), dtype=torch.int64, device='cuda') if C is None else C.long()
                cols = (4 * c).view(n, 1) + torch.arange(4, device='cuda').view(1, 4)
                expect = before.scatter(1, cols, torch.gather(after, 1, cols))
                yield _same_bits(after, expect), 'gx outside the selection untouched ' + detail
        return post

    # ---- target creators ---------------------------------------------------------------------
    @staticmethod
    def _host(addr, shape, dtype=torch.float32):
        """NumPy copy of `shape` elements at a device address (empty for NULL / no elements)."""
        shape = tuple(int(s) for s in shape)
        if not _addr(addr) or 0 in shape:
            return torch.zeros(shape, dtype=dtype).numpy()
        return read(addr, shape, dtype).cpu().numpy()

    def _bbox_iou_argmax(self, a, na, b, g, iou, max_iou, argmax, col_max, stream):
        A, B = self._host(a, (na, 4)), self._host(b, (g, 4))
        detail = 'na%d g%d matrix%d' % (na, g, bool(_addr(iou)))
        # na = 0 writes nothing (include/mrcnn_hip.h): col_max keeps its contents
        before = self._host(col_max, (g,), torch.int32) if na == 0 else None

        def post():
            if na == 0:
                yield _np_bits(self._host(col_max, (g,), torch.int32), before), \
                    'nothing written ' + detail
                return
            I = self._host(iou, (na, g)) if _addr(iou) else None
            C = self._host(col_max, (g,)) if _addr(col_max) else None
            for r, what in check_bbox_iou_argmax(A, B, self._host(max_iou, (na,)),
                                                 self._host(argmax, (na,), torch.int32), I, C):
                yield r, what + ' ' + detail
            yield _np_bits(self._host(a, (na, 4)), A), 'boxes_a untouched ' + detail
            yield _np_bits(self._host(b, (g, 4)), B), 'boxes_b untouched ' + detail
        return post

    def _anchor_labels(self, iou, max_iou, gt_max, na, g, neg, pos, label, stream):
        I, Mx, Gm = self._host(iou, (na, g)), self._host(max_iou, (na,)), self._host(gt_max, (g,))

        def post():
            for r, what in check_anchor_labels(I, Mx, Gm, neg, pos,
                                               self._host(label, (na,), torch.int32)):
                yield r, '%s na%d g%d' % (what, na, g)
        return post

    def _anchor_targets_finish(self, anchor_inside, inside_index, label_inside, argmax, bbox,
                               n_inside, disabled, n_disabled, n_anchor, loc, label, stream):
        i32 = torch.int32
        A = self._host(anchor_inside, (n_inside, 4))
        idx = self._host(inside_index, (n_inside,), i32)
        li = self._host(label_inside, (n_inside,), i32)
        am = self._host(argmax, (n_inside,), i32)
        B = self._host(bbox, (int(am.max()) + 1 if n_inside else 0, 4))
        dis = self._host(disabled, (n_disabled,), i32)
        detail = 'n_anchor%d n_inside%d n_disabled%d' % (n_anchor, n_inside, n_disabled)

        def post():
            for r, what in check_anchor_targets_finish(
                    A, idx, li, am, B, dis, n_anchor, self._host(label_inside, (n_inside,), i32),
                    self._host(loc, (n_anchor, 4)), self._host(label, (n_anchor,), i32)):
                yield r, what + ' ' + detail
            same = all(_np_bits(self._host(p, x.shape, t), x) == 0. for p, x, t in (
                (anchor_inside, A, torch.float32), (inside_index, idx, i32), (argmax, am, i32),
                (bbox, B, torch.float32), (disabled, dis, i32)))
            yield 0. if same else math.inf, 'operands untouched ' + detail
        return post

    def _proposal_targets_gather(self, cand, bbox, gt_label, assigned, chosen, n, n_fg, mean4,
                                 std4, sample_roi, loc, label, gt_index, stream):
        i32 = torch.int32
        ch = self._host(chosen, (n,), i32)
        nc = int(ch.max()) + 1 if n else 0
        C, asg = self._host(cand, (nc, 4)), self._host(assigned, (nc,), i32)
        g = int(asg[ch].max()) + 1 if n else 0
        B, gl = self._host(bbox, (g, 4)), self._host(gt_label, (g,), i32)
        mean, std = [float(v) for v in mean4], [float(v) for v in std4]
        detail = 'n%d n_fg%d' % (n, n_fg)

        def post():
            for r, what in check_proposal_targets_gather(
                    C, B, gl, asg, ch, n_fg, mean, std, self._host(sample_roi, (n, 4)),
                    self._host(loc, (n, 4)), self._host(label, (n,), i32),
                    self._host(gt_index, (n,), i32)):
                yield r, what + ' ' + detail
            same = all(_np_bits(self._host(p, x.shape, t), x) == 0. for p, x, t in (
                (cand, C, torch.float32), (bbox, B, torch.float32), (gt_label, gl, i32),
                (assigned, asg, i32), (chosen, ch, i32)))
            yield 0. if same else math.inf, 'operands untouched ' + detail
        return post

    def _mask_targets(self, masks, G, H, W, sample_roi, gt_index, n, n_fg, M, out, stream):
        i32 = torch.int32
        mk = read(masks, (G, H, W), torch.uint8)
        roi, gi = self._host(sample_roi, (n, 4)), self._host(gt_index, (n,), i32)
        detail = 'G%d H%d W%d n%d n_fg%d M%d' % (G, H, W, n, n_fg, M)

        def post():
            for r, what in check_mask_targets(mk.cpu().numpy(), roi, gi, n_fg, M,
                                              self._host(out, (n, M, M), i32)):
                yield r, what + ' ' + detail
            same = torch.equal(read(masks, (G, H, W), torch.uint8), mk) \
                and _np_bits(self._host(sample_roi, (n, 4)), roi) == 0. \
                and _np_bits(self._host(gt_index, (n,), i32), gi) == 0.
            yield 0. if same else math.inf, 'operands untouched ' + detail
        return post


def _desc_str(d, flags):
    return 'N%d H%d W%d C%d K%d %dx%d/s%d/p%d f%d' % (d.N, d.H, d.W, d.C, d.K, d.R, d.S, d.stride,
                                                     d.pad, flags)
