"""Whole-stage op: chainer BuildingBlock (BottleneckA + n x BottleneckB) as ONE autograd node.

Forward = 3 (4) fused implicit-GEMM launches per block; backward = 3 (4) dgrad + 3 (4) wgrad
launches per block and nothing else: every gradient tensor inside the stage is written ALREADY
multiplied by the ReLU mask (and affine scale) of the conv that consumes it — in the epilogue
of the dgrad that produces it — and the identity-shortcut gradient is added there too, so none
of the stage's backward GEMMs stages a mask: they all run the 168-register kernels, three
workgroups per CU.  Only the gradient entering the stage from autograd takes one elementwise
masking pass.

Pooling AFTER res5.a's 1x1 projections ("projected pooling", ``building_block(..., roi=)``).  The
RoI head applies ROIAlign to the C4 feature map and then res5 (models/mask_rcnn_resnet.py:
168-176), whose first block reads the pooled map only through two 1x1 convolutions (conv1 and the
shortcut conv4, each followed by AffineChannel2D).  ROIAlign is linear over positions per channel
with no constant term, a bias-free 1x1 convolution is linear over channels per position: they
commute exactly,
    bn(conv1x1(roi_align(x))) == bn(roi_align(conv1x1(x))),
so both projections run on the N*H*W map pixels (2 x 51 x 84 = 8 568 at the C2 shape) instead of
the R*7*7 pooled ones (50 176), and ROIAlign pools their 512- / 2048-channel outputs with the
affine (+ ReLU) in its epilogue.  Backward likewise: ROIAlign's adjoint first, then data and
weight gradient of the projections on the map.  Same sums in a different order (fp32 rounding
only); ``conv.PROJECTED_POOLING = False`` restores the reference order.

The knobs live in functions/conv.py and are read here at call time as ``conv.NAME``: tests, tools
and the benchmark assign them on that module.
"""
import collections

import torch

from .. import _lib
from ..streams import wgrad_stream
from ._layout import nhwc
from ._conv_launch import (make_desc, epilogue_bwd, _fwd_raw, _dgrad_raw, _uses_transposed_dgrad,
                           _flip_transpose_batched, wino_dgrad, _roi_pool_affine, _roi_pool_bwd,
                           _avgpool_fwd, _head_tail_bwd)
from ._wgrad import _wgrad
from . import conv


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


def _stage_transposes(blocks, device):
    """Flipped / transposed filters of every stride-1 convolution of a stage, built by ONE
    launch into one buffer.  ``blocks``: one ``_StageBlock`` per bottleneck (the affine scales
    s3 / s4 are folded into conv3 / conv4).  Returns a dict {'1','2','3','4'} -> flat tensor
    per block."""
    keys, jobs = [], []
    for bi, b in enumerate(blocks):
        for key, W, d, sc in (('1', b.W1, b.d1, None), ('2', b.W2, b.d2, None),
                              ('3', b.W3, b.d3, b.s3), ('4', b.W4, b.d4, b.s4)):
            if W is not None and _uses_transposed_dgrad(d) and not conv.uses_winograd(d):
                keys.append((bi, key))
                jobs.append((nhwc(W), d, sc))
    out = [dict() for _ in blocks]
    if jobs:
        for (bi, key), t in zip(keys, _flip_transpose_batched(jobs, device)):
            out[bi][key] = t
    return out


def _projection_pooled(h, W, d, z, roi, scale, shift, relu):
    """relu?(bn(roi_align(conv1x1(h, W)))): a 1x1 projection of block a on the MAP ``h`` — or ``z``,
    that projection computed before (an entry of ``RoiSpec.proj``) — pooled with the affine (and
    ReLU) in ROIAlign's epilogue."""
    if z is None:
        z = _fwd_raw(h, nhwc(W), d)
    return _roi_pool_affine(z, roi, scale, shift, relu)


def _block_forward(b, h, stride, roi, training, ng):
    """One bottleneck on the input ``h``; fills ``b.d1 .. b.d4``.  ``roi``: the stage's ``RoiSpec``
    for the block that pools (block a: ``h`` is then the feature map), None for every other.
    Returns ``(h1, h2, y)``, its three ReLU outputs, and conv2's kept Winograd input transform
    (or None)."""
    proj = (None, None) if roi is None or roi.proj is None else roi.proj
    b.d1 = make_desc(h.shape, b.W1.shape, stride, 0)
    if roi is not None:
        h1 = _projection_pooled(h, b.W1, b.d1, proj[0], roi, b.s1, b.b1, True)
    else:
        h1 = _fwd_raw(h, nhwc(b.W1), b.d1, b.s1, b.b1, None, True)
    b.d2 = make_desc(h1.shape, b.W2.shape, 1, 1)
    v2 = None
    if conv.uses_winograd(b.d2) and conv._wino_forward('stage', training):
        # (with a weight gradient to come, the transformed input is kept for it)
        h2, v2 = conv.wino_fwd(h1, nhwc(b.W2), b.d2, b.s2, b.b2, True,
                               keep_v=training and bool(ng[b.i2]),
                               cache_for=None if training else b.W2,
                               exact_signs=training)
    else:
        h2 = _fwd_raw(h1, nhwc(b.W2), b.d2, b.s2, b.b2, None, True)
    if b.W4 is None:
        shortcut = h
    else:
        b.d4 = make_desc(h.shape, b.W4.shape, stride, 0)
        if roi is not None:
            shortcut = _projection_pooled(h, b.W4, b.d4, proj[1], roi, b.s4, b.b4, False)
        else:
            shortcut = _fwd_raw(h, nhwc(b.W4), b.d4, b.s4, b.b4, None, False)
    b.d3 = make_desc(h2.shape, b.W3.shape, 1, 0)
    y = _fwd_raw(h2, nhwc(b.W3), b.d3, b.s3, b.b3, shortcut, True)
    if conv.RELU_TAP is not None:
        conv.RELU_TAP.append(('block', (h1, h2, y)))
    return (h1, h2, y), v2


def _block_backward(b, acts, v2, wT, gm, roi, first, ng, grads, side, poll):
    """Backward of one bottleneck.  ``gm``: the gradient w.r.t. the block's output, already through
    that output's ReLU; ``acts`` / ``v2`` / ``wT``: the block's ``_StageActs``, kept Winograd
    transform (or None) and transposed filters; ``roi``: as in ``_block_forward``; ``first``: block
    0 of the stage.  Queues the block's weight gradients, stores what autograd gets for them in
    ``grads`` and then calls ``poll`` (if any: see ``_StageFn.forward``).  Returns the gradient w.r.t. the block's input, through the ReLU that produced it
    unless that is the stage's input — or None where the stage's input needs no gradient."""
    x, h1, h2, _ = acts
    dev_ = gm.device
    need_w4 = b.W4 is not None and ng[b.i4]
    # what the gradient leaving this block must be masked with: the previous block's
    # output ReLU (= this block's input); the stage input belongs to someone else
    xm = None if first else x
    # the gradient the shortcut's conv4 reads: the block output's, or with pooling ...
    g4 = gm
    if roi is not None and (need_w4 or ng[0]):
        # ... that gradient back on the map (ROIAlign's adjoint commutes with the
        # per-channel scale s4, which stays folded into conv4's filter / gradient rows).
        # Queued BEFORE this block's weight gradients go to the side stream, and with the side
        # stream drained: see _pool_bwd_alone.
        _pool_bwd_alone(side, dev_)
        g4 = _roi_pool_bwd(gm, roi, (x.shape[0], b.d4.K, x.shape[2], x.shape[3]))
    if ng[b.i3]:
        grads[b.i3] = _wgrad(b.d3, h2, gm, b.W3, side, row_scale=b.s3)
    if need_w4:
        grads[b.i4] = _wgrad(b.d4, x, g4, b.W4, side, row_scale=b.s4)
    gh2 = _dgrad_raw(b.d3, gm, nhwc(b.W3), fold_scale=b.s3, out_mask_y=h2, out_scale=b.s2,
                     wT=wT.get('3'))
    if conv.uses_winograd(b.d2):
        if ng[b.i2]:
            grads[b.i2] = _wgrad(b.d2, h1 if v2 is None else None, gh2, b.W2, wino=True, v=v2)
        gh1 = wino_dgrad(b.d2, gh2, nhwc(b.W2), out_scale=b.s1, out_mask_y=h1)
    else:
        if ng[b.i2]:
            grads[b.i2] = _wgrad(b.d2, h1, gh2, b.W2, side)
        gh1 = _dgrad_raw(b.d2, gh2, nhwc(b.W2), out_mask_y=h1, out_scale=b.s1, wT=wT.get('2'))
    if roi is not None and (ng[b.i1] or ng[0]):
        _pool_bwd_alone(side, dev_)
        gh1 = _roi_pool_bwd(gh1, roi, (x.shape[0], b.d1.K, x.shape[2], x.shape[3]))
    if ng[b.i1]:
        grads[b.i1] = _wgrad(b.d1, x, gh1, b.W1, side)
    if poll is not None:
        poll()             # this block's weight gradients are queued
    if first and not ng[0]:
        return None
    if b.W4 is None:
        return _dgrad_raw(b.d1, gh1, nhwc(b.W1), res_g=gm, out_mask_y=xm, wT=wT.get('1'))
    # projection shortcut: both data gradients into one buffer; the input's ReLU mask is
    # fused into the second where conv1 has stride 1, else applied by a pass of its own
    fused = b.d1.stride == 1
    gx = _dgrad_raw(b.d1, gh1, nhwc(b.W1), wT=wT.get('1'))
    gx = _dgrad_raw(b.d4, g4, nhwc(b.W4), fold_scale=b.s4, out=gx, accum=True,
                    out_mask_y=xm if fused else None, wT=wT.get('4'))
    if xm is not None and not fused:
        gx = epilogue_bwd(gx, xm, None)
    return gx


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
            a, v2 = _block_forward(b, h, stride, roi if b is blocks[0] else None, training, ng)
            acts.append(a)
            wino_v.append(v2)
            h = a[-1]
        ctx.blocks = blocks
        ctx.poll = poll
        ctx.roi = roi
        _save_stage(ctx, x, acts, wino_v)
        ctx.tail = tail_rows is not None
        if not ctx.tail:
            return h
        # the two consumers of the stage output, produced here so that backward receives
        # their gradients separately (h itself is not an output of the node)
        R_, C_ = h.shape[0], h.shape[1]
        pooled = _avgpool_fwd(h)
        sub = h.permute(0, 2, 3, 1).index_select(0, tail_rows).permute(0, 3, 1, 2)
        if tail_slot is None:
            tail_slot = torch.full((R_,), -1, dtype=torch.int32, device=h.device)
            tail_slot[tail_rows] = torch.arange(tail_rows.numel(), dtype=torch.int32, device=h.device)
        ctx.tail_slot = tail_slot
        return pooled.reshape(R_, C_, 1, 1), sub

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
        side = wgrad_stream(dev_) if d_top.N * d_top.P * d_top.Q <= conv.SMALL_WGRAD_MAX_PIXELS else None
        # all the stage's filter transposes in one launch (built during the forward on the side
        # stream instead, they measured no faster: 53.2 vs 53.0 ms per step)
        stage_wT = _stage_transposes(blocks, dev_)
        # gm: gradient w.r.t. the block output, already through that output's ReLU
        y_top = acts[-1].y
        if ctx.tail:
            R_, C_ = y_top.shape[0], y_top.shape[1]
            if gy is None:
                gy = torch.zeros((R_, C_), dtype=torch.float32, device=dev_)
            gp = _lib.dense(gy.reshape(R_, C_), torch.float32, 'building_block', 'the pooled gradient',
                            align=True)
            gr = nhwc(g_rows) if g_rows is not None else None
            gm = _head_tail_bwd(gp, gr, ctx.tail_slot, y_top)
        else:
            gm = epilogue_bwd(gy, y_top, None)
        for i in range(len(blocks) - 1, -1, -1):
            gm = _block_backward(blocks[i], acts[i], wino_v.get(i), stage_wT[i], gm,
                                 ctx.roi if i == 0 else None, i == 0, ng, grads, side, poll)
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
