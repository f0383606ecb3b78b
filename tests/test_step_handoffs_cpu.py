"""The train step's hand-offs are arguments and attributes, not ambient state: the row-sparse hint
of a convolution is ``conv2d(..., grad_rows=)`` and refuses a convolution that cannot use it, the
names of the retired globals, option and switch stay retired, and the RoI head has ONE route for
"both branches and a row subset": the stage's two-output tail.  No device: launches are recorded
with the recorder of the launch-trace test."""
import pytest
import torch

import test_conv_launch_trace_cpu as T
from chainer_mask_rcnn_amd import functions as F
from chainer_mask_rcnn_amd import optimizers
from chainer_mask_rcnn_amd.functions import conv as C
from chainer_mask_rcnn_amd.models import mask_rcnn_resnet, mask_rcnn_train_chain
from chainer_mask_rcnn_amd.models.resnet_extractor import BuildingBlock


@pytest.fixture
def rec(monkeypatch):
    r = T.Recorder()
    r.install(monkeypatch)
    C.weights_changed()
    yield r
    C.weights_changed()


# ---- grad_rows: 2x8x5x6 input, 8 -> 16 channels (the sizes of the trace's conv2d cases) ----------

def _conv_case(rec, k):
    W, b = T._conv_layer(rec, 8, 16, k)
    return T._input(rec, (2, 8, 5, 6), True), W, b


@pytest.mark.parametrize('k,stride,pad,affine,names', [
    (1, 1, 0, False, '1x1'),
    (3, 2, 1, False, 'stride is 2'),
    (3, 1, 1, True, 'scale'),
], ids=['1x1', '3x3 stride 2', '3x3 with scale'])
def test_grad_rows_on_a_convolution_that_cannot_use_it(rec, k, stride, pad, affine, names):
    x, W, b = _conv_case(rec, k)
    kw = dict(scale=torch.ones(16), shift=torch.zeros(16)) if affine else {}
    with pytest.raises(ValueError, match=names):
        F.conv2d(x, W, None if affine else b, stride=stride, pad=pad, relu=True,
                 grad_rows=C.SparseRows(), **kw)
    assert rec.lines == []                              # refused before anything was launched
    F.conv2d(x, W, None if affine else b, stride=stride, pad=pad, relu=True, **kw)    # fine without
    assert len(rec.lines) == 1


def test_qualifying_convolution_records_the_hint_it_is_given_and_no_other(rec):
    x, W, b = _conv_case(rec, 3)
    hint = C.SparseRows()
    assert F.conv2d(x, W, b, stride=1, pad=1, relu=True).grad_fn.sparse_hint is None
    assert F.conv2d(x, W, b, stride=1, pad=1, relu=True, grad_rows=None).grad_fn.sparse_hint is None
    assert F.conv2d(x, W, b, stride=1, pad=1, relu=True, grad_rows=hint).grad_fn.sparse_hint is hint
    # nothing ambient is left behind by the call that had one
    assert F.conv2d(x, W, b, stride=1, pad=1, relu=True).grad_fn.sparse_hint is None


# ---- retired names --------------------------------------------------------------------------------

RETIRED = [
    (F, 'fanout_rows'),                    # the separate fan-out node: the stage's tail does it
    (C, '_DEFER'),                         # the defer queue hangs on the parameter arena
    (C, '_SPARSE_HINT'),                   # the hint is conv2d's grad_rows argument
    (C, 'sparse_output_grad'),
    (C, '_side_streams'),                  # the streams live in chainer_mask_rcnn_amd.streams
    (C, '_defer_streams'),
    (optimizers, 'DEFER_LAUNCH_AT'),       # the launch point is the proposal window's opening
    (mask_rcnn_train_chain, '_COPY_STREAMS'),
    (mask_rcnn_resnet.ResNetRoIHead, 'fused_tail'),     # (an instance attribute: checked on one)
]


@pytest.mark.parametrize('owner,name', RETIRED, ids=[n for _, n in RETIRED])
def test_retired_name_stays_retired(owner, name):
    """Bringing one of these back is a decision: say so here."""
    if isinstance(owner, type):
        owner = owner(50, 2, 7, 1 / 16.)
    assert not hasattr(owner, name)


def test_the_arena_owns_the_defer_queue():
    p = torch.nn.Parameter(torch.zeros(4))
    assert optimizers.ParamArena([p]).defer is None


# ---- the RoI head: both branches + mask_rows = the two-output tail ------------------------------------

def _small_head(rec, mp):
    """A head around a 5-RoI, 32 -> 16 -> 64-channel res5 (the sizes of the trace's head cases)."""
    _, rois5, order, tail = T._head_pieces(T.Recorder(), mp)        # (its module settings, its RoIs)
    torch.manual_seed(0)
    head = mask_rcnn_resnet.ResNetRoIHead(50, 3, 14, 1. / 16)
    head.res5 = BuildingBlock(3, 32, 16, 64, stride=2)
    head.cls_loc_score = mask_rcnn_resnet._Linear(64, head.cls_loc_score.W.shape[0])
    head.deconv6 = mask_rcnn_resnet._Deconvolution2D(64, 256, 0.01)
    for name in head.res5._names:
        T._freeze_affine(getattr(head.res5, name))
    x = T._input(rec, (2, 32, 6, 8), True)
    return head, x, rois5[:, [2, 1, 4, 3]].contiguous(), rois5[:, 0].to(torch.int32), order, tail


def _launches(rec):
    names = [l.split(' ', 1)[0] for l in rec.lines]
    return names[:names.index('#')], names[names.index('#') + 1:]


@pytest.mark.parametrize('with_hints', [False, True])
def test_head_with_both_branches_and_mask_rows_takes_the_two_output_tail(rec, monkeypatch, with_hints):
    head, x, rois, idx, order, tail = _small_head(rec, monkeypatch)
    hints = None
    if with_hints:
        slot = torch.full((5,), -1, dtype=torch.int32)
        slot[tail] = torch.arange(len(tail), dtype=torch.int32)
        hints = F.RoiHints(order=order, mask_slot=slot)
    locs, scores, masks = head(x, rois, idx, mask_rows=tail, hints=hints)
    assert locs.shape[0] == scores.shape[0] == 5 and tuple(masks.shape) == (len(tail), 2, 14, 14)
    rec.mark('backward')
    (locs.sum() + scores.sum() + masks.sum()).backward()
    fwd, bwd = _launches(rec)
    assert bwd.count('mrcnn_head_tail_bwd') == 1
    # it replaces the average pooling's own backward (the other route's sign)
    assert 'mrcnn_avgpool_bwd' not in bwd and fwd.count('mrcnn_avgpool_fwd') == 1


def test_head_without_the_box_branch_selects_the_mask_rows(rec, monkeypatch):
    head, x, rois, idx, order, tail = _small_head(rec, monkeypatch)
    locs, scores, masks = head(x, rois, idx, pred_bbox=False, mask_rows=tail)
    assert locs is None and scores is None
    assert tuple(masks.shape) == (len(tail), 2, 14, 14)
    rec.mark('backward')
    masks.sum().backward()
    fwd, bwd = _launches(rec)
    assert 'mrcnn_head_tail_bwd' not in bwd
    # and without a subset the mask branch sees every RoI
    assert head(x, rois, idx, pred_bbox=False)[2].shape[0] == 5
