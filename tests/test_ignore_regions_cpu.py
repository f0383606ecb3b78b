"""Ignore regions without a device: the thresholding rule, the ``ignore``
argument of the two target creators (results and ``np.random`` state), and the argument checks of
the transform, the copy-paste dataset and the converter."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


# ---- the rule --------------------------------------------------------------------------------
def test_ignored_from_counts_is_strict_and_skips_empty_boxes():
    from chainer_mask_rcnn_amd.functions import ignored_from_counts
    counts = np.array([[0, 0], [7, 10], [8, 10], [6, 10], [10, 10], [0, 10], [1, 1000000]], np.int32)
    assert ignored_from_counts(counts, 0.7).tolist() == [False, False, True, False, True, False, False]
    # threshold 0: any covered pixel; threshold 1: never (covered <= area), not even a full box
    assert ignored_from_counts(counts, 0.).tolist() == [False, True, True, True, True, False, True]
    assert ignored_from_counts(counts, 1.).tolist() == [False] * 7
    # equality is not "more than": 1/2, and a product that float64 holds exactly
    assert ignored_from_counts(np.array([[5, 10], [2 ** 30, 2 ** 31 - 2 ** 30]], np.int64), 0.5).tolist() \
        == [False, True]
    assert ignored_from_counts(np.zeros((0, 2), np.int32), 0.7).shape == (0,)
    out = ignored_from_counts(counts, 0.7)
    assert out.dtype == np.bool_


# ---- ProposalTargetCreator -------------------------------------------------------------------
def _proposal_case():
    rng = np.random.RandomState(3)
    bbox = np.array([[10, 10, 90, 80], [40, 100, 120, 180], [100, 20, 180, 90], [5, 150, 60, 195]], np.float32)
    label = np.array([2, 0, 5, 1], np.int32)
    # 300 proposals: jittered copies of the boxes (foreground) and random boxes (background)
    near = bbox[rng.randint(0, 4, 120)] + rng.uniform(-8, 8, (120, 4)).astype(np.float32)
    y, x = rng.uniform(0, 160, 180), rng.uniform(0, 160, 180)
    far = np.stack([y, x, y + rng.uniform(8, 40, 180), x + rng.uniform(8, 40, 180)], 1).astype(np.float32)
    roi = np.concatenate([near, far])[rng.permutation(300)]
    mask = np.zeros((4, 200, 200), np.int32)
    for g, b in enumerate(bbox.astype(int)):
        mask[g, b[0]:b[2], b[1]:b[3]] = 1
    return roi, bbox, label, mask


def _sample(ptc, how, roi, bbox, label, mask, **kw):
    np.random.seed(11)
    if how == 'method':
        out = ptc.sample(roi, bbox, label, **kw)[:3]
    else:
        out = ptc(roi, bbox, label, mask, **kw)
    return out, np.random.get_state()


@pytest.mark.parametrize('how', ['method', 'call'])
def test_proposal_sampling_with_ignored_proposals(how):
    from chainer_mask_rcnn_amd.models.utils import ProposalTargetCreator
    roi, bbox, label, mask = _proposal_case()
    ptc = ProposalTargetCreator(n_sample=64)
    base, state = _sample(ptc, how, roi, bbox, label, mask)
    assert len(base[0]) == 64 and (base[2] > 0).sum() == 16       # both pools are larger than their share
    for same in (None, np.zeros(300, bool)):
        out, st = _sample(ptc, how, roi, bbox, label, mask, ignore=same)
        assert all(np.array_equal(a, b) for a, b in zip(out, base)) and len(out) == len(base)
        assert _same_state(st, state)

    ignore = np.random.RandomState(5).rand(300) < 0.4
    out, _ = _sample(ptc, how, roi, bbox, label, mask, ignore=ignore)
    sample_roi = out[0]
    assert len(sample_roi) <= 64

    def rows_of(boxes):     # index into cat(roi, bbox) of every sampled row
        cand = np.concatenate([roi, bbox])
        idx = [np.flatnonzero((cand == b).all(1)) for b in boxes]
        assert all(len(i) == 1 for i in idx)
        return np.array([i[0] for i in idx])
    rows = rows_of(sample_roi)
    assert not ignore[rows[rows < 300]].any()
    assert len(set(rows.tolist())) == len(rows)
    # the ground-truth candidates still can be drawn: with every proposal ignored, only they are
    out, _ = _sample(ptc, how, roi, bbox, label, mask, ignore=np.ones(300, bool))
    rows = rows_of(out[0])
    assert len(rows) == 4 and sorted(rows.tolist()) == [300, 301, 302, 303]
    assert (out[2] > 0).all() and sorted(out[2].tolist()) == sorted((label + 1).tolist())
    with pytest.raises(ValueError):
        ptc.sample(roi, bbox, label, ignore=np.ones(299, bool))
    with pytest.raises(ValueError, match='neg_iou_thresh_lo'):
        ProposalTargetCreator(n_sample=64, neg_iou_thresh_lo=-0.1).sample(roi, bbox, label, ignore=np.ones(300, bool))


# ---- AnchorTargetCreator ---------------------------------------------------------------------
def _anchor_case():
    from chainer_mask_rcnn_amd.utils.bbox import enumerate_shifted_anchor, generate_anchor_base
    anchor = enumerate_shifted_anchor(generate_anchor_base(anchor_scales=[2, 4, 8]), 16, 12, 14)
    bbox = np.array([[10, 10, 90, 80], [40, 100, 120, 180], [100, 20, 180, 200]], np.float32)
    return bbox, anchor.astype(np.float32), (192, 224)


def test_anchor_sampling_with_ignored_anchors():
    from chainer_mask_rcnn_amd.models.utils import AnchorTargetCreator
    bbox, anchor, size = _anchor_case()
    S = len(anchor)
    atc = AnchorTargetCreator(n_sample=32)

    def run(**kw):
        state = atc.prepare(bbox, anchor, size)
        before = state[2].copy()
        np.random.seed(4)
        loc, label = atc.finish(state, **kw)
        full = np.full(S, -1, np.int32)
        full[state[1]] = before
        return loc, label, full, np.random.get_state()

    loc0, label0, rule, st0 = run()
    assert (rule == 0).sum() > 32 and (rule == 1).sum() >= 3        # negatives are subsampled
    for same in (None, np.zeros(S, bool)):
        loc, label, _, st = run(ignore=same)
        assert np.array_equal(loc, loc0) and np.array_equal(label, label0) and _same_state(st, st0)

    ignore = np.random.RandomState(2).rand(S) < 0.5
    loc, label, rule, _ = run(ignore=ignore)
    assert np.array_equal(loc, loc0)
    assert (label[ignore & (rule == 0)] == -1).all()                # ignored zeros never sampled
    assert np.array_equal(label == 1, label0 == 1)                  # positives kept, ignored or not
    assert (ignore & (rule == 1)).any()
    assert (label >= 0).sum() <= 32
    # "before the draws": the negatives are drawn from the pool without the ignored ones — with
    # all but 5 negatives ignored nothing is left to subsample, and exactly those 5 are taken
    neg = np.flatnonzero(rule == 0)
    ignore = np.zeros(S, bool)
    ignore[neg[5:]] = True
    np.random.seed(4)
    before = np.random.get_state()
    _, label, _, after = run(ignore=ignore)
    assert sorted(np.flatnonzero(label == 0).tolist()) == neg[:5].tolist()
    np.random.seed(4)
    assert _same_state(after, np.random.get_state()) and _same_state(before, after)   # no draw at all
    with pytest.raises(ValueError):
        atc.finish(atc.prepare(bbox, anchor, size), ignore=np.zeros(S - 1, bool))


# ---- argument checks -------------------------------------------------------------------------
def test_transform_argument_checks():
    from chainer_mask_rcnn_amd.datasets import MaskRCNNTransform
    for kw in (dict(train=False, device_masks=True), dict(train=True, device_masks=False),
               dict(train=False, device_masks=False)):
        with pytest.raises(ValueError, match='crowd_ignore'):
            MaskRCNNTransform(None, crowd_ignore=True, **kw)
    t = MaskRCNNTransform(None, train=True, device_masks=True, crowd_ignore=True)
    assert t.crowd_ignore is True
    assert MaskRCNNTransform(None).crowd_ignore is False
    img = np.zeros((8, 9, 3), np.uint8)
    bbox, label, mask = np.zeros((1, 4), np.float32), np.zeros(1, np.int32), np.zeros((1, 8, 9), np.int32)
    with pytest.raises(ValueError, match='crowd_ignore'):
        t((img, bbox, label, mask))                                 # no crowd flags
    with pytest.raises(ValueError, match='crowd'):
        t((img, bbox, label, mask, np.zeros(2, np.int32)))          # one flag per instance
    # off: the accepted lengths are today's
    with pytest.raises(ValueError):
        MaskRCNNTransform(None, train=True)((img, bbox, label, mask, np.zeros(1, np.int32)))


def test_copy_paste_refuses_mixed_lengths(monkeypatch):
    from chainer_mask_rcnn_amd.datasets import CopyPasteDataset
    five = ('img', 'bbox', 'label', 'mask', 1.0)
    six = five + (None,)

    class Two(object):
        def __len__(self):
            return 2

        def __getitem__(self, i):
            return five if i == 0 else six
    cp = CopyPasteDataset(Two(), prob=1.0)
    import random
    monkeypatch.setattr(random, 'randrange', lambda n: 1)
    with pytest.raises(ValueError, match='both'):
        cp[0]
    monkeypatch.setattr(random, 'randrange', lambda n: 0)
    with pytest.raises(ValueError, match='both'):
        cp[1]


def test_converter_leaves_the_planes_a_list():
    import torch
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import train_loop
    finally:
        sys.path.pop(0)
    conv = train_loop.make_converter(None)
    plane = torch.zeros((6, 1), dtype=torch.int64)
    ex = lambda p: (torch.zeros(3, 6, 8), np.zeros((2, 4), np.float32), np.zeros(2, np.int32),
                    torch.zeros((2, 6, 8), dtype=torch.uint8), 1.5, p)
    batch = conv([ex(plane), ex(None)])
    assert len(batch) == 6
    assert isinstance(batch[5], list) and batch[5][0] is plane and batch[5][1] is None
    assert tuple(batch[0].shape) == (2, 3, 6, 8) and isinstance(batch[1], list)
    assert len(conv([ex(None)[:5]])) == 5


def test_train_tool_argument_checks(capsys):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import train
    finally:
        sys.path.pop(0)
    base = ['--dataset', 'coco', '--device-masks']
    assert train.parse_args(base + ['--crowd-ignore']).crowd_ignore == 0.7
    assert train.parse_args(base + ['--crowd-ignore', '0.5']).crowd_ignore == 0.5
    assert not hasattr(train.parse_args(base), 'crowd_ignore')
    assert 'crowd_ignore' not in train.recorded_params(train.parse_args(base))
    assert train.recorded_params(train.parse_args(base + ['--crowd-ignore']))['crowd_ignore'] == 0.7
    for argv, word in ((['--dataset', 'coco', '--crowd-ignore'], '--device-masks'),
                       (['--dataset', 'synthetic', '--device-masks', '--crowd-ignore'], '--dataset coco'),
                       (base + ['--crowd-ignore', '1.5'], '[0, 1]')):
        with pytest.raises(SystemExit) as e:
            train.parse_args(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err
