"""Soft-NMS and box voting on the device (csrc/soft_nms.hip) against the NumPy statement of their
rules in tests/soft_nms_ref.py: keep lists, counts and scores bit for bit for the hard and linear
methods, within the rounding of the double exp for the gaussian one; voted boxes bit for bit; the
model's _suppress and predict_prepared with the options on, and unchanged with them off."""
import numpy as np
import pytest
import torch

from oracle import np_infer
import chainer_mask_rcnn_amd as cmr
from chainer_mask_rcnn_amd.functions import proposal_ops as P

import soft_nms_ref as ref
from test_soft_nms_cpu import random_sorted

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
GARBAGE = np.float32(1e30)          # behind every group's count: must never be read as a score


def make_groups(seed, counts, n_max=None):
    """One random problem per entry of counts, padded to n_max rows with garbage."""
    counts = np.asarray(counts, np.int32)
    n_max = int(n_max or max(int(counts.max()), 1))
    rng = np.random.RandomState(seed)
    bbox = rng.uniform(-1e4, 1e4, (len(counts), n_max, 4)).astype(np.float32)
    prob = np.full((len(counts), n_max), GARBAGE, np.float32)
    for g, n in enumerate(counts):
        if n:
            bbox[g, :n], prob[g, :n] = random_sorted(rng, int(n))
    return bbox, prob, counts


def run_soft_nms(dev, bbox, prob, counts, method, **kw):
    keep, n_keep, soft = P.soft_nms_sorted_batched(
        torch.tensor(bbox, device=dev), torch.tensor(prob, device=dev),
        torch.tensor(counts, device=dev), method, **kw)
    return keep.cpu().numpy(), n_keep.cpu().numpy(), soft.cpu().numpy()


def assert_exact(got, bbox, prob, counts, method, **kw):
    keep, n_keep, soft = got
    kept_fewer = False
    for g, n in enumerate(counts):
        r_keep, r_soft = ref.soft_nms(bbox[g, :n], prob[g, :n], method, **kw)
        assert n_keep[g] == len(r_keep), (g, n_keep[g], len(r_keep))
        assert np.array_equal(keep[g, :n_keep[g]], r_keep), g
        assert np.array_equal(soft[g, :n].view(np.int32), r_soft.view(np.int32)), g
        kept_fewer |= len(r_keep) < n
    return kept_fewer


SINGLE = (1, 2, 63, 64, 65, 129, 257, 1000, 1025)     # wave, workgroup and rows-per-thread edges


@pytest.mark.parametrize('n', SINGLE)
def test_linear_single_group(dev, n):
    bbox, prob, counts = make_groups(n, [n])
    for kw in (dict(), dict(overlap_thresh=0.5, min_score=0.05)):
        assert_exact(run_soft_nms(dev, bbox, prob, counts, 'linear', **kw), bbox, prob, counts,
                     'linear', **kw)


@pytest.mark.parametrize('n', SINGLE)
def test_hard_single_group_is_also_the_bit_mask_nms(dev, n):
    bbox, prob, counts = make_groups(1000 + n, [n])
    got = run_soft_nms(dev, bbox, prob, counts, 'hard', overlap_thresh=0.5)
    fewer = assert_exact(got, bbox, prob, counts, 'hard', overlap_thresh=0.5)
    assert fewer or n < 63
    keep, n_keep = P.nms_sorted_batched(torch.tensor(bbox, device=dev),
                                        torch.tensor(counts, device=dev), 0.5)
    assert np.array_equal(n_keep.cpu().numpy(), got[1])
    assert np.array_equal(keep.cpu().numpy()[0, :got[1][0]], got[0][0, :got[1][0]])


RAGGED = {5: [0, 1, 129, 64, 77],
          80: [0, 1, 70] + [int(v) for v in np.random.RandomState(80).randint(0, 71, 77)]}


@pytest.mark.parametrize('method', ['hard', 'linear'])
@pytest.mark.parametrize('G', sorted(RAGGED))
def test_ragged_groups_read_their_counts(dev, G, method):
    bbox, prob, counts = make_groups(G, RAGGED[G])
    assert counts.min() == 0 and 1 in counts and counts.max() == bbox.shape[1]
    kw = dict(overlap_thresh=0.5) if method == 'hard' else dict()
    got = run_soft_nms(dev, bbox, prob, counts, method, **kw)
    assert_exact(got, bbox, prob, counts, method, **kw)
    if method == 'hard':
        keep, n_keep = P.nms_sorted_batched(torch.tensor(bbox, device=dev),
                                            torch.tensor(counts, device=dev), 0.5)
        keep, n_keep = keep.cpu().numpy(), n_keep.cpu().numpy()
        assert np.array_equal(n_keep, got[1])
        for g in range(G):
            assert np.array_equal(keep[g, :n_keep[g]], got[0][g, :n_keep[g]])


def clustered(rng, n):
    """n boxes in a few tight clusters: most pairs of a cluster overlap by more than 0.3."""
    centres = rng.uniform(40, 160, (4, 2))[rng.randint(0, 4, n)]
    tl = centres + rng.uniform(-6, 6, (n, 2)) - 30
    bbox = np.concatenate([tl, tl + 60 + rng.uniform(-6, 6, (n, 2))], axis=1).astype(np.float32)
    return bbox, random_sorted(rng, n)[1]


def test_ties_and_degenerate_inputs_linear(dev):
    rng = np.random.RandomState(11)
    one = np.ones(1, np.int32)
    # all scores equal: the lowest row wins every tie
    bbox, _ = random_sorted(rng, 100)
    prob = np.full(100, 0.5, np.float32)
    got = run_soft_nms(dev, bbox[None], prob[None], one * 100, 'linear')
    assert_exact(got, bbox[None], prob[None], one * 100, 'linear')
    assert got[0][0, 0] == 0
    # 64 identical boxes: IoU 1, weight 0 from the first pick on
    same = np.tile(np.array([[10, 20, 50, 80]], np.float32), (64, 1))
    prob = random_sorted(rng, 64)[1]
    got = run_soft_nms(dev, same[None], prob[None], one * 64, 'linear')
    assert_exact(got, same[None], prob[None], one * 64, 'linear')
    assert got[1][0] == 1
    # two zero-area boxes: NaN IoU, both kept, scores untouched
    flat = np.array([[[5, 5, 5, 9], [5, 5, 5, 9]]], np.float32)
    prob = np.array([[0.9, 0.8]], np.float32)
    got = run_soft_nms(dev, flat, prob, one * 2, 'linear')
    assert got[1][0] == 2 and np.array_equal(got[0][0], [0, 1]) and np.array_equal(got[2], prob)
    # min_score above every score: nothing kept
    bbox, prob = random_sorted(rng, 65)
    got = run_soft_nms(dev, bbox[None], prob[None], one * 65, 'linear', min_score=0.99)
    assert got[1][0] == 0
    # limits at the wave edge, on an input that keeps all 65 rows without one
    assert len(ref.soft_nms(bbox, prob, 'linear', overlap_thresh=0.5)[0]) == 65
    for limit in (1, 64, 65):
        kw = dict(overlap_thresh=0.5, limit=limit)
        got = run_soft_nms(dev, bbox[None], prob[None], one * 65, 'linear', **kw)
        assert_exact(got, bbox[None], prob[None], one * 65, 'linear', **kw)
        assert got[1][0] == limit


def test_dense_cluster_prunes_below_min_score(dev):
    bbox, prob = clustered(np.random.RandomState(12), 200)
    n = np.array([200], np.int32)
    kw = dict(min_score=0.05)
    r_keep, r_soft = ref.soft_nms(bbox, prob, 'linear', **kw)
    assert 0 < len(r_keep) < 200 and (r_soft < np.float32(0.05)).any()   # the prune path is taken
    fewer = assert_exact(run_soft_nms(dev, bbox[None], prob[None], n, 'linear', **kw),
                         bbox[None], prob[None], n, 'linear', **kw)
    assert fewer


# Gaussian: the device's and NumPy's double exp may differ in the last bit, which can move the
# rounded fp32 weight by one ulp per decay: a score that d picks have decayed is within
# (d + 1) * 2^-23 of the reference, relatively.  The keep lists are equal as long as no decision
# of the reference is closer than that, which is a condition on the inputs, asserted first.
GAUSSIAN_SEEDS = {1: 1, 64: 2, 65: 2, 129: 4}       # the first seeds whose inputs satisfy the condition


@pytest.mark.parametrize('n', sorted(GAUSSIAN_SEEDS))
def test_gaussian_within_the_rounding_of_exp(dev, n):
    bbox, prob, counts = make_groups(GAUSSIAN_SEEDS[n], [n, n, max(n - 1, 1)])
    refs = [ref.soft_nms(bbox[g, :c], prob[g, :c], 'gaussian', with_margin=True)
            for g, c in enumerate(counts)]
    d_max = max(len(r[0]) for r in refs)
    margin = min(r[2] for r in refs)
    print('gaussian n=%d: pick margin %.3g, bound %.3g' % (n, margin, (d_max + 1) * EPS))
    assert margin > 10 * (d_max + 1) * EPS, (margin, d_max)
    keep, n_keep, soft = run_soft_nms(dev, bbox, prob, counts, 'gaussian')
    for g, (r_keep, r_soft, _) in enumerate(refs):
        assert n_keep[g] == len(r_keep)
        assert np.array_equal(keep[g, :n_keep[g]], r_keep)
        got, want = soft[g][r_keep].astype(np.float64), r_soft[r_keep].astype(np.float64)
        bound = (np.arange(len(r_keep)) + 1) * EPS * want
        print('  group %d: worst |got - ref| / bound = %.3g' % (g, np.max(np.abs(got - want) / bound)))
        assert np.all(np.abs(got - want) <= bound)


@pytest.mark.parametrize('source', ['hard', 'linear'])
@pytest.mark.parametrize('G', sorted(RAGGED))
def test_box_vote_bit_exact(dev, G, source):
    bbox, prob, counts = make_groups(300 + G, RAGGED[G])
    if G == 5:
        bbox[2, 0] = [7, 7, 7, 30]                      # a zero-area box with the best score
    kw = dict(overlap_thresh=0.5) if source == 'hard' else dict()
    t = lambda a: torch.tensor(a, device=dev)
    keep, n_keep, _ = P.soft_nms_sorted_batched(t(bbox), t(prob), t(counts), source, **kw)
    keep_h, n_keep_h = keep.cpu().numpy(), n_keep.cpu().numpy()
    for thresh in (0.8, 0.5):
        voted = P.box_vote(t(bbox), t(prob), t(counts), keep, n_keep, thresh).cpu().numpy()
        moved = 0
        for g, n in enumerate(counts):
            rows = keep_h[g, :n_keep_h[g]]
            want = ref.box_vote(bbox[g, :n], prob[g, :n], rows, thresh)
            assert np.array_equal(voted[g][rows].view(np.int32), want.view(np.int32)), (g, thresh)
            moved += int((want != bbox[g][rows]).any(axis=1).sum())
        assert moved > 0
        if G == 5:
            assert keep_h[2, 0] == 0 and np.array_equal(voted[2, 0], bbox[2, 0])


@pytest.mark.parametrize('thresh', [0.8, 0.5])
@pytest.mark.parametrize('n', SINGLE)
def test_box_vote_single_group_sizes(dev, n, thresh):
    """The single-group edges of the suppression tests (n = 257, 1000 and 1025 cross the vote's
    256-row LDS tile), kept rows of the linear kernel, both thresholds."""
    bbox, prob, counts = make_groups(400 + n, [n])
    t = lambda a: torch.tensor(a, device=dev)
    keep, n_keep, _ = P.soft_nms_sorted_batched(t(bbox), t(prob), t(counts), 'linear')
    voted = P.box_vote(t(bbox), t(prob), t(counts), keep, n_keep, thresh).cpu().numpy()
    rows = keep.cpu().numpy()[0, :int(n_keep.cpu().numpy()[0])]
    assert len(rows) > 0
    want = ref.box_vote(bbox[0], prob[0], rows, thresh)
    assert np.array_equal(voted[0][rows].view(np.int32), want.view(np.int32))
    if n >= 129:
        assert (want != bbox[0][rows]).any()             # some box did move


def _bare_model(n_class):
    model = cmr.models.MaskRCNN(None, None, None, mean=None)
    model.head = type('H', (), {'n_class': n_class, 'mask_size': 14})()
    return model


def test_suppress_with_the_options_and_unchanged_without(dev):
    R, n_class = 300, 6
    rng = np.random.RandomState(5)
    tl = rng.uniform(0, 150, (R, n_class, 2))
    cls_bbox = np.concatenate([tl, tl + rng.uniform(4, 100, (R, n_class, 2))], axis=2).astype(np.float32)
    logits = rng.standard_normal((R, n_class)) * 2
    prob = (np.exp(logits) / np.exp(logits).sum(1, keepdims=True)).astype(np.float32)
    model = _bare_model(n_class)
    args = torch.tensor(cls_bbox, device=dev), torch.tensor(prob, device=dev)
    before = model._suppress(*args)
    for g, r in zip(before, np_infer.suppress(cls_bbox, prob, n_class)):
        assert np.array_equal(g, r)

    model.soft_nms, model.bbox_vote_thresh = 'linear', 0.8
    got = model._suppress(*args)
    want = ref.suppress(cls_bbox, prob, n_class, 'linear', bbox_vote_thresh=0.8)
    assert len(want[1]) > len(before[1])                 # Soft-NMS keeps rows the hard rule deletes
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[2].view(np.int32), want[2].view(np.int32))
    assert np.array_equal(got[0].view(np.int32), want[0].view(np.int32))
    plain = ref.suppress(cls_bbox, prob, n_class, 'linear')
    assert (plain[0] != want[0]).any()                   # the vote moved boxes

    model.soft_nms, model.bbox_vote_thresh = None, 0.8   # the vote behind the hard NMS
    got = model._suppress(*args)
    want = ref.suppress(cls_bbox, prob, n_class, None, bbox_vote_thresh=0.8)
    for g, r in zip(got, want):
        assert g.dtype == r.dtype and np.array_equal(g, r)

    model.soft_nms, model.bbox_vote_thresh = None, None
    after = model._suppress(*args)
    for a, b in zip(after, before):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32))


def predict_case(dev, seed=4, sharpen=300.):
    """predict_prepared with gaussian Soft-NMS on the tiny model of tests/test_gpu_inference.py,
    and per image the reference's detections recomputed from the returned head outputs:
    (bbox, label, score after np_infer.finish, d of each, the margin of every decision)."""
    torch.manual_seed(0)
    rng = np.random.RandomState(seed)
    model = cmr.models.MaskRCNNResNet(50, n_fg_class=80, min_size=160, max_size=240,
                                      anchor_scales=(2, 4, 8, 16, 32), roi_size=14,
                                      proposal_creator_params=dict(min_size=0, n_test_pre_nms=300,
                                                                   n_test_post_nms=50)).to(dev)
    with torch.no_grad():
        model.extractor.bn1.W.fill_(1. / 64.)
        model.head.cls_loc_score.W[4 * 81:5 * 81] *= sharpen
    model.soft_nms = 'gaussian'
    imgs = [rng.randint(0, 256, (3, 100, 140)).astype(np.uint8),
            rng.randint(0, 256, (3, 120, 90)).astype(np.uint8)]
    x, sizes, scales = model.prepare(imgs)
    got = model.predict_prepared(x, scales, sizes, return_intermediates=True)
    mid = got[4]
    idx = mid['roi_indices'].cpu().numpy()
    rois, locs = mid['rois'].cpu().numpy(), mid['roi_cls_locs'].cpu().numpy()
    probs = cmr.functions.softmax(mid['roi_scores']).cpu().numpy()
    refs = []
    for i in range(2):
        sel = idx == i
        cls_bbox = np_infer.decode_cls_boxes(rois[sel], np.ascontiguousarray(locs[sel]), 81,
                                             scales[i], sizes[i])
        b, l, s, d, margin = ref.suppress(cls_bbox, probs[sel], 81, 'gaussian', with_picks=True,
                                          with_margin=True)
        # np_infer.finish on (b, l, s), with d carried through the same two selections
        fb, fl, fs = np_infer.finish(b, l, s)
        bbox_int = np.round(b).astype(np.int32)
        ok = (bbox_int[:, 2] - bbox_int[:, 0]) * (bbox_int[:, 3] - bbox_int[:, 1]) > 0
        order = np.arange(len(s))[ok]
        if len(order) > 100:
            # the detections_per_im cut is a decision on the decayed scores too
            by_score = np.sort(s[ok].astype(np.float64))
            margin = min(margin, (by_score[-100] - by_score[-101]) / by_score[-100])
        order = order[np.argsort(s[ok], kind='stable') >= len(order) - 100]
        assert np.array_equal(s[order], fs)
        refs.append((fb, fl, fs, d[order], margin, int(d.max()) if len(d) else 0))
    return got, refs


def test_predict_prepared_with_gaussian_soft_nms(dev):
    """The whole inference path with the option on, against the reference composition fed with the
    head outputs the model returns.  (Measured on this tiny random model: up to 47 picks per
    class, but its boxes are clipped flat, so their IoU is NaN, nothing decays and the margin is
    infinite; the decay itself is covered by the kernel-level tests above.)"""
    (bboxes, roi_masks, labels, scores, _), refs = predict_case(dev)
    total = 0
    for i, (fb, fl, fs, d, margin, d_max) in enumerate(refs):
        # a condition on the inputs, as in test_gaussian_within_the_rounding_of_exp: no decision
        # of the reference is closer than ten times what the rounding of exp can move a score
        print('image %d: %d detections, pick margin %.3g, bound %.3g'
              % (i, len(fb), margin, (d_max + 1) * EPS))
        assert margin > 10 * (d_max + 1) * EPS, (margin, d_max)
        assert len(bboxes[i]) == len(fb) <= 100
        assert np.array_equal(labels[i], fl)
        assert np.array_equal(bboxes[i], fb)
        assert np.all(np.abs(scores[i].astype(np.float64) - fs) <= (d + 1) * EPS * fs)
        assert roi_masks[i].shape == (len(fb), 80, 14, 14) and np.isfinite(roi_masks[i]).all()
        total += len(fb)
    assert total > 0


def test_user_level_soft_nms_maps_back_to_the_callers_order(dev):
    rng = np.random.RandomState(21)
    bbox, prob = random_sorted(rng, 150)
    perm = rng.permutation(150)
    indices, new_scores = P.soft_nms(torch.tensor(bbox[perm], device=dev),
                                     torch.tensor(prob[perm], device=dev))
    keep, soft = ref.soft_nms(bbox, prob, 'linear')
    inverse = np.argsort(perm)                           # sorted row -> the caller's row
    assert indices.dtype == torch.int32 and new_scores.dtype == torch.float32
    assert np.array_equal(indices.cpu().numpy(), inverse[keep])
    assert np.array_equal(new_scores.cpu().numpy(), soft[keep])
    empty = P.soft_nms(torch.zeros((0, 4), device=dev), torch.zeros((0,), device=dev))
    assert empty[0].shape == (0,) and empty[1].shape == (0,)
