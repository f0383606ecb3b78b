"""Device half of the target creators vs the host creators — which
tests/test_targets_cpu.py pins to the oracle and to the reference's own class body — with the
same global np.random seed: sampled sets, labels and mask targets are integer results and must
be identical; regression targets are fp32 (logs) within 1e-6."""
import numpy as np
import pytest
import torch

import chainer_mask_rcnn_amd as cmr
from chainer_mask_rcnn_amd.functions import target_ops as T
from chainer_mask_rcnn_amd.models.utils import ProposalTargetCreator, AnchorTargetCreator
from chainer_mask_rcnn_amd.utils import bbox as B
from oracle import np_ref
from test_targets_cpu import _scene

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_proposal_target_creator_device_matches_host(dev, seed):
    roi, bbox, label, mask, _ = _scene(seed)
    ptc = ProposalTargetCreator(n_sample=128)
    np.random.seed(7)
    ref = ptc(roi, bbox, label, mask)
    after_ref = np.random.randint(0, 2 ** 31 - 1)
    np.random.seed(7)
    s_roi, loc, lab, job = ptc.sample_device(torch.tensor(roi, device=dev), bbox, label)
    after = np.random.randint(0, 2 ** 31 - 1)
    assert after == after_ref                                   # same draws, same stream position
    assert np.array_equal(s_roi.cpu().numpy(), ref[0])
    assert lab.dtype == torch.int32 and np.array_equal(lab.cpu().numpy(), ref[2])
    np.testing.assert_allclose(loc.cpu().numpy(), ref[1], rtol=1e-6, atol=1e-6)
    for m in (torch.tensor(mask, device=dev), torch.tensor(mask != 0, device=dev).to(torch.uint8), mask):
        got = ptc.mask_targets_device(job, m)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), ref[3])
    assert job['n_fg'] == int((ref[2] > 0).sum()) > 0


def test_bbox_iou_argmax_matches_oracle(dev):
    rng = np.random.RandomState(3)
    roi, bbox, _, _, _ = _scene(4, R=3000, G=9)
    roi[5] = roi[6]                                             # exact ties in a row
    bbox[3] = bbox[2]                                           # duplicated ground truth: argmax tie
    best, arg, iou, col = T.bbox_iou_argmax(torch.tensor(roi, device=dev),
                                            torch.tensor(bbox, device=dev), want_matrix=True)
    ref = np_ref.bbox_iou(roi, bbox)
    assert np.array_equal(iou.cpu().numpy(), ref)               # fp32, same operation order
    assert np.array_equal(arg.cpu().numpy(), ref.argmax(1))
    assert np.array_equal(best.cpu().numpy(), ref.max(1))
    assert np.array_equal(col.cpu().numpy(), ref.max(0))


@pytest.mark.parametrize('seed', [0, 1])
def test_anchor_target_creator_device_matches_host(dev, seed):
    _, bbox, _, _, size = _scene(seed)
    ab = B.generate_anchor_base(16, (0.5, 1, 2), (2, 4, 8, 16, 32))
    anchor = B.enumerate_shifted_anchor(ab, 16, size[0] // 16, size[1] // 16)
    atc = AnchorTargetCreator()
    np.random.seed(9)
    loc_ref, label_ref = atc(bbox, anchor, size)
    after_ref = np.random.randint(0, 2 ** 31 - 1)
    np.random.seed(9)
    st = atc.prepare_device(bbox, torch.tensor(anchor, device=dev), anchor, size)
    loc, label = atc.finish_device(st)
    assert np.random.randint(0, 2 ** 31 - 1) == after_ref
    assert np.array_equal(label.cpu().numpy(), label_ref)
    assert (label_ref == 1).sum() > 0 and (label_ref == 0).sum() > 0
    np.testing.assert_allclose(loc.cpu().numpy(), loc_ref, rtol=1e-6, atol=1e-6)


def test_train_chain_device_targets_same_step(dev):
    """MaskRCNNTrainChain.device_targets: same sampled RoIs, labels, mask / RPN targets and the
    same six losses as the host creators (host masks AND device-resident masks)."""
    from test_gpu_model import _build
    model, chain, imgs, bboxes, labels, masks = _build(dev)
    x = torch.tensor(imgs, device=dev)
    out = {}
    for mode in ('host', 'device', 'device-masks'):
        chain.device_targets = mode != 'host'
        mm = masks if mode != 'device-masks' else [torch.tensor(m, device=dev) for m in masks]
        np.random.seed(123)
        with torch.no_grad():
            chain(x, bboxes, labels, mm, [1., 1.])
        t = chain.last_targets
        out[mode] = ({k: t[k].cpu().numpy() for k in ('sample_rois', 'gt_roi_labels', 'gt_roi_masks',
                                                       'gt_rpn_labels')},
                     {k: float(v) for k, v in chain.report.items()}, np.random.randint(0, 2 ** 31 - 1))
    chain.device_targets = False
    for mode in ('device', 'device-masks'):
        for k, v in out['host'][0].items():
            assert np.array_equal(out[mode][0][k], v), (mode, k)
        assert out[mode][2] == out['host'][2]
        for k, v in out['host'][1].items():
            assert abs(out[mode][1][k] - v) <= 1e-6 * max(abs(v), 1e-3), (mode, k)


# ---- the edge matrix, each call under the references of tests/launch_ref.py ---------------------

import launch_ref as L
import target_cases as TC
from chainer_mask_rcnn_amd import _lib

TARGET_ENTRY_POINTS = ('mrcnn_bbox_iou_argmax', 'mrcnn_anchor_labels', 'mrcnn_anchor_targets_finish',
                       'mrcnn_proposal_targets_gather', 'mrcnn_mask_targets')
I32 = torch.int32


@pytest.fixture
def chk(dev, monkeypatch):
    """A LaunchChecker on the five target entry points; every comparison of the test must hold."""
    c = L.LaunchChecker(only=TARGET_ENTRY_POINTS)
    c.install(monkeypatch)
    yield c
    print('\n' + c.table())
    c.assert_clean()
    assert c.stats, 'no target launch was checked'


def _d(a, dev, dtype=None):
    return torch.tensor(np.asarray(a), device=dev, dtype=dtype)


@pytest.mark.parametrize('g', [1, 2, 9, 100])
@pytest.mark.parametrize('na', [1, 255, 256, 257, 2008, 21000, 64260])
def test_bbox_iou_argmax_edges(dev, chk, na, g):
    for degenerate in (False, True):
        a, b = TC.iou_boxes(na, g, degenerate=degenerate)
        at, bt = _d(a, dev), _d(b, dev)
        best, arg, iou, col = T.bbox_iou_argmax(at, bt, want_matrix=True)
        best2, arg2 = T.bbox_iou_argmax(at, bt)
        assert torch.equal(arg, arg2) and np.array_equal(best.cpu().numpy(), best2.cpu().numpy(),
                                                         equal_nan=True)
        ref = L.bbox_iou_f32(a, b)
        assert np.array_equal(iou.cpu().numpy(), ref, equal_nan=True)   # fp32, same operation order
        if degenerate and g >= 2 and na > 5:
            assert np.isnan(ref).any() and np.isnan(col.cpu().numpy()).sum() == 1
    assert chk.launches['mrcnn_bbox_iou_argmax'] == 4


def test_bbox_iou_argmax_no_rows(dev, chk):
    """na = 0 (include/mrcnn_hip.h): nothing is written, col_max included; the wrapper refuses to
    hand out column maxima of no rows, as np.max does."""
    b = _d(TC.iou_boxes(4, 3)[1], dev)
    empty = torch.empty((0, 4), device=dev)
    best, arg = T.bbox_iou_argmax(empty, b)
    assert best.shape == (0,) and arg.shape == (0,)
    with pytest.raises(ValueError):
        T.bbox_iou_argmax(empty, b, want_matrix=True)
    col = torch.full((3,), -7., device=dev)
    iou = torch.empty((0, 3), device=dev)
    _lib.call('mrcnn_bbox_iou_argmax', _lib.ptr(empty), 0, _lib.ptr(b), 3, _lib.ptr(iou),
              _lib.ptr(best), _lib.ptr(arg), _lib.ptr(col), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert (col == -7.).all()


def _label_scenes():
    """(anchors, boxes, neg, pos, expected or None): IoU exactly 0.25 and 0.5 at the thresholds
    (< and >= at equality), an anchor below neg that is a column maximum, a box no anchor overlaps
    (gt_max = 0: every zero-IoU anchor becomes 1), a NaN column (== false everywhere)."""
    A = np.array([[0, 0, 10, 10], [100, 100, 110, 110], [100, 100, 105, 105],
                  [200, 200, 240, 240], [300, 300, 310, 310], [7, 7, 7, 7]], np.float32)
    base = np.array([[0, 0, 10, 5], [100, 100, 105, 105], [200, 200, 210, 210]], np.float32)
    yield A[:5], base, 0.25, 0.5, [1, -1, 1, 1, 0]
    yield A[:5], np.concatenate([base, [[600, 600, 650, 650]]]).astype(np.float32), 0.25, 0.5, [1] * 5
    yield A, np.concatenate([base, [[7, 7, 7, 7]]]).astype(np.float32), 0.25, 0.5, None
    yield A[:5], base, 0.3, 0.7, [1, 0, 1, 1, 0]


def test_anchor_labels_edges(dev, chk):
    for a, b, neg, pos, expected in _label_scenes():
        best, arg, iou, col = T.bbox_iou_argmax(_d(a, dev), _d(b, dev), want_matrix=True)
        label = T.anchor_labels(iou, best, col, neg, pos).cpu().numpy()
        if expected is not None:
            assert label.tolist() == expected
        else:
            assert np.isnan(col.cpu().numpy()).sum() == 1
    # realistic sizes: the inside anchors of an 800 x 1333 image against 100 boxes, one of which
    # no anchor overlaps
    anchor, inside = _full_size_anchors()
    _, b = TC.iou_boxes(8, 100, seed=1)
    b[17] = (5000, 5000, 5100, 5100)
    best, arg, iou, col = T.bbox_iou_argmax(_d(anchor[inside], dev), _d(b, dev), want_matrix=True)
    label = T.anchor_labels(iou, best, col, 0.3, 0.7)
    assert float(col[17]) == 0. and (label == 1).all()
    b[17] = b[16]
    best, arg, iou, col = T.bbox_iou_argmax(_d(anchor[inside], dev), _d(b, dev), want_matrix=True)
    label = T.anchor_labels(iou, best, col, 0.3, 0.7).cpu().numpy()
    assert set(np.unique(label)) == {-1, 0, 1}


def _full_size_anchors():
    ab = B.generate_anchor_base(16, (0.5, 1, 2), (2, 4, 8, 16, 32))
    anchor = B.enumerate_shifted_anchor(ab, 16, 51, 84)
    assert len(anchor) == 64260
    inside = np.where((anchor[:, 0] >= 0) & (anchor[:, 1] >= 0) & (anchor[:, 2] <= 800)
                      & (anchor[:, 3] <= 1333))[0].astype(np.int32)
    return anchor, inside


def _finish_in_bands(dev, a, inside, label_inside, argmax, bbox, disabled, n_anchor):
    """mrcnn_anchor_targets_finish with loc / label inside sentinel-filled buffers: returns
    (loc, label) after asserting that the bands on both sides are unchanged."""
    band = 64
    loc_buf = torch.full((n_anchor * 4 + 2 * band,), -77., device=dev)
    lab_buf = torch.full((n_anchor + 2 * band,), -99, dtype=I32, device=dev)
    loc, lab = loc_buf[band:band + 4 * n_anchor], lab_buf[band:band + n_anchor]
    t = lambda x, dt=None: None if x is None or len(x) == 0 else _d(x, dev, dt)
    keep = [t(a), t(inside, I32), t(label_inside, I32), t(argmax, I32), t(bbox), t(disabled, I32)]
    n_dis = 0 if disabled is None else len(disabled)
    _lib.call('mrcnn_anchor_targets_finish', *[_lib.ptr(x) for x in keep[:5]], len(inside),
              _lib.ptr(keep[5]), n_dis, n_anchor, _lib.ptr(loc), _lib.ptr(lab), _lib.stream_ptr())
    torch.cuda.synchronize()
    for buf, v in ((loc_buf, -77.), (lab_buf, -99)):
        assert (buf[:band] == v).all() and (buf[-band:] == v).all()
    return loc.view(n_anchor, 4).cpu().numpy(), lab.cpu().numpy()


def test_anchor_targets_finish_edges(dev, chk):
    rng = np.random.RandomState(0)
    anchor, inside = _full_size_anchors()
    _, bbox = TC.iou_boxes(8, 9, seed=2)
    cases = []
    a = anchor[inside]
    iou = L.bbox_iou_f32(a, bbox)
    argmax = iou.argmax(1).astype(np.int32)
    label = L.anchor_labels_ref(iou, iou.max(1), iou.max(0), 0.3, 0.7)
    pos, neg = np.where(label == 1)[0], np.where(label == 0)[0]
    assert len(pos) > 4 and len(neg) > 256 and 20000 < len(inside) < len(anchor)
    both = np.concatenate([pos[:len(pos) // 2], neg[:-200]]).astype(np.int32)
    cases.append(('full size', a, inside, label, argmax, both, len(anchor)))
    cases.append(('nothing disabled', a, inside, label, argmax, None, len(anchor)))
    cases.append(('only positives', a, inside, label, argmax, pos[:3].astype(np.int32), len(anchor)))
    cases.append(('only negatives', a, inside, label, argmax, neg[5:300].astype(np.int32), len(anchor)))
    perm = rng.permutation(len(inside))
    cases.append(('unsorted', a[perm], inside[perm], label[perm], argmax[perm],
                  np.arange(0, len(inside), 3, dtype=np.int32), len(anchor)))
    k = 1000
    cases.append(('all inside', a[:k], np.arange(k, dtype=np.int32), label[:k], argmax[:k],
                  np.arange(0, k, 7, dtype=np.int32), k))
    cases.append(('none inside', a[:0], inside[:0], label[:0], argmax[:0], None, 777))
    for name, a_, in_, lab_, am_, dis_, n_anchor in cases:
        loc, lab = _finish_in_bands(dev, a_, in_, lab_, am_, bbox, dis_, n_anchor)
        if name == 'none inside':
            assert (lab == -1).all() and not loc.any()
        else:
            expect = lab_.copy()
            if dis_ is not None:
                expect[dis_] = -1
            assert np.array_equal(lab[in_], expect), name
    assert chk.launches['mrcnn_anchor_targets_finish'] == len(cases)


def test_proposal_targets_gather_edges(dev, chk):
    rng = np.random.RandomState(4)
    cand, bbox = TC.iou_boxes(2100, 100, seed=3)
    cand[10] = (40, 40, 40, 90)                      # zero-height source: the eps clamp
    bbox[5] = (300, 300, 300, 400)                   # zero-height destination: log 0 = -inf
    gt_label = rng.randint(0, 80, 100).astype(np.int32)
    iou = L.bbox_iou_f32(cand, bbox)
    assigned = iou.argmax(1).astype(np.int32)
    assigned[10], assigned[11], assigned[12] = 3, 5, 5
    args = [_d(cand, dev), _d(bbox, dev), _d(gt_label, dev), _d(assigned, dev)]
    uneven = ((0.1, -0.2, 0.3, 0.05), (0.1, 0.3, 0.2, 0.7))
    plain = ((0., 0., 0., 0.), (1., 1., 1., 1.))
    for n, n_fg, (mean, std) in ((1, 0, uneven), (1, 1, uneven), (512, 0, uneven), (512, 512, plain),
                                 (512, 128, uneven), (257, 31, plain)):
        chosen = rng.randint(0, len(cand), n).astype(np.int32)
        if n > 8:
            chosen[:8] = (10, 11, 12, 12, 11, 2099, 0, 10)     # repeats, first, last, degenerate
        s_roi, loc, lab, gi = T.proposal_targets_gather(*args, _d(chosen, dev), n_fg, mean, std)
        loc = loc.cpu().numpy()
        if n > 8:
            assert np.isneginf(loc[1:5, 2]).all() and np.isfinite(loc[0]).all()
            assert np.isfinite(loc[:, [0, 1, 3]]).all()
        if (mean, std) == plain:
            # the header's claim: dy, dx operation for operation as NumPy; dh, dw the double log
            # of the fp32 quotient rounded once.  The device's double log is within 1 ulp (double)
            # of the true value, so after the rounding it is at most one fp32 step from NumPy's
            # double log rounded the same way.
            with np.errstate(divide='ignore'):
                ref = B.bbox2loc(cand[chosen], bbox[assigned[chosen]])
                src, dst = cand[chosen], bbox[assigned[chosen]]
                eps = np.finfo(np.float32).eps
                q = np.stack([(dst[:, 2] - dst[:, 0]) / np.maximum(src[:, 2] - src[:, 0], eps),
                              (dst[:, 3] - dst[:, 1]) / np.maximum(src[:, 3] - src[:, 1], eps)], 1)
                assert q.dtype == np.float32
                once = np.log(q.astype(np.float64)).astype(np.float32)
            assert np.array_equal(loc[:, :2], ref[:, :2])
            fin = np.isfinite(once)
            assert np.array_equal(np.isneginf(loc[:, 2:]), np.isneginf(once))
            step = np.abs(loc[:, 2:][fin] - once[fin]) / np.spacing(np.abs(once[fin]))
            print('dh, dw: %d of %d differ from the once-rounded double log, worst %.1f steps'
                  % ((step > 0).sum(), step.size, step.max()))
            assert (step <= 1).all()
    assert chk.launches['mrcnn_proposal_targets_gather'] == 6


@pytest.fixture(scope='module')
def edge_masks(dev):
    masks = TC.mask_patterns(100)
    return masks, torch.tensor(masks, device=dev)


def test_mask_targets_edges_m14(dev, chk, edge_masks):
    """The crop set of tests/target_cases.py against the literal one-hot / resize / argmax
    reference, after asserting that the hard cases are in it: coordinates at x.5 whose two
    roundings differ, and pixels at exactly prob = 0.5, counted in integer arithmetic."""
    masks, masks_d = edge_masks
    roi, gt = TC.mask_rows(100)
    n = len(roi)
    prob, valid = TC.tie_stats(masks, roi, gt)
    ties = (prob == 392) & valid[:, None, None]
    correct = (prob > 392) & valid[:, None, None]
    mixed = correct.any((1, 2)) & ~correct.all((1, 2))
    print('rows %d, half-way rows %d, tie pixels %d, tie pixels in rows with 0s and 1s %d, empty '
          'crops %d' % (n, TC.halfway_rows(roi).sum(), ties.sum(), ties[mixed].sum(), (~valid).sum()))
    assert n >= 4000 and len(np.unique(gt)) == 100
    assert TC.halfway_rows(roi).sum() >= 100
    assert ties.sum() >= 1000 and ties[mixed].sum() > 0 and (~valid).sum() >= 1
    out = T.mask_targets(masks_d, _d(roi, dev), _d(gt, dev), n, 14).cpu().numpy()
    assert np.array_equal(out, correct.astype(np.int32))          # no row skipped: no -1 anywhere
    assert chk.launches['mrcnn_mask_targets'] == 1


@pytest.mark.parametrize('M', [7, 28])
def test_mask_targets_edges_other_sizes(dev, chk, edge_masks, M):
    masks, masks_d = edge_masks
    roi, gt = TC.mask_rows(100, per_crop=1)
    n = len(roi)
    out = T.mask_targets(masks_d, _d(roi, dev), _d(gt, dev), n, M)
    assert out.shape == (n, M, M) and int(out.min()) == 0 and int(out.max()) == 1
    none = T.mask_targets(masks_d, _d(roi, dev), _d(gt, dev), 0, M)
    assert (none == -1).all()
    some = T.mask_targets(masks_d, _d(roi, dev), _d(gt, dev), n // 3, M)
    assert torch.equal(some[:n // 3], out[:n // 3]) and (some[n // 3:] == -1).all()


def test_mask_targets_input_types(dev, chk, edge_masks):
    """uint8 (values 1, 2, 255), bool and int32 device tensors and a host array give one result."""
    masks, masks_d = edge_masks
    roi, gt = TC.mask_rows(100, per_crop=1)
    ptc = ProposalTargetCreator()
    job = dict(n=len(roi), n_fg=len(roi) - 10, sample_roi=_d(roi, dev), gt_index=_d(gt, dev))
    ref = ptc.mask_targets_device(job, masks_d)
    assert (ref[-10:] == -1).all()
    for m in (masks_d != 0, masks_d.to(torch.int32), masks):
        assert torch.equal(ptc.mask_targets_device(job, m), ref)
    assert chk.launches['mrcnn_mask_targets'] == 4
