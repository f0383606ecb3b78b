"""Test-time augmentation on the device (csrc/test_aug.hip): the union decode against
mrcnn_decode_cls_boxes on every view plus the fp32 un-mirror, the mask combine against the NumPy
statement of its rules (tests/test_aug_ref.py), and MaskRCNN.predict_images against the same path
restated from the model's public pieces; unchanged with the options off."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import chainer_mask_rcnn_amd as cmr
from chainer_mask_rcnn_amd import _lib
from chainer_mask_rcnn_amd.datasets.transforms import flip_bbox
from chainer_mask_rcnn_amd.functions import aug_merge

import test_aug_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN4, STD4 = (0., 0., 0., 0.), (0.1, 0.1, 0.2, 0.2)
GUARD = 1024                         # floats behind every output that must stay untouched
SENTINEL = np.float32(-12345.5)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _guarded(dev, n):
    """A NaN-filled device buffer of n floats with the guard band behind it."""
    host = np.full((n + GUARD,), np.nan, np.float32)
    host[n:] = SENTINEL
    return torch.tensor(host, device=dev)


def _check_guard(buf, n):
    host = buf.cpu().numpy()
    assert np.array_equal(_bits(host[n:]), _bits(np.full((GUARD,), SENTINEL))), 'wrote past the end'
    assert not np.isnan(host[:n]).any(), 'left output unwritten'
    return host[:n]


# ---- decode ------------------------------------------------------------------------------------
SIZE = (200, 333)                    # the original image (H, W)


def make_views(seed, rows, n_class, wide=False):
    """One (roi, cls_loc, scale, flip) per entry of rows, on the host: RoIs in the view's scaled
    frame reaching past every side of the image, cls_loc rows ``ld`` floats apart."""
    rng = np.random.RandomState(seed)
    scales = (0.8, 1.0, 1.7, 0.5, 1.2345, 2.0, 0.61, 1.5)
    views = []
    for v, R in enumerate(rows):
        s = scales[v % len(scales)]
        y0 = rng.uniform(-30, SIZE[0] * s, R)
        x0 = rng.uniform(-30, SIZE[1] * s, R)
        roi = np.stack([y0, x0, y0 + rng.uniform(1, 150, R) * s, x0 + rng.uniform(1, 150, R) * s],
                       1).astype(np.float32)
        ld = 4 * n_class + (12 if wide else 0)
        loc = rng.standard_normal((R, ld)).astype(np.float32) * 3
        views.append((roi, loc, s, bool((v + seed) % 2)))
    return views


def decode_one(dev, roi, loc, n_class, scale):
    """mrcnn_decode_cls_boxes on one view: the entry point the plain path uses."""
    R = roi.shape[0]
    roi_d, loc_d = torch.tensor(roi, device=dev), torch.tensor(loc, device=dev)
    out = torch.empty((R, n_class, 4), dtype=torch.float32, device=dev)
    mean = (ctypes.c_double * 4)(*MEAN4)
    std = (ctypes.c_double * 4)(*STD4)
    _lib.call('mrcnn_decode_cls_boxes', _lib.ptr(roi_d), _lib.ptr(loc_d), loc.shape[1], _lib.ptr(out),
              R, n_class, float(scale), mean, std, float(SIZE[0]), float(SIZE[1]), _lib.stream_ptr())
    return out.cpu().numpy()


def decode_views_guarded(dev, views, n_class):
    total = sum(v[0].shape[0] for v in views)
    recs = (_lib.TestAugView * max(len(views), 1))()
    keep = []
    for i, (roi, loc, scale, flip) in enumerate(views):
        roi_d, loc_d = torch.tensor(roi, device=dev), torch.tensor(loc, device=dev)
        keep.append((roi_d, loc_d))
        R = roi.shape[0]
        recs[i] = _lib.TestAugView(roi_d.data_ptr() if R else None, loc_d.data_ptr() if R else None,
                                   loc.shape[1], R, float(scale), int(flip))
    n = total * n_class * 4
    buf = _guarded(dev, n)
    mean = (ctypes.c_double * 4)(*MEAN4)
    std = (ctypes.c_double * 4)(*STD4)
    _lib.call('mrcnn_decode_cls_boxes_views', recs, len(views), n_class, mean, std, float(SIZE[0]),
              float(SIZE[1]), _lib.ptr(buf), _lib.stream_ptr())
    torch.cuda.synchronize()
    return _check_guard(buf, n).reshape(total, n_class, 4)


DECODE_CASES = [
    # rows per view, n_class, ld_loc wider than 4 * n_class
    ((300,), 81, False),
    ((1,), 2, True),
    ((0,), 81, False),
    ((0, 300), 2, False),
    ((63, 0), 81, True),
    ((300, 63), 81, False),
    ((0, 1, 63, 300, 0, 300, 1, 0), 81, False),
    ((300, 0, 0, 63, 1, 63, 300, 1), 2, True),
    ((63, 300, 1, 0, 300, 0, 63, 300), 81, True),
    ((0, 0, 0, 0, 0, 0, 0, 0), 2, False),
]


@pytest.mark.parametrize('rows,n_class,wide', DECODE_CASES)
def test_decode_views_equals_every_views_decode_and_unmirror(dev, rows, n_class, wide):
    views = make_views(len(rows) + n_class, rows, n_class, wide)
    got = decode_views_guarded(dev, views, n_class)
    per_view = [decode_one(dev, roi, loc, n_class, s) for roi, loc, s, _ in views]
    flips = [f for _, _, _, f in views]
    want = ref.union_boxes(per_view, flips, SIZE[1])
    assert got.shape == want.shape
    assert np.array_equal(_bits(got), _bits(want))
    lo = 0
    for b, f in zip(per_view, flips):                 # an unmirrored view: the plain decode's bits
        if not f:
            assert np.array_equal(_bits(got[lo:lo + len(b)]), _bits(b))
        lo += len(b)
    if sum(rows) >= 300:
        # the clip clips on every side, and not everything: the un-mirror acts on clipped boxes
        flat = np.concatenate(per_view).reshape(-1, 4)
        assert (flat[:, 0] == 0).any() and (flat[:, 1] == 0).any()
        assert (flat[:, 2] == SIZE[0]).any() and (flat[:, 3] == SIZE[1]).any()
        inside = (flat[:, 0] > 0) & (flat[:, 1] > 0) & (flat[:, 2] < SIZE[0]) & (flat[:, 3] < SIZE[1])
        assert inside.any()
        if len(rows) > 1:
            assert any(flips) and not all(flips)
    assert (got[..., 1] >= 0).all() and (got[..., 3] <= SIZE[1]).all()
    assert (got[..., 1] <= got[..., 3]).all()


def test_decode_views_wrapper(dev):
    views = make_views(3, (63, 0, 300), 81, wide=True)
    dev_views = []
    for roi, loc, s, f in views:
        loc_d = torch.tensor(loc, device=dev)[:, :4 * 81]          # strided: ld_loc > 4 * n_class
        dev_views.append((torch.tensor(roi, device=dev), loc_d, s, f))
    got = aug_merge.decode_cls_boxes_views(dev_views, 81, MEAN4, STD4, SIZE).cpu().numpy()
    want = decode_views_guarded(dev, views, 81)
    assert np.array_equal(_bits(got), _bits(want))
    assert aug_merge.decode_cls_boxes_views(
        [(torch.zeros((0, 4), device=dev), torch.zeros((0, 8), device=dev), 1., True)], 2, MEAN4,
        STD4, SIZE).shape == (0, 2, 4)


# ---- combine -----------------------------------------------------------------------------------
def make_maps(seed, V, D, M, Kc):
    rng = np.random.RandomState(seed)
    maps = [rng.uniform(-50, 50, (D, M, M, Kc)).astype(np.float32) for _ in range(V)]
    if D:
        for v, m in enumerate(maps):
            m[0, 0] = 300. if v % 2 else -300.          # saturated, the views disagreeing
            m[0, 1] = -300.                             # saturated, the views agreeing
            m[0, 2] = 300.
            m[0, 3] = 0.                                # exact zeros in every view
            m[0, 4, :, 0] = 0. if v else 7.25           # zeros against one value
    return maps


def combine_guarded(dev, maps, flips, heur, misalign=0):
    """mrcnn_mask_aug_combine into a guarded buffer; ``misalign``: floats by which every map and
    the output are shifted off their 16-byte alignment."""
    D, M, _, Kc = maps[0].shape
    n = D * M * M * Kc
    bufs = [torch.zeros((n + 4,), dtype=torch.float32, device=dev) for _ in maps]
    for b, m in zip(bufs, maps):
        b[misalign:misalign + n] = torch.tensor(m.reshape(-1), device=dev)
    out = _guarded(dev, n + misalign)
    ptrs = (_lib.c_vp * len(maps))(*[b.data_ptr() + 4 * misalign for b in bufs])
    flags = (ctypes.c_int32 * len(maps))(*[int(f) for f in flips])
    _lib.call('mrcnn_mask_aug_combine', ptrs, flags, len(maps), D, M, Kc,
              _lib.MASK_AUG_HEURS[heur], ctypes.c_void_p(out.data_ptr() + 4 * misalign),
              _lib.stream_ptr())
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert np.array_equal(_bits(host[n + misalign:]), _bits(np.full((GUARD,), SENTINEL)))
    assert np.isnan(host[:misalign]).all()
    got = host[misalign:misalign + n]
    assert not np.isnan(got).any(), 'left output unwritten'
    return got.reshape(D, M, M, Kc)


def check_combine(got, maps, flips, heur):
    want = ref.mask_aug_combine(maps, flips, heur)
    assert got.shape == want.shape and np.isfinite(want).all()
    if heur != 'soft_avg':
        assert np.array_equal(_bits(got), _bits(want)), heur
        return
    # both sides do the same double operations (relative error 2^-52 each, exp and log within an
    # ulp of double), so the fp32 results differ only where the double value falls on a rounding
    # boundary: one fp32 ulp, plus a few thousand double ulps of O(1) logarithms where P ~ Q
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    bound = 2.0 ** -23 * np.abs(want.astype(np.float64)) + 2.0 ** -40
    same = float(np.mean(_bits(got) == _bits(want))) if want.size else 1.0
    print('soft_avg: %.4f%% of %d entries bit-equal, max err / bound %.3g'
          % (100 * same, want.size, float((err / bound).max()) if want.size else 0.))
    assert (err <= bound).all()


def _flips(mode, V):
    return {'none': [False] * V, 'all': [True] * V,
            'mixed': [bool(v % 2) for v in range(V)] if V > 1 else [True]}[mode]


COMBINE_CASES = [
    # D, M, Kc, V, mirrored views
    (100, 14, 80, 2, 'mixed'),       # the real problem: 16-byte loads
    (3, 14, 80, 8, 'mixed'),
    (3, 7, 80, 3, 'all'),            # odd M: the middle column maps to itself
    (1, 28, 80, 1, 'none'),
    (1, 28, 80, 1, 'all'),
    (100, 7, 3, 2, 'all'),           # scalar loads
    (3, 28, 3, 8, 'none'),
    (3, 14, 1, 3, 'mixed'),
    (1, 7, 1, 2, 'mixed'),
    (100, 28, 1, 1, 'all'),
    (3, 7, 3, 1, 'none'),
    (1, 14, 3, 8, 'all'),
]


@pytest.mark.parametrize('heur', ref.HEURS)
@pytest.mark.parametrize('D,M,Kc,V,mode', COMBINE_CASES)
def test_mask_combine_equals_reference(dev, D, M, Kc, V, mode, heur):
    maps = make_maps(D + M + Kc + V, V, D, M, Kc)
    flips = _flips(mode, V)
    got = combine_guarded(dev, maps, flips, heur)
    check_combine(got, maps, flips, heur)
    if V == 1 and mode == 'none' and heur != 'soft_avg':
        assert np.array_equal(_bits(got), _bits(maps[0]))


@pytest.mark.parametrize('heur', ref.HEURS)
def test_mask_combine_off_alignment_takes_scalar_loads(dev, heur):
    maps = make_maps(11, 3, 3, 14, 80)
    flips = [False, True, True]
    got = combine_guarded(dev, maps, flips, heur, misalign=1)
    check_combine(got, maps, flips, heur)
    aligned = combine_guarded(dev, maps, flips, heur)
    assert np.array_equal(_bits(got), _bits(aligned))              # one result on both load paths


@pytest.mark.parametrize('heur', ref.HEURS)
@pytest.mark.parametrize('M,Kc', [(14, 80), (7, 3)])
def test_mask_combine_of_nothing_launches_nothing(dev, heur, M, Kc):
    maps = [np.zeros((0, M, M, Kc), np.float32)] * 2
    assert combine_guarded(dev, maps, [False, True], heur).shape == (0, M, M, Kc)
    empty = torch.zeros((0, Kc, M, M), device=dev)
    assert aug_merge.mask_aug_combine([empty, empty], [False, True], heur).shape == (0, Kc, M, M)


def test_mask_combine_wrapper_takes_the_heads_layout(dev):
    maps = make_maps(5, 3, 3, 14, 80)
    flips = [False, True, False]
    # the head's tensors: logical (D, Kc, M, M) over NHWC memory; one given as plain NCHW memory
    tens = [torch.tensor(m, device=dev).permute(0, 3, 1, 2) for m in maps]
    tens[2] = tens[2].contiguous()
    for heur in ref.HEURS:
        out = aug_merge.mask_aug_combine(tens, flips, heur)
        assert tuple(out.shape) == (3, 80, 14, 14)
        check_combine(out.permute(0, 2, 3, 1).contiguous().cpu().numpy(), maps, flips, heur)


# ---- model ---------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def setup(dev):
    """The small ResNet-50 of the other model tests and two images of different sizes."""
    torch.manual_seed(0)
    rng = np.random.RandomState(4)
    model = cmr.models.MaskRCNNResNet(50, n_fg_class=80, min_size=160, max_size=240,
                                      anchor_scales=(2, 4, 8, 16, 32), roi_size=14,
                                      proposal_creator_params=dict(min_size=0, n_test_pre_nms=300,
                                                                   n_test_post_nms=50)).to(dev)
    from chainer_mask_rcnn_amd.models.resnet_extractor import Bottleneck
    with torch.no_grad():
        # no trained weights: keep the activations O(1) (the recipe of tests/test_gpu_inference.py:
        # test_c5_full_size_predict) and spread the class scores a little
        model.extractor.bn1.W.fill_(1. / 64.)
        for m in model.modules():
            if isinstance(m, Bottleneck):
                m.bn3.W.fill_(0.25)
                if m.projection:
                    m.bn4.W.fill_(0.5)
        model.head.cls_loc_score.W[4 * 81:5 * 81] *= 10.
    model.score_thresh = SCORE_THRESH
    model.eval()
    imgs = [rng.randint(0, 256, (3, 100, 140)).astype(np.uint8),
            rng.randint(0, 256, (3, 120, 90)).astype(np.uint8)]
    return model, imgs


# these random weights give class probabilities of 0.005 .. 0.06: at this threshold most RoIs are
# candidates in several classes, some thirty classes keep boxes and the cut to detections_per_im
# decides (at the default 0.05 an image keeps rows of four classes only)
SCORE_THRESH = 0.005


def _reset(model):
    model.test_aug_h_flip, model.test_aug_scales = False, ()
    model.test_aug_max_size, model.test_aug_scale_h_flip = None, False
    model.mask_aug_heur = 'soft_avg'
    model.soft_nms, model.bbox_vote_thresh = None, None


def test_options_off_is_prepare_and_predict_prepared(dev, setup):
    model, imgs = setup
    _reset(model)
    x, sizes, scales = model.prepare(imgs)
    want = model.predict_prepared(x, scales, sizes, return_intermediates=True)
    got = model.predict_images(imgs)
    assert len(got) == 5 and got[4] == sizes == [(100, 140), (120, 90)]
    for i in range(2):
        print('image %d: %d detections' % (i, len(want[0][i])))
        assert len(want[0][i]) >= 20
        for k in range(4):
            assert got[k][i].dtype == want[k][i].dtype and got[k][i].shape == want[k][i].shape
            assert np.array_equal(got[k][i].view(np.int32), want[k][i].view(np.int32)), (i, k)
    on_device = model.predict_images(imgs, masks_to_host=False)
    for i in range(2):
        assert on_device[1][i].is_cuda
        assert np.array_equal(on_device[1][i].cpu().numpy().view(np.int32), want[1][i].view(np.int32))
    # predict goes the same way
    b, m, l, s = model.predict(imgs)
    for i in range(2):
        assert np.array_equal(b[i], want[0][i]) and np.array_equal(l[i], want[2][i])
        assert m[i].shape == (len(b[i]),) + imgs[i].shape[1:] and m[i].dtype == bool


def restate(model, imgs, dev):
    """predict_images with views, from the public pieces: per view prepare / extractor /
    rpn.propose / head, the existing decode entry point, the NumPy un-mirror and concatenation,
    the model's suppression; then the per-view mask passes.  Returns (bboxes, labels, scores,
    per-image list of the views' (D, M, M, Kc) host maps, flips)."""
    views = model.test_aug_views()
    n_img, n_class = len(imgs), model.n_class
    mean = (ctypes.c_double * 4)(*model.loc_normalize_mean)
    std = (ctypes.c_double * 4)(*model.loc_normalize_std)
    passes = []
    with torch.no_grad():
        for min_size, max_size, flip in views:
            x, sizes, scales = model.prepare(imgs, x_flips=[flip] * n_img, min_size=min_size,
                                             max_size=max_size)
            h = model.extractor(x)
            prop = model.rpn.propose(h, x.shape[2:], scales)
            bounds = np.concatenate([[0], np.cumsum(prop.counts)]).astype(int)
            boxes, probs = [], []
            for i in range(n_img):
                roi = prop.rois[bounds[i]:bounds[i + 1]].contiguous()
                loc, score, _ = model.head(h, roi, prop.roi_indices[bounds[i]:bounds[i + 1]],
                                           pred_mask=False)
                loc = loc.contiguous()
                R = roi.shape[0]
                cls_bbox = torch.empty((R, n_class, 4), dtype=torch.float32, device=dev)
                _lib.call('mrcnn_decode_cls_boxes', _lib.ptr(roi), _lib.ptr(loc), loc.stride(0),
                          _lib.ptr(cls_bbox), R, n_class, float(scales[i]), mean, std,
                          float(sizes[i][0]), float(sizes[i][1]), _lib.stream_ptr())
                boxes.append(cls_bbox.cpu().numpy())
                probs.append(cmr.functions.softmax(score))
            passes.append((h, scales, boxes, probs))
    flips = [f for _, _, f in views]
    bboxes, labels, scores = [], [], []
    for i in range(n_img):
        union = ref.union_boxes([p[2][i] for p in passes], flips, sizes[i][1])
        prob = torch.cat([p[3][i] for p in passes], dim=0)
        b, l, s = model._finish_detections(
            model._suppress_queue(torch.tensor(union, device=dev), prob))
        bboxes.append(b)
        labels.append(l)
        scores.append(s)
    maps = [[] for _ in range(n_img)]
    for (h, scales, _, _), flip in zip(passes, flips):
        boxes = [flip_bbox(b, size, x_flip=True) if flip else b for b, size in zip(bboxes, sizes)]
        for i, m in enumerate(model._roi_masks_group(h, boxes, list(range(n_img)), scales)):
            maps[i].append(m.permute(0, 2, 3, 1).contiguous().cpu().numpy())
    return bboxes, labels, scores, maps, flips


VIEW_SETS = {
    'h_flip': dict(test_aug_h_flip=True),
    'scale_and_its_flip': dict(test_aug_scales=(120,), test_aug_scale_h_flip=True,
                               test_aug_max_size=200),
}


@pytest.mark.parametrize('name', sorted(VIEW_SETS))
def test_predict_images_with_views_equals_the_restated_path(dev, setup, name):
    model, imgs = setup
    _reset(model)
    for k, v in VIEW_SETS[name].items():
        setattr(model, k, v)
    try:
        n_views = len(model.test_aug_views())
        assert n_views == (2 if name == 'h_flip' else 3)
        bboxes, labels, scores, maps, flips = restate(model, imgs, dev)
        for heur in ref.HEURS:
            model.mask_aug_heur = heur
            got = model.predict_images(imgs)
            assert got[4] == [(100, 140), (120, 90)]
            for i in range(2):
                assert len(bboxes[i]) >= 20
                for g, w in ((got[0][i], bboxes[i]), (got[2][i], labels[i]), (got[3][i], scores[i])):
                    assert g.dtype == w.dtype and g.shape == w.shape
                    assert np.array_equal(g.view(np.int32), w.view(np.int32)), (heur, i)
                assert got[1][i].shape == (len(bboxes[i]), 80, 14, 14)
                assert got[1][i].dtype == np.float32
                check_combine(np.ascontiguousarray(got[1][i].transpose(0, 2, 3, 1)), maps[i], flips,
                              heur)
        # the views add candidates: the union is not the identity view's result
        _reset(model)
        plain = model.predict_images(imgs)
        assert any(len(plain[0][i]) != len(bboxes[i]) or not np.array_equal(plain[0][i], bboxes[i])
                   for i in range(2))
    finally:
        _reset(model)


def test_soft_nms_and_voting_decide_the_union(dev, setup):
    model, imgs = setup
    _reset(model)
    model.test_aug_h_flip, model.test_aug_scales, model.test_aug_scale_h_flip = True, (120,), True
    model.soft_nms, model.bbox_vote_thresh = 'linear', 0.8
    try:
        assert len(model.test_aug_views()) == 4
        bboxes, roi_masks, labels, scores, sizes = model.predict_images(imgs, masks_to_host=False)
        for i, (H, W) in enumerate(sizes):
            b = bboxes[i]
            assert 0 < len(b) <= 100 and len(labels[i]) == len(scores[i]) == len(b)
            assert (b[:, :2] >= 0).all() and (b[:, 2] <= H).all() and (b[:, 3] <= W).all()
            assert (b[:, 2] >= b[:, 0]).all() and (b[:, 3] >= b[:, 1]).all()
            assert roi_masks[i].is_cuda and tuple(roi_masks[i].shape) == (len(b), 80, 14, 14)
            assert torch.isfinite(roi_masks[i]).all()
        # more rows than one Soft-NMS workgroup holds: the error says what the rows are
        big = torch.zeros((4097, 81, 4), device=dev), torch.zeros((4097, 81), device=dev)
        with pytest.raises(ValueError, match='4096.*4097.*union of 5 test-time augmentation views'):
            model._suppress_queue(*big, n_views=5)
        with pytest.raises(ValueError) as plain:
            model._suppress_queue(*big)
        assert 'views' not in str(plain.value)
    finally:
        _reset(model)


def test_evaluate_tool_with_h_flip(dev, tmp_path):
    out = str(tmp_path / 'aug_eval.json')
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'evaluate.py'), '--synthetic', '2',
           '--test-aug-h-flip', '--out', out]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    path = out if os.path.exists(out) else os.path.splitext(out)[0] + '.json'
    text = open(path).read()
    try:
        payload = json.loads(text)
    except ValueError:                      # YAML when PyYAML is installed
        import yaml
        payload = yaml.safe_load(text)
    post = payload['postprocessing']
    assert post['test_aug_views'] == [[800, 1333, False], [800, 1333, True]]
    assert post['mask_aug_heur'] == 'soft_avg'
    assert payload['timing']['images'] == 2
