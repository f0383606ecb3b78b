"""Boundary AP on the device: the boundary kernel bit for bit against the NumPy statement of the
rule (tests/boundary_ref.py), the host functions, the evaluation functions, both evaluators through
a small model and the results files."""
import numpy as np
import pytest
import torch

import boundary_ref as BR
import instseg_eval_ref as R
import chainer_mask_rcnn_amd as cmr
from chainer_mask_rcnn_amd import _lib
from chainer_mask_rcnn_amd.utils.evaluations import coco_results as CR
from chainer_mask_rcnn_amd.utils.evaluations import masks as M
from chainer_mask_rcnn_amd.utils.evaluations.records import EvalRecords

pytestmark = pytest.mark.gpu


def same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


# ----------------------------------------------------------------------------------- the kernel
CASES, N_MASKS = BR.KERNEL_CASES, BR.N_KERNEL_MASKS
_masks, _packbits, _blob = BR.kernel_masks, BR.packbits, BR.blob


def _run(packed, extent, H, W, d):
    """mrcnn_mask_boundary into buffers pre-filled with ones, so an unwritten word shows."""
    N = packed.shape[0]
    out = torch.full_like(packed, -1)
    area = torch.full((N,), -12345, dtype=torch.int32, device=packed.device)
    nbytes = _lib.load().mrcnn_mask_boundary_workspace_bytes(N, H, W)
    ws = torch.full((max(nbytes, 8),), 0xA5, dtype=torch.uint8, device=packed.device)
    _lib.call('mrcnn_mask_boundary', _lib.ptr(packed), _lib.ptr(extent), N, H, W, d,
              _lib.ptr(out), _lib.ptr(area), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    return out.cpu().numpy(), area.cpu().numpy()


@pytest.mark.parametrize('H,W,d', CASES)
def test_kernel_is_the_rule_bit_for_bit_whatever_the_extent(dev, H, W, d):
    masks = _masks(H, W, d)
    want_bits = BR.boundaries(masks, d)
    want = _packbits(want_bits)
    want_area = want_bits.reshape(N_MASKS, -1).sum(1)
    assert np.array_equal(want_bits[0], ~BR.erode(np.ones((H, W), bool), d))    # a frame of width d
    if H > 2 * d and W > 2 * d:
        frame = np.ones((H, W), bool)
        frame[d:H - d, d:W - d] = False
        assert np.array_equal(want_bits[0], frame)
        square = np.zeros((H, W), bool)                      # the hole's (2d+1)^2 square, and the frame
        square[max(H // 2 - d, 0):H // 2 + d + 1, max(W // 2 - d, 0):W // 2 + d + 1] = True
        square[H // 2, W // 2] = False
        assert np.array_equal(want_bits[3], square | frame)
    Wq = (W + 63) // 64
    packed, area, tight = M.pack_masks(torch.as_tensor(masks.astype(np.uint8), device=dev))
    assert np.array_equal(packed.cpu().numpy(), _packbits(masks))
    whole = torch.tensor([[0, H, 0, Wq]] * N_MASKS, dtype=torch.int32, device=dev)
    rng = np.random.RandomState(d)
    t = tight.cpu().numpy()
    loose = t.copy()
    for n in range(N_MASKS):
        if t[n, 0] < t[n, 1]:                                # a random superset of the tight extent
            loose[n] = [rng.randint(0, t[n, 0] + 1), rng.randint(t[n, 1], H + 1),
                        rng.randint(0, t[n, 2] + 1), rng.randint(t[n, 3], Wq + 1)]
        else:                                                # an empty mask: any extent will do
            loose[n] = [rng.randint(0, H + 1), rng.randint(0, H + 1), 0, rng.randint(0, Wq + 1)]
    loose = torch.tensor(loose, dtype=torch.int32, device=dev)
    for name, extent in (('tight', tight), ('whole', whole), ('loose', loose)):
        got, got_area = _run(packed, extent, H, W, d)
        bad = np.flatnonzero((got != want).reshape(N_MASKS, -1).any(1))
        assert len(bad) == 0, '%s extents: masks %s differ' % (name, bad.tolist())
        assert np.array_equal(got_area, want_area), name
    # N = 1 and N = 0, and the host function (which allocates its own output)
    got, got_area = _run(packed[5:6].contiguous(), tight[5:6].contiguous(), H, W, d)
    assert np.array_equal(got, want[5:6]) and got_area[0] == want_area[5]
    got, got_area = _run(packed[:0], tight[:0], H, W, d)
    assert got.shape == (0, H, Wq) and got_area.shape == (0,)
    b, b_area, b_extent = M.boundary_packed((packed, area, tight), (H, W), dilation=d)
    assert b_extent is tight and b.data_ptr() != packed.data_ptr()
    assert np.array_equal(b.cpu().numpy(), want) and np.array_equal(b_area.cpu().numpy(), want_area)
    e, e_area, _ = M.boundary_packed((packed[:0], area[:0], tight[:0]), (H, W), dilation=d)
    assert e.shape == (0, H, Wq) and e_area.shape == (0,)


def test_dilation_from_the_ratio_and_argument_errors(dev):
    masks = _masks(70, 130, 3)
    p = M.pack_masks(torch.as_tensor(masks.astype(np.uint8), device=dev))
    d = BR.dilation(70, 130, 0.05)
    assert d == 7
    got = M.boundary_packed(p, (70, 130), dilation_ratio=0.05)
    assert np.array_equal(got[0].cpu().numpy(), _packbits(BR.boundaries(masks, d)))
    with pytest.raises(ValueError):
        M.boundary_packed(p, (70, 131 + 64))
    with pytest.raises(ValueError):
        M.boundary_packed(p, (70, 130), dilation=0)
    with pytest.raises(_lib.MrcnnHipError):
        M.boundary_packed(tuple(t.cpu() for t in p), (70, 130))


# --------------------------------------------------------------------------- the host functions
@pytest.mark.parametrize('H,W,d', [(40, 129, 5), (96, 160, None), (66, 130, 70)])
def test_mask_to_boundary_and_boundary_iou_equal_the_reference(dev, H, W, d):
    rng = np.random.RandomState(H + W)
    a = np.stack([_blob(rng, H, W) for _ in range(5)] + [np.zeros((H, W), bool)]).astype(np.uint8)
    b = np.stack([_blob(rng, H, W) for _ in range(3)] + [a[0] != 0]).astype(np.uint8)
    dd = BR.dilation(H, W) if d is None else d
    got = cmr.utils.mask_to_boundary(a, dilation=d)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == a.shape
    assert np.array_equal(got, BR.boundaries(a, dd).astype(np.uint8))
    on_dev = cmr.utils.mask_to_boundary(torch.as_tensor(a, device=dev), dilation=d)
    assert on_dev.is_cuda and np.array_equal(on_dev.cpu().numpy(), got)
    assert cmr.utils.mask_to_boundary(a[:0], dilation=d).shape == (0, H, W)
    inter, aa, ab = cmr.utils.boundary_counts(a, b, dilation=d)
    ri, ra, rb = BR.boundary_counts(a, b, dd)
    assert np.array_equal(inter, ri) and np.array_equal(aa, ra) and np.array_equal(ab, rb)
    iou = cmr.utils.boundary_iou(a, b, dilation=d)
    assert iou.dtype == np.float64 and np.array_equal(iou, BR.boundary_iou(a, b, dd))
    assert iou[0, 3] == 1. and (iou[5] == 0).all() and 0 < iou.max()
    if d is None:
        assert np.array_equal(cmr.utils.boundary_iou(a, b), iou)
        assert cmr.utils.boundary_dilation((H, W)) == dd
    with pytest.raises(ValueError):
        cmr.utils.boundary_iou(a, b[:, :-1])


# --------------------------------------------------------------------- the evaluation functions
@pytest.fixture(scope='module')
def data():
    return BR.crafted_set()


@pytest.mark.parametrize('with_flags', [True, False])
def test_eval_instseg_coco_boundary_equals_the_reference(dev, data, with_flags):
    args = (data['pred_masks'], data['pred_labels'], data['pred_scores'], data['gt_masks'],
            data['gt_labels']) + ((data['gt_crowdeds'], data['gt_areas']) if with_flags else ())
    got = cmr.utils.eval_instseg_coco(*args, iou_type='boundary')
    p, r, cats = BR.coco_eval(*args)
    assert np.array_equal(got['coco_eval']['precision'], p)
    assert np.array_equal(got['coco_eval']['recall'], r)
    assert got['coco_eval']['params']['catIds'] == cats
    want = R.coco_summary(p, r)
    same({k: v for k, v in got.items() if k != 'coco_eval'}, want)
    # the default is what it was
    default = cmr.utils.eval_instseg_coco(*args)
    p0, r0, _ = R.coco_eval(*args)
    assert np.array_equal(default['coco_eval']['precision'], p0)
    same({k: v for k, v in default.items() if k != 'coco_eval'}, R.coco_summary(p0, r0))
    same({k: v for k, v in cmr.utils.eval_instseg_coco(*args, iou_type='segm').items()
          if k != 'coco_eval'}, R.coco_summary(p0, r0))
    key = 'map/iou=0.50:0.95/area=all/maxDets=100'
    assert 0 < got[key] < default[key]
    # a wider boundary is a different measure
    wide = cmr.utils.eval_instseg_coco(*args, iou_type='boundary', dilation_ratio=0.1)
    pw, rw, _ = BR.coco_eval(*args, ratio=0.1)
    assert np.array_equal(wide['coco_eval']['precision'], pw) and not np.array_equal(pw, p)
    with pytest.raises(ValueError):
        cmr.utils.eval_instseg_coco(*args, iou_type='bbox')


@pytest.mark.parametrize('use_07_metric', [False, True])
@pytest.mark.parametrize('with_flags', [True, False])
def test_eval_instseg_voc_boundary_equals_the_reference(dev, data, with_flags, use_07_metric):
    args = (data['pred_masks'], data['pred_labels'], data['pred_scores'], data['gt_masks'],
            data['gt_labels'], data['gt_difficults'] if with_flags else None)
    prec, rec = cmr.utils.calc_instseg_voc_prec_rec(*args, iou_type='boundary')
    want_prec, want_rec = BR.voc_prec_rec(*args)
    assert len(prec) == len(want_prec) and len(rec) == len(want_rec)
    for g, w in zip(prec + rec, want_prec + want_rec):
        assert (g is None and w is None) or np.array_equal(g, w, equal_nan=True)
    got = cmr.utils.eval_instseg_voc(*args, use_07_metric=use_07_metric, iou_type='boundary')
    want = R.voc_ap(want_prec, want_rec, use_07_metric)
    assert np.array_equal(got['ap'], want, equal_nan=True) and got['map'] == np.nanmean(want)
    default = cmr.utils.eval_instseg_voc(*args, use_07_metric=use_07_metric)
    want0 = R.voc_ap(*R.voc_prec_rec(*args), use_07_metric=use_07_metric)
    assert np.array_equal(default['ap'], want0, equal_nan=True)
    assert got['map'] < default['map']
    with pytest.raises(ValueError):
        cmr.utils.eval_instseg_voc(*args, iou_type='bbox')


# ------------------------------------------------------------------------------- the evaluators
@pytest.fixture(scope='module')
def model(dev):
    from test_gpu_detection_eval import _small_model
    return _small_model(dev)


@pytest.fixture(scope='module', params=['voc', 'coco'])
def runs(request, dev, model):
    """The same batches evaluated with and without 'boundary', and ``predict``'s masks for them."""
    from test_gpu_detection_eval import NAMES, _evaluator, _synthetic
    kind = request.param
    examples = _synthetic(np.random.RandomState(11), 5, with_crowd=kind == 'coco')
    batches = [examples[0:2], examples[2:4], examples[4:5]]
    out = dict(kind=kind, data=examples, batches=batches, names=NAMES)
    out['plain_records'] = _evaluator(kind, batches, model).collect()
    out['plain'] = _evaluator(kind, None, model).evaluate_collected(out['plain_records'])
    ev = _evaluator(kind, batches, model, ('segm', 'bbox'))
    out['boxed_records'] = ev.collect()
    out['boxed'] = ev.evaluate_collected(out['boxed_records'])
    ev = _evaluator(kind, batches, model, ('segm', 'bbox', 'boundary'))
    out['records'] = ev.collect()
    out['all'] = ev.evaluate_collected(out['records'])
    ev = _evaluator(kind, batches, model, ('boundary',))
    out['only_records'] = ev.collect()
    out['only'] = ev.evaluate_collected(out['only_records'])
    masks, labels, scores = [], [], []
    for b in batches:                      # same batch composition (padding) as the evaluator
        _, m, l, s = model.predict([ex[0] for ex in b])
        masks += m
        labels += l
        scores += s
    out['predict'] = (masks, labels, scores)
    return out


def test_boundary_keys_equal_the_function_route_on_predict(runs):
    masks, labels, scores = runs['predict']
    examples, names = runs['data'], runs['names']
    assert sum(len(l) for l in labels) > 0
    gm, gl = [ex[3] for ex in examples], [ex[2] for ex in examples]
    if runs['kind'] == 'voc':
        r = cmr.utils.eval_instseg_voc(masks, labels, scores, gm, gl, use_07_metric=True,
                                       iou_type='boundary')
        exp = {'map': r['map']}
        exp.update({'ap/' + n: (r['ap'][l] if l < len(r['ap']) else np.nan)
                    for l, n in enumerate(names)})
    else:
        r = cmr.utils.eval_instseg_coco(masks, labels, scores, gm, gl, [ex[4] for ex in examples],
                                        [ex[5] for ex in examples], iou_type='boundary')
        cats = r['coco_eval']['params']['catIds']
        exp = {'map': r['map/iou=0.50:0.95/area=all/maxDets=100'],
               'map@0.5': r['map/iou=0.50/area=all/maxDets=100'],
               'map@0.75': r['map/iou=0.75/area=all/maxDets=100']}
        per = r['ap/iou=0.50:0.95/area=all/maxDets=100']
        exp.update({'ap/' + n: (per[cats.index(l)] if l in cats else np.nan)
                    for l, n in enumerate(names)})
    got = {k: v for k, v in runs['all'].items() if '/boundary/' in k}
    same(got, {'validation/main/boundary/' + k: v for k, v in exp.items()})


def test_boundary_alone_reports_the_same_keys_and_changes_no_other(runs):
    boundary = {k: v for k, v in runs['all'].items() if '/boundary/' in k}
    assert len(boundary) == (1 if runs['kind'] == 'voc' else 3) + len(runs['names'])
    same(runs['only'], boundary)
    same({k: v for k, v in runs['all'].items() if '/boundary/' not in k}, runs['boxed'])
    same({k: v for k, v in runs['boxed'].items() if '/bbox/' not in k}, runs['plain'])


def test_record_widths(runs):
    n = len(runs['data'])
    assert set(runs['plain_records'].tables) == {'segm'}
    assert set(runs['boxed_records'].tables) == {'segm', 'bbox'}
    assert set(runs['records'].tables) == {'segm', 'bbox', 'boundary'}
    assert set(runs['only_records'].tables) == {'segm', 'boundary'}
    for rec in (runs['records'], runs['only_records']):
        assert all(len(part) == n for part in list(rec.tables.values()) + [
            rec.pred_labels, rec.pred_scores, rec.gt_labels])
        for (inter, pa, ga), (b_inter, b_pa, b_ga) in zip(rec.tables['segm'],
                                                          rec.tables['boundary']):
            assert b_inter.shape == inter.shape and (b_inter <= inter).all()
            assert (b_pa <= pa).all() and (b_ga <= ga).all() and ((b_pa > 0) == (pa > 0)).all()
    assert 'bbox' not in runs['only_records'].tables
    assert all(b is not None for b in runs['records'].tables['bbox'])
    for k in ('segm', 'boundary'):
        for a, b in zip(runs['records'].tables[k], runs['only_records'].tables[k]):
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # the mask counts as they were
    for a, b in zip(runs['records'].tables['segm'], runs['plain_records'].tables['segm']):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_two_shards_merged_equal_the_single_run_at_batch_size_one(runs, model):
    from test_gpu_detection_eval import _evaluator
    kind, examples = runs['kind'], runs['data']
    types = ('segm', 'boundary')
    single = _evaluator(kind, [[ex] for ex in examples], model, types).evaluate()
    shards = [_evaluator(kind, [[ex] for ex in part], model, types).collect()
              for part in (examples[:3], examples[3:])]
    merged = EvalRecords.merge(shards)
    assert set(merged.tables) == {'segm', 'boundary'}
    same(_evaluator(kind, None, model, types).evaluate_collected(merged), single)
    assert any('/boundary/' in k for k in single)


# -------------------------------------------------------------------------------- results files
def test_results_file_scores_the_evaluators_boundary_keys(dev, tmp_path):
    from test_gpu_coco_results import write_coco
    from test_gpu_detection_eval import _small_model
    root = str(tmp_path)
    write_coco(root)
    dataset = cmr.datasets.COCOInstanceSegmentationDataset(
        'minival', root_dir=root, use_crowd=True, return_crowd=True, return_area=True)
    names = list(dataset.class_names)
    model = _small_model(dev, len(names))
    transform = cmr.datasets.MaskRCNNTransform(model, train=False)
    batches = [[transform(dataset[j])] for j in range(len(dataset))]
    path = str(tmp_path / 'res.json')
    with CR.ResultsWriter(path, dataset.img_ids, dataset.class_id_to_cat_id) as w:
        mem = cmr.extensions.InstanceSegmentationCOCOEvaluator(
            batches, model, label_names=names, results_sink=w,
            iou_types=('segm', 'boundary')).evaluate()
    assert w.n_entries > 0
    boundary = {k: v for k, v in mem.items() if '/boundary/' in k}
    assert len(boundary) == 3 + len(names)
    same(CR.eval_coco_results(path, dataset, label_names=names, iou_type='boundary'), boundary)
    same(CR.eval_coco_results(path, dataset, label_names=names),
         {k: v for k, v in mem.items() if '/boundary/' not in k})
    # the sink encodes the masks, not the boundaries: a boundary-only run writes the same file
    other = str(tmp_path / 'only.json')
    with CR.ResultsWriter(other, dataset.img_ids, dataset.class_id_to_cat_id) as w:
        only = cmr.extensions.InstanceSegmentationCOCOEvaluator(
            batches, model, label_names=names, results_sink=w, iou_types=('boundary',)).evaluate()
    same(only, boundary)
    assert open(other).read() == open(path).read()
