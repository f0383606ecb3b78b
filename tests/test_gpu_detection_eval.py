"""Box AP on the GPU: the ragged box-IoU launch bit-identical to the NumPy reference in both
conventions, eval_detection_voc / eval_detection_coco equal to the host matching fed NumPy
tables, the evaluators' ``bbox/`` keys equal to those functions fed ``predict``'s boxes (with the
segm keys untouched), the sharded route, and bbox results files."""
import json

import numpy as np
import pytest
import torch

import detection_eval_ref as R
import chainer_mask_rcnn_amd as cmr
from chainer_mask_rcnn_amd.utils.evaluations import boxes as B
from chainer_mask_rcnn_amd.utils.evaluations import coco_results as CR
from chainer_mask_rcnn_amd.utils.evaluations import matching
from chainer_mask_rcnn_amd.utils.evaluations.records import EvalRecords, Readback

pytestmark = pytest.mark.gpu

NAMES = ['c%d' % l for l in range(80)]


def same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), (k, a[k], b[k])


# --------------------------------------------------------------------------------------- kernel
def _as_bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32 if x.dtype == np.float32 else np.int64)


@pytest.mark.parametrize('on_device', [False, True])
@pytest.mark.parametrize('convention', ['voc', 'coco'])
def test_ragged_batch_is_bit_identical_to_numpy(dev, convention, on_device):
    A, Bx, C = R.ragged_kernel_batch()
    if convention == 'voc':
        a, b, crowd = A, Bx, None
        want = [R.voc_iou(x, y) for x, y in zip(a, b)]
        dtype = np.float32
    else:
        a, b, crowd = [R.xywh64(x) for x in A], [R.xywh64(x) for x in Bx], C
        assert np.array_equal(B.to_xywh64(A[3]), a[3])
        want = [R.bb_iou(x, y, c) for x, y, c in zip(a, b, crowd)]
        plain = R.bb_iou(a[3], b[3])
        dtype = np.float64
    if on_device:
        a = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in a]
        b = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in b]
    iou, shapes = B.queue_box_ious(a, b, convention, crowd_b=crowd)
    assert shapes == [(0, 3), (5, 0), (1, 1), (100, 7), (65, 64)]
    assert iou.is_cuda and iou.shape == (1 + 700 + 65 * 64,)
    readback = Readback()
    readback.add_split(iou, shapes)
    got = readback.fetch()
    for g, w in zip(got, want):
        assert g.dtype == dtype and w.dtype == dtype and g.shape == w.shape
        assert np.array_equal(_as_bits(g), _as_bits(w))
    # the cases the batch is built around, from the reference's side
    t = want[3]
    assert abs(want[2][0, 0] - 1) < 1e-12 and t[5, 3] == (1 if convention == 'voc' else 0)
    if convention == 'voc':       # a shared edge is a one-pixel-wide overlap: 41 / (41*41 + 41*31 - 41)
        assert t[1, 1] == np.float32(41.) / np.float32(41 * 41 + 41 * 31 - 41)
        assert t[4, 1] > 0                                 # zero width counts one pixel column
    else:
        assert t[1, 1] == 0 and t[2, 1] == 0 and t[4, 1] == 0 and t[6, 4] == 0
        for k in (5, 6):                                   # crowd columns: i / detection area
            assert (t[:, k] >= plain[:, k]).all() and (t[:, k] > plain[:, k]).any()
        assert np.array_equal(t[:, :5], plain[:, :5])
    assert 0 < t[3, 1] < 1 and t[3, 2] < t[3, 1]            # nested pairs


@pytest.mark.parametrize('convention', ['voc', 'coco'])
def test_batches_without_pairs_return_without_a_launch(dev, convention):
    z = np.zeros((0, 4), np.float32)
    some = np.array([[0, 0, 5, 5], [1, 2, 3, 4]], np.float32)
    for a, b in (([z, some], [some, z]), ([z], [z]), ([], [])):
        iou, shapes = B.queue_box_ious(a, b, convention)
        torch.cuda.synchronize()
        assert iou.shape == (0,) and shapes == [(len(x), len(y)) for x, y in zip(a, b)]
        readback = Readback()
        readback.add_split(iou, shapes)
        assert [t.shape for t in readback.fetch()] == shapes
    with pytest.raises(ValueError):
        B.queue_box_ious([some], [some, some], convention)


# ------------------------------------------------------------------- eval_detection_{voc, coco}
def _random_detections(seed, n_img=7, n_class=5):
    rng = np.random.RandomState(seed)
    out = dict(pb=[], pl=[], ps=[], gb=[], gl=[], gc=[], ga=[], gd=[])

    def boxes(n):
        y1, x1 = rng.uniform(0, 300, n), rng.uniform(0, 400, n)
        return np.stack([y1, x1, y1 + rng.uniform(1, 150, n), x1 + rng.uniform(1, 150, n)],
                        1).astype(np.float32).reshape(n, 4)
    for i in range(n_img):
        G = 0 if i == 2 else rng.randint(1, 8)
        P = 0 if i == 4 else rng.randint(1, 30)
        gb, pb = boxes(G), boxes(P)
        gl, pl = rng.randint(0, n_class, G).astype(np.int32), rng.randint(0, n_class, P).astype(np.int32)
        for p in range(P):                            # most detections near a ground truth
            if G and rng.uniform() < 0.7:
                g = rng.randint(G)
                pb[p] = gb[g] + rng.uniform(-12, 12, 4).astype(np.float32)
                pb[p, 2:] = np.maximum(pb[p, 2:], pb[p, :2])
                pl[p] = gl[g]
        out['pb'].append(pb)
        out['pl'].append(pl)
        out['ps'].append(rng.uniform(0.05, 1, P).astype(np.float32))
        out['gb'].append(gb)
        out['gl'].append(gl)
        out['gc'].append((rng.uniform(size=G) < 0.25).astype(np.int32))
        out['gd'].append(rng.uniform(size=G) < 0.25)
        out['ga'].append(rng.uniform(100, 20000, G).astype(np.float32))
    return out


@pytest.mark.parametrize('difficult', [False, True])
@pytest.mark.parametrize('use_07_metric', [False, True])
def test_eval_detection_voc_equals_numpy_table_route(dev, difficult, use_07_metric):
    d = _random_detections(1)
    gd = d['gd'] if difficult else None
    got = cmr.utils.eval_detection_voc(d['pb'], d['pl'], d['ps'], d['gb'], d['gl'], gd,
                                       use_07_metric=use_07_metric)
    tables = [R.voc_iou(p, g) for p, g in zip(d['pb'], d['gb'])]
    prec, rec = matching.voc_prec_rec_from_ious(tables, d['pl'], d['ps'], d['gl'], gd)
    ap = matching.calc_detection_voc_ap(prec, rec, use_07_metric=use_07_metric)
    assert sorted(got) == ['ap', 'map']
    assert np.array_equal(got['ap'], ap, equal_nan=True) and got['map'] == np.nanmean(ap)
    assert 0 < got['map'] < 1
    # another threshold, and device tensors in
    got = cmr.utils.eval_detection_voc([torch.from_numpy(b).to(dev) for b in d['pb']], d['pl'],
                                       d['ps'], d['gb'], d['gl'], gd, iou_thresh=0.75)
    prec, rec = matching.voc_prec_rec_from_ious(tables, d['pl'], d['ps'], d['gl'], gd,
                                                iou_thresh=0.75)
    assert np.array_equal(got['ap'], matching.calc_detection_voc_ap(prec, rec), equal_nan=True)


@pytest.mark.parametrize('areas', [False, True])
@pytest.mark.parametrize('crowds', [False, True])
def test_eval_detection_coco_equals_numpy_table_route(dev, crowds, areas):
    d = _random_detections(2)
    gc = d['gc'] if crowds else None
    ga = d['ga'] if areas else None
    got = cmr.utils.eval_detection_coco(d['pb'], d['pl'], d['ps'], d['gb'], d['gl'], ga, gc)
    px, gx = [R.xywh64(b) for b in d['pb']], [R.xywh64(b) for b in d['gb']]
    tables = [(R.bb_iou(p, g, None if gc is None else c), p[:, 2] * p[:, 3], g[:, 2] * g[:, 3])
              for p, g, c in zip(px, gx, d['gc'])]
    want = matching.coco_results(matching.coco_evaluate_from_ious(
        tables, d['pl'], d['ps'], d['gl'], gc, ga))
    assert sorted(got) == sorted(want) and len(got) == 25    # eval_instseg_coco's key set
    assert np.array_equal(got['coco_eval']['precision'], want['coco_eval']['precision'])
    assert np.array_equal(got['coco_eval']['recall'], want['coco_eval']['recall'])
    same({k: v for k, v in got.items() if k != 'coco_eval'},
         {k: v for k, v in want.items() if k != 'coco_eval'})
    assert 0 < got['map/iou=0.50:0.95/area=all/maxDets=100'] < 1


# ----------------------------------------------------------------------------------- evaluators
def _small_model(dev, n_fg=80):
    torch.manual_seed(0)
    model = cmr.models.MaskRCNNResNet(50, n_fg_class=n_fg, min_size=160, max_size=240,
                                      anchor_scales=(2, 4, 8, 16, 32), roi_size=14,
                                      proposal_creator_params=dict(min_size=0, n_test_pre_nms=300,
                                                                   n_test_post_nms=50)).to(dev)
    with torch.no_grad():
        model.extractor.bn1.W.fill_(1. / 64.)
        model.head.cls_loc_score.W[4 * (n_fg + 1):5 * (n_fg + 1)] *= 300.
    model.eval()
    return model


def _synthetic(rng, n, with_crowd):
    """Examples whose ``bbox`` is the mask's tight box, as the datasets give it."""
    out = []
    for i in range(n):
        H, W = [(100, 140), (120, 90), (96, 128)][i % 3]
        img = rng.randint(0, 256, (3, H, W)).astype(np.uint8)
        G = rng.randint(1, 5)
        mask = np.zeros((G, H, W), np.int32)
        bbox = np.zeros((G, 4), np.float32)
        for g in range(G):
            y0, x0 = rng.randint(0, H - 20), rng.randint(0, W - 20)
            y1, x1 = min(H, y0 + rng.randint(8, 60)), min(W, x0 + rng.randint(8, 60))
            mask[g, y0:y1, x0:x1] = 1
            bbox[g] = [y0, x0, y1, x1]
        ex = (img, bbox, rng.randint(0, 80, G).astype(np.int32), mask)
        if with_crowd:
            ex += ((rng.uniform(size=G) < 0.3).astype(np.int32), mask.sum((1, 2)).astype(np.float32))
        out.append(ex)
    return out


@pytest.fixture(scope='module')
def model(dev):
    return _small_model(dev)


def _evaluator(kind, batches, model, iou_types=None, **kw):
    if iou_types is not None:
        kw['iou_types'] = iou_types
    if kind == 'voc':
        return cmr.extensions.InstanceSegmentationVOCEvaluator(
            batches, model, use_07_metric=True, label_names=NAMES, **kw)
    return cmr.extensions.InstanceSegmentationCOCOEvaluator(batches, model, label_names=NAMES, **kw)


@pytest.fixture(scope='module', params=['voc', 'coco'])
def runs(request, dev, model):
    """One default, one ('segm', 'bbox') and one ('bbox',) evaluation of the same batches, and
    ``predict``'s boxes for them."""
    kind = request.param
    data = _synthetic(np.random.RandomState(11), 5, with_crowd=kind == 'coco')
    batches = [data[0:2], data[2:4], data[4:5]]
    out = dict(kind=kind, data=data, batches=batches)
    out['default'] = _evaluator(kind, batches, model).evaluate()
    ev = _evaluator(kind, batches, model, ('segm', 'bbox'))
    out['records'] = ev.collect()
    out['both'] = ev.evaluate_collected(out['records'])
    out['bbox'] = _evaluator(kind, batches, model, ('bbox',)).evaluate()
    boxes, labels, scores = [], [], []
    for b in batches:                      # same batch composition (padding) as the evaluator
        bb, _, l, s = model.predict([ex[0] for ex in b])
        boxes += bb
        labels += l
        scores += s
    out['predict'] = (boxes, labels, scores)
    return out


def test_segm_keys_are_the_default_evaluators(runs):
    segm = {k: v for k, v in runs['both'].items() if '/bbox/' not in k}
    same(segm, runs['default'])
    assert not any('bbox' in k for k in runs['default'])
    assert set(runs['records'].tables) == {'segm', 'bbox'}
    assert len(runs['records'].tables['bbox']) == len(runs['data'])


def test_bbox_keys_equal_eval_detection_on_predict(runs):
    boxes, labels, scores = runs['predict']
    data = runs['data']
    assert sum(len(l) for l in labels) > 0
    gb, gl = [ex[1] for ex in data], [ex[2] for ex in data]
    if runs['kind'] == 'voc':
        r = cmr.utils.eval_detection_voc(boxes, labels, scores, gb, gl, use_07_metric=True)
        exp = {'map': r['map']}
        exp.update({'ap/c%d' % l: (r['ap'][l] if l < len(r['ap']) else np.nan) for l in range(80)})
    else:
        r = cmr.utils.eval_detection_coco(boxes, labels, scores, gb, gl,
                                          [ex[5] for ex in data], [ex[4] for ex in data])
        cats = r['coco_eval']['params']['catIds']
        exp = {'map': r['map/iou=0.50:0.95/area=all/maxDets=100'],
               'map@0.5': r['map/iou=0.50/area=all/maxDets=100'],
               'map@0.75': r['map/iou=0.75/area=all/maxDets=100']}
        per = r['ap/iou=0.50:0.95/area=all/maxDets=100']
        exp.update({'ap/c%d' % l: (per[cats.index(l)] if l in cats else np.nan) for l in range(80)})
    got = {k: v for k, v in runs['both'].items() if '/bbox/' in k}
    same(got, {'validation/main/bbox/' + k: v for k, v in exp.items()})


def test_bbox_alone_reports_the_same_bbox_keys(runs):
    same(runs['bbox'], {k: v for k, v in runs['both'].items() if '/bbox/' in k})


def test_two_shards_merged_equal_the_single_run_at_batch_size_one(runs, model):
    kind, data = runs['kind'], runs['data']
    types = ('segm', 'bbox')
    single = _evaluator(kind, [[ex] for ex in data], model, types).evaluate()
    shards = [_evaluator(kind, [[ex] for ex in part], model, types).collect()
              for part in (data[:3], data[3:])]
    merged = EvalRecords.merge(shards)
    assert set(merged.tables) == {'segm', 'bbox'}
    same(_evaluator(kind, None, model, types).evaluate_collected(merged), single)
    assert any('/bbox/' in k for k in single)


# -------------------------------------------------------------------------------- results files
def test_results_files_score_the_evaluators_bbox_keys(dev, tmp_path):
    from test_gpu_coco_results import write_coco
    root = str(tmp_path)
    write_coco(root)
    data = cmr.datasets.COCOInstanceSegmentationDataset(
        'minival', root_dir=root, use_crowd=True, return_crowd=True, return_area=True)
    names = list(data.class_names)
    model = _small_model(dev, len(names))
    transform = cmr.datasets.MaskRCNNTransform(model, train=False)
    batches = [[transform(data[j])] for j in range(len(data))]
    full, bare = str(tmp_path / 'res.json'), str(tmp_path / 'det.json')
    with CR.ResultsWriter(full, data.img_ids, data.class_id_to_cat_id) as w:
        mem = cmr.extensions.InstanceSegmentationCOCOEvaluator(
            batches, model, label_names=names, results_sink=w, iou_types=('segm', 'bbox')).evaluate()
    assert w.n_entries > 0
    mem_bbox = {k: v for k, v in mem.items() if '/bbox/' in k}
    mem_segm = {k: v for k, v in mem.items() if '/bbox/' not in k}
    assert len(mem_bbox) == 3 + len(names)
    # the sink's file: its bbox fields score the evaluator's bbox keys, its masks the segm keys
    same(CR.eval_coco_results(full, data, label_names=names, iou_type='bbox'), mem_bbox)
    same(CR.eval_coco_results(full, data, label_names=names), mem_segm)
    # a bbox-only file, written by the same sink from a bbox-only evaluation
    with CR.ResultsWriter(bare, data.img_ids, data.class_id_to_cat_id) as w:
        only = cmr.extensions.InstanceSegmentationCOCOEvaluator(
            batches, model, label_names=names, results_sink=w, iou_types=('bbox',)).evaluate()
    same(only, mem_bbox)
    entries = json.load(open(bare))
    assert entries and all(sorted(e) == ['bbox', 'category_id', 'image_id', 'score']
                           for e in entries)
    assert [e['bbox'] for e in entries] == [e['bbox'] for e in json.load(open(full))]
    same(CR.eval_coco_results(bare, data, label_names=names, iou_type='bbox'), mem_bbox)
    assert sum(len(v) for v in CR.load_results(bare, data, iou_type='bbox').values()) == len(entries)
    with pytest.raises(ValueError, match="results entry 0 has no 'segmentation'"):
        CR.eval_coco_results(bare, data, label_names=names)
    broken = [dict(entries[0]), {k: v for k, v in entries[0].items() if k != 'bbox'}]
    with pytest.raises(ValueError, match="results entry 1 has no 'bbox'"):
        CR.eval_coco_results(broken, data, iou_type='bbox')
