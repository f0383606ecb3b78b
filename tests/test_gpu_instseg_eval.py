"""Packed-mask kernels and the device path of the instance-segmentation evaluations on the GPU:
pack / packed paste bit-exact against np.packbits, intersections exact against NumPy, IoU and
both evaluations equal to the reference fixture and the NumPy restatement, the evaluators equal
to the eval functions fed predict's host masks."""
import os

import numpy as np
import pytest
import torch

import instseg_eval_ref as R
import chainer_mask_rcnn_amd as cmr
from chainer_mask_rcnn_amd import _lib
from chainer_mask_rcnn_amd.utils.evaluations import masks as M

pytestmark = pytest.mark.gpu


def np_pack(m):
    """Host reference of the packed format."""
    m = np.asarray(m) != 0
    N, H, W = m.shape
    Wq = (W + 63) // 64
    pad = np.zeros((N, H, Wq * 64), bool)
    pad[:, :, :W] = m
    return np.packbits(pad, axis=-1, bitorder='little').view('<u8').reshape(N, H, Wq)


def _check_extent(m, area, extent, tight=True):
    """Exact areas; extents containing every set bit (and empty for an empty mask when
    ``tight``: the packed paste's extent is the clipped box, whatever the mask holds)."""
    m = np.asarray(m) != 0
    Wq = (m.shape[2] + 63) // 64
    for n in range(len(m)):
        assert area[n] == m[n].sum()
        y_lo, y_hi, w_lo, w_hi = extent[n]
        ys, xs = np.nonzero(m[n])
        if len(ys) == 0:
            assert not tight or y_lo >= y_hi or w_lo >= w_hi
            continue
        assert 0 <= y_lo <= ys.min() and ys.max() < y_hi <= m.shape[1]
        assert 0 <= w_lo <= xs.min() // 64 and xs.max() // 64 < w_hi <= Wq


@pytest.mark.parametrize('W', [1, 63, 64, 65, 640, 1333])
@pytest.mark.parametrize('dtype', [np.uint8, np.bool_, np.int32])
def test_pack_bit_exact(dev, W, dtype):
    rng = np.random.RandomState(W)
    H = 37
    m = rng.uniform(size=(5, H, W)) < 0.3
    m[1] = False                                      # empty
    m[2] = True                                       # full
    m[3] = False
    m[3, 5:9, W // 2:] = True                         # a block
    a = m.astype(dtype)
    if dtype == np.int32:
        a = a * rng.randint(1, 7, a.shape).astype(np.int32)   # any nonzero value is foreground
    packed, area, extent = M.pack_masks(a)
    torch.cuda.synchronize()
    got = packed.cpu().numpy().view(np.uint64)
    assert np.array_equal(got, np_pack(m))
    _check_extent(m, area.cpu().numpy(), extent.cpu().numpy())
    # device input, same result
    p2, a2, e2 = M.pack_masks(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
    assert np.array_equal(p2.cpu().numpy(), packed.cpu().numpy())
    assert np.array_equal(a2.cpu().numpy(), area.cpu().numpy())
    assert np.array_equal(e2.cpu().numpy(), extent.cpu().numpy())


def _detections(rng, D, H, W, Kc=81, Msz=14):
    y0 = rng.uniform(-40, H, D)
    x0 = rng.uniform(-40, W, D)
    bbox = np.stack([y0, x0, y0 + rng.uniform(0, 200, D), x0 + rng.uniform(0, 200, D)],
                    1).astype(np.float32)
    bbox[0] = [10, 10, 10, 10]                        # degenerate
    bbox[1] = [H - 2, W - 3, H + 50, W + 60]          # mostly outside
    bbox[2] = [-30, -30, 5, 5]                        # partly outside, top-left
    bbox[3] = [H + 5, W + 5, H + 20, W + 30]          # entirely outside
    label = rng.randint(0, Kc, D).astype(np.int32)
    logits = (rng.standard_normal((D, Kc, Msz, Msz)) * 3).astype(np.float32)
    return bbox, label, logits


@pytest.mark.parametrize('H,W', [(100, 140), (480, 640), (77, 65)])
def test_packed_paste_equals_pack_of_paste(dev, H, W):
    rng = np.random.RandomState(H + W)
    D = 40
    bbox, label, logits = _detections(rng, D, H, W)
    roi = torch.tensor(logits, device=dev)
    from chainer_mask_rcnn_amd.functions._layout import nhwc
    lg = nhwc(roi)
    out = torch.empty((D, H, W), dtype=torch.uint8, device=dev)
    label_d, bbox_d = torch.tensor(label, device=dev), torch.tensor(bbox, device=dev)
    _lib.call('mrcnn_paste_masks', _lib.ptr(lg), _lib.ptr(label_d), _lib.ptr(bbox_d), D,
              lg.shape[2], lg.shape[1], H, W, _lib.ptr(out), _lib.stream_ptr())
    packed, area, extent = M.paste_packed(roi, label, bbox, (H, W))
    torch.cuda.synchronize()
    ref = out.cpu().numpy()
    assert ref.any()
    assert np.array_equal(packed.cpu().numpy().view(np.uint64), np_pack(ref))
    _check_extent(ref, area.cpu().numpy(), extent.cpu().numpy(), tight=False)


def _intersect_np(a, b):
    # float32 BLAS: every partial sum is an integer below 2^24, so the counts are exact
    a = (a.reshape(len(a), -1) != 0).astype(np.float32)
    b = (b.reshape(len(b), -1) != 0).astype(np.float32)
    return (a @ b.T).astype(np.int64)


def test_intersections_small_cases(dev):
    H, W = 50, 130
    a = np.zeros((4, H, W), bool)
    a[0, :10, :10] = True
    a[1, 20:30, 100:] = True
    a[2] = a[0]                                       # identical to a[0]
    # a[3] empty
    b = np.zeros((3, H, W), bool)
    b[0, :10, :10] = True
    b[1, 40:, :] = True                               # disjoint from every a
    pa, pb = M.pack_masks(a), M.pack_masks(b)
    inter = M.queue_intersections(pa, pb, W).cpu().numpy()
    assert np.array_equal(inter, _intersect_np(a, b))
    assert inter[0, 0] == 100 and inter[2, 0] == 100 and inter[:, 1].sum() == 0 and inter[3].sum() == 0


def test_intersections_large_with_tight_and_full_extents(dev):
    rng = np.random.RandomState(0)
    H, W, P, G = 800, 1333, 100, 50
    a = np.zeros((P, H, W), np.uint8)
    b = np.zeros((G, H, W), np.uint8)
    for arr in (a, b):
        for n in range(len(arr)):
            y0, x0 = rng.randint(0, H - 1), rng.randint(0, W - 1)
            h, w = rng.randint(1, 400), rng.randint(1, 700)
            arr[n, y0:y0 + h, x0:x0 + w] = rng.uniform(size=(min(h, H - y0), min(w, W - x0))) < 0.7
    b[3] = a[7]
    exp = _intersect_np(a, b)
    pa, pb = M.pack_masks(a), M.pack_masks(b)
    got = M.queue_intersections(pa, pb, W).cpu().numpy()
    assert np.array_equal(got, exp)
    Wq = (W + 63) // 64
    full = lambda n: torch.tensor([[0, H, 0, Wq]] * n, dtype=torch.int32, device=dev)
    got_full = M.queue_intersections((pa[0], pa[1], full(P)), (pb[0], pb[1], full(G)), W)
    assert np.array_equal(got_full.cpu().numpy(), exp)


def test_mask_iou_bit_identical_to_reference(dev, golden_dir):
    d = np.load(os.path.join(golden_dir, 'instseg_voc.npz'))
    n = 0
    for c in range(int(d['n_case'])):
        for i in range(int(d['c%d/n_img' % c])):
            pm, gm = d['c%d/i%d/pm' % (c, i)], d['c%d/i%d/gm' % (c, i)]
            iou = cmr.utils.mask_iou(pm, gm)
            assert iou.dtype == np.float64
            assert np.array_equal(iou, d['c%d/i%d/iou' % (c, i)])
            n += iou.size
    assert n > 0


def test_eval_instseg_voc_on_device_equals_fixture(dev, golden_dir):
    from test_instseg_eval_cpu import load_voc_cases, _same_list
    for imgs, exp, _ in load_voc_cases(golden_dir):
        pm, pl, ps, gm, gl, gd = zip(*imgs)
        for dif in (0, 1):
            prec, rec = cmr.utils.calc_instseg_voc_prec_rec(pm, pl, ps, gm, gl, gd if dif else None)
            _same_list(prec, exp[dif][0])
            _same_list(rec, exp[dif][1])
            for m07, e_ap in ((False, exp[dif][2]), (True, exp[dif][3])):
                r = cmr.utils.eval_instseg_voc(pm, pl, ps, gm, gl, gd if dif else None,
                                               use_07_metric=m07)
                assert np.array_equal(r['ap'], e_ap, equal_nan=True)
                assert np.array_equal(r['map'], np.nanmean(e_ap), equal_nan=True)


@pytest.mark.parametrize('seed', [0, 3])
def test_eval_instseg_coco_on_device_equals_restatement(dev, seed):
    from test_instseg_eval_cpu import _coco_case
    pms, pls, pss, gms, gls, gcs, gas = _coco_case(seed)
    got = cmr.utils.eval_instseg_coco(pms, pls, pss, gms, gls, gcs, gas)
    precision, recall, _ = R.coco_eval(pms, pls, pss, gms, gls, gcs, gas)
    assert np.array_equal(got['coco_eval']['precision'], precision)
    assert np.array_equal(got['coco_eval']['recall'], recall)
    for k, v in R.coco_summary(precision, recall).items():
        assert np.array_equal(np.asarray(got[k]), np.asarray(v), equal_nan=True), k


def _small_model(dev):
    torch.manual_seed(0)
    model = cmr.models.MaskRCNNResNet(50, n_fg_class=80, min_size=160, max_size=240,
                                      anchor_scales=(2, 4, 8, 16, 32), roi_size=14,
                                      proposal_creator_params=dict(min_size=0, n_test_pre_nms=300,
                                                                   n_test_post_nms=50)).to(dev)
    with torch.no_grad():
        model.extractor.bn1.W.fill_(1. / 64.)
        model.head.cls_loc_score.W[4 * 81:5 * 81] *= 300.
    return model


def _synthetic(rng, n, with_crowd):
    out = []
    for i in range(n):
        H, W = [(100, 140), (120, 90), (96, 128)][i % 3]
        img = rng.randint(0, 256, (3, H, W)).astype(np.uint8)
        G = rng.randint(1, 5)
        mask = np.zeros((G, H, W), np.int32)
        for g in range(G):
            y0, x0 = rng.randint(0, H - 20), rng.randint(0, W - 20)
            mask[g, y0:y0 + rng.randint(8, 60), x0:x0 + rng.randint(8, 60)] = 1
        label = rng.randint(0, 80, G).astype(np.int32)
        bbox = np.zeros((G, 4), np.float32)
        ex = (img, bbox, label, mask)
        if with_crowd:
            ex += ((rng.uniform(size=G) < 0.3).astype(np.int32), mask.sum((1, 2)).astype(np.float32))
        out.append(ex)
    return out


@pytest.mark.parametrize('kind', ['voc', 'coco'])
def test_evaluator_equals_eval_functions_on_predict(dev, kind):
    rng = np.random.RandomState(11)
    model = _small_model(dev)
    data = _synthetic(rng, 5, with_crowd=kind == 'coco')
    batches = [data[0:2], data[2:4], data[4:5]]
    names = ['c%d' % l for l in range(80)]
    if kind == 'voc':
        ev = cmr.extensions.InstanceSegmentationVOCEvaluator(batches, model, use_07_metric=True,
                                                             label_names=names)
    else:
        ev = cmr.extensions.InstanceSegmentationCOCOEvaluator(batches, model, label_names=names)
    obs = ev.evaluate()
    masks, labels, scores = [], [], []
    for b in batches:                      # same batch composition (padding) as the evaluator
        _, m, l, s = model.predict([ex[0] for ex in b])
        masks += m
        labels += l
        scores += s
    assert sum(len(l) for l in labels) > 0
    gm = [ex[3] for ex in data]
    gl = [ex[2] for ex in data]
    if kind == 'voc':
        r = cmr.utils.eval_instseg_voc(masks, labels, scores, gm, gl, use_07_metric=True)
        exp = {'map': r['map']}
        exp.update({'ap/c%d' % l: (r['ap'][l] if l < len(r['ap']) else np.nan) for l in range(80)})
    else:
        r = cmr.utils.eval_instseg_coco(masks, labels, scores, gm, gl, [ex[4] for ex in data],
                                        [ex[5] for ex in data])
        cats = r['coco_eval']['params']['catIds']
        exp = {'map': r['map/iou=0.50:0.95/area=all/maxDets=100'],
               'map@0.5': r['map/iou=0.50/area=all/maxDets=100'],
               'map@0.75': r['map/iou=0.75/area=all/maxDets=100']}
        per = r['ap/iou=0.50:0.95/area=all/maxDets=100']
        exp.update({'ap/c%d' % l: (per[cats.index(l)] if l in cats else np.nan) for l in range(80)})
    assert set(obs) == {'validation/main/' + k for k in exp}
    for k, v in exp.items():
        assert np.array_equal(np.asarray(obs['validation/main/' + k]), np.asarray(v),
                              equal_nan=True), k


def test_ground_truth_as_prediction_gives_map_one(dev):
    rng = np.random.RandomState(5)
    data = _synthetic(rng, 4, with_crowd=False)
    gm = [ex[3] for ex in data]
    gl = [ex[2] for ex in data]
    ones = [np.ones(len(l), np.float32) for l in gl]
    assert cmr.utils.eval_instseg_voc(gm, gl, ones, gm, gl)['map'] == 1.
    r = cmr.utils.eval_instseg_coco(gm, gl, ones, gm, gl)
    assert r['map/iou=0.50:0.95/area=all/maxDets=100'] == 1.
    assert r['map/iou=0.75/area=all/maxDets=100'] == 1.


# ----------------------------------------------------------------- the records and the read-back
def test_readback_of_device_tensors_equals_each_tensors_own_copy(dev):
    from records_util import check_readback, readback_parts
    from chainer_mask_rcnn_amd.utils.evaluations.records import Readback
    on_device = [t.to(dev) for t in readback_parts()]
    readback = Readback()
    for t in on_device:
        readback.add(t)
    check_readback([t.cpu() for t in on_device], readback.fetch())


def test_one_readback_per_batch_and_results_files_score_the_observation(dev, tmp_path,
                                                                        monkeypatch):
    """Two batches of two images, all three IoU types: ``collect()`` reads back once per batch
    (once more per batch for the sink's strings), ``eval_coco_results`` once per image, and the
    file the sink wrote scores the evaluator's observation for every IoU type."""
    from test_gpu_coco_results import same
    from test_gpu_detection_eval import _small_model as small_model, _synthetic as synthetic
    from chainer_mask_rcnn_amd.utils.evaluations import coco_results as CR
    from chainer_mask_rcnn_amd.utils.evaluations import records, rle
    calls = {'fetch': 0, 'fetch_encoded': 0}

    def counting(name, fn):
        def wrapper(*args, **kwargs):
            calls[name] += 1
            return fn(*args, **kwargs)
        return wrapper
    monkeypatch.setattr(records.Readback, 'fetch', counting('fetch', records.Readback.fetch))
    monkeypatch.setattr(rle, 'fetch_encoded', counting('fetch_encoded', rle.fetch_encoded))

    class Annotations(object):
        """What eval_coco_results reads of a COCOInstanceSegmentationDataset."""
        def __init__(self, examples):
            self.examples = examples
            self.img_ids = [100 + i for i in range(len(examples))]
            self.img_sizes = {i: tuple(ex[0].shape[1:]) for i, ex in zip(self.img_ids, examples)}
            self.class_id_to_cat_id = {l: 2 * l + 1 for l in range(80)}
            self.cat_id_to_class_id = {c: l for l, c in self.class_id_to_cat_id.items()}

        def __len__(self):
            return len(self.examples)

        def get_annotations(self, i):
            return self.examples[i][1:]

    examples = synthetic(np.random.RandomState(11), 4, with_crowd=True)
    data = Annotations(examples)
    names = ['c%d' % l for l in range(80)]
    model = small_model(dev)
    batches = [examples[0:2], examples[2:4]]
    types = ('segm', 'bbox', 'boundary')
    path = str(tmp_path / 'res.json')
    with CR.ResultsWriter(path, data.img_ids, data.class_id_to_cat_id) as w:
        ev = cmr.extensions.InstanceSegmentationCOCOEvaluator(
            batches, model, label_names=names, results_sink=w, iou_types=types)
        rec = ev.collect()
    assert calls == {'fetch': 2, 'fetch_encoded': 2} and w.n_entries > 0
    assert set(rec.tables) == set(types) and len(rec) == 4
    plain = cmr.extensions.InstanceSegmentationCOCOEvaluator(
        batches, model, label_names=names, iou_types=types).collect()
    assert calls == {'fetch': 4, 'fetch_encoded': 2}
    for k in types:
        for a, b in zip(rec.tables[k], plain.tables[k]):
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), k
    mem = ev.evaluate_collected(rec)
    assert len(mem) == 3 * (3 + len(names)) and calls['fetch'] == 4
    # once per image; the box tables of all images are one launch and one read-back
    for iou_type, prefix, per_call in (('segm', '', 4), ('boundary', 'boundary/', 4),
                                       ('bbox', 'bbox/', 1)):
        before = calls['fetch']
        got = CR.eval_coco_results(path, data, limit=4, label_names=names, iou_type=iou_type)
        assert calls['fetch'] - before == per_call, iou_type
        keys = ['validation/main/' + prefix + k
                for k in ['map', 'map@0.5', 'map@0.75'] + ['ap/' + n for n in names]]
        same(got, {k: mem[k] for k in keys})
    assert calls['fetch_encoded'] == 2
