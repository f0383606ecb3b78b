"""COCO results files end to end on a small COCO-layout directory with sparse category ids:
``tools/evaluate.py --save-results`` then ``--results`` (images deleted) reproduce the in-memory
evaluation exactly, ground truth written as results scores 1, the file's masks are ``predict``'s,
and a test-dev directory yields a file of its images."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import chainer_mask_rcnn_amd as cmr
from chainer_mask_rcnn_amd.datasets.coco import rle_decode
from chainer_mask_rcnn_amd.utils.evaluations import coco_results as CR
from chainer_mask_rcnn_amd.utils.evaluations import rle as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CATS = (1, 3, 18, 90)        # four classes: the mask head needs a multiple of 4


def write_coco(root, n_images=5, H=96, W=128, test_dev=False):
    import PIL.Image
    rng = np.random.RandomState(0)
    folder = 'test2015' if test_dev else 'val2014'
    os.makedirs(os.path.join(root, 'annotations'), exist_ok=True)
    os.makedirs(os.path.join(root, folder))
    images, anns = [], []
    for i in range(n_images):
        img_id = 11 + 3 * i
        h, w = H + 8 * (i % 2), W
        img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        PIL.Image.fromarray(img).save(
            os.path.join(root, folder, 'COCO_%s_%012d.jpg' % (folder, img_id)), quality=95)
        images.append(dict(id=img_id, height=h, width=w))
        for g in range(1 + i % 3):
            y0, x0 = int(rng.randint(4, h // 2)), int(rng.randint(4, w // 2))
            bh, bw = int(rng.randint(24, h // 2 - 4)), int(rng.randint(24, w // 2 - 4))
            poly = [x0, y0, x0 + bw, y0, x0 + bw, y0 + bh, x0 + bw // 2, y0 + bh + 3, x0, y0 + bh]
            anns.append(dict(id=len(anns) + 1, image_id=img_id, category_id=CATS[g],
                             segmentation=[[float(v) for v in poly]], iscrowd=0,
                             area=float(bh * bw), bbox=[x0, y0, bw, bh]))
    cats = [dict(id=c, name='cat%d' % c) for c in CATS]
    name = 'image_info_test-dev2015.json' if test_dev else 'instances_minival2014.json'
    with open(os.path.join(root, 'annotations', name), 'w') as f:
        json.dump(dict(images=images, categories=cats) if test_dev else
                  dict(images=images, annotations=anns, categories=cats), f)
    return [im['id'] for im in images]


def run_tool(*args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'evaluate.py')] + list(args),
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return p.stdout


def same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])), (k, a[k], b[k])


@pytest.mark.parametrize('limit', [0, 2])
def test_tool_save_then_score_equals_in_memory(dev, tmp_path, limit):
    root = str(tmp_path / 'coco')
    write_coco(root)
    res, mem, scored = (str(tmp_path / n) for n in ('res.json', 'mem.yaml', 'scored.yaml'))
    lim = ['--limit', str(limit)] if limit else []
    run_tool('--coco-root', root, '--save-results', res, '--out', mem, *lim)
    entries = json.load(open(res))
    assert entries and {e['category_id'] for e in entries} <= set(CATS)
    shutil.rmtree(os.path.join(root, 'val2014'))             # scoring needs no image
    run_tool('--coco-root', root, '--results', res, '--out', scored, *lim)
    a, b = yaml.safe_load(open(mem)), yaml.safe_load(open(scored))
    assert a['results_file'] == os.path.abspath(res)
    assert a['result'] and 'validation/main/map' in a['result']
    same(a['result'], b['result'])


def small_model(dev, n_fg):
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


def test_sink_file_is_predict_and_scores_as_in_memory(dev, tmp_path):
    root = str(tmp_path)
    write_coco(root)
    data = cmr.datasets.COCOInstanceSegmentationDataset(
        'minival', root_dir=root, use_crowd=True, return_crowd=True, return_area=True)
    model = small_model(dev, len(data.class_names))
    transform = cmr.datasets.MaskRCNNTransform(model, train=False)
    path = str(tmp_path / 'res.json')
    for batch in (2, 1):              # batch 1 last: its file is compared with predict below
        batches = [[transform(data[j]) for j in range(i, min(i + batch, len(data)))]
                   for i in range(0, len(data), batch)]
        with CR.ResultsWriter(path, data.img_ids, data.class_id_to_cat_id) as w:
            ev = cmr.extensions.InstanceSegmentationCOCOEvaluator(
                batches, model, label_names=list(data.class_names), results_sink=w)
            mem = ev.evaluate()
        assert w.image_ids == data.img_ids
        same(mem, CR.eval_coco_results(path, data, label_names=list(data.class_names)))
        off = cmr.extensions.InstanceSegmentationCOCOEvaluator(
            batches, model, label_names=list(data.class_names)).evaluate()
        same(mem, off)                                       # the sink changes no number
    grouped = CR.load_results(path, data)
    n_dets = 0
    for i, img_id in enumerate(data.img_ids):
        chw = data[i][0].transpose(2, 0, 1)
        bboxes, masks, labels, scores = model.predict([chw])
        ents = grouped.get(img_id, [])
        assert len(ents) == len(masks[0])
        n_dets += len(ents)
        H, W = data.img_sizes[img_id]
        for e, m, b, l, s in zip(ents, masks[0], bboxes[0], labels[0], scores[0]):
            assert np.array_equal(rle_decode(e['segmentation'], H, W), m.astype(np.uint8))
            assert e['category_id'] == data.class_id_to_cat_id[int(l)]
            assert np.float32(e['score']) == s
            assert e['bbox'] == [float(b[1]), float(b[0]), float(b[3]) - float(b[1]),
                                 float(b[2]) - float(b[0])]
    assert n_dets > 0


def test_ground_truth_as_results_scores_one(dev, tmp_path):
    root = str(tmp_path)
    write_coco(root)
    data = cmr.datasets.COCOInstanceSegmentationDataset(
        'minival', root_dir=root, use_crowd=True, return_crowd=True, return_area=True)
    results = []
    for i, img_id in enumerate(data.img_ids):
        bboxes, labels, masks, crowds, areas = data.get_annotations(i)
        keep = crowds == 0
        segs = R.encode_masks(masks[keep])
        results += CR.results_entries(img_id, bboxes[keep], labels[keep],
                                      np.ones(int(keep.sum()), np.float32), segs,
                                      data.class_id_to_cat_id)
    shutil.rmtree(os.path.join(root, 'val2014'))
    got = CR.eval_coco_results(results, data)
    assert got['validation/main/map'] == 1.0
    assert got['validation/main/map@0.5'] == 1.0
    # scored twice: the same numbers
    same(got, CR.eval_coco_results(results, data))
    # an entry that is not a valid RLE names itself
    bad = [dict(r) for r in results]
    bad[2] = dict(bad[2], segmentation=dict(bad[2]['segmentation'], counts='0'))
    with pytest.raises(ValueError, match='results entry 2 '):
        CR.eval_coco_results(bad, data)


def test_test_dev_writes_every_image(dev, tmp_path):
    root = str(tmp_path / 'coco')
    ids = write_coco(root, n_images=3, test_dev=True)
    res = str(tmp_path / 'test-dev.json')
    out = run_tool('--coco-root', root, '--split', 'test-dev', '--save-results', res,
                   '--out', str(tmp_path / 'r.yaml'))
    assert 'not scored' in out
    assert ' %d images)' % len(ids) in out
    entries = json.load(open(res))
    assert entries and {e['image_id'] for e in entries} <= set(ids)
    data = cmr.datasets.COCOInstanceSegmentationDataset('test-dev', root_dir=root)
    assert data.img_ids == ids
    assert len(CR.load_results(res, data)) == len({e['image_id'] for e in entries})
