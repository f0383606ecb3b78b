"""VOC2012 / SBD datasets on the MI355X: synthetic trees (palette PNGs with 255 borders, .mat
label files, JPEGs, split lists) under tmp_path; every example equals the reference's
get_example restated on the host, the VOC evaluator over the decoded dataset equals
eval_instseg_voc, tools/evaluate.py runs on the tree, and two VOC-settings train steps are
finite and reproducible."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import label_instances_ref as R
import chainer_mask_rcnn_amd as cmr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
pytestmark = pytest.mark.gpu

SIZES = [(120, 160), (97, 131), (150, 112), (128, 128)]


def _label_pair(rng, H, W):
    ins = np.zeros((H, W), np.uint8)
    cls = np.zeros((H, W), np.uint8)
    for k in range(1, rng.randint(2, 5)):
        c = rng.randint(1, 21)
        y0, x0 = rng.randint(2, H - 30), rng.randint(2, W - 30)
        y1, x1 = y0 + rng.randint(10, 28), x0 + rng.randint(10, 28)
        ins[y0 - 2:y1 + 2, x0 - 2:x1 + 2] = 255
        cls[y0 - 2:y1 + 2, x0 - 2:x1 + 2] = 255
        ins[y0:y1, x0:x1] = k
        cls[y0:y1, x0:x1] = c
    cls[(ins > 0) & (ins < 255) & (rng.uniform(size=(H, W)) < 0.05)] = 255
    return ins, cls


def _palette_png(path, a):
    import PIL.Image
    im = PIL.Image.fromarray(a).convert('P')       # palette indices = the label values
    im.putpalette(list(np.random.RandomState(0).randint(0, 256, 768)))
    im.save(path)


def _jpeg(path, rng, H, W, gray=False):
    import PIL.Image
    a = rng.randint(0, 256, (H, W) if gray else (H, W, 3)).astype(np.uint8)
    PIL.Image.fromarray(a).save(path, quality=95)


@pytest.fixture(scope='module')
def trees(tmp_path_factory):
    import scipy.io
    rng = np.random.RandomState(7)
    base = tmp_path_factory.mktemp('voc')
    voc = base / 'VOC2012'
    sbd = base / 'dataset'
    for d in ('ImageSets/Segmentation', 'JPEGImages', 'SegmentationClass', 'SegmentationObject'):
        (voc / d).mkdir(parents=True)
    for d in ('img', 'cls', 'inst'):
        (sbd / d).mkdir(parents=True)
    ids = ['2008_%06d' % i for i in range(len(SIZES))]
    raw = {}
    for i, (did, (H, W)) in enumerate(zip(ids, SIZES)):
        ins, cls = _label_pair(rng, H, W)
        raw[did] = (ins, cls)
        _jpeg(str(voc / 'JPEGImages' / (did + '.jpg')), rng, H, W, gray=i == 1)
        _palette_png(str(voc / 'SegmentationClass' / (did + '.png')), cls)
        _palette_png(str(voc / 'SegmentationObject' / (did + '.png')), ins)
        _jpeg(str(sbd / 'img' / (did + '.jpg')), rng, H, W)
        scipy.io.savemat(str(sbd / 'cls' / (did + '.mat')),
                         {'GTcls': {'Segmentation': cls, 'Boundaries': np.zeros((1, 1))}})
        scipy.io.savemat(str(sbd / 'inst' / (did + '.mat')),
                         {'GTinst': {'Segmentation': ins, 'Categories': np.zeros((1, 1))}})
    for root, lst in ((voc / 'ImageSets/Segmentation', ids), (sbd, ids)):
        (root / 'train.txt').write_text(''.join(d + '\n' for d in lst[:3]))
        (root / 'val.txt').write_text(''.join(d + '\n' for d in lst))
    return str(voc), str(sbd), raw


def _reference_example(img_path, ins_u8, cls_u8):
    """The reference's get_example (datasets/voc/voc.py, sbd.py) on the host."""
    ins, cls = R.voc_preprocess(ins_u8, cls_u8)
    labels, bboxes, masks = R.label2instance_boxes(ins, cls, return_masks=True)
    from chainer_mask_rcnn_amd.datasets.voc import read_rgb
    return (read_rgb(img_path), bboxes.astype(np.float32), labels.astype(np.int32) - 1,
            masks.astype(np.int32))


@pytest.mark.parametrize('kind', ['voc', 'sbd'])
def test_examples_equal_restated_reference(dev, trees, kind):
    voc, sbd, raw = trees
    ds = (cmr.datasets.VOC2012InstanceSegmentationDataset('val', root_dir=voc) if kind == 'voc'
          else cmr.datasets.SBDInstanceSegmentationDataset('val', root_dir=sbd))
    assert len(ds) == len(SIZES)
    for i, ex in enumerate(ds[0:len(ds)]):
        did = os.path.basename(ds.files[i]['img'])[:-4]
        exp = _reference_example(ds.files[i]['img'], *raw[did])
        img, bboxes, labels, masks = ex
        assert img.dtype == np.uint8 and img.shape == SIZES[i] + (3,)
        assert bboxes.dtype == np.float32 and labels.dtype == np.int32 and masks.dtype == np.int32
        for g, e in zip(ex, exp):
            assert g.shape == e.shape and np.array_equal(g, e), (kind, i)
        assert len(labels) > 0 and labels.min() >= 0 and labels.max() < 20


def test_voc_evaluator_over_decoded_dataset(dev, trees):
    voc, _, raw = trees
    ds = cmr.datasets.VOC2012InstanceSegmentationDataset('val', root_dir=voc)
    data = [ds[i] for i in range(len(ds))]
    torch.manual_seed(0)
    model = cmr.models.MaskRCNNResNet(50, n_fg_class=20, min_size=160, max_size=240,
                                      anchor_scales=(4, 8, 16, 32), roi_size=14,
                                      proposal_creator_params=dict(min_size=0, n_test_pre_nms=300,
                                                                   n_test_post_nms=50)).to(dev)
    with torch.no_grad():
        model.extractor.bn1.W.fill_(1. / 64.)
        model.head.cls_loc_score.W[4 * 21:5 * 21] *= 300.
    chw = [(np.ascontiguousarray(ex[0].transpose(2, 0, 1)),) + ex[1:] for ex in data]
    batches = [chw[0:2], chw[2:4]]
    names = [str(n) for n in ds.class_names]
    ev = cmr.extensions.InstanceSegmentationVOCEvaluator(batches, model, use_07_metric=True,
                                                         label_names=names)
    obs = ev.evaluate()
    masks, labels, scores = [], [], []
    for b in batches:
        _, m, l, s = model.predict([ex[0] for ex in b])
        masks += m
        labels += l
        scores += s
    gm, gl = [], []
    for i in range(len(ds)):                # ground truth decoded on the host
        did = os.path.basename(ds.files[i]['img'])[:-4]
        _, _, l, m = _reference_example(ds.files[i]['img'], *raw[did])
        gm.append(m)
        gl.append(l)
    r = cmr.utils.eval_instseg_voc(masks, labels, scores, gm, gl, use_07_metric=True)
    assert np.array_equal(np.asarray(obs['validation/main/map']), np.asarray(r['map']),
                          equal_nan=True)


def test_evaluate_tool_on_voc_tree(dev, trees, tmp_path):
    voc, _, _ = trees
    out = str(tmp_path / 'voc_eval.json')
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'evaluate.py'), '--dataset', 'voc',
           '--voc-root', voc, '--limit', '3', '--out', out]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    path = out if os.path.exists(out) else os.path.splitext(out)[0] + '.json'
    text = open(path).read()
    try:
        payload = json.loads(text)
    except ValueError:                      # YAML when PyYAML is installed
        import yaml
        payload = yaml.safe_load(text)
    assert payload['evaluator'] == 'voc' and payload['split'] == 'val'
    assert 'validation/main/map' in payload['result'] or 'map' in payload['result']


def test_two_voc_train_steps_finite_and_reproducible(dev, trees):
    import train_loop as TL
    _, sbd, _ = trees
    runs = []
    for _ in range(2):
        data = cmr.datasets.SBDInstanceSegmentationDataset('train', root_dir=sbd)
        loop, model, chain, opt = TL.build(data, 50, dev, batch_size=2, seed=3, prefetch=False,
                                           model_settings='voc')
        assert (model.min_size, model.max_size) == (600, 1000)
        losses = [float(l.detach()) for l in loop.run(2)]
        opt.flush()
        torch.cuda.synchronize()
        loop.close()
        runs.append(losses)
    assert all(np.isfinite(runs[0])) and len(runs[0]) == 2
    assert runs[0] == runs[1]
