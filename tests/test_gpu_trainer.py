"""tools/trainer.py + tools/train.py on the device: the loss-observation accumulator, training with
evaluation / visual report / snapshot / log between the steps against a run with none of them, the
log's means and lr, the best snapshot and tools/evaluate.py --log-dir, and the VOC-like dataset."""
import io
import json
import os
import random
import sys

import numpy as np
import pytest
import torch

import chainer_mask_rcnn_amd as cmr
from chainer_mask_rcnn_amd import optimizers, serializers
from chainer_mask_rcnn_amd.functions import loss as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import train_loop as TL  # noqa: E402
import trainer as T  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ['loss', 'rpn_loc_loss', 'rpn_cls_loss', 'roi_loc_loss', 'roi_cls_loss', 'roi_mask_loss']


def test_observe_accumulate_is_a_float32_sequential_sum(dev):
    rng = np.random.RandomState(0)
    n_iter, n = 300, 6
    vals = (rng.standard_normal((n_iter, n)) * np.array([1e3, 1., 1e-3, 7., 0.1, 3e2])).astype(np.float32)
    sums = torch.zeros(8, dtype=torch.float32, device=dev)
    dv = torch.tensor(vals, device=dev)
    for i in range(n_iter):
        L.observe_accumulate([dv[i, k] for k in range(n)], sums)
    ref = np.zeros(n, np.float32)
    for i in range(n_iter):
        ref = (ref + vals[i]).astype(np.float32)
    got = sums.cpu().numpy()
    assert np.array_equal(got[:n].view(np.uint32), ref.view(np.uint32))
    assert np.all(got[n:] == 0)
    with pytest.raises(ValueError):
        L.observe_accumulate([dv[0, 0]] * 9, sums)


def _write_voc_like(root, n=3, H=96, W=128):
    import PIL.Image
    rng = np.random.RandomState(3)
    for d in ('JPEGImages', 'SegmentationClass', 'SegmentationObject'):
        os.makedirs(os.path.join(root, d))
    for i in range(n):
        img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
        cls = np.zeros((H, W), np.int32)
        ins = np.zeros((H, W), np.int32)
        for g in range(1 + i % 3):
            y0, x0 = rng.randint(0, H // 2), rng.randint(0, W // 2)
            h, w = rng.randint(20, H // 2), rng.randint(20, W // 2)
            cls[y0:y0 + h, x0:x0 + w] = rng.randint(1, 21)
            ins[y0:y0 + h, x0:x0 + w] = g + 1
            img[y0:y0 + h, x0:x0 + w] //= 2
        PIL.Image.fromarray(img).save(os.path.join(root, 'JPEGImages', 'img%02d.jpg' % i), quality=95)
        np.save(os.path.join(root, 'SegmentationClass', 'img%02d.npy' % i), cls)
        np.save(os.path.join(root, 'SegmentationObject', 'img%02d.npy' % i), ins)


def test_voc_like_dataset_matches_label2instance_boxes(tmp_path, dev):
    root = str(tmp_path / 'custom')
    _write_voc_like(root)
    ds = T.VOCLikeDataset(root)
    assert len(ds) == 3 and ds._ids == ['img00', 'img01', 'img02']
    for i in range(3):
        img, bboxes, labels, masks = ds[i]
        cls = np.load(os.path.join(root, 'SegmentationClass', 'img%02d.npy' % i))
        ins = np.load(os.path.join(root, 'SegmentationObject', 'img%02d.npy' % i))
        ins[ins == 0] = -1
        l_ref, b_ref, m_ref = cmr.utils.label2instance_boxes(ins, cls, return_masks=True)
        assert img.shape == cls.shape + (3,) and img.dtype == np.uint8
        assert bboxes.dtype == np.float32 and labels.dtype == np.int32 and masks.dtype == np.int32
        assert np.array_equal(bboxes, b_ref.astype(np.float32))
        assert np.array_equal(labels, l_ref.astype(np.int32) - 1)
        assert np.array_equal(masks, m_ref.astype(np.int32))
    cat = T.ConcatenatedDataset(ds, ds)
    assert len(cat) == 6 and np.array_equal(cat[4][1], ds[1][1])


def _build(dev, data, seed=4):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    model = cmr.models.MaskRCNNResNet(
        50, n_fg_class=20, anchor_scales=(4, 8, 16, 32), roi_size=14, min_size=144, max_size=192,
        proposal_creator_params=dict(min_size=0, n_train_pre_nms=600, n_train_post_nms=100,
                                     n_test_pre_nms=6000, n_test_post_nms=1000))
    chain = cmr.models.MaskRCNNTrainChain(
        model, proposal_target_creator=cmr.models.utils.ProposalTargetCreator(n_sample=32)).to(dev)
    chain.train()
    opt = optimizers.MomentumSGD(lr=0.0025, momentum=0.9)
    opt.setup(chain)
    opt.add_hook(optimizers.WeightDecay(1e-4))
    for link in (model.extractor.conv1, model.extractor.bn1, model.extractor.res2):
        optimizers.disable_update(link)
    for m in chain.modules():
        if isinstance(m, cmr.links.AffineChannel2D):
            optimizers.disable_update(m)
    with torch.no_grad():
        model.extractor.bn1.W.fill_(1. / 64.)
        for m in model.modules():
            if isinstance(m, cmr.models.resnet_extractor.Bottleneck):
                m.bn3.W.fill_(0.25)
    opt.defer_weight_gradients([model.head.res5.a.conv2.W, model.head.res5.b1.conv2.W])
    train = TL.TransformDataset(data, cmr.datasets.MaskRCNNTransform(model))
    loop = TL.TrainLoop(TL.SerialIterator(train, 2), chain, opt, dev, prefetch=True)
    return loop, model, chain, opt


class _Recorder(object):
    """Per step: the chain's report (device copies) and the lr the step used."""
    priority = 1000

    def __init__(self):
        self.reports, self.lrs = [], []

    def __call__(self, trainer):
        self.reports.append({k: v.clone() for k, v in trainer.loop.chain.report.items()})
        self.lrs.append(trainer.loop.optimizer.lr)


class _WeightsAtEval(object):
    """After each evaluation (before the snapshot): the map and the weights."""
    priority = 200

    def __init__(self, model):
        self.model, self.maps, self.weights = model, [], []

    def __call__(self, trainer):
        self.maps.append(float(trainer.observation['validation/main/map']))
        self.weights.append(serializers.state_arrays(self.model))


STEP_POINTS = [1.5, 2.5]      # inside epochs 2 and 3 (3 iterations per epoch)


def _run(dev, root, out, full):
    data = T.ConcatenatedDataset(T.VOCLikeDataset(root), T.VOCLikeDataset(root))   # 6 examples
    loop, model, chain, opt = _build(dev, data)
    tr = T.Trainer(loop, (3, 'epoch'), out=out)
    rec = _Recorder()
    tr.extend(rec)
    extra = {}
    if full:
        test = TL.TransformDataset(T.VOCLikeDataset(root),
                                   cmr.datasets.MaskRCNNTransform(model, train=False))
        test_iter = TL.SerialIterator(test, 1, shuffle=False)
        evaluator = cmr.extensions.InstanceSegmentationVOCEvaluator(
            test_iter, model, use_07_metric=True, label_names=list(T.VOCLikeDataset(root).class_names))
        params = dict(model='resnet50', pooling_func='align', anchor_scales=[4, 8, 16, 32],
                      mean=[123.152, 115.903, 103.063], min_size=144, max_size=192, roi_size=14,
                      class_names=[str(c) for c in T.VOCLikeDataset(root).class_names],
                      dataset='custom', custom_root=root, synthetic=0)
        extra['print'] = io.StringIO()
        T.extend_reference_set(tr, model, evaluator=evaluator, vis_iterator=test_iter,
                               class_names=params['class_names'], step_size=STEP_POINTS,
                               params=params, eval_interval=(1, 'epoch'),
                               log_interval=(2, 'iteration'), plot_interval=(0.5, 'epoch'),
                               print_interval=(2, 'iteration'), print_out=extra['print'])
        extra['at_eval'] = _WeightsAtEval(model)
        tr.extend(extra['at_eval'], trigger=(1, 'epoch'))
    else:
        tr.extend(T.ExponentialShift('lr', 0.1), trigger=T.ManualScheduleTrigger(STEP_POINTS, 'epoch'))
    tr.run()
    opt.flush()
    torch.cuda.synchronize()
    loop.close()
    states = (random.getstate(), np.random.get_state())
    return tr, rec, states, extra, model


def test_trainer_with_evaluation_matches_plain_training(tmp_path, dev):
    root = str(tmp_path / 'custom')
    _write_voc_like(root)
    out_a, out_b = str(tmp_path / 'a'), str(tmp_path / 'b')
    tr_a, rec_a, st_a, extra, model = _run(dev, root, out_a, full=True)
    tr_b, rec_b, st_b, _, _ = _run(dev, root, out_b, full=False)

    # (1) same training: losses bit-identical, random streams at the same place
    assert tr_a.iteration == tr_b.iteration == 9
    for ra, rb in zip(rec_a.reports, rec_b.reports):
        for k in KEYS:
            assert torch.equal(ra[k], rb[k]), k
    assert st_a[0] == st_b[0]
    assert all(np.array_equal(x, y) for x, y in zip(st_a[1], st_b[1]))
    # lr of the step: 0.1 shifts after the points 1.5 (iteration 5) and 2.5 (iteration 8)
    assert rec_a.lrs == rec_b.lrs == [0.0025] * 5 + [0.0025 * 0.1] * 3 + [0.0025 * 0.1 ** 2]

    # (2) the log: float32 means of the steps' reports, lr, validation keys only with an eval
    with open(os.path.join(out_a, 'log')) as f:
        log = json.load(f)
    assert [e['iteration'] for e in log] == [2, 4, 6, 8]
    host = [{k: np.float32(v.item()) for k, v in r.items()} for r in rec_a.reports]
    for e in log:
        window = host[e['iteration'] - 2:e['iteration']]
        for k in KEYS:
            s = np.float32(0)
            for h in window:
                s = np.float32(s + h[k])
            assert e['main/' + k] == float(s / np.float32(len(window))), (e['iteration'], k)
        assert e['lr'] == rec_a.lrs[e['iteration'] - 1]
        has_eval = e['iteration'] in (4, 6)             # evaluations at iterations 3, 6, 9
        assert ('validation/main/map' in e) == has_eval
        assert e['epoch'] == e['iteration'] * 2 // 6
    assert 'main/loss' in extra['print'].getvalue()
    for f in ('params.yaml', 'loss.png', 'accuracy.png', 'snapshot_model.npz',
              os.path.join('visualizations', 'iteration=00000003.jpg')):
        assert os.path.exists(os.path.join(out_a, f)), f

    # (3) the snapshot holds the weights of the evaluation with the highest map (first of equals)
    maps = extra['at_eval'].maps
    assert len(maps) == 3
    best, best_i = None, None
    for i, m in enumerate(maps):
        if best is None or m > best:
            best, best_i = m, i
    snap = np.load(os.path.join(out_a, 'snapshot_model.npz'))
    want = extra['at_eval'].weights[best_i]
    assert sorted(snap.files) == sorted(want)
    for k in want:
        assert np.array_equal(snap[k], want[k]), k

    # (4) tools/evaluate.py --log-dir reproduces that map from params.yaml + the snapshot
    # (in this process: the same convolution routes as the trainer's evaluator, tests/conftest.py)
    import argparse
    import evaluate
    import yaml
    evaluate.evaluate_log_dir(argparse.Namespace(log_dir=out_a, limit=0, coco_root=None,
                                                 sbd_root=None, custom_root=None))
    with open(os.path.join(out_a, 'snapshot_model.npz.eval_result.yaml')) as f:
        result = yaml.safe_load(f)
    got = result['validation/main/map']
    assert (got == best) or (np.isnan(got) and np.isnan(best)), (got, maps)
    assert os.path.exists(os.path.join(out_a, 'iteration=best.jpg'))
