"""Train Mask R-CNN to a snapshot: examples/train_common.py with examples/{coco,voc,
custom_dataset}/train.py, on tools/train_loop.py's loop and tools/trainer.py's Trainer.

    python tools/train.py --dataset coco --coco-root DIR --imagenet-weights ResNet-50-model.npz
    python tools/train.py --dataset voc --sbd-root DIR            # ImageNet weights at chainer's path
    python tools/train.py --dataset custom --custom-root DIR --allow-random-init
    python tools/train.py --dataset synthetic --synthetic 64 --max-epoch 0.05

writes ``<logs-dir>/<YYYYmmdd_HHMMSS>/``: params.yaml, log (JSON), loss.png, accuracy.png,
visualizations/, and snapshot_model.npz at the best ``validation/main/map``; read it back with
``tools/evaluate.py --log-dir`` and summarise runs with ``tools/summarize_logs.py``.
One device only: data-parallel training (world size > 1) is refused.
"""
import argparse
import datetime
import os
import os.path as osp
import random
import socket
import sys

import numpy as np

HERE = osp.dirname(osp.abspath(__file__))
ROOT = osp.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import train_loop  # noqa: E402
import trainer as T  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    # examples/train_common.py:parse_args
    ap.add_argument('--model', '-m', choices=['resnet50', 'resnet101'], default='resnet50')
    ap.add_argument('--pooling-func', '-p', choices=['pooling', 'align', 'resize'],
                    default='align')
    ap.add_argument('--roi-size', '-r', type=int, default=14)
    ap.add_argument('--initializer', choices=['normal', 'he_normal'], default='normal')
    ap.add_argument('--max-epoch', type=float, default=180e3 * 8 / 118287,
                    help='epochs (180k iterations of batch 8 on COCO train+valminusminival)')
    ap.add_argument('--batch-size-per-gpu', type=int, default=1)
    ap.add_argument('--multi-node', action='store_true',
                    help='data-parallel training: not supported (refused)')
    # this driver
    ap.add_argument('--dataset', choices=['coco', 'voc', 'custom', 'synthetic'], default='coco')
    ap.add_argument('--coco-root', default=None, help='COCO-layout directory')
    ap.add_argument('--sbd-root', default=None, help='benchmark_RELEASE/dataset directory of SBD')
    ap.add_argument('--custom-root', default=None,
                    help='VOC-like directory (JPEGImages/, SegmentationClass/, SegmentationObject/)')
    ap.add_argument('--synthetic', type=int, default=64, help='synthetic examples (--dataset synthetic)')
    ap.add_argument('--synthetic-epoch', type=int, default=4096,
                    help='examples per epoch of --dataset synthetic (index modulo --synthetic, as '
                         'tools/train_loop.py --synthetic)')
    ap.add_argument('--imagenet-weights', default=None,
                    help="chainer's ResNet-{50,101}-model.npz (default: chainer's location under "
                         "$CHAINER_DATASET_ROOT)")
    ap.add_argument('--allow-random-init', action='store_true',
                    help='train a real dataset from random weights when no ImageNet weights exist')
    ap.add_argument('--logs-dir', default=osp.join(ROOT, 'logs'))
    ap.add_argument('--no-plot', action='store_true', help='do not write loss.png / accuracy.png')
    return ap.parse_args(argv)


def world_size(args):
    if args.multi_node:
        return 2
    return int(os.environ.get('WORLD_SIZE', '1') or 1)


COCO_MODEL = dict(min_size=800, max_size=1333, anchor_scales=(2, 4, 8, 16, 32))
VOC_MODEL = dict(min_size=600, max_size=1000, anchor_scales=(4, 8, 16, 32))
SYNTHETIC_CLASS_NAMES = np.array(['class%d' % i for i in range(80)])


def test_dataset(args):
    """(test_data, evaluator type) of ``args.dataset`` (also used by tools/evaluate.py --log-dir)."""
    import chainer_mask_rcnn_amd as cmr
    if args.dataset == 'coco':                       # examples/coco/train.py
        return cmr.datasets.COCOInstanceSegmentationDataset(
            'minival', root_dir=args.coco_root, use_crowd=True, return_crowd=True,
            return_area=True), 'coco'
    if args.dataset == 'voc':                        # examples/voc/train.py
        return cmr.datasets.SBDInstanceSegmentationDataset('val', root_dir=args.sbd_root), 'voc'
    if args.dataset == 'custom':                     # examples/custom_dataset/train.py
        if args.custom_root is None:
            raise SystemExit('--dataset custom needs --custom-root')
        return T.VOCLikeDataset(args.custom_root), 'voc'
    return train_loop.SyntheticInstances(min(args.synthetic, 8), seed=1), 'coco'


def datasets(args):
    """(train_data, test_data, class_names, model settings, evaluator type) of the dataset."""
    import chainer_mask_rcnn_amd as cmr
    test_data, evaluator_type = test_dataset(args)
    if args.dataset == 'coco':
        train_data = T.ConcatenatedDataset(
            cmr.datasets.COCOInstanceSegmentationDataset('train', root_dir=args.coco_root),
            cmr.datasets.COCOInstanceSegmentationDataset('valminusminival', root_dir=args.coco_root))
        return train_data, test_data, test_data.class_names, COCO_MODEL, evaluator_type
    if args.dataset == 'voc':
        train_data = cmr.datasets.SBDInstanceSegmentationDataset('train', root_dir=args.sbd_root)
        return train_data, test_data, train_data.class_names, VOC_MODEL, evaluator_type
    if args.dataset == 'custom':
        train_data = T.ConcatenatedDataset(*([T.VOCLikeDataset(args.custom_root)] * 20))
        return train_data, test_data, test_data.class_names, VOC_MODEL, evaluator_type
    train_data = train_loop.SyntheticInstances(args.synthetic, seed=0, virtual_len=args.synthetic_epoch)
    return train_data, test_data, SYNTHETIC_CLASS_NAMES, COCO_MODEL, evaluator_type


def main(argv=None):
    args = parse_args(argv)
    if world_size(args) > 1:
        sys.stderr.write('tools/train.py trains on one device: world size %d is not supported '
                         '(data-parallel training is not implemented in this driver)\n'
                         % world_size(args))
        return 2
    weights = args.imagenet_weights
    n_layers = int(args.model[len('resnet'):])
    if weights is None and args.dataset != 'synthetic':
        from chainer_mask_rcnn_amd import serializers
        default = serializers.default_imagenet_path(n_layers)
        if osp.exists(default):
            weights = default
        elif not args.allow_random_init:
            sys.stderr.write('no ImageNet weights: %s does not exist; pass --imagenet-weights PATH '
                             'or --allow-random-init to train from random weights\n' % default)
            return 2
    if args.dataset == 'synthetic':
        weights = None

    import torch
    import chainer_mask_rcnn_amd as cmr
    train_data, test_data, class_names, settings, evaluator_type = datasets(args)

    args.seed = 0
    now = datetime.datetime.now()
    args.timestamp = now.isoformat()
    args.out = osp.join(args.logs_dir, now.strftime('%Y%m%d_%H%M%S'))
    args.n_node, args.n_gpu = 1, 1
    args.batch_size = args.batch_size_per_gpu * args.n_gpu
    args.lr = 0.00125 * args.batch_size
    args.weight_decay = 0.0001
    args.step_size = [(120e3 / 180e3) * args.max_epoch, (160e3 / 180e3) * args.max_epoch]
    args.class_names = tuple(str(n) for n in class_names)
    args.min_size, args.max_size = settings['min_size'], settings['max_size']
    args.anchor_scales = settings['anchor_scales']
    args.mean = (123.152, 115.903, 103.063)

    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    dev = torch.device('cuda:0')
    pooling_func = getattr(cmr.functions, train_loop.POOLING_FUNCS[args.pooling_func])
    mask_initialW = 0.01 if args.initializer == 'normal' else 'he_normal'
    model = cmr.models.MaskRCNNResNet(
        n_layers=n_layers, n_fg_class=len(class_names), pooling_func=pooling_func,
        anchor_scales=args.anchor_scales, roi_size=args.roi_size, min_size=args.min_size,
        max_size=args.max_size, mask_initialW=mask_initialW, mean=args.mean,
        pretrained_model='imagenet' if weights else None, imagenet_weights=weights)
    args.imagenet_weights = weights
    chain, opt = train_loop.setup_training(model, dev, args.batch_size,
                                           synthetic_weights=weights is None)

    train = train_loop.TransformDataset(train_data, cmr.datasets.MaskRCNNTransform(model))
    test = train_loop.TransformDataset(test_data, cmr.datasets.MaskRCNNTransform(model, train=False))
    loop = train_loop.TrainLoop(train_loop.SerialIterator(train, args.batch_size_per_gpu),
                                chain, opt, dev)
    test_iter = train_loop.SerialIterator(test, args.batch_size_per_gpu, shuffle=False)
    if evaluator_type == 'voc':
        evaluator = cmr.extensions.InstanceSegmentationVOCEvaluator(
            test_iter, model, use_07_metric=True, label_names=args.class_names)
    else:
        evaluator = cmr.extensions.InstanceSegmentationCOCOEvaluator(
            test_iter, model, label_names=args.class_names)

    args.git_hash = cmr.utils.git_hash(__file__)
    args.hostname = socket.gethostname()
    params = {k: v for k, v in vars(args).items()}
    tr = T.Trainer(loop, (args.max_epoch, 'epoch'), out=args.out)
    T.extend_reference_set(tr, model, evaluator=evaluator, vis_iterator=test_iter,
                           class_names=args.class_names, step_size=args.step_size,
                           params=params, plot=not args.no_plot)
    try:
        tr.run()
    finally:
        loop.close()
    print('Saved logs:', args.out)
    return 0


if __name__ == '__main__':
    sys.exit(main())
