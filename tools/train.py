"""Train Mask R-CNN to a snapshot: examples/train_common.py with examples/{coco,voc,
custom_dataset}/train.py, on tools/train_loop.py's loop and tools/trainer.py's Trainer.

    python tools/train.py --dataset coco --coco-root DIR --imagenet-weights ResNet-50-model.npz
    python tools/train.py --dataset voc --sbd-root DIR            # ImageNet weights at chainer's path
    python tools/train.py --dataset custom --custom-root DIR --allow-random-init
    python tools/train.py --dataset synthetic --synthetic 64 --max-epoch 0.05

writes ``<logs-dir>/<YYYYmmdd_HHMMSS>/``: params.yaml, log (JSON), loss.png, accuracy.png,
visualizations/, and snapshot_model.npz at the best ``validation/main/map``; read it back with
``tools/evaluate.py --log-dir`` and summarise runs with ``tools/summarize_logs.py``.

Data-parallel training (examples/train_common.py's ChainerMN set-up) is ``--multi-node`` under a
launcher, one process per GPU:

    torchrun --standalone --nproc-per-node 8 tools/train.py --multi-node --dataset voc --sbd-root DIR
    mpirun -n 4 python tools/train.py --multi-node ...      # single node: Open MPI's variables

The global batch is ``--batch-size-per-gpu`` x world size and the lr 0.00125 x global batch.  Every
rank trains on its shard of the training set (datasets.scatter_dataset, equal lengths, shuffled
with the run's seed), gradients are averaged by parallel.DataParallelGradSync, evaluation is
sharded and exact (extensions.create_multi_node_evaluator), the logged losses are means over all
ranks, and only rank 0 writes the run directory and prints.  Without --multi-node a world size
above 1 is refused, and --multi-node is refused without a launcher's environment.
"""
import argparse
import collections
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
                    help='data-parallel training, one process per GPU, under torchrun '
                         '(RANK / WORLD_SIZE / LOCAL_RANK) or mpirun (OMPI_COMM_WORLD_*); the global '
                         'batch is --batch-size-per-gpu x world size')
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
    ap.add_argument('--device-masks', action='store_true',
                    help='ground-truth masks cross PCIe as bits and are resized / flipped by a HIP '
                         'kernel (COCO: the dataset also keeps them packed on the host)')
    train_loop.add_scale_jitter_arguments(ap)
    train_loop.add_copy_paste_argument(ap)
    ap.add_argument('--crowd-ignore', nargs='?', type=float, const=0.7, default=argparse.SUPPRESS,
                    metavar='THRESH',
                    help="COCO crowd regions are ignored in training instead of being background: a "
                         "proposal or an anchor more than THRESH of which a crowd mask covers is not "
                         "sampled (Detectron's TRAIN.CROWD_FILTER_THRESH, 0.7; DESIGN.md section 24).  "
                         "Needs --device-masks and --dataset coco.  Recorded in params.yaml when given")
    ap.add_argument('--polygon-rule', choices=['pil', 'coco'], default=argparse.SUPPRESS,
                    help="how COCO polygon annotations become masks, in training and evaluation: pil "
                         "(PIL.ImageDraw, the reference's; the default) or coco (COCO's own rule, "
                         "pycocotools' rleFrPoly; DESIGN.md section 25).  Recorded in params.yaml when given")
    ap.add_argument('--device-polygons', action='store_true', default=argparse.SUPPRESS,
                    help='COCO polygons cross PCIe as vertices and are drawn by a HIP kernel: no '
                         'ground-truth mask exists on the host.  Needs --device-masks --polygon-rule coco')
    ap.add_argument('--eval-bbox', action='store_true',
                    help='the evaluator also scores the boxes: validation/main/bbox/map joins the '
                         'log and the printed report (the best snapshot stays on the mask map)')
    ap.add_argument('--eval-boundary', action='store_true', default=argparse.SUPPRESS,
                    help='the evaluator also scores Boundary AP (min of mask and boundary IoU): '
                         'validation/main/boundary/map joins the log and the printed report (the '
                         'best snapshot stays on the mask map)')
    ap.add_argument('--grad-clip', type=float, default=0.,
                    help='clip the global L2 norm of the averaged gradient at T '
                         '(optimizers.GradientClipping; 0: off).  Like --skip-nonfinite it turns '
                         'the deferred weight gradients off')
    ap.add_argument('--skip-nonfinite', action='store_true',
                    help='an update whose gradients hold a NaN or an infinity is skipped '
                         '(optimizers.SkipNonFiniteUpdate); a log window of nothing but skipped '
                         'updates ends the run')
    ap.add_argument('--warmup-iters', type=int, default=0,
                    help="Detectron's linear lr warm-up over the first N updates (0: off)")
    ap.add_argument('--warmup-factor', type=float, default=1. / 3.,
                    help='lr factor of update 0 with --warmup-iters')
    ap.add_argument('--arithmetic', default=argparse.SUPPRESS, choices=['fp32', 'split_bf16x3', 'split_bf16x2', 'bf16x1'],
                    help='arithmetic of the convolution GEMMs (functions.conv.set_gemm_arithmetic; default '
                         'split_bf16x3: fp32-accurate; split_bf16x2: 16-bit-class operands; bf16x1: bf16 '
                         'operands; all with fp32 accumulation and fp32 weights).  Recorded in params.yaml when given')
    ap.add_argument('--logs-dir', default=osp.join(ROOT, 'logs'))
    ap.add_argument('--no-plot', action='store_true', help='do not write loss.png / accuracy.png')
    args = ap.parse_args(argv)
    train_loop.scale_jitter_options(ap, args)
    train_loop.copy_paste_option(ap, args)
    if getattr(args, 'crowd_ignore', None) is not None:
        if not args.device_masks:
            ap.error('--crowd-ignore needs --device-masks (the ignore plane is built on the device)')
        if args.dataset != 'coco':
            ap.error('--crowd-ignore needs --dataset coco (crowd regions are COCO annotations)')
        if not 0 <= args.crowd_ignore <= 1:
            ap.error('--crowd-ignore THRESH must lie in [0, 1], got %r' % (args.crowd_ignore,))
    if getattr(args, 'device_polygons', False) and not (
            args.device_masks and getattr(args, 'polygon_rule', 'pil') == 'coco'):
        ap.error('--device-polygons needs --device-masks --polygon-rule coco')
    return args


OMPI_TO_TORCH = (('OMPI_COMM_WORLD_RANK', 'RANK'), ('OMPI_COMM_WORLD_SIZE', 'WORLD_SIZE'),
                 ('OMPI_COMM_WORLD_LOCAL_RANK', 'LOCAL_RANK'),
                 ('OMPI_COMM_WORLD_LOCAL_SIZE', 'LOCAL_WORLD_SIZE'))


def torch_env_from_ompi(environ):
    """The torch launcher variables an Open MPI launch implies (``mpirun -n N``: one node,
    rendezvous on 127.0.0.1), or {} where RANK is already set or Open MPI's are not."""
    if environ.get('RANK') or not environ.get('OMPI_COMM_WORLD_RANK'):
        return {}
    env = {dst: environ[src] for src, dst in OMPI_TO_TORCH if environ.get(src)}
    env.setdefault('LOCAL_RANK', env['RANK'])
    if 'MASTER_ADDR' not in environ:
        env['MASTER_ADDR'] = '127.0.0.1'
    if 'MASTER_PORT' not in environ:
        env['MASTER_PORT'] = '29500'
    return env


def world_size(environ=None):
    environ = os.environ if environ is None else environ
    return int(environ.get('WORLD_SIZE', '1') or 1)


def launch_error(args, environ):
    """Why this launch is refused, or None."""
    if not args.multi_node and world_size(environ) > 1:
        return ('tools/train.py: world size %d is not supported without --multi-node (launch one '
                'process per GPU with --multi-node for data-parallel training)\n'
                % world_size(environ))
    if args.multi_node and not environ.get('RANK'):
        return ('tools/train.py: --multi-node is not supported without a launcher (torchrun / '
                'mpirun) environment: RANK / WORLD_SIZE or OMPI_COMM_WORLD_* are not set\n')
    return None


class Comm(collections.namedtuple('Comm', 'rank world local n_node device')):
    """Where this process trains: its rank, the world size, the local rank, the number of hosts
    and the device."""

    @property
    def parallel(self):
        return self.world > 1

    def gather(self, obj):
        """Every rank's ``obj`` in rank order (the control plane: gloo, CPU tensors)."""
        from chainer_mask_rcnn_amd import parallel
        return parallel.all_gather_object_cpu(obj)

    def broadcast(self, obj):
        if not self.parallel:
            return obj
        from chainer_mask_rcnn_amd import parallel
        return parallel.broadcast_object_cpu(obj, src=0)

    def close(self):
        import torch.distributed as dist
        if self.parallel and dist.is_initialized():
            dist.destroy_process_group()


def setup_comm(args):
    """Join the process group (``--multi-node``: parallel.init_from_env, which puts every rank on
    device 0 under MRCNN_DP_REHEARSAL=1) and select the rank's device."""
    import torch
    if not args.multi_node:
        return Comm(0, 1, 0, 1, torch.device('cuda:0'))
    from chainer_mask_rcnn_amd import parallel
    rank, world, local = parallel.init_from_env()
    local_world = int(os.environ.get('LOCAL_WORLD_SIZE', str(world)) or world)
    dev = torch.device('cuda', local)
    if world > 1:
        torch.cuda.set_device(dev)
    return Comm(rank, world, local, max(1, world // local_world), dev)


COCO_MODEL = dict(min_size=800, max_size=1333, anchor_scales=(2, 4, 8, 16, 32))
VOC_MODEL = dict(min_size=600, max_size=1000, anchor_scales=(4, 8, 16, 32))
SYNTHETIC_CLASS_NAMES = np.array(['class%d' % i for i in range(80)])


def test_dataset(args):
    """(test_data, evaluator type) of ``args.dataset`` (also used by tools/evaluate.py --log-dir)."""
    import chainer_mask_rcnn_amd as cmr
    if args.dataset == 'coco':                       # examples/coco/train.py
        return cmr.datasets.COCOInstanceSegmentationDataset(
            'minival', root_dir=args.coco_root, use_crowd=True, return_crowd=True,
            return_area=True, polygon_rule=getattr(args, 'polygon_rule', 'pil')), 'coco'
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
        packed = getattr(args, 'device_masks', False)
        # --crowd-ignore: the crowd regions come along, flagged, and leave the transform as a plane
        crowds = dict(use_crowd=True, return_crowd=True) \
            if getattr(args, 'crowd_ignore', None) is not None else {}
        crowds.update(polygon_rule=getattr(args, 'polygon_rule', 'pil'),
                      device_polygons=getattr(args, 'device_polygons', False))
        train_data = T.ConcatenatedDataset(
            cmr.datasets.COCOInstanceSegmentationDataset('train', root_dir=args.coco_root,
                                                         packed_masks=packed, **crowds),
            cmr.datasets.COCOInstanceSegmentationDataset('valminusminival', root_dir=args.coco_root,
                                                         packed_masks=packed, **crowds))
        return train_data, test_data, test_data.class_names, COCO_MODEL, evaluator_type
    if args.dataset == 'voc':
        train_data = cmr.datasets.SBDInstanceSegmentationDataset('train', root_dir=args.sbd_root)
        return train_data, test_data, train_data.class_names, VOC_MODEL, evaluator_type
    if args.dataset == 'custom':
        train_data = T.ConcatenatedDataset(*([T.VOCLikeDataset(args.custom_root)] * 20))
        return train_data, test_data, test_data.class_names, VOC_MODEL, evaluator_type
    train_data = train_loop.SyntheticInstances(args.synthetic, seed=0, virtual_len=args.synthetic_epoch)
    return train_data, test_data, SYNTHETIC_CLASS_NAMES, COCO_MODEL, evaluator_type


def configure(args, comm, class_names, settings, now=None):
    """The run's derived settings (examples/train_common.py:96-136): seed, run directory (rank
    0's clock, broadcast), n_gpu / n_node, global batch, lr, lr steps and the model settings;
    then the seeds."""
    import torch
    args.seed = 0
    if comm.rank == 0:
        now = now or datetime.datetime.now()
        args.timestamp = now.isoformat()
        args.out = osp.join(args.logs_dir, now.strftime('%Y%m%d_%H%M%S'))
    args.timestamp, args.out = comm.broadcast((getattr(args, 'timestamp', None),
                                               getattr(args, 'out', None)))
    args.n_node, args.n_gpu = comm.n_node, comm.world
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


def build_model(args, weights, **kwargs):
    """MaskRCNNResNet of the run (``kwargs``: further constructor arguments)."""
    import chainer_mask_rcnn_amd as cmr
    pooling_func = getattr(cmr.functions, train_loop.POOLING_FUNCS[args.pooling_func])
    mask_initialW = 0.01 if args.initializer == 'normal' else 'he_normal'
    return cmr.models.MaskRCNNResNet(
        n_layers=int(args.model[len('resnet'):]), n_fg_class=len(args.class_names),
        pooling_func=pooling_func, anchor_scales=args.anchor_scales, roi_size=args.roi_size,
        min_size=args.min_size, max_size=args.max_size, mask_initialW=mask_initialW,
        mean=args.mean, pretrained_model='imagenet' if weights else None,
        imagenet_weights=weights, **kwargs)


# switches recorded in params.yaml only when set: a default run's file stays as it was
OPTIONAL_PARAMS = ('eval_bbox', 'grad_clip', 'skip_nonfinite', 'warmup_iters')


def recorded_params(args):
    """vars(args) as params.yaml records them."""
    params = {k: v for k, v in vars(args).items() if k not in OPTIONAL_PARAMS or v}
    if not params.get('warmup_iters'):
        params.pop('warmup_factor', None)
    if 'scale_jitter' in params:                      # (present only when given, with crop_size)
        params['scale_jitter'] = [float(v) for v in params['scale_jitter']]
    return params


Run = collections.namedtuple('Run', 'trainer loop chain optimizer evaluator train test')


def assemble(args, comm, model, train_data, test_data, evaluator_type, synthetic_weights,
             print_out=sys.stdout, **intervals):
    """Train chain, optimizer (with the gradient sync under data parallelism), the rank's shards
    of the data, loop, evaluator and the trainer with the reference's extensions; ``intervals``:
    eval_interval / log_interval / plot_interval / print_interval of
    trainer.extend_reference_set.  Returns a Run; ``trainer.run()`` trains."""
    import chainer_mask_rcnn_amd as cmr
    make_sync = None
    if comm.parallel:
        from chainer_mask_rcnn_amd import parallel

        def make_sync(opt):
            return parallel.DataParallelGradSync(opt)
    hooks = train_loop.norm_hooks(getattr(args, 'grad_clip', 0.),
                                  getattr(args, 'skip_nonfinite', False))
    # a gradient-norm hook needs every gradient in the arena at the step: no deferral
    chain, opt = train_loop.setup_training(model, comm.device, args.batch_size,
                                           synthetic_weights=synthetic_weights,
                                           make_sync=make_sync, hooks=hooks,
                                           **({'defer': 0} if hooks else {}))

    # examples/train_common.py:200-205: scattered train / test data
    train_data = cmr.datasets.scatter_dataset(train_data, comm.rank, comm.world, shuffle=True,
                                              seed=args.seed)
    test_data = cmr.datasets.scatter_dataset(test_data, comm.rank, comm.world,
                                             force_equal_length=False)
    train = train_loop.TransformDataset(train_data, cmr.datasets.MaskRCNNTransform(
        model, device_masks=getattr(args, 'device_masks', False),
        scale_jitter=getattr(args, 'scale_jitter', None), crop_size=getattr(args, 'crop_size', 1024),
        crowd_ignore=getattr(args, 'crowd_ignore', None) is not None))
    if getattr(args, 'crowd_ignore', None) is not None:
        chain.crowd_ignore_thresh = float(args.crowd_ignore)
    if getattr(args, 'copy_paste', None) is not None:   # the partner comes from the rank's own shard
        train = cmr.datasets.CopyPasteDataset(train, args.copy_paste)
    test = train_loop.TransformDataset(test_data, cmr.datasets.MaskRCNNTransform(model, train=False))
    loop = train_loop.TrainLoop(train_loop.SerialIterator(train, args.batch_size_per_gpu),
                                chain, opt, comm.device)
    test_iter = train_loop.SerialIterator(test, args.batch_size_per_gpu, shuffle=False)
    eval_bbox = bool(getattr(args, 'eval_bbox', False))
    eval_boundary = bool(getattr(args, 'eval_boundary', False))
    iou_types = ('segm',) + (('bbox',) if eval_bbox else ()) + (
        ('boundary',) if eval_boundary else ())
    kw = {'iou_types': iou_types} if len(iou_types) > 1 else {}
    if evaluator_type == 'voc':
        evaluator = cmr.extensions.InstanceSegmentationVOCEvaluator(
            test_iter, model, use_07_metric=True, label_names=args.class_names, **kw)
    else:
        evaluator = cmr.extensions.InstanceSegmentationCOCOEvaluator(
            test_iter, model, label_names=args.class_names, **kw)
    if comm.parallel:
        evaluator = cmr.extensions.create_multi_node_evaluator(evaluator)

    args.git_hash = cmr.utils.git_hash(__file__)
    args.hostname = socket.gethostname()
    params = recorded_params(args)
    warmup_iters = getattr(args, 'warmup_iters', 0)
    warmup = T.LinearWarmup(warmup_iters, getattr(args, 'warmup_factor', 1. / 3.)) \
        if warmup_iters else None
    tr = T.Trainer(loop, (args.max_epoch, 'epoch'), out=args.out if comm.rank == 0 else None)
    T.extend_reference_set(tr, model, evaluator=evaluator, vis_iterator=test_iter,
                           class_names=args.class_names, step_size=args.step_size,
                           params=params, plot=not args.no_plot,
                           print_out=print_out if comm.rank == 0 else None, rank=comm.rank,
                           gather=comm.gather if comm.parallel else None, eval_bbox=eval_bbox,
                           eval_boundary=eval_boundary,
                           warmup=warmup, grad_report=bool(hooks), **intervals)
    return Run(tr, loop, chain, opt, evaluator, train_data, test_data)


def main(argv=None):
    args = parse_args(argv)
    os.environ.update(torch_env_from_ompi(os.environ))
    err = launch_error(args, os.environ)
    if err:
        sys.stderr.write(err)
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

    comm = setup_comm(args)
    try:
        train_data, test_data, class_names, settings, evaluator_type = datasets(args)
        configure(args, comm, class_names, settings)
        if getattr(args, 'arithmetic', None) is not None:
            from chainer_mask_rcnn_amd.functions import conv
            conv.set_gemm_arithmetic(args.arithmetic)
        model = build_model(args, weights)
        args.imagenet_weights = weights
        run = assemble(args, comm, model, train_data, test_data, evaluator_type,
                       synthetic_weights=weights is None)
        try:
            run.trainer.run()
        finally:
            run.loop.close()
        if comm.rank == 0:
            print('Saved logs:', args.out)
    finally:
        comm.close()
    return 0


if __name__ == '__main__':
    sys.exit(main())
