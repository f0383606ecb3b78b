"""Train-loop counterpart of the reference's examples/train_common.py:200-231 for the HIP path:

    seeds (:135-136) -> dataset -> TransformDataset(MaskRCNNTransform) (:192-195)
          -> SerialIterator(batch_size_per_gpu) (:207-210) -> converter = concat_examples(padding=0,
             indices_concat=[0, 2, 3, 4], ...) (:219-225) -> StandardUpdater: optimizer.update(model,
             *batch) (:226-231)

chainer's iterator / updater classes are third-party (not in the reference repository); what is
restated here is their contract as train_common.py uses it: `SerialIterator` draws its order from
the GLOBAL `np.random` stream (a permutation at construction, a shuffle whenever an epoch ends,
batches wrap around the epoch boundary), `TransformDataset` applies the transform at access time
(so `MaskRCNNTransform`'s flip draws from Python's `random` happen in iteration order), and the
updater calls `optimizer.update(lossfun, *converter(batch))`.

MI355X arrangement: the input pipeline runs ONE BATCH AHEAD of the model on a worker thread and its
own HIP stream — JPEG decode / mask rasterisation and the host half of the transform (boxes, masks)
on the host cores, the image as decoded (uint8 HWC) over PCIe, resize + mean + flip + zero-padded
channels-last batch assembly in device kernels on that stream; the compute stream waits on an
event.  The random streams are consumed in the reference's order: the worker is the only consumer
of `random`; the iterator's `np.random` shuffle at an epoch end is drawn where the reference's
`next(iterator)` would draw it relative to the samplers' draws, so a batch that needs the NEXT
epoch's order is simply not fetched early.  `prefetch=False` is the reference's serial order and
gives bit-identical losses (tests/test_gpu_train_loop.py).

    python tools/train_loop.py --coco-root DIR --iterations 100      # a COCO-layout directory
    python tools/train_loop.py --synthetic 64 --iterations 20        # in-memory synthetic examples
    python tools/train_loop.py --dataset sbd --sbd-root DIR --split train   # VOC settings (20 classes)
    python tools/train_loop.py --synthetic 64 --device-masks        # masks as bits, resized on the device
    python tools/train_loop.py --synthetic 64 --device-masks --scale-jitter 0.1,2.0   # 1024 x 1024 crops
"""
import functools
import os
import random
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


class TransformDataset(object):
    """chainer.datasets.TransformDataset: ``transform(dataset[i])`` at access time."""

    def __init__(self, dataset, transform):
        self._dataset, self._transform = dataset, transform

    def __len__(self):
        return len(self._dataset)

    def __getitem__(self, i):
        return self._transform(self._dataset[i])


class SerialIterator(object):
    """chainer.iterators.SerialIterator(dataset, batch_size) with its defaults repeat=True,
    shuffle=True, split into the index decision (`next_indices`, where the global `np.random`
    stream is consumed exactly as `__next__` consumes it) and the data access."""

    def __init__(self, dataset, batch_size, shuffle=True):
        self.dataset, self.batch_size = dataset, batch_size
        self._order = np.random.permutation(len(dataset)) if shuffle else None
        self.current_position, self.epoch, self.is_new_epoch = 0, 0, False

    def crosses_epoch(self):
        """Will the next batch end an epoch (and therefore shuffle)?"""
        return self.current_position + self.batch_size >= len(self.dataset)

    def next_indices(self):
        i, N = self.current_position, len(self.dataset)
        i_end = i + self.batch_size
        order = self._order
        idx = list(range(i, min(i_end, N))) if order is None else [int(j) for j in order[i:i_end]]
        if i_end >= N:
            rest = i_end - N
            if order is not None:
                np.random.shuffle(order)
            if rest > 0:
                idx += list(range(rest)) if order is None else [int(j) for j in order[:rest]]
            self.current_position = rest
            self.epoch += 1
            self.is_new_epoch = True
        else:
            self.current_position = i_end
            self.is_new_epoch = False
        return idx

    def __next__(self):
        return [self.dataset[j] for j in self.next_indices()]

    next = __next__


def make_converter(device):
    """examples/train_common.py:219-225.  The reference also moves the boxes to the device, where
    its (cupy) target creators run; this build's creators consume boxes / labels / masks on the
    host (models/mask_rcnn_train_chain.py), so only the image batch is a device tensor.  A sixth
    field (the ignore planes of MaskRCNNTransform(crowd_ignore=True), a device tensor or None per
    example) is neither stacked nor moved: it stays a list."""
    from chainer_mask_rcnn_amd.datasets import concat_examples
    return functools.partial(concat_examples, device=device, padding=0,
                             indices_concat=[0, 2, 3, 4],   # img, _, labels, masks, scales
                             indices_to_device=[0])


def keep_host_buffers_mapped():
    """glibc serves every allocation above 128 KB by a fresh mmap and returns it to the kernel on
    free: the input pipeline's ~100 MB of mask arrays per batch would be page-faulted in again
    every iteration (measured: that costs more than producing their contents).  Raise the mmap /
    trim thresholds so that those blocks come from — and go back to — the process heap."""
    import ctypes
    try:
        libc = ctypes.CDLL('libc.so.6')
        M_TRIM_THRESHOLD, M_MMAP_THRESHOLD = -1, -3
        libc.mallopt(M_MMAP_THRESHOLD, 1 << 30)
        libc.mallopt(M_TRIM_THRESHOLD, 2147483647)
        return True
    except OSError:
        return False


class TrainLoop(object):
    """iterator -> converter -> optimizer.update, the input pipeline one batch ahead."""

    def __init__(self, iterator, chain, optimizer, device, prefetch=True, prefetch_frozen=True):
        self.iterator, self.chain, self.optimizer = iterator, chain, optimizer
        self.prefetch_frozen = prefetch_frozen
        self.device = torch.device(device)
        self.converter = make_converter(self.device)
        self.prefetch = prefetch and self.device.type == 'cuda'
        self.iteration = 0
        self.host_seconds = dict(fetch=0., wait=0.)
        keep_host_buffers_mapped()
        self._pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix='mrcnn-input') \
            if self.prefetch else None
        from chainer_mask_rcnn_amd.streams import copy_stream
        self._stream = copy_stream(self.device) if self.prefetch else None
        self._pending = None

    # -- input pipeline -----------------------------------------------------------------------
    def _assemble(self, indices):
        t0 = time.perf_counter()
        if self._stream is None:
            batch = self.converter([self.iterator.dataset[j] for j in indices])
            self.host_seconds['fetch'] += time.perf_counter() - t0
            return batch, None
        torch.cuda.set_device(self.device)
        with torch.cuda.stream(self._stream):
            examples = [self.iterator.dataset[j] for j in indices]
            t1 = time.perf_counter()
            batch = self.converter(examples)
            ready = torch.cuda.Event()
            ready.record(self._stream)
        self.host_seconds['fetch'] += time.perf_counter() - t0
        self.host_seconds['examples'] = self.host_seconds.get('examples', 0.) + t1 - t0
        return batch, ready

    def _submit(self):
        # a batch that ends an epoch shuffles the order from the global np.random stream: that
        # draw belongs AFTER the samplers' draws of the step before it, so it is not fetched early
        if self._pool is None or self.iterator.crosses_epoch():
            return None
        return self._pool.submit(self._assemble, self.iterator.next_indices())

    def _take(self):
        t0 = time.perf_counter()
        fut, self._pending = self._pending, None
        batch, ready = fut.result() if fut is not None else self._assemble(self.iterator.next_indices())
        self.host_seconds['wait'] += time.perf_counter() - t0
        if ready is not None:
            main = torch.cuda.current_stream(self.device)
            main.wait_event(ready)
            # allocated on the copy stream, read on the compute stream: the image batch and, with
            # device masks, the mask batch (the allocator must not reuse either under the step)
            # (and, with --crowd-ignore, the ignore planes: a list, one plane or None per image)
            for field in batch:
                for t in field if isinstance(field, list) else (field,):
                    if isinstance(t, torch.Tensor) and t.is_cuda:
                        t.record_stream(main)
        return batch

    def _peek_next_images(self):
        fut = self._pending
        if fut is None or not fut.done():
            return None
        batch, ready = fut.result()
        if ready is not None:
            torch.cuda.current_stream(self.device).wait_event(ready)
        return batch[0]

    # -- updater ------------------------------------------------------------------------------
    def step(self):
        """One iteration of StandardUpdater.update_core: returns the loss (device tensor)."""
        batch = self._take()
        self._pending = self._submit()          # batch k+1 is prepared while step k runs
        if self.prefetch_frozen and hasattr(self.chain, 'next_imgs'):
            # the extractor's frozen prefix of batch k+1 runs beside step k's backbone backward,
            # if the worker has delivered that batch by then (never waits for it)
            self.chain.next_imgs = self._peek_next_images
        imgs, bboxes, labels, masks, scales = batch[:5]
        # a sixth field (MaskRCNNTransform(crowd_ignore=True)): the ignore planes, a list
        extra = dict(ignores=batch[5]) if len(batch) > 5 else {}
        loss = self.optimizer.update(self.chain, imgs, bboxes, labels, masks, scales, **extra)
        self.iteration += 1
        return loss

    def run(self, n_iterations, report=None):
        losses = []
        for _ in range(n_iterations):
            losses.append(self.step())
            if report is not None:
                report(self, losses[-1])
        return losses

    def settle(self):
        """Wait until the worker has assembled the pending batch, without taking it: afterwards
        nothing runs on the worker (nor draws from Python's `random`) until the next step."""
        if self._pending is not None:
            self._pending.result()

    def close(self):
        if self._pool is not None:
            if self._pending is not None:
                self._pending.result()
                self._pending = None
            self._pool.shutdown()
            self._pool = None


class SyntheticInstances(object):
    """In-memory stand-in for COCOInstanceSegmentationDataset.get_example: decoded uint8 HWC
    images with ellipse instances, (img, bboxes, labels, masks) in the dataset's dtypes.  Source
    images are 480 x 800, which MaskRCNN.prepare scales to 800 x 1333 (scale 5/3)."""

    def __init__(self, n, seed=0, height=480, width=800, n_gt=8, n_fg_class=80, virtual_len=None):
        # ``virtual_len``: report that many examples (index modulo n) — an epoch as long as a real
        # dataset's with a handful of distinct images in memory
        self.virtual_len = virtual_len
        rng = np.random.RandomState(seed)
        yy, xx = np.mgrid[0:height, 0:width]
        self.examples = []
        for _ in range(n):
            img = rng.randint(0, 256, (height, width, 3)).astype(np.uint8)
            hh, ww = rng.uniform(20, 240, n_gt), rng.uniform(20, 240, n_gt)
            y0, x0 = rng.uniform(0, height - 20, n_gt), rng.uniform(0, width - 20, n_gt)
            b = np.stack([y0, x0, np.minimum(y0 + hh, height), np.minimum(x0 + ww, width)], 1)
            masks = np.zeros((n_gt, height, width), np.int32)
            bboxes = np.zeros((n_gt, 4), np.float32)
            for g in range(n_gt):
                cy, cx = (b[g, 0] + b[g, 2]) / 2, (b[g, 1] + b[g, 3]) / 2
                ry, rx = (b[g, 2] - b[g, 0]) / 2, (b[g, 3] - b[g, 1]) / 2
                masks[g] = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
                ys, xs = np.nonzero(masks[g])          # utils.mask_to_bbox: tight box of the mask
                bboxes[g] = (ys.min(), xs.min(), ys.max() + 1, xs.max() + 1)
            labels = rng.randint(0, n_fg_class, n_gt).astype(np.int32)
            self.examples.append((img, bboxes, labels, masks))

    def __len__(self):
        return self.virtual_len or len(self.examples)

    def __getitem__(self, i):
        return self.examples[i % len(self.examples)]


# --pooling-func -> the head's RoI feature extractor (examples/train_common.py:138-147)
POOLING_FUNCS = {'align': 'roi_align_2d', 'pooling': 'roi_pooling_2d', 'resize': 'crop_and_resize'}
# model settings of examples/voc/train.py (SBD / VOC2012: 20 foreground classes)
VOC_MODEL = dict(n_fg_class=20, min_size=600, max_size=1000, anchor_scales=(4, 8, 16, 32))


def build_voc_trainer(n_layers, device, lr_batch, defer=5):
    """``bench.build_trainer`` (which is fixed to the COCO settings) with examples/voc/train.py's
    model: the same optimizer, frozen layers, synthetic-weight scaling and deferred gradients."""
    import chainer_mask_rcnn_amd as cmr
    model = cmr.models.MaskRCNNResNet(n_layers=n_layers, pretrained_model=None, roi_size=14,
                                      pooling_func=cmr.functions.roi_align_2d, **VOC_MODEL)
    chain, opt = setup_training(model, device, lr_batch, defer=defer)
    return model, chain, opt, None


def setup_training(model, device, lr_batch, defer=5, synthetic_weights=True, make_sync=None,
                   hooks=()):
    """Train chain and optimizer of examples/train_common.py:171-190 for ``model``: MomentumSGD
    (lr 0.00125 * batch, momentum 0.9) + WeightDecay(1e-4), conv1 / bn1 / res2 and every
    AffineChannel2D frozen; ``synthetic_weights``: bench.stabilise_synthetic_weights (random
    init); ``defer``: the res5 weight gradients held back into the next step (optimizers.py);
    ``make_sync(opt)``: data parallel, creates the gradient sync (parallel.DataParallelGradSync)
    before the deferred parameters are chosen, as bench.build_trainer does; ``hooks``: further
    optimizer hooks (the gradient-norm hooks of optimizers.py need ``defer=0``)."""
    import bench
    import chainer_mask_rcnn_amd as cmr
    from chainer_mask_rcnn_amd import optimizers
    from chainer_mask_rcnn_amd.links import AffineChannel2D
    chain = cmr.models.MaskRCNNTrainChain(model).to(device)
    chain.train()
    opt = optimizers.MomentumSGD(lr=0.00125 * lr_batch, momentum=0.9)
    opt.setup(chain)
    opt.add_hook(optimizers.WeightDecay(rate=0.0001))
    for hook in hooks:
        opt.add_hook(hook)
    for link in (model.extractor.conv1, model.extractor.bn1, model.extractor.res2):
        optimizers.disable_update(link)
    for m in chain.modules():
        if isinstance(m, AffineChannel2D):
            optimizers.disable_update(m)
    if synthetic_weights:
        bench.stabilise_synthetic_weights(model)
    if make_sync is not None:
        make_sync(opt)
    if defer > 0:
        a, b1, b2 = model.head.res5.a, model.head.res5.b1, model.head.res5.b2
        opt.defer_weight_gradients([a.conv2.W, a.conv3.W, b1.conv2.W, b1.conv1.W, b1.conv3.W,
                                    b2.conv2.W, b2.conv1.W, b2.conv3.W, a.conv1.W,
                                    a.conv4.W][:defer])
    return chain, opt


def norm_hooks(grad_clip=0., skip_nonfinite=False):
    """The optimizer hooks of --grad-clip T / --skip-nonfinite (tools/train.py, this file)."""
    from chainer_mask_rcnn_amd import optimizers
    hooks = []
    if grad_clip:
        hooks.append(optimizers.GradientClipping(grad_clip))
    if skip_nonfinite:
        hooks.append(optimizers.SkipNonFiniteUpdate())
    return hooks


def scale_jitter_range(text):
    """``--scale-jitter LO,HI`` -> (lo, hi)."""
    import argparse
    try:
        lo, hi = (float(v) for v in text.split(','))
    except ValueError:
        raise argparse.ArgumentTypeError('expected LO,HI (two numbers), got %r' % (text,))
    if not 0 < lo <= hi:
        raise argparse.ArgumentTypeError('needs 0 < LO <= HI, got %r' % (text,))
    return lo, hi


def add_scale_jitter_arguments(ap):
    """--scale-jitter / --crop-size of this tool and tools/train.py.  Neither has an attribute
    when it is not given (a default run's recorded arguments stay as they were): read them with
    ``scale_jitter_options``."""
    import argparse
    ap.add_argument('--scale-jitter', type=scale_jitter_range, default=argparse.SUPPRESS,
                    metavar='LO,HI',
                    help='large-scale jitter: resize the longer side to r * crop size, r uniform in '
                         '[LO, HI], then crop or zero-pad to the square (needs --device-masks; '
                         'evaluation keeps min_size / max_size; off by default)')
    ap.add_argument('--crop-size', type=int, default=argparse.SUPPRESS,
                    help='side of the square training canvas of --scale-jitter (1024)')


def scale_jitter_options(ap, args):
    """(scale_jitter or None, crop_size) of the parsed ``args``; misuse ends in ``ap.error``.  With
    jitter on, ``args`` carries both values afterwards."""
    jitter, crop = getattr(args, 'scale_jitter', None), getattr(args, 'crop_size', 1024)
    if jitter is not None and not args.device_masks:
        ap.error('--scale-jitter needs --device-masks: the crops are built on the device')
    if crop <= 0:
        ap.error('--crop-size must be positive')
    if jitter is not None:
        args.crop_size = crop
    return jitter, crop


def copy_paste_probability(text):
    """``--copy-paste P`` -> P."""
    import argparse
    try:
        p = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError('expected a probability, got %r' % (text,))
    if not 0 < p <= 1:
        raise argparse.ArgumentTypeError('needs 0 < P <= 1, got %r' % (text,))
    return p


def add_copy_paste_argument(ap):
    """--copy-paste of this tool and tools/train.py; no attribute when it is not given, like
    --scale-jitter: read it with ``copy_paste_option``."""
    import argparse
    ap.add_argument('--copy-paste', type=copy_paste_probability, default=argparse.SUPPRESS,
                    metavar='P',
                    help='copy-paste augmentation: with probability P, instances of another training '
                         'example are pasted onto the example on the device (needs --scale-jitter: '
                         'both examples lie on its square; training data only; off by default)')


def copy_paste_option(ap, args):
    """The probability of the parsed ``args`` or None; misuse ends in ``ap.error``."""
    prob = getattr(args, 'copy_paste', None)
    if prob is not None and getattr(args, 'scale_jitter', None) is None:
        ap.error('--copy-paste needs --scale-jitter: examples are pasted on its fixed-size canvas')
    return prob


def build(dataset, n_layers=50, device='cuda:0', batch_size=2, seed=0, defer=5, prefetch=True,
          world=1, pooling_func='align', model_settings='coco', device_masks=False,
          scale_jitter=None, crop_size=1024, copy_paste=None):
    """Model, optimizer and loop as examples/train_common.py:135-231 builds them (COCO settings of
    examples/coco/train.py:36-38, or with ``model_settings='voc'`` those of
    examples/voc/train.py); ``pooling_func`` one of POOLING_FUNCS; ``device_masks``: the
    ground-truth masks travel as bits and are resized on the device (MaskRCNNTransform);
    ``scale_jitter`` = (lo, hi) with ``crop_size``: its large-scale jitter; ``copy_paste`` = P: the
    jittered examples go through ``datasets.CopyPasteDataset(prob=P)``."""
    import bench
    import chainer_mask_rcnn_amd as cmr
    random.seed(seed)                                   # :135-136
    np.random.seed(seed)
    torch.manual_seed(seed)
    device = torch.device(device)
    if pooling_func not in POOLING_FUNCS:
        raise ValueError('Unsupported pooling_func: {}'.format(pooling_func))
    if model_settings == 'voc':
        if world != 1:
            raise ValueError('the VOC settings are built for one device')
        model, chain, opt, sync = build_voc_trainer(n_layers, device, batch_size, defer=defer)
    elif model_settings == 'coco':
        model, chain, opt, sync = bench.build_trainer(n_layers, device, world, batch_size * world,
                                                      defer=defer)
    else:
        raise ValueError('model_settings must be coco or voc, got %r' % (model_settings,))
    model.head.pooling_func = getattr(cmr.functions, POOLING_FUNCS[pooling_func])
    train_data = TransformDataset(dataset, cmr.datasets.MaskRCNNTransform(
        model, device_masks=device_masks, scale_jitter=scale_jitter, crop_size=crop_size))
    if copy_paste is not None:
        train_data = cmr.datasets.CopyPasteDataset(train_data, copy_paste)
    it = SerialIterator(train_data, batch_size)
    return TrainLoop(it, chain, opt, device, prefetch=prefetch), model, chain, opt


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument('--dataset', default=None, choices=['coco', 'voc', 'sbd', 'synthetic'],
                    help='coco (default; synthetic with --synthetic N), voc (VOC2012) or sbd; voc '
                         'and sbd train the 20-class model of examples/voc/train.py')
    ap.add_argument('--coco-root', default=None, help='COCO-layout directory (annotations/, train2014/ ...)')
    ap.add_argument('--voc-root', default=None, help='VOCdevkit/VOC2012 directory')
    ap.add_argument('--sbd-root', default=None, help='benchmark_RELEASE/dataset directory of SBD')
    ap.add_argument('--split', default=None, help='minival (coco) / train (voc, sbd) by default')
    ap.add_argument('--synthetic', type=int, default=0, help='use N in-memory synthetic examples')
    ap.add_argument('--iterations', type=int, default=20)
    ap.add_argument('--layers', type=int, default=50, choices=[50, 101])
    ap.add_argument('--batch', type=int, default=2)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--no-prefetch', action='store_true')
    ap.add_argument('--pooling-func', default='align', choices=sorted(POOLING_FUNCS),
                    help='RoI feature extractor of the head: align (roi_align_2d), pooling '
                         '(roi_pooling_2d) or resize (crop_and_resize)')
    ap.add_argument('--device-masks', action='store_true',
                    help='ground-truth masks cross PCIe as bits and are resized / flipped by a HIP '
                         'kernel (COCO: the dataset also keeps them packed on the host)')
    ap.add_argument('--polygon-rule', choices=['pil', 'coco'], default='pil',
                    help="how COCO polygon annotations become masks: pil (PIL.ImageDraw, the "
                         "reference's) or coco (COCO's own rule; DESIGN.md section 25)")
    ap.add_argument('--device-polygons', action='store_true',
                    help='COCO polygons cross PCIe as vertices and are drawn by a HIP kernel '
                         '(needs --device-masks --polygon-rule coco)')
    add_scale_jitter_arguments(ap)
    add_copy_paste_argument(ap)
    ap.add_argument('--defer', type=int, default=5,
                    help='res5 weight gradients held back into the next step (0: none)')
    ap.add_argument('--grad-clip', type=float, default=0.,
                    help='optimizers.GradientClipping threshold (0: off; needs --defer 0)')
    ap.add_argument('--skip-nonfinite', action='store_true',
                    help='optimizers.SkipNonFiniteUpdate (needs --defer 0)')
    args = ap.parse_args()
    scale_jitter, crop_size = scale_jitter_options(ap, args)
    copy_paste = copy_paste_option(ap, args)
    if args.device_polygons and not (args.device_masks and args.polygon_rule == 'coco'):
        ap.error('--device-polygons needs --device-masks --polygon-rule coco')
    import chainer_mask_rcnn_amd as cmr
    if os.environ.get('TORCH_THREADS'):
        torch.set_num_threads(int(os.environ['TORCH_THREADS']))
    dataset = args.dataset or ('synthetic' if args.synthetic else 'coco')
    settings = 'voc' if dataset in ('voc', 'sbd') else 'coco'
    if dataset == 'synthetic':
        data = SyntheticInstances(args.synthetic or 64, seed=args.seed, virtual_len=4096)
    elif dataset == 'voc':
        data = cmr.datasets.VOC2012InstanceSegmentationDataset(args.split or 'train',
                                                               root_dir=args.voc_root)
    elif dataset == 'sbd':
        data = cmr.datasets.SBDInstanceSegmentationDataset(args.split or 'train',
                                                           root_dir=args.sbd_root)
    else:
        data = cmr.datasets.COCOInstanceSegmentationDataset(args.split or 'minival',
                                                            root_dir=args.coco_root,
                                                            packed_masks=args.device_masks,
                                                            polygon_rule=args.polygon_rule,
                                                            device_polygons=args.device_polygons)
    loop, model, chain, opt = build(data, args.layers, 'cuda:0', args.batch, args.seed,
                                    defer=args.defer, prefetch=not args.no_prefetch,
                                    pooling_func=args.pooling_func, model_settings=settings,
                                    device_masks=args.device_masks,
                                    scale_jitter=scale_jitter, crop_size=crop_size,
                                    copy_paste=copy_paste)
    for hook in norm_hooks(args.grad_clip, args.skip_nonfinite):
        opt.add_hook(hook)            # (refused with deferred weight gradients: --defer 0)
    for _ in range(int(os.environ.get('WARMUP', 3))):
        loop.step()
    opt.flush()
    torch.cuda.synchronize()
    loop.host_seconds = dict(fetch=0., wait=0.)
    t0 = time.perf_counter()
    losses = loop.run(args.iterations)
    opt.flush()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    loop.close()
    print('%d iterations, %.2f ms/step, %.2f img/s, loss %.5f; input pipeline: %.1f ms/batch on the '
          'worker, the step waited %.2f ms/batch for it'
          % (args.iterations, dt / args.iterations * 1e3, args.iterations * args.batch / dt,
             float(losses[-1].detach()), loop.host_seconds['fetch'] / args.iterations * 1e3,
             loop.host_seconds['wait'] / args.iterations * 1e3))


if __name__ == '__main__':
    main()
