"""Times of large-scale jitter on the device: 480x640 sources onto a
1024 x 1024 canvas, the longer side resized to r * 1024 for r in {0.1, 1.0, 2.0}, the crop window
in the middle, with a flip, for G in {1, 8, 64} instances.

  image       — device time of one mrcnn_prepare_image_crop launch, and of the same result composed
                from the primitives that predate it: mrcnn_prepare_image at the full resized size,
                then a slice into a zeroed canvas
  masks       — device time of one mrcnn_mask_resize_crop call (its two launches), and of the
                composition: mrcnn_mask_resize_nearest at the full resized size, a slice into a
                zeroed (G, S, S) stack, and torch reductions for the boxes and areas
                (inputs prepared once; device events around back-to-back launches; the two versions
                alternate, and the outputs are compared before anything is timed)
  transform   — one whole ``MaskRCNNTransform(scale_jitter=(r, r))`` call from a host example with a
                PackedMasks: uploads, the launches, the read-back of boxes and areas (host clock
                around a call that ends in a synchronise)
  worker      — `tools/train_loop.py --synthetic 64 --device-masks` with and without
                `--scale-jitter 0.1,2.0`, each in a fresh process: the worker's fetch ms/batch, the
                step's wait and ms/step

Writes profiles/scale_jitter.json.

    python tools/bench_scale_jitter.py [--reps 50] [--iterations 30] [--out profiles/scale_jitter.json]
"""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import chainer_mask_rcnn_amd as cmr  # noqa: E402
from chainer_mask_rcnn_amd import _lib  # noqa: E402
from chainer_mask_rcnn_amd import functions as F  # noqa: E402
from chainer_mask_rcnn_amd.datasets import PackedMasks, transforms as T  # noqa: E402
from chainer_mask_rcnn_amd.functions import scale_jitter as SJ  # noqa: E402

from bench_gt_masks import median_ms, polygons  # noqa: E402

IN_SIZE, S = (480, 640), 1024
MEAN = np.array([122.7717, 115.9465, 102.9801], np.float32)
X_FLIP = True


def geometry(r):
    scale = min(r * S / IN_SIZE[0], r * S / IN_SIZE[1])
    resized = T._resized_size(IN_SIZE, scale)
    return scale, resized, (max(resized[0] - S, 0) // 2, max(resized[1] - S, 0) // 2)


def event_ms(fns, reps):
    """Device time per call of each of ``fns``, alternating them: three warm-up rounds, then
    ``reps`` rounds with events around every call."""
    for _ in range(3):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    pairs = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            pairs[i].append((e0, e1))
    torch.cuda.synchronize()
    return [float(np.median([a.elapsed_time(b) for a, b in p])) for p in pairs]


def back_to_back_ms(fn, reps):
    """Device events around ``reps`` back-to-back calls (tools/bench_gt_masks.py:kernel_ms)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def image_ms(dev, img_chw, r, reps):
    scale, (rH, rW), (oy, ox) = geometry(r)
    src = torch.from_numpy(img_chw).to(dev)
    mean = (_lib.c_f32 * 3)(*MEAN)
    canvas = torch.empty((1, S, S, 3), dtype=torch.float32, device=dev)
    full = torch.zeros((1, rH, rW, 3), dtype=torch.float32, device=dev)
    composed = torch.empty((1, S, S, 3), dtype=torch.float32, device=dev)
    h, w = min(rH - oy, S), min(rW - ox, S)

    def fused():
        _lib.call('mrcnn_prepare_image_crop', _lib.ptr(src), 1, 3, IN_SIZE[0], IN_SIZE[1], scale, mean,
                  _lib.ptr(canvas), S, S, rH, rW, oy, ox, 0, int(X_FLIP), _lib.stream_ptr())

    def composition():
        _lib.call('mrcnn_prepare_image', _lib.ptr(src), 1, 3, IN_SIZE[0], IN_SIZE[1], scale, mean,
                  _lib.ptr(full), rH, rW, rH, rW, 0, int(X_FLIP), _lib.stream_ptr())
        composed.zero_()
        composed[0, :h, :w] = full[0, oy:oy + h, ox:ox + w]

    fused(), composition()
    assert torch.equal(canvas, composed)
    alt = event_ms([fused, composition], reps)
    return {'resized': [rH, rW], 'offset': [oy, ox], 'fused_ms': back_to_back_ms(fused, reps),
            'composition_ms': back_to_back_ms(composition, reps),
            'alternating_fused_ms': alt[0], 'alternating_composition_ms': alt[1],
            'intermediate_MB': rH * rW * 12 / 1e6}


def boxes_by_torch(masks):
    """Tight boxes (G, 4) and areas (G) of a (G, S, S) uint8 stack with torch reductions."""
    fg = masks != 0
    rows, cols = fg.any(dim=2), fg.any(dim=1)                         # (G, S) each
    n = masks.shape[1]
    idx = torch.arange(n, device=masks.device)
    big = torch.full_like(idx, n)

    def lo_hi(hit):
        lo = torch.where(hit, idx, big).min(dim=1).values
        hi = torch.where(hit, idx + 1, torch.zeros_like(idx)).max(dim=1).values
        return torch.where(hi > 0, lo, torch.zeros_like(lo)), hi
    y_lo, y_hi = lo_hi(rows)
    x_lo, x_hi = lo_hi(cols)
    area = masks.sum(dim=(1, 2), dtype=torch.int32)
    return torch.stack([y_lo, x_lo, y_hi, x_hi], 1).to(torch.int32), area


def masks_ms(dev, packed, r, reps):
    scale, (rH, rW), offset = geometry(r)
    oy, ox = offset
    G, H, W = packed.shape
    words, _ = F.upload_packed_masks(packed, dev)
    ys, xs = SJ.crop_tables((H, W), (rH, rW), offset, S, X_FLIP)
    tables = torch.from_numpy(np.concatenate([ys, xs])).to(dev)
    out = torch.empty((G, S, S), dtype=torch.uint8, device=dev)
    meta = torch.empty((G * 5,), dtype=torch.int32, device=dev)
    stats = torch.empty((G * S * 3,), dtype=torch.int32, device=dev)
    fys = T._nearest_index(rH, H)
    fxs = T._nearest_index(rW, W)[::-1] if X_FLIP else T._nearest_index(rW, W)
    ftab = torch.from_numpy(np.concatenate([fys, fxs]).astype(np.int32)).to(dev)
    full = torch.empty((G, rH, rW), dtype=torch.uint8, device=dev)
    composed = torch.empty((G, S, S), dtype=torch.uint8, device=dev)
    h, w = min(rH - oy, S), min(rW - ox, S)
    result = {}

    def fused():
        _lib.call('mrcnn_mask_resize_crop', _lib.ptr(words), G, H, W, _lib.ptr(tables[:S]),
                  _lib.ptr(tables[S:]), S, _lib.ptr(out), _lib.ptr(meta), _lib.ptr(meta[4 * G:]),
                  _lib.ptr(stats), _lib.stream_ptr())

    def composition():
        _lib.call('mrcnn_mask_resize_nearest', _lib.ptr(words), G, H, W, _lib.ptr(ftab[:rH]),
                  _lib.ptr(ftab[rH:]), rH, rW, _lib.ptr(full), _lib.stream_ptr())
        composed.zero_()
        composed[:, :h, :w] = full[:, oy:oy + h, ox:ox + w]
        result['boxes'], result['areas'] = boxes_by_torch(composed)

    fused(), composition()
    assert torch.equal(out, composed)
    assert torch.equal(meta[:4 * G].view(G, 4), result['boxes']) and torch.equal(meta[4 * G:], result['areas'])
    alt = event_ms([fused, composition], reps)
    fused_ms = back_to_back_ms(fused, reps)
    return {'fused_ms': fused_ms, 'composition_ms': back_to_back_ms(composition, reps),
            'alternating_fused_ms': alt[0], 'alternating_composition_ms': alt[1],
            'write_GB_per_s': G * S * S / (fused_ms * 1e-3) / 1e9,
            'intermediate_MB': G * rH * rW / 1e6}


class _Model(torch.nn.Module):
    """What the transform reads of a model: the mean and the device of its parameters."""

    def __init__(self, dev):
        super(_Model, self).__init__()
        self.mean = MEAN.reshape(3, 1, 1)
        self.p = torch.nn.Parameter(torch.zeros(1, device=dev))


def transform_ms(dev, example, r, reps):
    t = cmr.datasets.MaskRCNNTransform(_Model(dev), device_masks=True, scale_jitter=(r, r), crop_size=S)

    def call():
        t(example)
        torch.cuda.synchronize()
    return median_ms(call, reps)


def worker_ms(scale_jitter, iterations):
    """One `train_loop.py --synthetic 64 --device-masks` run in a fresh process."""
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'train_loop.py'), '--synthetic', '64',
           '--iterations', str(iterations), '--device-masks']
    if scale_jitter:
        cmd += ['--scale-jitter', scale_jitter]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        raise RuntimeError('train_loop.py failed:\n' + out.stdout + out.stderr)
    m = re.search(r'([\d.]+) ms/step.*input pipeline: ([\d.]+) ms/batch on the worker, the step '
                  r'waited ([\d.]+) ms/batch', out.stdout)
    return {'step_ms': float(m.group(1)), 'fetch_ms_per_batch': float(m.group(2)),
            'wait_ms_per_batch': float(m.group(3))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--iterations', type=int, default=30, help='train_loop.py steps per worker run '
                    '(0: skip the worker runs)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'scale_jitter.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_scale_jitter.py: no ROCm device')
    rng = np.random.RandomState(0)
    dev = torch.device('cuda:0')
    img = rng.randint(0, 256, IN_SIZE + (3,)).astype(np.uint8)
    chw = np.ascontiguousarray(img.transpose(2, 0, 1))
    raster = cmr.datasets.COCOInstanceSegmentationDataset._rasterise
    res = {'in_size': list(IN_SIZE), 'crop_size': S, 'x_flip': X_FLIP, 'image': {}, 'masks': {},
           'transform_ms': {}}
    packed = {G: PackedMasks.from_instances([raster(s, *IN_SIZE) for s in polygons(rng, G, *IN_SIZE)],
                                            *IN_SIZE) for G in (1, 8, 64)}
    for r in (0.1, 1.0, 2.0):
        res['image']['r=%g' % r] = image_ms(dev, chw, r, args.reps)
        for G in (1, 8, 64):
            key = 'r=%g,G=%d' % (r, G)
            res['masks'][key] = masks_ms(dev, packed[G], r, args.reps)
            example = (img, np.zeros((G, 4), np.float32), np.zeros((G,), np.int32), packed[G])
            res['transform_ms'][key] = transform_ms(dev, example, r, max(5, args.reps // 5))
    res['device'] = torch.cuda.get_device_name(0)
    if args.iterations > 0:
        res['worker'] = {'device_masks': worker_ms(None, args.iterations),
                         'scale_jitter_0.1_2.0': worker_ms('0.1,2.0', args.iterations)}
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
