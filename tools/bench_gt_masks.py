"""Times of the ground-truth mask path:

  kernel      — device time of one mrcnn_mask_resize_nearest launch, 480x640 -> 800x1333 with a
                flip, for G in {1, 8, 64} instances, and the write bandwidth it reaches (the
                kernel is bound by its G * 800 * 1333 uint8 writes; inputs prepared once; device
                events around back-to-back launches)
  call        — functions.resize_masks_nearest from a host PackedMasks (upload of the words and
                the tables, launch, synchronise)
  host        — the dense host path for one 480x640 example with 8 polygon instances: PIL
                rasterisation, the int32 stack, resize_nearest + flip to 800x1333, _concat_arrays
                of a 2-image batch, the 14x14 targets of 64 foreground RoIs; and np.packbits of
                the same masks (PackedMasks.from_instances)
  worker      — `tools/train_loop.py --synthetic` with and without --device-masks, each in a
                fresh process: the worker's fetch ms/batch, the step's wait and ms/step

Writes profiles/gt_masks.json.

    python tools/bench_gt_masks.py [--reps 50] [--iterations 30] [--out profiles/gt_masks.json]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import chainer_mask_rcnn_amd as cmr  # noqa: E402
from chainer_mask_rcnn_amd import _lib  # noqa: E402
from chainer_mask_rcnn_amd import functions as F  # noqa: E402
from chainer_mask_rcnn_amd.datasets import PackedMasks, transforms as T  # noqa: E402
from chainer_mask_rcnn_amd.datasets.concat_examples import _concat_arrays  # noqa: E402

IN_SIZE, OUT_SIZE = (480, 640), (800, 1333)


def polygons(rng, G, H, W):
    """G octagons as COCO polygon segmentations ([[x0, y0, x1, y1, ...]])."""
    segs = []
    for _ in range(G):
        cy, cx = rng.uniform(60, H - 60), rng.uniform(60, W - 60)
        ry, rx = rng.uniform(20, 160), rng.uniform(20, 200)
        a = np.arange(8) * (2 * np.pi / 8)
        xy = np.stack([np.clip(cx + rx * np.cos(a), 0, W - 1), np.clip(cy + ry * np.sin(a), 0, H - 1)], 1)
        segs.append([[float(v) for v in xy.reshape(-1)]])
    return segs


def median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts) * 1e3)


def kernel_ms(packed, reps):
    dev = torch.device('cuda:0')
    G, H, W = packed.shape
    words, _ = F.upload_packed_masks(packed, dev)
    ys = T._nearest_index(OUT_SIZE[0], H)
    xs = T._nearest_index(OUT_SIZE[1], W)[::-1]
    ys_d = torch.from_numpy(ys.astype(np.int32)).to(dev)
    xs_d = torch.from_numpy(xs.astype(np.int32)).to(dev)
    out = torch.empty((G,) + OUT_SIZE, dtype=torch.uint8, device=dev)

    def launch():
        _lib.call('mrcnn_mask_resize_nearest', _lib.ptr(words), G, H, W, _lib.ptr(ys_d),
                  _lib.ptr(xs_d), OUT_SIZE[0], OUT_SIZE[1], _lib.ptr(out), _lib.stream_ptr())
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def host_path_ms(rng, reps):
    """The dense host path of one example, step by step (the table of the issue that asked for
    the device path, on this host)."""
    H, W = IN_SIZE
    segs = polygons(rng, 8, H, W)
    raster = cmr.datasets.COCOInstanceSegmentationDataset._rasterise
    insts = [raster(s, H, W) for s in segs]
    stack = np.asarray(insts, dtype=np.int32)
    big = T.resize_nearest(stack, OUT_SIZE, x_flip=True)
    ptc = cmr.models.utils.ProposalTargetCreator()
    y0, x0 = rng.uniform(0, 600, 64), rng.uniform(0, 1100, 64)
    boxes = np.round(np.stack([y0, x0, y0 + rng.uniform(20, 200, 64), x0 + rng.uniform(20, 230, 64)], 1))
    job = (64, 64, boxes.astype(np.int32), rng.randint(0, 8, 64))
    res = {
        'pil_rasterise_ms': median_ms(lambda: [raster(s, H, W) for s in segs], reps),
        'int32_stack_ms': median_ms(lambda: np.asarray(insts, dtype=np.int32), reps),
        'resize_nearest_flip_ms': median_ms(lambda: T.resize_nearest(stack, OUT_SIZE, x_flip=True), reps),
        'concat_arrays_2_images_ms': median_ms(lambda: _concat_arrays([big, big], 0), reps),
        'mask_targets_64_rois_ms': median_ms(lambda: ptc.mask_targets(job, big), reps),
        'packbits_from_instances_ms': median_ms(lambda: PackedMasks.from_instances(insts, H, W), reps),
        'dense_MB_per_image': big.nbytes / 1e6,
        'packed_MB_per_image': PackedMasks.from_instances(insts, H, W).words.nbytes / 1e6,
    }
    return res


def worker_ms(device_masks, iterations):
    """One `train_loop.py --synthetic` run in a fresh process: the numbers of its last line."""
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'train_loop.py'), '--synthetic', '64',
           '--iterations', str(iterations)] + (['--device-masks'] if device_masks else [])
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gt_masks.json'))
    args = ap.parse_args()
    rng = np.random.RandomState(0)
    dev = torch.device('cuda:0')
    res = {'in_size': list(IN_SIZE), 'out_size': list(OUT_SIZE), 'kernel_ms': {}, 'write_GB_per_s': {},
           'call_ms': {}}
    raster = cmr.datasets.COCOInstanceSegmentationDataset._rasterise
    for G in (1, 8, 64):
        packed = PackedMasks.from_instances([raster(s, *IN_SIZE) for s in polygons(rng, G, *IN_SIZE)],
                                            *IN_SIZE)
        ms = kernel_ms(packed, args.reps)
        res['kernel_ms']['G=%d' % G] = ms
        res['write_GB_per_s']['G=%d' % G] = G * OUT_SIZE[0] * OUT_SIZE[1] / (ms * 1e-3) / 1e9

        def call():
            F.resize_masks_nearest(F.upload_packed_masks(packed, dev), OUT_SIZE, x_flip=True)
            torch.cuda.synchronize()
        res['call_ms']['G=%d' % G] = median_ms(call, max(5, args.reps // 5))
    res['host'] = host_path_ms(rng, max(5, args.reps // 5))
    res['device'] = torch.cuda.get_device_name(0)
    if args.iterations > 0:
        res['worker'] = {'host_masks': worker_ms(False, args.iterations),
                         'device_masks': worker_ms(True, args.iterations)}
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
