"""Times of instance drawing and of the visual report:

  kernel      — device time of one mrcnn_draw_instances launch on an 800x1333 image with N in
                {10, 100} instances, with and without captions (inputs prepared once; device
                events around back-to-back launches)
  call        — utils.draw_instance_bboxes with a host image and host (N, H, W) masks in, the
                drawn host image out (record build, caption rendering, uploads, packing,
                kernel, read-back)
  report      — one InstanceSegmentationVisReport.render() of a 3x3 mosaic with an R-50 model
                at min_size 480 (nine 480x640 images, prediction included)
  numpy       — the NumPy restatement (tests/visualize_ref.py) on the host, the reference's way
                of drawing: per-instance crops, boolean indexing and boundaries

Writes profiles/visualize.json.

    python tools/bench_visualize.py [--reps 50] [--out profiles/visualize.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import chainer_mask_rcnn_amd as cmr  # noqa: E402
from chainer_mask_rcnn_amd import _lib  # noqa: E402
from chainer_mask_rcnn_amd.utils import visualizations as V  # noqa: E402
from chainer_mask_rcnn_amd.utils.evaluations import masks as M  # noqa: E402
import visualize_ref as R  # noqa: E402

H, W = 800, 1333


def scene(rng, N):
    img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    y1, x1 = rng.uniform(0, H - 40, N), rng.uniform(0, W - 40, N)
    bboxes = np.stack([y1, x1, np.minimum(y1 + rng.uniform(30, 300, N), H),
                       np.minimum(x1 + rng.uniform(30, 400, N), W)], 1).astype(np.float32)
    yy, xx = np.mgrid[:H, :W]
    masks = np.zeros((N, H, W), bool)
    for i, b in enumerate(bboxes):
        cy, cx = (b[0] + b[2]) / 2, (b[1] + b[3]) / 2
        masks[i] = ((yy - cy) / ((b[2] - b[0]) * 0.55)) ** 2 + \
                   ((xx - cx) / ((b[3] - b[1]) * 0.55)) ** 2 <= 1
    labels = rng.randint(1, 81, N).astype(np.int32)
    captions = ['class%d %.1f%%' % (l, s) for l, s in zip(labels, rng.uniform(70, 100, N))]
    return img, bboxes, labels, masks, captions


def kernel_ms(img, bboxes, labels, masks, captions, reps):
    """Device time of the launch alone: the records and masks of draw_instances_device are
    prepared once, then the same launch is timed."""
    dev = torch.device('cuda:0')
    N = len(bboxes)
    boxes = bboxes.astype(int)
    on = [True] * N
    cmap, cmap_inst = V.label_colormap(81), V.label_colormap(N + 1)[1:]
    rec = np.zeros(N, V.INSTANCE_DTYPE)
    rec['box'], rec['draw'] = boxes, 1
    rec['t'] = ((cmap_inst * 255) * np.float32(0.5)).astype(np.float64)
    col = np.round(cmap[labels] * 255).astype(np.uint32)[:, ::-1]
    rec['rgb'] = col[:, 0] | (col[:, 1] << 8) | (col[:, 2] << 16)
    chunks, off = [], 0
    for i, c in enumerate(V.caption_layout(captions, boxes, on)):
        if c is not None:
            rec['cap'][i] = (c[0], c[1]) + c[2].shape
            rec['cap_offset'][i] = off
            chunks.append(c[2].reshape(-1))
            off += c[2].size
    buf = torch.from_numpy(np.concatenate([rec.view(np.uint8)] + chunks)).to(dev)
    packed, _, extent = M.pack_masks(masks, device=dev)
    img_d = torch.from_numpy(img).to(dev)

    def launch():
        _lib.call('mrcnn_draw_instances', _lib.ptr(img_d), H, W, _lib.ptr(packed),
                  _lib.ptr(extent), N, _lib.c_vp(buf.data_ptr()),
                  _lib.c_vp(buf.data_ptr() + rec.nbytes), off, 0.5, 1, _lib.stream_ptr())
    launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def host_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts) * 1e3)


def report_ms(reps):
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    model = cmr.models.MaskRCNNResNet(50, n_fg_class=80, roi_size=14, min_size=480,
                                      max_size=640).to(dev)
    import bench
    bench.stabilise_synthetic_weights(model)
    with torch.no_grad():                 # random weights: sharpen scores to get detections
        model.head.cls_loc_score.W[4 * 81:5 * 81] *= 60.
    rng = np.random.RandomState(1)
    data = []
    for _ in range(9):
        img = rng.randint(0, 256, (3, 480, 640)).astype(np.uint8)
        m = np.zeros((3, 480, 640), bool)
        b = np.zeros((3, 4), np.float32)
        for g in range(3):
            y, x = rng.randint(0, 380), rng.randint(0, 540)
            m[g, y:y + 100, x:x + 100] = True
            b[g] = (y, x, y + 100, x + 100)
        data.append((img, b, rng.randint(0, 80, 3).astype(np.int32), m))
    rep = cmr.extensions.InstanceSegmentationVisReport([[ex] for ex in data], model,
                                                       ['c%d' % i for i in range(80)])
    shape = rep.render().shape
    return host_ms(rep.render, reps), list(shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'visualize.json'))
    args = ap.parse_args()
    rng = np.random.RandomState(0)
    res = {'image': [H, W], 'kernel_ms': {}, 'call_ms': {}, 'numpy_host_ms': {}}
    for N in (10, 100):
        img, bboxes, labels, masks, captions = scene(rng, N)
        for cap in (False, True):
            key = 'N=%d%s' % (N, ' captions' if cap else '')
            c = captions if cap else None
            res['kernel_ms'][key] = kernel_ms(img, bboxes, labels, masks, c, args.reps)
            res['call_ms'][key] = host_ms(lambda: cmr.utils.draw_instance_bboxes(
                img, bboxes, labels, 81, masks=masks, captions=c), max(5, args.reps // 10))
        t0 = time.perf_counter()
        R.draw(img, bboxes, labels, 81, masks, None)
        res['numpy_host_ms']['N=%d' % N] = (time.perf_counter() - t0) * 1e3
    res['host_byte_masks_MB'] = {'N=%d' % N: N * H * W / 1e6 for N in (10, 100)}
    res['report_render_ms'], res['report_mosaic_shape'] = report_ms(5)
    res['device'] = torch.cuda.get_device_name(0)
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
