"""Per-image time of the instance-segmentation evaluation's mask work, three paths:

  device  — packed paste of the predicted masks + pack of the ground truth + intersections,
            one read-back of the counts (the evaluators' path)
  host    — predict's current route: full-image uint8 masks pasted on the device, copied to
            the host, then utils.mask_iou on those host masks (upload + pack + intersect)
  numpy   — the NumPy restatement on host masks (tests/instseg_eval_ref.py's definition:
            boolean AND / OR per pair), P x G pairs

at two shapes: COCO-like (100 detections, 7 ground-truth masks, 480x640) and heavy (100 x 100
at 800x1333).  Informational: writes profiles/instseg_eval.json.

    python tools/bench_instseg_eval.py [--reps 20] [--out profiles/instseg_eval.json]
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

from chainer_mask_rcnn_amd import _lib  # noqa: E402
from chainer_mask_rcnn_amd.functions._layout import nhwc  # noqa: E402
from chainer_mask_rcnn_amd.utils.evaluations import masks as M  # noqa: E402
from chainer_mask_rcnn_amd.utils.evaluations.records import Readback  # noqa: E402


def make(rng, D, G, H, W, dev):
    y0, x0 = rng.uniform(0, H - 30, D), rng.uniform(0, W - 30, D)
    bbox = np.stack([y0, x0, np.minimum(y0 + rng.uniform(20, 300, D), H),
                     np.minimum(x0 + rng.uniform(20, 300, D), W)], 1).astype(np.float32)
    label = rng.randint(0, 80, D).astype(np.int32)
    logits = torch.tensor((rng.standard_normal((D, 80, 14, 14)) * 3).astype(np.float32), device=dev)
    gt = np.zeros((G, H, W), np.int32)
    for g in range(G):
        a, b = rng.randint(0, H - 50), rng.randint(0, W - 50)
        gt[g, a:a + rng.randint(20, 300), b:b + rng.randint(20, 300)] = 1
    return bbox, label, logits, gt


def device_path(bbox, label, logits, gt, H, W):
    pred = M.paste_packed(logits, label, bbox, (H, W))
    g = M.pack_masks(gt, device=logits.device)
    readback = Readback()
    M.queue_counts(readback, pred, g, (H, W))
    return readback.fetch()


def host_masks(bbox, label, logits, H, W):
    D = len(bbox)
    lg = nhwc(logits)
    out = torch.empty((D, H, W), dtype=torch.uint8, device=logits.device)
    label_d = torch.tensor(label, device=logits.device)
    bbox_d = torch.tensor(bbox, device=logits.device)
    _lib.call('mrcnn_paste_masks', _lib.ptr(lg), _lib.ptr(label_d), _lib.ptr(bbox_d), D,
              lg.shape[2], lg.shape[1], H, W, _lib.ptr(out), _lib.stream_ptr())
    return out.cpu().numpy().astype(bool)


def host_path(bbox, label, logits, gt, H, W):
    return M.mask_iou(host_masks(bbox, label, logits, H, W), gt)


def numpy_path(pm, gt):
    gt = gt.astype(bool)
    iou = np.zeros((len(pm), len(gt)))
    for i, a in enumerate(pm):
        for j, b in enumerate(gt):
            u = np.logical_or(a, b).sum()
            iou[i, j] = 0. if u == 0 else 1.0 * np.logical_and(a, b).sum() / u
    return iou


def timed(fn, reps, warmup=True):
    if warmup:
        fn()
        torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--numpy-reps', type=int, default=1)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'instseg_eval.json'))
    args = ap.parse_args()
    _lib.load()
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(0)
    result = {'unit': 'seconds per image (median, min over reps)', 'shapes': {}}
    for name, (D, G, H, W) in [('coco_like', (100, 7, 480, 640)), ('heavy', (100, 100, 800, 1333))]:
        bbox, label, logits, gt = make(rng, D, G, H, W, dev)
        pm = host_masks(bbox, label, logits, H, W)
        r = {'detections': D, 'gt': G, 'H': H, 'W': W}
        r['device'] = timed(lambda: device_path(bbox, label, logits, gt, H, W), args.reps)
        r['host_masks'] = timed(lambda: host_path(bbox, label, logits, gt, H, W), args.reps)
        r['numpy'] = timed(lambda: numpy_path(pm, gt), args.numpy_reps, warmup=False)
        # the three paths agree on the IoU
        iou = M.iou_from_counts(*device_path(bbox, label, logits, gt, H, W))
        assert np.array_equal(iou, host_path(bbox, label, logits, gt, H, W))
        if G <= 10:
            assert np.array_equal(iou, numpy_path(pm, gt))
        result['shapes'][name] = r
        print(name, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
