"""Kernel times of the three RoI feature extractors of the head (roi_align_2d, roi_pooling_2d,
crop_and_resize) at the headline head's shape: a (2, 1024, 50, 84) feature map, 1024
proposal-shaped RoIs, 14 x 14 bins with bin_stride 2 (the bins res5.a reads).

Forward and backward are timed separately with device events around `--iters` back-to-back calls
after `--warmup` calls; the backward is torch.autograd.grad through the op's saved graph (the
workspace-table kernel and the pixel-owner kernel).  Algorithmic GB/s counts the bytes the op must
move: forward = the feature map once + the pooled output (+ the int32 argmax for max pooling);
backward = the pooled gradient (+ the argmax) + the feature-map gradient.  Prints one JSON line.

    python tools/bench_roi_pool_variants.py [--iters 50] [--warmup 10] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from chainer_mask_rcnn_amd import functions as F  # noqa: E402

N, C, H, W = 2, 1024, 50, 84
R, SIZE, STRIDE, SCALE = 1024, 14, 2, 1 / 16.


def proposal_rois(rng):
    """(batch, x1, y1, x2, y2) boxes shaped like sampled proposals on an 800 x 1333 image, grouped
    by image."""
    Hi, Wi = H * 16, W * 16
    s = np.exp(rng.uniform(np.log(24), np.log(600), R))
    ar = np.exp(rng.uniform(np.log(0.5), np.log(2), R))
    h, w = s * np.sqrt(ar), s / np.sqrt(ar)
    cy, cx = rng.uniform(0, Hi, R), rng.uniform(0, Wi, R)
    y1, x1 = np.clip(cy - h / 2, 0, Hi - 1), np.clip(cx - w / 2, 0, Wi - 1)
    y2, x2 = np.clip(cy + h / 2, 0, Hi - 1), np.clip(cx + w / 2, 0, Wi - 1)
    b = np.repeat(np.arange(N), R // N)
    return np.stack([b, x1, y1, x2, y2], 1).astype(np.float32)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters      # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(0)
    x = torch.tensor(rng.standard_normal((N, C, H, W)).astype(np.float32), device=dev)
    x = x.contiguous(memory_format=torch.channels_last).requires_grad_(True)
    rois = torch.tensor(proposal_rois(rng), device=dev)
    o = (SIZE + STRIDE - 1) // STRIDE
    pooled, fmap = 4.0 * R * o * o * C, 4.0 * N * H * W * C
    ops = [('roi_align_2d', lambda a: F.roi_align_2d(a, rois, SIZE, SIZE, SCALE, bin_stride=STRIDE), 0.),
           ('roi_pooling_2d', lambda a: F.roi_pooling_2d(a, rois, SIZE, SIZE, SCALE, bin_stride=STRIDE), pooled),
           ('crop_and_resize', lambda a: F.crop_and_resize(a, rois, SIZE, SIZE, SCALE, bin_stride=STRIDE), 0.)]
    out = dict(shape=dict(x=[N, C, H, W], rois=R, outh=SIZE, outw=SIZE, bin_stride=STRIDE,
                          spatial_scale=SCALE), iters=args.iters, warmup=args.warmup,
               device=torch.cuda.get_device_name(0), ops={})
    for name, f, extra in ops:
        with torch.no_grad():
            fwd_us = timed(lambda: f(x), args.iters, args.warmup)
        y = f(x)
        gy = torch.randn_like(y)
        bwd_us = timed(lambda: torch.autograd.grad(y, x, gy, retain_graph=True), args.iters, args.warmup)
        fb, bb = fmap + pooled + extra, pooled + extra + fmap
        out['ops'][name] = dict(fwd_us=round(fwd_us, 2), fwd_GBps=round(fb / fwd_us * 1e-3, 1),
                                bwd_us=round(bwd_us, 2), bwd_GBps=round(bb / bwd_us * 1e-3, 1))
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
