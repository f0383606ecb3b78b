"""Times of the mask-boundary kernel behind Boundary AP.

  kernel_ms — mrcnn_mask_boundary (both launches) on 100 packed masks, at 800 x 1333 (d = 31) and
              at 1024 x 1024 (d = 29): discs, ellipses and rectangles of 20..300 pixels, as many
              cut by the image border as fall there
  torch_ms  — the same boundaries from torch ops on the same device in the same process: the
              float masks zero-padded by d, ``-max_pool2d(-m, 2d+1, 1)`` for the erosion,
              ``m * (1 - e)``; compared with the kernel's result (unpacked) before anything is timed
  pack_ms / unpack_ms — what turning dense uint8 masks into the packed format and back costs, for
              a reader who holds dense masks (the evaluators hold packed ones already)
  collect   — ``InstanceSegmentationCOCOEvaluator.collect()`` on one batch of two 800 x 1333 images
              (100 detections and 7 ground-truth masks each) behind a target that returns
              prepared detections, with iou_types ('segm',) and ('segm', 'boundary'): what the
              boundary adds to a batch's mask work, read-back included

Every figure is the median (and the minimum) of ``--reps`` timed calls after warm-up, the two
sides of a comparison alternating; kernel and torch calls are timed with device events, collect()
with the host clock around a call that ends in its read-back.  Writes profiles/boundary.json.
Nothing is gated on these numbers.

    python tools/bench_boundary.py [--reps 25] [--out profiles/boundary.json]
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

import chainer_mask_rcnn_amd as cmr  # noqa: E402
from chainer_mask_rcnn_amd import _lib  # noqa: E402
from chainer_mask_rcnn_amd.utils.evaluations import masks as M  # noqa: E402

N_MASKS = 100


def make_masks(rng, N, H, W):
    yy, xx = np.mgrid[:H, :W]
    out = np.zeros((N, H, W), np.uint8)
    for n in range(N):
        cy, cx = rng.randint(0, H), rng.randint(0, W)
        ry, rx = rng.randint(10, 151), rng.randint(10, 151)
        if n % 3 == 2:
            out[n] = (abs(yy - cy) <= ry) & (abs(xx - cx) <= rx)
        else:
            out[n] = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.
    return out


def torch_boundary(m, d):
    """m (N, 1, H, W) float {0, 1} -> its boundaries, by the rule: the erosion is the minimum over
    the (2d+1)^2 window of the mask zero-padded by d."""
    p = torch.nn.functional.pad(m, (d, d, d, d))
    e = -torch.nn.functional.max_pool2d(-p, 2 * d + 1, 1)
    return m * (1. - e)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(fns, reps, clock, warmup=3):
    """{name: (median, min)} of ``reps`` timed calls of each function, taken in turn."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(clock(fn))
    return {k: (float(np.median(v)), float(np.min(v))) for k, v in ts.items()}


class PreparedTarget(object):
    """predict_images of a model that has its detections ready: the evaluator's mask work alone."""

    def __init__(self, rng, D, H, W, dev):
        y0, x0 = rng.uniform(0, H - 30, D), rng.uniform(0, W - 30, D)
        self.bbox = np.stack([y0, x0, np.minimum(y0 + rng.uniform(20, 300, D), H),
                              np.minimum(x0 + rng.uniform(20, 300, D), W)], 1).astype(np.float32)
        self.label = rng.randint(0, 80, D).astype(np.int32)
        self.score = rng.uniform(0.05, 1, D).astype(np.float32)
        self.logits = torch.tensor((rng.standard_normal((D, 80, 14, 14)) * 3).astype(np.float32),
                                   device=dev)
        self.size = (H, W)

    def predict_images(self, imgs, masks_to_host=False):
        n = len(imgs)
        return ([self.bbox] * n, [self.logits] * n, [self.label] * n, [self.score] * n,
                [self.size] * n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=25)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'boundary.json'))
    args = ap.parse_args()
    if args.reps < 20:
        ap.error('--reps: at least 20 timed calls')
    if not torch.cuda.is_available():
        raise SystemExit('bench_boundary.py: no ROCm device')
    dev = torch.device('cuda:0')
    _lib.load()
    rng = np.random.RandomState(0)
    res = {'unit': 'ms (median, min)', 'reps': args.reps, 'masks': N_MASKS, 'shapes': {}}
    for H, W in ((800, 1333), (1024, 1024)):
        d = M.boundary_dilation((H, W))
        dense = torch.from_numpy(make_masks(rng, N_MASKS, H, W)).to(dev)
        packed = M.pack_masks(dense)
        as_float = dense[:, None].float()
        # the two routes give the same boundaries
        b = M.boundary_packed(packed, (H, W), dilation=d)
        unpacked = torch.empty_like(dense)
        _lib.call('mrcnn_mask_unpack', _lib.ptr(b[0]), N_MASKS, H, W, _lib.ptr(unpacked),
                  _lib.stream_ptr())
        ref = torch_boundary(as_float, d)
        assert torch.equal(unpacked, ref[:, 0].to(torch.uint8)), (H, W)
        assert torch.equal(b[1].long(), ref.sum((1, 2, 3)).long()), (H, W)
        del ref
        r = {'d': d, 'mean_mask_area': float(packed[1].float().mean()),
             'mean_boundary_area': float(b[1].float().mean())}
        t = alternate({'kernel_ms': lambda: M.boundary_packed(packed, (H, W), dilation=d),
                       'torch_ms': lambda: torch_boundary(as_float, d)}, args.reps, event_ms)
        r.update(t)
        r['torch_over_kernel'] = t['torch_ms'][0] / t['kernel_ms'][0]

        def unpack():
            _lib.call('mrcnn_mask_unpack', _lib.ptr(b[0]), N_MASKS, H, W, _lib.ptr(unpacked),
                      _lib.stream_ptr())
        r.update(alternate({'pack_ms': lambda: M.pack_masks(dense), 'unpack_ms': unpack},
                           args.reps, event_ms))
        res['shapes']['%dx%d' % (H, W)] = r
        print('%dx%d' % (H, W), json.dumps(r), flush=True)
        del dense, packed, as_float, b, unpacked
        torch.cuda.empty_cache()

    H, W, D, G = 800, 1333, 100, 7
    target = PreparedTarget(rng, D, H, W, dev)
    batch = []
    for _ in range(2):
        gt = make_masks(rng, G, H, W).astype(np.int32)
        batch.append((np.zeros((3, H, W), np.float32), np.zeros((G, 4), np.float32),
                      rng.randint(0, 80, G).astype(np.int32), gt))
    plain = cmr.extensions.InstanceSegmentationCOCOEvaluator([batch], target)
    both = cmr.extensions.InstanceSegmentationCOCOEvaluator([batch], target,
                                                            iou_types=('segm', 'boundary'))
    assert set(plain.collect().tables) == {'segm'}
    assert set(both.collect().tables) == {'segm', 'boundary'}
    t = alternate({'segm_ms': plain.collect, 'segm_boundary_ms': both.collect}, args.reps, host_ms)
    res['collect'] = dict(t, images=2, detections=D, gt=G, H=H, W=W,
                          boundary_adds_ms_per_image=(t['segm_boundary_ms'][0] - t['segm_ms'][0]) / 2)
    print('collect', json.dumps(res['collect']), flush=True)
    res['device'] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
