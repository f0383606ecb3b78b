"""Times of the ignore-region kernels at the size of a COCO train step: one
800 x 1333 image with 3 crowd masks, and the boxes of one image of the step — the 63 000 anchors of
its 50 x 84 feature map (15 per position) plus 2 000 proposals.

  union_pack   — device time of one mrcnn_mask_union_pack launch (3 masks -> the plane)
  box_coverage — device time of one mrcnn_box_coverage launch over the 65 000 boxes
  composition  — the same (covered, area) pairs from torch ops on the same device in the same
                 process: ``any`` over the masks, a 2-D inclusive ``cumsum`` (the summed-area
                 table, int32), ``round`` / ``clamp`` of the boxes and four gathers
                 (inputs prepared once; device events around ``--reps`` back-to-back calls; the
                 outputs are compared, exactly, before anything is timed)
  step_added   — what a crowd image adds to a train step: host clock around
                 ``box_coverage(...).cpu()`` of cat(anchors, proposals) — the launch and the
                 read-back the step waits for — median and minimum over ``--reps`` calls, beside
                 ``--step-ms``, the step time ``bench.py --gpus 1`` printed for the same tree
                 (``ms_per_step``; not measured here)
  plane_KB / read_GB_per_s — the plane's size, and the plane bytes the boxes' rectangles span
                 (whole words, computed from the boxes) over the box_coverage time

Writes profiles/ignore_regions.json.  Nothing is gated on these numbers.

    python tools/bench_ignore_regions.py [--reps 200] [--step-ms MS] [--out profiles/ignore_regions.json]
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
from chainer_mask_rcnn_amd import functions as F  # noqa: E402
from chainer_mask_rcnn_amd.utils.bbox import enumerate_shifted_anchor, generate_anchor_base  # noqa: E402

from bench_scale_jitter import back_to_back_ms  # noqa: E402

H, W = 800, 1333
N_CROWD, N_PROPOSALS = 3, 2000


def crowd_masks(rng):
    """(3, H, W) uint8: filled ellipses 200 to 700 pixels across, as crowd regions are."""
    yy, xx = np.mgrid[:H, :W]
    out = np.zeros((N_CROWD, H, W), np.uint8)
    for g in range(N_CROWD):
        cy, cx = rng.uniform(0, H), rng.uniform(0, W)
        ry, rx = rng.uniform(100, 350, 2)
        out[g] = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
    return out


def step_boxes(rng):
    """(63 000 + 2 000, 4) float32: the anchors of the 50 x 84 map and proposals clipped to the image."""
    anchor = enumerate_shifted_anchor(generate_anchor_base(anchor_scales=[2, 4, 8, 16, 32]), 16, 50, 84)
    y, x = rng.uniform(0, H, N_PROPOSALS), rng.uniform(0, W, N_PROPOSALS)
    h, w = rng.uniform(8, 500, N_PROPOSALS), rng.uniform(8, 500, N_PROPOSALS)
    prop = np.stack([y, x, np.minimum(y + h, H), np.minimum(x + w, W)], 1)
    return np.concatenate([anchor, prop]).astype(np.float32)


def spanned_bytes(boxes):
    """Bytes of the plane's words inside the rounded, clipped boxes."""
    b = np.round(boxes.astype(np.float64))
    y0, y1 = np.clip(b[:, 0], 0, H), np.clip(b[:, 2], 0, H)
    x0, x1 = np.clip(b[:, 1], 0, W), np.clip(b[:, 3], 0, W)
    ok = (y1 > y0) & (x1 > x0)
    words = np.where(ok, (np.floor((x1 - 1) / 64) - np.floor(x0 / 64) + 1) * (y1 - y0), 0)
    return float(words.sum() * 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--step-ms', type=float, default=None,
                    help="ms_per_step of `bench.py --gpus 1` on the same tree, recorded beside step_added")
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ignore_regions.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_ignore_regions.py: no ROCm device')
    rng = np.random.RandomState(0)
    dev = torch.device('cuda:0')
    masks = torch.from_numpy(crowd_masks(rng)).to(dev)
    boxes_h = step_boxes(rng)
    boxes = torch.from_numpy(boxes_h).to(dev)
    n = boxes.shape[0]
    Wq = (W + 63) // 64
    plane = torch.empty((H, Wq), dtype=torch.int64, device=dev)
    out = torch.empty((n, 2), dtype=torch.int32, device=dev)
    result = {}

    def union_pack():
        _lib.call('mrcnn_mask_union_pack', _lib.ptr(masks), N_CROWD, H, W, None, _lib.ptr(plane),
                  _lib.stream_ptr())

    def box_coverage():
        _lib.call('mrcnn_box_coverage', _lib.ptr(plane), H, W, _lib.ptr(boxes), n, _lib.ptr(out),
                  _lib.stream_ptr())

    lim = torch.tensor([H, W, H, W], dtype=torch.float32, device=dev)

    def composition():
        u = (masks != 0).any(0)
        sat = torch.zeros((H + 1, W + 1), dtype=torch.int32, device=dev)
        sat[1:, 1:] = u.to(torch.int32).cumsum(0, dtype=torch.int32).cumsum(1, dtype=torch.int32)
        finite = torch.isfinite(boxes).all(1)
        b = torch.minimum(torch.round(torch.nan_to_num(boxes)).clamp_min(0), lim).long()    # round: half to even
        y0, x0, y1, x1 = b.unbind(1)
        y1, x1 = torch.maximum(y1, y0), torch.maximum(x1, x0)
        covered = sat[y1, x1] - sat[y0, x1] - sat[y1, x0] + sat[y0, x0]
        area = ((y1 - y0) * (x1 - x0)).to(torch.int32)
        result['out'] = torch.stack([covered, area], 1) * finite[:, None].to(torch.int32)

    union_pack(), box_coverage(), composition()
    torch.cuda.synchronize()
    assert torch.equal(out, result['out'])
    covered_fraction = float((plane.cpu().numpy().view(np.uint8)[:, :, None] >> np.arange(8) & 1).sum()) / (H * W)

    def step_added():
        return F.ignored_from_counts(F.box_coverage(plane, W, boxes).cpu().numpy(), 0.7)

    for _ in range(5):
        step_added()
    torch.cuda.synchronize()
    host = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        ign = step_added()
        host.append((time.perf_counter() - t0) * 1e3)
    coverage_ms = back_to_back_ms(box_coverage, args.reps)
    res = {
        'image': [H, W], 'crowd_masks': N_CROWD, 'boxes': int(n), 'reps': args.reps,
        'union_pack_ms': back_to_back_ms(union_pack, args.reps),
        'box_coverage_ms': coverage_ms,
        'composition_ms': back_to_back_ms(composition, args.reps),
        'step_added_ms_median': float(np.median(host)), 'step_added_ms_min': float(np.min(host)),
        'bench_step_ms': args.step_ms,
        'step_added_percent_of_step': None if not args.step_ms else 100. * float(np.median(host)) / args.step_ms,
        'plane_KB': H * Wq * 8 / 1e3, 'read_GB_per_s': spanned_bytes(boxes_h) / (coverage_ms * 1e-3) / 1e9,
        'spanned_MB': spanned_bytes(boxes_h) / 1e6, 'plane_covered_fraction': covered_fraction,
        'ignored_boxes': int(ign.sum()), 'device': torch.cuda.get_device_name(0),
    }
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
