"""Times of the detection post-processing with Soft-NMS and box voting: one
image's worth of candidates, R = 1000 RoIs and 80 foreground classes, boxes clustered around a few
objects per class so that a class holds tens to hundreds of overlapping rows above the score
threshold.  Every variant is measured as MaskRCNN._suppress_queue runs it, sort -> suppress
(-> vote) -> compact, device events around ``--reps`` back-to-back calls:

  hard            — mrcnn_nms_sorted_batched at 0.5, the default path
  linear/gaussian — mrcnn_soft_nms_sorted_batched in its place
  +vote           — mrcnn_box_vote at 0.8 behind each

  composition_ms  — the same result from torch ops on the same device in the same process: a masked
                    batched sort, one arg-max / IoU / decay step per pick over all classes at once
                    (as many steps as the longest class needs, found beforehand so that the loop
                    never waits for the host), a float64 masked matrix product for the vote and
                    boolean indexing for the packing; compared with the kernels' result before
                    anything is timed (labels and order exactly; boxes and scores exactly where
                    the arithmetic is the same; gaussian scores to 1e-4 relative, since torch's
                    double exp is another library's, voted boxes to 1e-4 pixels, since the
                    matrix product sums in another order)
  picks           — the longest chain of picks in a class / the picks of all classes
  sort_and_compact_ms — the same call with a Soft-NMS launch that stops at its first pick: the
                    sort in full, a compact that packs nothing
  chain_us_per_pick — Soft-NMS variants: (variant - sort_and_compact_ms) / longest chain, an
                    upper estimate of what one link of the serial chain costs (it also holds
                    the launch and the packing of the kept rows)

Writes profiles/soft_nms.json.  Nothing is gated on these numbers.

    python tools/bench_soft_nms.py [--reps 50] [--out profiles/soft_nms.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import chainer_mask_rcnn_amd as cmr  # noqa: E402
from chainer_mask_rcnn_amd import _lib  # noqa: E402

from bench_scale_jitter import back_to_back_ms  # noqa: E402

R, N_CLASS = 1000, 81
VARIANTS = (('hard', None, None), ('hard+vote', None, 0.8), ('linear', 'linear', None),
            ('linear+vote', 'linear', 0.8), ('gaussian', 'gaussian', None),
            ('gaussian+vote', 'gaussian', 0.8))


def candidates(rng):
    """prob (R, 81), cls_bbox (R, 81, 4): per class 20..300 rows above the score threshold,
    scattered around 2..6 objects of 60..300 pixels on an 800 x 1333 image."""
    prob = rng.uniform(0, 0.01, (R, N_CLASS)).astype(np.float32)
    y0 = rng.uniform(0, 700, (R, N_CLASS))
    x0 = rng.uniform(0, 1200, (R, N_CLASS))
    cls_bbox = np.stack([y0, x0, y0 + rng.uniform(10, 100, y0.shape),
                         x0 + rng.uniform(10, 100, y0.shape)], axis=2)
    for l in range(1, N_CLASS):
        m = int(rng.randint(20, 301))
        rows = rng.permutation(R)[:m]
        prob[rows, l] = rng.uniform(0.06, 0.95, m)
        objects = np.concatenate([rng.uniform(0, 500, (6, 1)), rng.uniform(0, 1000, (6, 1)),
                                  rng.uniform(60, 300, (6, 2))], axis=1)[:int(rng.randint(2, 7))]
        o = objects[rng.randint(0, len(objects), m)]
        jitter = rng.normal(0, 0.08, (m, 4)) * o[:, [2, 3, 2, 3]]
        cls_bbox[rows, l] = np.stack([o[:, 0], o[:, 1], o[:, 0] + o[:, 2], o[:, 1] + o[:, 3]], 1) + jitter
    return prob, cls_bbox.astype(np.float32)


def bare_model(soft_nms, vote):
    model = cmr.models.MaskRCNN(None, None, None, mean=None)
    model.head = type('H', (), {'n_class': N_CLASS, 'mask_size': 14})()
    model.soft_nms, model.bbox_vote_thresh = soft_nms, vote
    return model


def iou_rows(box, boxes):
    """bbox_iou.h's expression: box (G, 1, 4) against boxes (G, n, 4), fp32, one op per step."""
    tl = torch.maximum(box[..., :2], boxes[..., :2])
    br = torch.minimum(box[..., 2:], boxes[..., 2:])
    side = br - tl
    inter = side[..., 0] * side[..., 1] * (tl < br).all(-1)
    area = lambda b: (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    return inter / (area(box) + area(boxes) - inter)


class Composition(object):
    """sort -> suppress (-> vote) -> compact from torch ops, all classes batched."""

    def __init__(self, model, steps, width):
        self.m, self.steps, self.width = model, steps, width     # longest chain, fullest class

    def __call__(self, cls_bbox, prob):
        m = self.m
        p = prob[:, 1:].t().contiguous()                                   # (G, R)
        valid = p > m.score_thresh
        p_sorted, order = torch.sort(torch.where(valid, p, p.new_tensor(-1.)), dim=1,
                                     descending=True, stable=True)
        boxes = cls_bbox[:, 1:].permute(1, 0, 2)                           # (G, R, 4)
        p_sorted, order = p_sorted[:, :self.width], order[:, :self.width]
        boxes = torch.gather(boxes, 1, order[:, :, None].expand(-1, -1, 4))
        alive = p_sorted > m.score_thresh
        s = torch.where(alive, p_sorted, p_sorted.new_tensor(0.))
        G = s.shape[0]
        rank = torch.full_like(order, -1)
        out_score = torch.zeros_like(s)
        method = m.soft_nms or 'hard'
        nt = m.soft_nms_thresh if m.soft_nms else m.nms_thresh
        rows = torch.arange(G, device=s.device)
        done = torch.zeros((G,), dtype=torch.bool, device=s.device)
        for t in range(self.steps):
            live = torch.where(alive, s, s.new_tensor(-1.))
            best, i = live.max(dim=1)                                      # first maximum
            done = done | ~(best >= m.soft_nms_min_score)
            pick = ~done
            rank[rows, i] = torch.where(pick, torch.full_like(i, t), rank[rows, i])
            out_score[rows, i] = torch.where(pick, best, out_score[rows, i])
            alive[rows, i] = alive[rows, i] & done
            iou = iou_rows(boxes[rows, i][:, None], boxes)
            if method == 'hard':
                w = torch.where(iou >= nt, 0., 1.)
            elif method == 'linear':
                w = torch.where(iou >= nt, 1. - iou, 1.)
            else:
                i64 = iou.double()
                w = torch.where(iou > 0, torch.exp(-(i64 * i64) / float(np.float32(m.soft_nms_sigma))).float(), 1.)
            s = torch.where(alive & pick[:, None], s * w.to(s.dtype), s)
        kept = rank >= 0
        if m.bbox_vote_thresh is not None:
            # (G, R, R) overlaps of every row with every candidate of its class, float64 product
            cand = (p_sorted > m.score_thresh)
            hit = (iou_rows(boxes[:, :, None], boxes[:, None]) >= m.bbox_vote_thresh) & cand[:, None]
            wgt = hit.double() * p_sorted.double()[:, None]
            wsum = wgt.sum(2, keepdim=True)
            voted = (torch.bmm(wgt, boxes.double()) / wsum).float()
            boxes = torch.where(wsum != 0, voted, boxes)
        # pack: class after class, in pick order inside a class
        key = torch.where(kept, rank, torch.full_like(rank, s.shape[1]))
        by_pick = torch.argsort(key, dim=1, stable=True)
        sel = torch.gather(kept, 1, by_pick)
        label = rows[:, None].expand_as(sel)[sel].int()
        bbox = torch.gather(boxes, 1, by_pick[:, :, None].expand(-1, -1, 4))[sel]
        score = torch.gather(out_score, 1, by_pick)[sel]
        return bbox, label, score


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'soft_nms.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_soft_nms.py: no ROCm device')
    dev = torch.device('cuda:0')
    _lib.load()
    prob_h, cls_bbox_h = candidates(np.random.RandomState(0))
    prob, cls_bbox = torch.from_numpy(prob_h).to(dev), torch.from_numpy(cls_bbox_h).to(dev)
    per_class = (prob_h[:, 1:] > 0.05).sum(0)
    res = {'R': R, 'n_fg_class': N_CLASS - 1, 'reps': args.reps,
           'rows_per_class': {'min': int(per_class.min()), 'median': int(np.median(per_class)),
                              'max': int(per_class.max()), 'total': int(per_class.sum())},
           'variants': {}}

    # the launches around the suppression: min_score above every score makes the Soft-NMS launch
    # stop at its first pick, so the sort runs in full but compact packs NO row; the figure
    # understates the packing of a real result, and chain_us_per_pick, which subtracts it,
    # therefore holds that packing too
    alone = bare_model('linear', None)
    alone.soft_nms_min_score = 2.0
    res['sort_and_compact_ms'] = back_to_back_ms(lambda: alone._suppress_queue(cls_bbox, prob),
                                                 args.reps)

    for name, soft_nms, vote in VARIANTS:
        model = bare_model(soft_nms, vote)
        bbox, label, score, total = model._suppress_queue(cls_bbox, prob)
        d = int(total.item())
        bbox, label, score = bbox[:d], label[:d], score[:d]
        picks = np.bincount(label.cpu().numpy(), minlength=N_CLASS - 1)
        composition = Composition(model, int(picks.max()) + 1, int(per_class.max()))
        c_bbox, c_label, c_score = composition(cls_bbox, prob)
        torch.cuda.synchronize()
        assert torch.equal(c_label, label), name
        if soft_nms == 'gaussian':
            assert torch.allclose(c_score, score, rtol=1e-4, atol=0), name
        else:
            assert torch.equal(c_score, score), name
        if vote is None:
            assert torch.equal(c_bbox, bbox), name
        else:
            assert torch.allclose(c_bbox, bbox, rtol=1e-6, atol=1e-4), name
        ms = back_to_back_ms(lambda: model._suppress_queue(cls_bbox, prob), args.reps)
        res['variants'][name] = {
            'ms': ms, 'composition_ms': back_to_back_ms(lambda: composition(cls_bbox, prob),
                                                        max(args.reps // 10, 3)),
            'detections': d, 'longest_chain': int(picks.max()), 'picks': int(picks.sum()),
            'chain_us_per_pick': ((ms - res['sort_and_compact_ms']) * 1e3 / max(int(picks.max()), 1)
                                  if soft_nms else None)}
    res['device'] = torch.cuda.get_device_name(0)
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
