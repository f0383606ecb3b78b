"""Times of copy-paste on the device: two examples on the 1024 x 1024 canvas
of large-scale jitter, K instances of the source pasted over the Gt instances of the target, for
(Gt, K) in {(1, 1), (8, 8), (64, 32)}; the source has K instances, all of them pasted.

  fused        — device time of one mrcnn_copy_paste call (its two launches)
  composition  — the same result from torch ops on the same device in the same process: a gather
                 and ``any`` for the alpha, ``where`` for the image, a masked product and ``cat`` for
                 the masks, torch reductions for the boxes and areas
                 (inputs prepared once; device events around ``--reps`` back-to-back calls; the
                 outputs are compared, exactly, before anything is timed)
  write_GB_per_s   — bytes of the outputs (image, masks, boxes, areas) over the fused time
  traffic_GB_per_s — the algorithmic traffic over the fused time: every mask read once and written
                 once, (2 Gt + 2 K) MB at this size, and the three images, 3 x 12.6 MB
  intermediate_MB  — the (G, S, S)-sized tensors the composition materialises besides its outputs

Writes profiles/copy_paste.json.  Nothing is gated on these numbers.

    python tools/bench_copy_paste.py [--reps 50] [--out profiles/copy_paste.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chainer_mask_rcnn_amd import _lib  # noqa: E402

from bench_scale_jitter import back_to_back_ms, boxes_by_torch  # noqa: E402

S = 1024
CASES = ((1, 1), (8, 8), (64, 32))


def blobs(rng, G):
    """(G, S, S) uint8: one filled ellipse per instance, 40 to 400 pixels across."""
    yy, xx = np.mgrid[:S, :S]
    out = np.zeros((G, S, S), np.uint8)
    for g in range(G):
        cy, cx = rng.uniform(0, S, 2)
        ry, rx = rng.uniform(20, 200, 2)
        out[g] = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
    return out


def case_ms(dev, rng, Gt, K, reps):
    n = Gt + K
    img_t, img_s = (torch.from_numpy(rng.standard_normal((S, S, 3)).astype(np.float32)).to(dev)
                    for _ in range(2))
    masks_t, masks_s = torch.from_numpy(blobs(rng, Gt)).to(dev), torch.from_numpy(blobs(rng, K)).to(dev)
    idx = torch.arange(K, dtype=torch.int32, device=dev)
    idx64 = idx.long()
    out = torch.empty((S, S, 3), dtype=torch.float32, device=dev)
    masks = torch.empty((n, S, S), dtype=torch.uint8, device=dev)
    meta = torch.empty((5 * n,), dtype=torch.int32, device=dev)
    rows = torch.empty((n * S * 3,), dtype=torch.int32, device=dev)
    result = {}

    def fused():
        _lib.call('mrcnn_copy_paste', _lib.ptr(img_t), _lib.ptr(img_s), _lib.ptr(masks_t), Gt,
                  _lib.ptr(masks_s), K, _lib.ptr(idx), K, S, _lib.ptr(out), _lib.ptr(masks),
                  _lib.ptr(meta), _lib.ptr(meta[4 * n:]), _lib.ptr(rows),
                  _lib.stream_ptr())

    def composition():
        pasted = masks_s[idx64] != 0                                   # (K, S, S) gather, bool
        a = pasted.any(0)
        result['img'] = torch.where(a[:, :, None], img_s, img_t)
        occluded = (masks_t != 0) & ~a                                  # (Gt, S, S)
        result['masks'] = torch.cat([occluded, pasted]).to(torch.uint8)
        result['boxes'], result['areas'] = boxes_by_torch(result['masks'])

    fused(), composition()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), result['img'].view(torch.int32))
    assert torch.equal(masks, result['masks'])
    assert torch.equal(meta[:4 * n].view(n, 4), result['boxes']) and torch.equal(meta[4 * n:], result['areas'])
    fused_ms = back_to_back_ms(fused, reps)
    px = S * S
    written = px * 12 + n * px + n * 20
    traffic = 3 * px * 12 + 2 * n * px
    return {'fused_ms': fused_ms, 'composition_ms': back_to_back_ms(composition, reps),
            'write_GB_per_s': written / (fused_ms * 1e-3) / 1e9,
            'traffic_GB_per_s': traffic / (fused_ms * 1e-3) / 1e9,
            'written_MB': written / 1e6, 'traffic_MB': traffic / 1e6,
            # pasted (K), alpha (1), occluded (Gt), the bool cat (n), the reductions' fg (n)
            'intermediate_MB': (K + 1 + Gt + 2 * n) * px / 1e6,
            'pasted_fraction': float(result['img'].ne(img_t).any(2).float().mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'copy_paste.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_copy_paste.py: no ROCm device')
    rng = np.random.RandomState(0)
    dev = torch.device('cuda:0')
    res = {'crop_size': S, 'reps': args.reps, 'cases': {}}
    for Gt, K in CASES:
        res['cases']['Gt=%d,K=%d' % (Gt, K)] = case_ms(dev, rng, Gt, K, args.reps)
    res['device'] = torch.cuda.get_device_name(0)
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
