"""Timings of COCO results export: the device RLE codec against the host path.

    python tools/bench_coco_results.py [--reps 20]

For 100 ``paste_packed`` detections (random mask logits and boxes) at 480x640 and 800x1333:

* ``encode_ms``: device encode of the packed masks, strings read back to the host
  (``rle.queue_encode`` + ``rle.fetch_encoded``; what the COCO evaluator's results sink adds);
* ``decode_ms``: device decode of those strings into packed masks, status read back;
* ``host_ms``: the host path of the reference's ``_create_ann`` restated with NumPy: the byte
  paste (``MaskRCNN._to_masks``, which copies the masks to the host) and a vectorised NumPy
  encode (transpose, diff, rleToString on whole arrays).

Medians over ``--reps`` runs after a warm-up (host path: ``--host-reps`` runs).  Prints one JSON
line per shape; the strings of both paths are checked equal first.
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


def np_encode(mask):
    """(H, W) mask -> compressed COCO RLE string, vectorised."""
    flat = mask.T.reshape(-1).astype(np.int8)
    change = np.flatnonzero(np.diff(flat, prepend=np.int8(0)))
    c = np.diff(np.concatenate([[0], change, [flat.size]])).astype(np.int64)
    v = c.copy()
    v[3:] = c[3:] - c[1:-2]
    chars = np.zeros((len(v), 7), np.uint8)
    n = np.zeros(len(v), np.int64)
    active = np.ones(len(v), bool)
    for k in range(7):
        d = v & 0x1f
        v = v >> 5
        more = np.where(d & 0x10, v != -1, v != 0)
        chars[:, k] = (d | np.where(more, 0x20, 0)) + 48
        n += active
        active &= more
    return chars[np.arange(7)[None, :] < n[:, None]].tobytes().decode('ascii')


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--detections', type=int, default=100)
    args = ap.parse_args()
    from chainer_mask_rcnn_amd.models.mask_rcnn import MaskRCNN
    from chainer_mask_rcnn_amd.utils.evaluations import masks as M
    from chainer_mask_rcnn_amd.utils.evaluations import rle as R
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(0)
    D = args.detections
    for H, W in ((480, 640), (800, 1333)):
        bbox = np.zeros((D, 4), np.float32)
        bbox[:, :2] = rng.uniform(0, [H * 0.8, W * 0.8], (D, 2))
        bbox[:, 2:] = bbox[:, :2] + rng.uniform(16, [H / 2, W / 2], (D, 2))
        label = rng.randint(0, 80, D).astype(np.int32)
        logits = torch.tensor(rng.standard_normal((D, 80, 14, 14)).astype(np.float32),
                              device=dev)
        pk = M.paste_packed(logits, label, bbox, (H, W))

        def encode():
            return R.fetch_encoded([R.queue_encode(pk[0], pk[1], pk[2], (H, W))])[0]

        def host():
            byte = MaskRCNN._to_masks(None, [bbox], [label], None, [logits], [(H, W)])[0]
            return [np_encode(m) for m in byte]

        rles = encode()
        assert [r['counts'] for r in rles] == host(), 'device and host strings differ'
        encode()                                         # warm-up (buffer estimate settled)
        R.decode_masks(rles, packed=True)
        enc = median_ms(encode, args.reps)
        dec = median_ms(lambda: R.decode_masks(rles, packed=True), args.reps)
        hst = median_ms(host, args.host_reps)
        n_chars = sum(len(r['counts']) for r in rles)
        print(json.dumps({'shape': [H, W], 'detections': D, 'encode_ms': round(enc, 3),
                          'decode_ms': round(dec, 3), 'host_ms': round(hst, 1),
                          'host_over_device_encode': round(hst / enc, 1),
                          'string_bytes': n_chars}), flush=True)


if __name__ == '__main__':
    main()
