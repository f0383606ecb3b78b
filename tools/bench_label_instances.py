"""Times of the device label conversion (utils.label2instance_boxes, return_masks=True):

  kernels    — device label images in, device outputs (two synchronisations per call)
  round_trip — host int32 arrays in, host NumPy out (upload, kernels, read-back of the masks)

at 375x500 with 3 and 8 instances, 800x1333 with 15 and 1080x1920 with 30, next to the host
times of the reference's own function measured on a build host (CPU, mean of 5 calls).  Also
times the train loop's per-batch fetch (two SBD examples through MaskRCNNTransform with the
VOC model settings) on a synthetic SBD tree.  Writes profiles/label_instances.json.

    python tools/bench_label_instances.py [--reps 20] [--out profiles/label_instances.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import chainer_mask_rcnn_amd as cmr  # noqa: E402

# the reference's label2instance_boxes(..., return_masks=True) on the build host's CPU, ms
HOST_REFERENCE_MS = {'375x500_3': 3.4, '375x500_8': 8.1, '800x1333_15': 60., '1080x1920_30': 211.}
SHAPES = [(375, 500, 3), (375, 500, 8), (800, 1333, 15), (1080, 1920, 30)]


def label_pair(rng, H, W, n):
    ins = -np.ones((H, W), np.int32)
    cls = np.zeros((H, W), np.int32)
    for k in range(n):
        y0, x0 = rng.randint(0, H - H // 8), rng.randint(0, W - W // 8)
        y1, x1 = y0 + rng.randint(H // 10, H // 3), x0 + rng.randint(W // 10, W // 3)
        ins[y0:y1, x0:x1] = k
        cls[y0:y1, x0:x1] = rng.randint(1, 21)
    noise = (ins >= 0) & (rng.uniform(size=(H, W)) < 0.05)
    cls[noise] = rng.randint(1, 21, noise.sum())
    return ins, cls


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts) * 1e3), float(np.mean(ts) * 1e3)


def sbd_tree(root, rng, n=4, H=375, W=500):
    import PIL.Image
    import scipy.io
    for d in ('img', 'cls', 'inst'):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    ids = ['%04d' % i for i in range(n)]
    for did in ids:
        ins, cls = label_pair(rng, H, W, 6)
        ins_u8 = np.where(ins < 0, 0, ins + 1).astype(np.uint8)
        cls_u8 = cls.astype(np.uint8)
        PIL.Image.fromarray(rng.randint(0, 256, (H, W, 3)).astype(np.uint8)).save(
            os.path.join(root, 'img', did + '.jpg'), quality=90)
        scipy.io.savemat(os.path.join(root, 'cls', did + '.mat'), {'GTcls': {'Segmentation': cls_u8}})
        scipy.io.savemat(os.path.join(root, 'inst', did + '.mat'), {'GTinst': {'Segmentation': ins_u8}})
    with open(os.path.join(root, 'train.txt'), 'w') as f:
        f.write(''.join(d + '\n' for d in ids))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'label_instances.json'))
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(0)
    rows = {}
    for H, W, n in SHAPES:
        ins, cls = label_pair(rng, H, W, n)
        ti, tc = torch.from_numpy(ins).to(dev), torch.from_numpy(cls).to(dev)
        key = '%dx%d_%d' % (H, W, n)
        k_med, k_mean = timed(lambda: cmr.utils.label2instance_boxes(ti, tc, return_masks=True),
                              args.reps)
        r_med, r_mean = timed(lambda: cmr.utils.label2instance_boxes(ins, cls, return_masks=True),
                              args.reps)
        rows[key] = {'instances': n, 'kernels_ms_median': k_med, 'kernels_ms_mean': k_mean,
                     'round_trip_ms_median': r_med, 'round_trip_ms_mean': r_mean,
                     'host_reference_ms': HOST_REFERENCE_MS[key]}
        print(key, json.dumps(rows[key]))
    with tempfile.TemporaryDirectory() as d:
        sbd_tree(d, rng)
        import train_loop as TL
        data = cmr.datasets.SBDInstanceSegmentationDataset('train', root_dir=d)
        model = cmr.models.MaskRCNNResNet(50, pretrained_model=None, roi_size=14,
                                          **TL.VOC_MODEL).to(dev)
        train = TL.TransformDataset(data, cmr.datasets.MaskRCNNTransform(model))
        f_med, f_mean = timed(lambda: [train[j] for j in (0, 1)], args.reps)
        g_med, _ = timed(lambda: [data[j] for j in (0, 1)], args.reps)
    fetch = {'batch': 2, 'image': '375x500, 6 instances', 'fetch_ms_median': f_med,
             'fetch_ms_mean': f_mean, 'get_example_ms_median': g_med}
    print('fetch', json.dumps(fetch))
    payload = {'what': 'utils.label2instance_boxes(return_masks=True) on one MI355X; host_reference_ms '
                       'is the reference function on a CPU build host (mean of 5 calls)',
               'reps': args.reps, 'conversion': rows, 'train_fetch_sbd': fetch,
               'device': torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(payload, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
