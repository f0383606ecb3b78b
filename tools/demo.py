"""Predict on image files and save the drawings: the counterpart of the reference's
examples/demo.py.

    python tools/demo.py --detectron model.pkl --img a.jpg b.jpg --out demo_out
    python tools/demo.py --snapshot snapshot_model.npz --dataset voc --img a.jpg

Detections with a score of at least 0.7 are drawn in ascending score order (the best one on
top), captioned '<class>: <score>'; the drawing runs on the device (utils.draw_instance_bboxes
on the packed masks of ``paste_packed``).  Images are local files read with Pillow.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from evaluate import (add_postprocessing_flags, apply_postprocessing_flags,  # noqa: E402
                      check_postprocessing_flags)

POOLING_FUNCS = {'align': 'roi_align_2d', 'pooling': 'roi_pooling_2d', 'resize': 'crop_and_resize'}


def main():
    ap = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument('--img', '-i', nargs='+', required=True, help='image files')
    ap.add_argument('--snapshot', default=None, help='snapshot_model.npz of this package / the reference')
    ap.add_argument('--detectron', default=None, help='Detectron R-50-C4 / R-101-C4 .pkl')
    ap.add_argument('--layers', type=int, default=50, choices=[50, 101])
    ap.add_argument('--pooling-func', default='align', choices=sorted(POOLING_FUNCS))
    ap.add_argument('--dataset', default='coco', choices=['coco', 'voc'],
                    help='class names and model sizes (COCO: 800 / 1333, VOC: 600 / 1000)')
    ap.add_argument('--class-names', default=None,
                    help='text file with one foreground class name per line (default: the VOC '
                         'names for --dataset voc, class0..class79 for coco)')
    ap.add_argument('--out', default='demo_out', help='output directory')
    add_postprocessing_flags(ap)
    ap.add_argument('--arithmetic', default=None, choices=['fp32', 'split_bf16x3', 'split_bf16x2', 'bf16x1'],
                    help='arithmetic of the convolution GEMMs (functions.conv.set_gemm_arithmetic; default '
                         'split_bf16x3: fp32-accurate; split_bf16x2: 16-bit-class operands; bf16x1: bf16 '
                         'operands; all with fp32 accumulation and fp32 weights)')
    args = ap.parse_args()
    if args.arithmetic is not None:
        from chainer_mask_rcnn_amd.functions import conv
        conv.set_gemm_arithmetic(args.arithmetic)
    check_postprocessing_flags(ap, args)
    if not (args.snapshot or args.detectron):
        ap.error('--snapshot or --detectron is required')

    from PIL import Image
    import chainer_mask_rcnn_amd as cmr
    from chainer_mask_rcnn_amd import serializers
    from chainer_mask_rcnn_amd.utils.evaluations import masks as M
    from chainer_mask_rcnn_amd.utils import visualizations as V
    dev = torch.device('cuda:0')

    if args.dataset == 'voc':
        class_names = [str(n) for n in cmr.datasets.VOC2012InstanceSegmentationDataset.class_names]
        size = dict(min_size=600, max_size=1000, anchor_scales=(4, 8, 16, 32))
    else:
        class_names = ['class%d' % i for i in range(80)]
        size = dict(min_size=800, max_size=1333, anchor_scales=(2, 4, 8, 16, 32))
    if args.class_names:
        with open(args.class_names) as f:
            class_names = [line.strip() for line in f if line.strip()]
    model = cmr.models.MaskRCNNResNet(
        n_layers=args.layers, n_fg_class=len(class_names), roi_size=14,
        pooling_func=getattr(cmr.functions, POOLING_FUNCS[args.pooling_func]), **size).to(dev)
    if args.snapshot:
        serializers.load_npz(args.snapshot, model)
    else:
        serializers.load_detectron(args.detectron, model, n_layers=args.layers)
    model.eval()
    apply_postprocessing_flags(model, args)
    os.makedirs(args.out, exist_ok=True)

    for img_file in args.img:
        img = np.asarray(Image.open(img_file).convert('RGB'))
        bboxes, roi_masks, labels, scores, sizes = model.predict_images(
            [img.transpose(2, 0, 1)], masks_to_host=False)
        bbox, label, score = bboxes[0], labels[0], scores[0]
        k = np.flatnonzero(score >= 0.7)
        k = k[np.argsort(score[k], kind='stable')]
        bbox, label, score = bbox[k], label[k], score[k]
        packed = M.paste_packed(roi_masks[0][torch.from_numpy(k).to(dev)], label, bbox, sizes[0])
        captions = ['{}: {:.1%}'.format(class_names[l], s) for l, s in zip(label, score)]
        for caption in captions:
            print(caption)
        viz = torch.from_numpy(np.ascontiguousarray(img)).to(dev)
        V.draw_instances_device(viz, bbox, label + 1, len(class_names) + 1, masks=packed,
                                captions=captions)
        out_file = os.path.join(args.out, os.path.basename(img_file))
        Image.fromarray(viz.cpu().numpy()).save(out_file)
        print('Saved result: {}'.format(out_file))


if __name__ == '__main__':
    main()
