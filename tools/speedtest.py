"""The reference's only published speed protocol (examples/coco/speedtest.py:14-56, result in
examples/coco/README.md:48-72: 3.24 Hz on a GTX 1080 Ti): `model.predict([img])` on ONE image,
5 warm-up calls, then N timed calls including host<->device copies, box NMS, the mask head and
the mask paste.  Synthetic image and random weights here (no dataset / snapshot offline), head
scores scaled so that detections exist (100 per image, the maximum)."""
import argparse, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import chainer_mask_rcnn_amd as cmr
import bench


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('times', nargs='?', type=int, default=10, help='timed calls')
    ap.add_argument('--arithmetic', default=None, choices=['fp32', 'split_bf16x3', 'split_bf16x2', 'bf16x1'],
                    help='arithmetic of the convolution GEMMs (functions.conv.set_gemm_arithmetic; default '
                         'split_bf16x3: fp32-accurate; split_bf16x2: 16-bit-class operands; bf16x1: bf16 '
                         'operands; all with fp32 accumulation and fp32 weights)')
    args = ap.parse_args()
    times = args.times
    if args.arithmetic is not None:
        cmr.functions.conv.set_gemm_arithmetic(args.arithmetic)
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    model = cmr.models.MaskRCNNResNet(50, n_fg_class=80, min_size=800, max_size=1333,
                                      anchor_scales=(2, 4, 8, 16, 32), roi_size=14).to(dev)
    bench.stabilise_synthetic_weights(model)
    with torch.no_grad():
        model.head.cls_loc_score.W[4 * 81:5 * 81] *= 60.
    # random weights never reach the reference's 0.7: keep the default 0.05 so that the NMS, the
    # mask head and the paste all run, on the maximum of 100 detections (more than a real image has)
    img = np.random.RandomState(0).randint(0, 256, (3, 480, 640)).astype(np.uint8)   # COCO-sized
    for _ in range(5):
        out = model.predict([img])
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(times):
        out = model.predict([img])
    torch.cuda.synchronize()
    dt = time.time() - t0
    print('detections: %d' % len(out[0][0]))
    print('Elapsed time: %.3f [s / %d evals]' % (dt, times))
    print('Hz: %.2f [hz]' % (times / dt))


if __name__ == '__main__':
    main()
