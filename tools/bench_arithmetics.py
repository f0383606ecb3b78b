"""The four arithmetics of the convolution GEMMs (functions.conv.set_gemm_arithmetic: fp32,
split_bf16x3, split_bf16x2, bf16x1) side by side, on the synthetic model of bench.py:

* per convolution shape of the train step (batch 2 x 800 x 1333) and of inference (batch 8 x 1024 x 1024),
  collected by tracing the library calls of one step as tools/step_shapes.py does: the time per launch and
  the maximum and rms error against float64, both relative to max|ref|, for the forward, the forward-form
  data gradient and the weight gradient entry points, on N(0, 1) operands (filters / sqrt(C R S));
* the whole train step and the whole ``predict`` under each arithmetic;
* the largest differences of ``predict``'s boxes, scores and 14x14 mask probabilities from 'fp32'.

One JSON object per line; ``--table`` adds a readable table.  Numbers for DESIGN.md section 23."""
import argparse
import collections
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as TF

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench                                                                      # noqa: E402
from chainer_mask_rcnn_amd import _lib                                             # noqa: E402
from chainer_mask_rcnn_amd.functions import conv as C                              # noqa: E402
from chainer_mask_rcnn_amd.functions._layout import empty_nhwc                     # noqa: E402

NAMES = ('fp32', 'split_bf16x3', 'split_bf16x2', 'bf16x1')
ENTRIES = {'mrcnn_conv2d_fwd': 'fwd', 'mrcnn_conv2d_dgrad_wt': 'dgrad_wt', 'mrcnn_conv2d_wgrad': 'wgrad',
           'mrcnn_conv2d_wgrad_ex': 'wgrad'}
Shape = collections.namedtuple('Shape', 'entry N C H W K R stride pad')


class Trace(object):
    """Counts the (entry, descriptor) pairs of the GEMM entry points called inside."""

    def __init__(self):
        self.seen = collections.OrderedDict()

    def __enter__(self):
        self.orig = _lib.call

        def traced(name, *args):
            if name in ENTRIES:
                d = args[0]._obj
                key = Shape(ENTRIES[name], d.N, d.C, d.H, d.W, d.K, d.R, d.stride, d.pad)
                self.seen[key] = self.seen.get(key, 0) + 1
            return self.orig(name, *args)
        _lib.call = traced
        return self

    def __exit__(self, *exc):
        _lib.call = self.orig
        return False


def timed(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def float64_reference(s, x, w, gy):
    """The entry's result in float64 (torch on the device; the CPU where the device has no float64 path)."""
    for device in (x.device, torch.device('cpu')):
        try:
            xd, wd, gd = (t.to(device, torch.float64) for t in (x, w, gy))
            if s.entry == 'fwd':
                return TF.conv2d(xd, wd, stride=s.stride, padding=s.pad).cpu()
            if s.entry == 'dgrad_wt':
                return torch.nn.grad.conv2d_input(x.shape, wd, gd, stride=s.stride, padding=s.pad).cpu()
            return torch.nn.grad.conv2d_weight(xd, w.shape, gd, stride=s.stride, padding=s.pad).cpu()
        except RuntimeError:
            continue
    raise RuntimeError('no float64 convolution for %s' % (s,))


def layer(s, dev, iters, with_error):
    """{'ms': {name: .}, 'max_err': {name: .}, 'rms_err': {name: .}} of one shape."""
    lib = _lib.load()
    seed = (((s.N * 131 + s.C) * 131 + s.H) * 131 + s.W) * 131 + s.K * 7 + s.R + len(s.entry)
    g = torch.Generator(device=dev).manual_seed(seed & 0x7fffffff)
    x = torch.randn((s.N, s.H, s.W, s.C), device=dev, generator=g).permute(0, 3, 1, 2)
    w = (torch.randn((s.K, s.R, s.R, s.C), device=dev, generator=g) / (s.C * s.R * s.R) ** 0.5).permute(0, 3, 1, 2)
    d = C.make_desc(x.shape, w.shape, s.stride, s.pad)
    gy = torch.randn((d.N, d.P, d.Q, d.K), device=dev, generator=g).permute(0, 3, 1, 2)
    sp, sw = _lib.stream_ptr(), _lib.ptr(C.split_ws(dev))
    if s.entry == 'fwd':
        out = empty_nhwc((d.N, d.K, d.P, d.Q), dev)
        run = lambda: _lib.call('mrcnn_conv2d_fwd', C.ctx_desc(d), _lib.ptr(x), _lib.ptr(w), None, None, None,   # noqa: E731
                                None, _lib.ptr(out), 0, sw, sp)
    elif s.entry == 'dgrad_wt':
        out = empty_nhwc((s.N, s.C, s.H, s.W), dev)
        wT = torch.empty((w.numel(),), device=dev)
        _lib.call('mrcnn_filter_flip_transpose', _lib.ptr(w), _lib.ptr(wT), s.K, s.R, s.R, s.C, None, sp)
        run = lambda: _lib.call('mrcnn_conv2d_dgrad_wt', C.ctx_desc(d), _lib.ptr(gy), _lib.ptr(wT), _lib.ptr(out), 0,   # noqa: E731
                                None, None, None, None, sw if s.stride == 1 else None, sp)
    else:
        out = torch.empty_like(w)
        ws = _lib.workspace(lib.mrcnn_conv2d_wgrad_workspace_bytes(C.ctx_desc(d)), dev, 'wgrad')
        run = lambda: _lib.call('mrcnn_conv2d_wgrad', C.ctx_desc(d), _lib.ptr(x), _lib.ptr(gy), _lib.ptr(out),   # noqa: E731
                                _lib.ptr(ws), sp)
    ref = float64_reference(s, x, w, gy) if with_error else None
    res = {'ms': {}, 'max_err': {}, 'rms_err': {}}
    for name in NAMES:
        C.set_gemm_arithmetic(name)
        res['ms'][name] = round(timed(run, iters), 5)
        if ref is not None:
            torch.cuda.synchronize()
            err = (out.detach().cpu().double() - ref).abs()
            scale = ref.abs().max().item()
            res['max_err'][name] = err.max().item() / scale
            res['rms_err'][name] = err.pow(2).mean().sqrt().item() / scale
    C.set_gemm_arithmetic(C.DEFAULT_GEMM_ARITHMETIC)
    return res


def infer_setup(dev, batch):
    import chainer_mask_rcnn_amd as cmr
    torch.manual_seed(0)
    model = cmr.models.MaskRCNNResNet(n_layers=50, n_fg_class=80, min_size=800, max_size=1333,
                                      anchor_scales=(2, 4, 8, 16, 32), roi_size=14).to(dev)
    bench.stabilise_synthetic_weights(model)
    with torch.no_grad():
        model.head.cls_loc_score.W[4 * 81:5 * 81] *= 60.
    mean = np.asarray(bench.MEAN, np.float32)[:, None, None]
    x = torch.tensor(np.random.RandomState(0).uniform(0, 255, (batch, 3, 1024, 1024)).astype(np.float32) - mean,
                     device=dev).contiguous(memory_format=torch.channels_last)
    return model, lambda: model.predict_prepared(x, [1.6] * batch, [(640, 640)] * batch)


def predict_diff(out, base):
    """Largest |difference| of boxes, scores and sigmoid(mask logits) between two predict outputs.  On random
    weights many scores are nearly tied, so the order of the detections is not stable: every detection of
    ``base`` is paired with the detection of ``out`` of the same label that overlaps it most, pairs of
    IoU >= 0.5 are compared and the others counted."""
    diff = {'boxes_px': 0., 'scores': 0., 'mask_prob': 0., 'paired': 0, 'unpaired': 0}
    sig = lambda a: 1. / (1. + np.exp(-np.asarray(a, np.float64)))                  # noqa: E731
    for i in range(len(base[0])):
        bb, ob = np.asarray(base[0][i], np.float64), np.asarray(out[0][i], np.float64)
        for j in range(len(bb)):
            same = np.nonzero(np.asarray(out[2][i]) == base[2][i][j])[0]
            if len(same) == 0:
                diff['unpaired'] += 1
                continue
            tl = np.maximum(bb[j, :2], ob[same, :2])
            br = np.minimum(bb[j, 2:], ob[same, 2:])
            inter = np.prod(np.clip(br - tl, 0, None), axis=1)
            union = np.prod(bb[j, 2:] - bb[j, :2]) + np.prod(ob[same, 2:] - ob[same, :2], axis=1) - inter
            k = int(np.argmax(inter / np.maximum(union, 1e-12)))
            if inter[k] / max(union[k], 1e-12) < 0.5:
                diff['unpaired'] += 1
                continue
            k = same[k]
            diff['paired'] += 1
            diff['boxes_px'] = max(diff['boxes_px'], float(np.abs(ob[k] - bb[j]).max()))
            diff['scores'] = max(diff['scores'], float(abs(out[3][i][k] - base[3][i][j])))
            lab = int(base[2][i][j])
            diff['mask_prob'] = max(diff['mask_prob'],
                                    float(np.abs(sig(out[1][i][k][lab]) - sig(base[1][i][j][lab])).max()))
    return diff


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--iters', type=int, default=10, help='timed launches per layer and arithmetic')
    ap.add_argument('--steps', type=int, default=10, help='timed train steps / predict calls per arithmetic')
    ap.add_argument('--infer-batch', type=int, default=8)
    ap.add_argument('--error-on', default='both', choices=['train', 'infer', 'both', 'none'],
                    help='the workloads whose layers are also compared with float64')
    ap.add_argument('--no-layers', action='store_true', help='whole step and predict only')
    ap.add_argument('--table', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    _lib.load()
    emit = lambda **kw: print(json.dumps(kw), flush=True)                           # noqa: E731

    # ---- train step ---------------------------------------------------------------------------------
    import random
    random.seed(0); np.random.seed(0); torch.manual_seed(0)
    imgs, bboxes, labels, masks, scales = bench.synthetic_batch(np.random.RandomState(0), 2, 800, 1333)
    model, chain, opt, sync = bench.build_trainer(50, dev, 1, 2)
    imgs_d = torch.tensor(imgs, device=dev).contiguous(memory_format=torch.channels_last)
    step = lambda: opt.update(chain, imgs_d, bboxes, labels, masks, scales)         # noqa: E731
    for _ in range(3):
        step()
    with Trace() as train_trace:
        step()
    for name in NAMES:
        C.set_gemm_arithmetic(name)
        for _ in range(3):
            loss = step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            loss = step()
        torch.cuda.synchronize()
        emit(what='train_step', arithmetic=name, ms_per_step=round((time.perf_counter() - t0) / args.steps * 1e3, 3),
             loss=float(loss.item()))
    C.set_gemm_arithmetic(C.DEFAULT_GEMM_ARITHMETIC)
    del model, chain, opt, sync, imgs_d

    # ---- predict ------------------------------------------------------------------------------------
    model, predict = infer_setup(dev, args.infer_batch)
    predict()
    with Trace() as infer_trace:
        predict()
    outs = {}
    for name in NAMES:
        C.set_gemm_arithmetic(name)
        for _ in range(2):
            predict()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            outs[name] = predict()
        torch.cuda.synchronize()
        emit(what='predict', arithmetic=name, ms_per_call=round((time.perf_counter() - t0) / args.steps * 1e3, 3),
             detections=[len(b) for b in outs[name][0]])
    C.set_gemm_arithmetic(C.DEFAULT_GEMM_ARITHMETIC)
    for name in NAMES[1:]:
        emit(what='predict_vs_fp32', arithmetic=name, **predict_diff(outs[name], outs['fp32']))
    del model, outs

    # ---- layers -------------------------------------------------------------------------------------
    if args.no_layers:
        return
    rows = []
    for workload, trace in (('train', train_trace), ('infer', infer_trace)):
        for s, count in trace.seen.items():
            r = layer(s, dev, args.iters, args.error_on in (workload, 'both'))
            emit(what='layer', workload=workload, calls=count, shape=s._asdict(), **r)
            rows.append((workload, count, s, r))
    if args.table:
        print('%-6s %5s %-9s %-34s | %s' % ('', 'calls', 'entry', '(N,C,H,W,K,R,stride,pad)',
                                            ' | '.join('%-28s' % n for n in NAMES)))
        for workload, count, s, r in rows:
            cells = ['%7.3f ms %8.1e %8.1e' % (r['ms'][n], r['max_err'].get(n, float('nan')),
                                               r['rms_err'].get(n, float('nan'))) for n in NAMES]
            print('%-6s %5d %-9s %-34s | %s' % (workload, count, s.entry, tuple(s[1:]), ' | '.join(cells)))


if __name__ == '__main__':
    main()
