"""ResNetRoIHead and the train / predict paths with roi_pooling_2d and crop_and_resize as the
head's pooling_func (the reference's --pooling-func pooling / resize)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import chainer_mask_rcnn_amd as cmr
from chainer_mask_rcnn_amd import functions, optimizers

import pool_variants_ref as ref
import ref_model

pytestmark = pytest.mark.gpu

FUNCS = [functions.roi_pooling_2d, functions.crop_and_resize]
IDS = ['pooling', 'resize']


class _RefPool(torch.autograd.Function):
    """The NumPy restatement as a float64 CPU autograd op (rois: xy rows)."""

    @staticmethod
    def forward(ctx, x, rois, fn, size):
        xs = x.detach().numpy().astype(np.float32)
        r = rois.numpy()
        if fn is functions.roi_pooling_2d:
            y, am = ref.roi_pooling_2d_fwd(xs, r, size, size, 1 / 16.)
            ctx.am = am
        else:
            y = ref.crop_and_resize_fwd(xs, r, size, size, 1 / 16.)
        ctx.meta = (fn, r, tuple(x.shape))
        return torch.tensor(y, dtype=x.dtype)

    @staticmethod
    def backward(ctx, gy):
        fn, r, shape = ctx.meta
        if fn is functions.roi_pooling_2d:
            gx = ref.roi_pooling_2d_bwd(gy.numpy().astype(np.float32), ctx.am, r, shape)
        else:
            gx = ref.crop_and_resize_bwd(gy.numpy(), r, shape, 1 / 16.)
        return torch.tensor(gx, dtype=gy.dtype), None, None, None


def _ref_head(x, rois_xy, P, n_class, roi_size, fn):
    return _ref_head_from_pool(_RefPool.apply(x, rois_xy, fn, roi_size), P, n_class, roi_size)


def _ref_head_from_pool(pool, P, n_class, roi_size):
    res5 = ref_model.building_block(pool, P, 'res5', 3, roi_size // 7)
    pool5 = TF.avg_pool2d(res5, 7, 7).flatten(1)
    fc = TF.linear(pool5, P['cls_loc_score.W'], P['cls_loc_score.b'])
    d = TF.relu(TF.conv_transpose2d(res5, P['deconv6.W'], P['deconv6.b'], stride=2))
    masks = TF.conv2d(d, P['mask.W'], P['mask.b'])
    return fc[:, :4 * n_class], fc[:, 4 * n_class:5 * n_class], masks


def _setup(dev, roi_size, seed=0):
    torch.manual_seed(seed)
    head = cmr.models.mask_rcnn_resnet.ResNetRoIHead(50, 5, roi_size, 1 / 16.).to(dev)
    with torch.no_grad():
        for name, p in head.named_parameters():
            if '.bn' in name and name.endswith('.W'):
                p.uniform_(0.5, 1.0)
            elif '.bn' in name:
                p.normal_(0, 0.1)
    rng = np.random.RandomState(seed + 1)
    x = torch.tensor(rng.standard_normal((2, 1024, 13, 17)).astype(np.float32), device=dev)
    n, H, W = 16, 13 * 16, 17 * 16
    y1 = rng.uniform(0, 0.7 * H, n)
    x1 = rng.uniform(0, 0.7 * W, n)
    yx = np.stack([y1, x1, y1 + rng.uniform(16, 0.5 * H, n), x1 + rng.uniform(16, 0.5 * W, n)], 1)
    idx = np.sort(rng.randint(0, 2, n)).astype(np.int32)           # grouped by image
    return head, x, torch.tensor(yx.astype(np.float32), device=dev), torch.tensor(idx, device=dev)


def _rel_l2(got, want):
    got, want = got.detach().cpu().double(), want.detach().double()
    return ((got - want).norm() / want.norm().clamp_min(1e-300)).item()


def _head_errors(dev, fn, roi_size):
    """Outputs (max error / scale) and gradients (relative L2) of the HIP head with ``fn`` against
    the float64 CPU head with the matching restatement (ROIAlign: the C oracle)."""
    head, x, rois, idx = _setup(dev, roi_size)
    head.pooling_func = fn
    xg = x.clone().requires_grad_(True)
    outs = head(xg, rois, idx)
    rng = np.random.RandomState(3)
    gs = [torch.tensor(rng.standard_normal(tuple(o.shape)).astype(np.float32)) for o in outs]
    sum(((o * g.to(dev)).sum() for o, g in zip(outs, gs))).backward()
    torch.cuda.synchronize()
    P = ref_model.RefParams(head)
    xr = x.detach().cpu().double().requires_grad_(True)
    rois_xy = torch.cat([idx.cpu().float()[:, None], rois.cpu()], 1)[:, [0, 2, 1, 4, 3]].contiguous()
    if fn is functions.roi_align_2d:
        pool = ref_model._RefROIAlign.apply(xr, rois_xy, roi_size, roi_size, 1 / 16.)
        refs = _ref_head_from_pool(pool, P, 5, roi_size)
    else:
        refs = _ref_head(xr, rois_xy, P, 5, roi_size, fn)
    sum(((o * g.double()).sum() for o, g in zip(refs, gs))).backward()
    out_err = [(o.detach().cpu().double() - r.detach()).abs().max().item() / r.detach().abs().max().item()
               for o, r in zip(outs, refs)]
    grad_err = {'x': _rel_l2(xg.grad, xr.grad)}
    for name, p in head.named_parameters():
        if p.grad is not None and P[name].grad is not None:
            grad_err[name] = _rel_l2(p.grad, P[name].grad)
    return out_err, grad_err


@pytest.mark.parametrize('roi_size', [14, 7])
@pytest.mark.parametrize('fn', FUNCS, ids=IDS)
def test_head_against_float64_reference(dev, fn, roi_size):
    """Outputs within 1e-4 of their scale.  Gradients (relative L2) within 5e-3, or within twice
    the error the same head shows with ROIAlign against its float64 reference.  The gradients pass
    backwards through res5's ReLUs, and a unit whose pre-activation sits within fp32 rounding of
    zero is decided differently from float64 (ROIAlign's own head gradients miss float64 by up to
    1.5e-3 here).  Max pooling and crop-and-resize of the small test RoIs repeat one feature value
    over many bins, so one such decision repeats over many positions: measured up to 3.8e-3.  The
    operators themselves are pinned bit for bit / per element by tests/test_gpu_pool_variants.py."""
    out_err, grad_err = _head_errors(dev, fn, roi_size)
    _, align_err = _head_errors(dev, functions.roi_align_2d, roi_size)
    print('outputs', out_err, 'gradients', grad_err, 'ROIAlign gradients', align_err)
    assert max(out_err) <= 1e-4, out_err
    assert len(grad_err) >= 12
    for k, e in grad_err.items():
        assert e <= max(5e-3, 2 * align_err[k]), (k, e, align_err[k])


@pytest.mark.parametrize('fn', FUNCS, ids=IDS)
def test_bin_stride_route_equals_reference_shaped_route(dev, fn):
    head, x, rois, idx = _setup(dev, 14)
    outs = {}
    with torch.no_grad():
        for name, f in (('strided', fn), ('plain', lambda *a, **k: fn(*a, **k))):
            head.pooling_func = f
            outs[name] = [t.cpu() for t in head(x, rois, idx)]
    for a, b in zip(outs['strided'], outs['plain']):
        assert (a - b).abs().max().item() <= 1e-5 * b.abs().max().item()


def _chain(dev, fn):
    import test_gpu_model as M
    model, chain, imgs, bboxes, labels, masks = M._build(dev)
    model.head.pooling_func = fn
    return model, chain, imgs, bboxes, labels, masks, M.freeze_like_reference


@pytest.mark.parametrize('fn', FUNCS, ids=IDS)
def test_training_steps_finite_and_bit_reproducible(dev, fn):
    def run():
        model, chain, imgs, bboxes, labels, masks, freeze = _chain(dev, fn)
        opt = optimizers.MomentumSGD(lr=0.002, momentum=0.9)
        opt.setup(chain)
        opt.add_hook(optimizers.WeightDecay(1e-4))
        freeze(model, chain)
        x = torch.tensor(imgs, device=dev)
        np.random.seed(5)
        losses = [opt.update(chain, x, bboxes, labels, masks, [1., 1.]).item() for _ in range(3)]
        torch.cuda.synchronize()
        return losses, opt.arena.values.clone()
    l1, w1 = run()
    l2, w2 = run()
    assert all(np.isfinite(l1)) and l1 == l2
    assert torch.equal(w1, w2)


@pytest.mark.parametrize('fn', ['pooling', 'resize'])
def test_full_size_training_is_bit_reproducible(dev, fn):
    """configs[1] size: batch 2 x 800 x 1333, 512 RoIs per image, tools/train_loop.py's trainer."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import train_loop as TL
    runs = []
    for _ in range(2):
        data = TL.SyntheticInstances(2, seed=0)
        loop, model, chain, opt = TL.build(data, 50, 'cuda:0', 2, 0, prefetch=False, pooling_func=fn)
        assert model.head.pooling_func is getattr(functions, TL.POOLING_FUNCS[fn])
        losses = [float(l.detach()) for l in loop.run(2)]
        opt.flush()
        torch.cuda.synchronize()
        loop.close()
        runs.append((losses, opt.arena.values.clone()))
    assert all(np.isfinite(runs[0][0])) and runs[0][0] == runs[1][0]
    assert torch.equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize('fn', FUNCS, ids=IDS)
def test_predict_end_to_end(dev, fn):
    import test_gpu_model as M
    model, chain, imgs, *_ = _chain(dev, fn)
    model.eval()
    bboxes, roi_masks, labels, scores = model.predict_prepared(
        torch.tensor(imgs, device=dev), [1., 1.], [(M.H, M.W), (M.H, M.W)])
    assert len(bboxes) == len(roi_masks) == len(labels) == len(scores) == 2
    for b, m, l, s in zip(bboxes, roi_masks, labels, scores):
        assert b.shape[1] == 4 and len(b) == len(m) == len(l) == len(s)
        assert np.isfinite(np.asarray(b)).all() and np.isfinite(np.asarray(s)).all()
