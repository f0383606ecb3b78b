"""roi_pooling_2d / crop_and_resize kernels on the device against the NumPy restatements of
tests/pool_variants_ref.py.

Max pooling: forward values and argmax bit-exact; the backward is bit-exact as well (the kernel
sums every pixel's contributions in the stated (RoI, bin row, bin column) order, as the
restatement does).  Crop-and-resize: the forward is bit-exact (same fp32 operations in the same
order, no contraction), the backward within |got - ref| <= 1e-4 |ref| + 1e-5 max|ref| of a float64
adjoint."""
import numpy as np
import pytest
import torch

from chainer_mask_rcnn_amd import functions as F

import pool_variants_ref as ref

pytestmark = pytest.mark.gpu


def _close(got, want, rtol=1e-4, atol_of_max=1e-5):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    tol = rtol * np.abs(want) + atol_of_max * max(np.abs(want).max(), 1e-30)
    bad = np.abs(got - want) > tol
    assert not bad.any(), 'max err %g (scale %g), %d elements' % (
        np.abs(got - want).max(), np.abs(want).max(), bad.sum())


def _rois(rng, R, N, H, W, scale):
    """Proposal-like boxes plus the awkward cases: degenerate, off the map, on .5 ties, batch 1."""
    Hi, Wi = H / scale, W / scale
    y1 = rng.uniform(-0.1 * Hi, 0.9 * Hi, R)
    x1 = rng.uniform(-0.1 * Wi, 0.9 * Wi, R)
    h = rng.uniform(2, 0.6 * Hi, R)
    w = rng.uniform(2, 0.6 * Wi, R)
    b = rng.randint(0, N, R)
    rois = np.stack([b, x1, y1, x1 + w, y1 + h], 1).astype(np.float32)
    extra = np.array([[1, 40, 40, 72, 72],                       # 2.5 / 4.5 at 1/16
                      [1, 24, 8, 24, 8],                          # zero size
                      [1, 90, 90, 10, 10],                        # x2 < x1
                      [0, 4 * Wi, 4 * Hi, 5 * Wi, 5 * Hi],        # past the map
                      [1, -3 * Wi, -3 * Hi, -2 * Wi, -2 * Hi],    # before the map
                      [1, -8, -8, 0.5 * Wi, 8],
                      [0, 0, 0, Wi - 1, Hi - 1]], np.float32)
    return np.concatenate([rois, extra])


def _run(fn, x, rois, outh, outw, scale, gy=None, axes='xy', **kw):
    dev = torch.device('cuda:0')
    xt = torch.tensor(x, device=dev, requires_grad=True)
    rt = torch.tensor(rois, device=dev)
    if axes == 'yx':
        rt = rt[:, [0, 2, 1, 4, 3]]
    y = fn(xt, rt, outh, outw, scale, axes=axes, **kw)
    if gy is not None:
        y.backward(torch.tensor(gy, device=dev))
    torch.cuda.synchronize()
    return y.detach().cpu().numpy(), (xt.grad.cpu().numpy() if gy is not None else None)


SHAPES = [(3, 7, 7), (8, 7, 5), (64, 14, 14), (260, 7, 5), (1024, 7, 7)]


@pytest.mark.parametrize('C,outh,outw', SHAPES)
@pytest.mark.parametrize('axes', ['xy', 'yx'])
@pytest.mark.parametrize('scale', [1 / 16., 0.3])
def test_roi_pooling_matches_restatement(dev, C, outh, outw, axes, scale):
    rng = np.random.RandomState(C + outh)
    N, H, W = 2, 13, 19
    x = rng.standard_normal((N, C, H, W)).astype(np.float32)
    x[:, :, 3, 4:6] = 2.5          # exact ties inside bins: the first maximum must stay
    rois = _rois(rng, 12, N, H, W, scale)
    y_ref, am_ref = ref.roi_pooling_2d_fwd(x, rois, outh, outw, scale)
    gy = rng.standard_normal(y_ref.shape).astype(np.float32)
    gx_ref = ref.roi_pooling_2d_bwd(gy, am_ref, rois, x.shape)
    y, gx = _run(F.roi_pooling_2d, x, rois, outh, outw, scale, gy, axes)
    assert np.array_equal(y, y_ref)
    assert np.array_equal(gx, gx_ref)          # same summation order: bit-exact
    # the argmax the forward saves for the backward
    import importlib
    M = importlib.import_module('chainer_mask_rcnn_amd.functions.roi_pooling_2d')

    class Ctx(object):
        def save_for_backward(self, *t):
            self.saved = t
    ctx = Ctx()
    M._ROIPooling2DFn.forward(ctx, torch.tensor(x, device=dev), torch.tensor(rois, device=dev),
                              outh, outw, scale)
    am = ctx.saved[1]
    assert np.array_equal(am.cpu().numpy(), am_ref)


@pytest.mark.parametrize('C,outh,outw', SHAPES)
@pytest.mark.parametrize('axes', ['xy', 'yx'])
@pytest.mark.parametrize('scale', [1 / 16., 0.3])
def test_crop_and_resize_matches_restatement(dev, C, outh, outw, axes, scale):
    rng = np.random.RandomState(100 + C + outw)
    N, H, W = 2, 13, 19
    x = rng.standard_normal((N, C, H, W)).astype(np.float32)
    rois = _rois(rng, 12, N, H, W, scale)
    y_ref = ref.crop_and_resize_fwd(x, rois, outh, outw, scale)
    gy = rng.standard_normal(y_ref.shape).astype(np.float32)
    gx_ref = ref.crop_and_resize_bwd(gy, rois, x.shape, scale)
    y, gx = _run(F.crop_and_resize, x, rois, outh, outw, scale, gy, axes)
    assert np.array_equal(y, y_ref)
    _close(gx, gx_ref)


@pytest.mark.parametrize('fn', [F.roi_pooling_2d, F.crop_and_resize], ids=['pooling', 'resize'])
@pytest.mark.parametrize('C', [8, 6, 256])
def test_bin_stride_order_and_run_to_run(dev, fn, C):
    rng = np.random.RandomState(7)
    N, H, W = 2, 21, 30
    x = rng.standard_normal((N, C, H, W)).astype(np.float32)
    rois = _rois(rng, 40, N, H, W, 1 / 16.)
    rois = rois[np.argsort(rois[:, 0], kind='stable')]       # grouped by image, as the head passes them
    dev_ = torch.device('cuda:0')
    xt = torch.tensor(x, device=dev_)
    rt = torch.tensor(rois, device=dev_)
    full = fn(xt, rt, 14, 14, 1 / 16.)
    half = fn(xt, rt, 14, 14, 1 / 16., bin_stride=2)
    assert torch.equal(half, full[:, :, ::2, ::2])
    perm = torch.tensor(rng.permutation(len(rois)).astype(np.int32), device=dev_)
    assert torch.equal(fn(xt, rt, 14, 14, 1 / 16., bin_stride=2, order=perm), half)
    # backward of the strided form = the full backward with zeros on the skipped bins
    gy = torch.tensor(rng.standard_normal(tuple(half.shape)).astype(np.float32), device=dev_)
    gfull = torch.zeros_like(full)
    gfull[:, :, ::2, ::2] = gy
    grads = []
    for kw, g in ((dict(bin_stride=2), gy), (dict(bin_stride=2, order=perm), gy), (dict(bin_stride=2), gy),
                  ({}, gfull)):
        xg = xt.clone().requires_grad_(True)
        fn(xg, rt, 14, 14, 1 / 16., **kw).backward(g)
        grads.append(xg.grad)
    assert torch.equal(grads[0], grads[1]) and torch.equal(grads[0], grads[2])   # run to run
    if fn is F.roi_pooling_2d:
        assert torch.equal(grads[0], grads[3])
    else:
        _close(grads[0].cpu().numpy(), grads[3].cpu().numpy())


@pytest.mark.parametrize('fn', [F.roi_pooling_2d, F.crop_and_resize], ids=['pooling', 'resize'])
def test_no_rois_and_an_image_without_rois(dev, fn):
    rng = np.random.RandomState(2)
    x = rng.standard_normal((3, 8, 9, 10)).astype(np.float32)
    y, gx = _run(fn, x, np.zeros((0, 5), np.float32), 7, 7, 1 / 16., np.zeros((0, 8, 7, 7), np.float32))
    assert y.shape == (0, 8, 7, 7) and gx.shape == x.shape and not gx.any()
    # image 1 has no RoI: its gradient is zero, the others match the restatement
    rois = np.array([[2, 8, 8, 100, 90], [0, 0, 0, 150, 140], [2, 30, 10, 60, 130]], np.float32)
    gy = rng.standard_normal((3, 8, 7, 7)).astype(np.float32)
    y, gx = _run(fn, x, rois, 7, 7, 1 / 16., gy)
    if fn is F.roi_pooling_2d:
        y_ref, am = ref.roi_pooling_2d_fwd(x, rois, 7, 7, 1 / 16.)
        gx_ref = ref.roi_pooling_2d_bwd(gy, am, rois, x.shape)
        assert np.array_equal(gx, gx_ref)
    else:
        y_ref = ref.crop_and_resize_fwd(x, rois, 7, 7, 1 / 16.)
        gx_ref = ref.crop_and_resize_bwd(gy, rois, x.shape, 1 / 16.)
        _close(gx, gx_ref)
    assert np.array_equal(y, y_ref) and not gx[1].any()


def test_crop_and_resize_output_rows_in_batch_order(dev):
    rng = np.random.RandomState(5)
    x = rng.standard_normal((2, 4, 9, 10)).astype(np.float32)
    rois = np.array([[1, 0, 0, 80, 90], [0, 10, 10, 60, 60], [1, 20, 30, 150, 140],
                     [0, 0, 0, 150, 140]], np.float32)
    y, _ = _run(F.crop_and_resize, x, rois, 5, 5, 1 / 16.)
    y_ref = ref.crop_and_resize_fwd(x, rois, 5, 5, 1 / 16.)
    assert np.array_equal(y, y_ref)
    one = [_run(F.crop_and_resize, x, rois[i:i + 1], 5, 5, 1 / 16.)[0][0] for i in range(4)]
    for row, i in enumerate([1, 3, 0, 2]):                    # image 0's RoIs, then image 1's
        assert np.array_equal(y[row], one[i])


@pytest.mark.parametrize('fn', [F.roi_pooling_2d, F.crop_and_resize], ids=['pooling', 'resize'])
def test_headline_shape(dev, fn):
    """(2, 1024, 50, 84) map, 1024 proposal-shaped RoIs, 14 x 14 bins, bin_stride 2; the
    restatement is checked on a seeded subset of RoIs (the full backward on the device, the
    subset's backward on its own)."""
    rng = np.random.RandomState(9)
    N, C, H, W = 2, 1024, 50, 84
    x = rng.standard_normal((N, C, H, W)).astype(np.float32)
    rois = _rois(rng, 1017, N, H, W, 1 / 16.)
    rois = rois[np.argsort(rois[:, 0], kind='stable')]
    dev_ = torch.device('cuda:0')
    xt = torch.tensor(x, device=dev_)
    rt = torch.tensor(rois, device=dev_)
    y = fn(xt, rt, 14, 14, 1 / 16., bin_stride=2)
    torch.cuda.synchronize()
    pick = np.sort(rng.choice(len(rois), 12, replace=False))
    sub = rois[pick]
    if fn is F.roi_pooling_2d:
        y_ref = ref.roi_pooling_2d_fwd(x, sub, 14, 14, 1 / 16.)[0]
    else:
        y_ref = ref.crop_and_resize_fwd(x, sub, 14, 14, 1 / 16.)
    assert np.array_equal(y[pick].cpu().numpy(), ref.strided(y_ref, 2))
    # backward of the subset through the device path against the restatement
    gy = rng.standard_normal((len(sub), C, 7, 7)).astype(np.float32)
    xg = xt.clone().requires_grad_(True)
    fn(xg, torch.tensor(sub, device=dev_), 14, 14, 1 / 16., bin_stride=2).backward(
        torch.tensor(gy, device=dev_))
    gfull = np.zeros(y_ref.shape, np.float32)
    gfull[:, :, ::2, ::2] = gy
    if fn is F.roi_pooling_2d:
        am = ref.roi_pooling_2d_fwd(x, sub, 14, 14, 1 / 16.)[1]
        assert np.array_equal(xg.grad.cpu().numpy(), ref.roi_pooling_2d_bwd(gfull, am, sub, x.shape))
    else:
        _close(xg.grad.cpu().numpy(), ref.crop_and_resize_bwd(gfull, sub, x.shape, 1 / 16.))
    # the full backward runs and is bit-reproducible
    g = torch.randn_like(y)
    outs = []
    for _ in range(2):
        xg = xt.clone().requires_grad_(True)
        fn(xg, rt, 14, 14, 1 / 16., bin_stride=2).backward(g)
        outs.append(xg.grad)
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
