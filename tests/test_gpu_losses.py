"""Loss / optimizer kernels vs the NumPy oracle, and the loss kernels vs the float64 references
of tests/launch_ref.py under the bounds derived there (units of 2^-24, from the kernels' own
arithmetic): sizes around every grid and lane boundary, logits where log1pf(expf(-|x|)), sigmoidf
and the max-subtracted softmax exist to matter, strided and padded buffers, the no-gradient path,
shared scratch.  Each comparison prints its worst |got - ref| / bound; the module prints the worst
per group at the end (run with -s)."""
import collections

import numpy as np
import pytest
import torch

import launch_ref as L
from oracle import np_ref
from chainer_mask_rcnn_amd import functions as F
from chainer_mask_rcnn_amd import _lib

pytestmark = pytest.mark.gpu

F64 = torch.float64
FLT_MAX = float(np.finfo(np.float32).max)
WORST = collections.OrderedDict()


def _t(a, dev, grad=False):
    t = torch.tensor(a, device=dev)
    if grad:
        t.requires_grad_(True)
    return t


@pytest.fixture(scope='module', autouse=True)
def _worst_ratios():
    yield
    print('\n== worst |got - ref| / bound per group ==')
    for k, (r, n) in WORST.items():
        print('%-44s %6d comparisons %10.4g' % (k, n, r))


def _within(group, got, ref, tol, what=''):
    """got within tol of the float64 ref (launch_ref.tol_ratio <= 1), recorded under `group`."""
    r = L.tol_ratio(got.detach(), ref, tol)
    w = WORST.setdefault(group, [0., 0])
    w[0], w[1] = max(w[0], r), w[1] + 1
    print('%s %s: %.4g of the bound' % (group, what, r))
    assert r <= 1., '%s %s: %.4g of the bound' % (group, what, r)


def _sce(dev, x, t, group, what=''):
    """sigmoid CE through the wrapper against the reference; returns (loss, gx)."""
    xt = _t(np.asarray(x, np.float32), dev, True)
    tt = _t(np.asarray(t, np.int32), dev)
    loss = F.sigmoid_cross_entropy(xt, tt)
    loss.backward()
    l_ref, g_ref, l_tol, g_tol = L.sigmoid_ce(xt.detach().to(F64), tt)
    _within(group, loss, l_ref, l_tol, 'loss ' + what)
    _within(group, xt.grad, g_ref, g_tol, 'gx ' + what)
    return loss.detach(), xt.grad


def _sce_input(n, seed, ignore=True):
    """N(0, 3) logits, targets in {-1, 0, 1}; the first and the last element are valid and carry
    about three times the mean element loss, so that a lost head or tail shows."""
    rng = np.random.RandomState(seed)
    x = (rng.standard_normal(n) * 3).astype(np.float32)
    t = rng.randint(-1 if ignore else 0, 2, n).astype(np.int32)
    if n:
        x[0] = x[-1] = -4.
        t[0] = t[-1] = 1
    return x, t


# parts_for saturates at n > 262 144, grid_for at n > 524 288; 2^24 + 3 gives every thread of the
# first pass an fp32 run of 256 positive terms, where the accumulation error is largest
FLAT_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 300, 1023, 1024, 1025, 128520, 262144, 262145,
              524288, 524289]


@pytest.mark.parametrize('n', FLAT_SIZES + [2 ** 24 + 3])
def test_sigmoid_cross_entropy(dev, n):
    x, t = _sce_input(n, n, ignore=n < 2 ** 24)
    xt = _t(x, dev, True)
    loss = F.sigmoid_cross_entropy(xt, _t(t, dev))
    loss.backward()
    l_ref, g_ref = np_ref.sigmoid_cross_entropy(x, t)
    np.testing.assert_allclose(loss.item(), l_ref, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(xt.grad.cpu().numpy(), g_ref, rtol=1e-4, atol=1e-8)
    l64, g64, l_tol, g_tol = L.sigmoid_ce(xt.detach().to(F64), _t(t, dev))
    if n:
        el = L._sce_terms(xt.detach().to(F64), _t(t, dev))[1]
        assert min(float(el[0]), float(el[-1])) >= float(l64)       # head and tail >= the mean
    _within('sigmoid CE sizes', loss, l64, l_tol, 'loss n=%d' % n)
    _within('sigmoid CE sizes', xt.grad, g64, g_tol, 'gx n=%d' % n)


def test_sigmoid_cross_entropy_all_ignored(dev):
    xt = _t(np.ones(10, np.float32), dev, True)
    loss = F.sigmoid_cross_entropy(xt, _t(np.full(10, -1, np.int32), dev))
    loss.backward()
    assert loss.item() == 0. and float(xt.grad.abs().sum()) == 0.


def _mask_check(xt, label_t, t_t, loss, group, what):
    """loss and xt.grad (logical (R, Kc, M, M)) against the reference on (R, HW, Kc) rows."""
    R, Kc, M, _ = xt.shape
    rows = xt.detach().permute(0, 2, 3, 1).reshape(R, M * M, Kc).to(F64)
    l64, g64, l_tol, g_tol = L.mask_sigmoid_ce(rows, label_t, t_t.reshape(R, M * M))
    _within(group, loss, l64, l_tol, 'loss ' + what)
    _within(group, xt.grad.permute(0, 2, 3, 1).reshape(R, M * M, Kc), g64, g_tol, 'gx ' + what)
    return l64, g64


def test_mask_sigmoid_cross_entropy(dev):
    rng = np.random.RandomState(1)
    R, Kc, M = 64, 80, 14
    x = rng.standard_normal((R, Kc, M, M)).astype(np.float32)
    label = rng.randint(0, Kc + 1, R).astype(np.int32)      # 0 = background
    t = rng.randint(0, 2, (R, M, M)).astype(np.int32)
    t[label == 0] = -1
    xt = _t(x, dev, True)
    loss = F.mask_sigmoid_cross_entropy(xt, _t(label, dev), _t(t, dev))
    loss.backward()
    sel = x[np.arange(R), label - 1]
    l_ref, g_sel = np_ref.sigmoid_cross_entropy(sel, t)
    g_ref = np.zeros_like(x)
    g_ref[np.arange(R), label - 1] = g_sel
    np.testing.assert_allclose(loss.item(), l_ref, rtol=1e-4)
    np.testing.assert_allclose(xt.grad.cpu().numpy(), g_ref, rtol=1e-4, atol=1e-8)
    _mask_check(xt, _t(label, dev), _t(t, dev), loss, 'mask CE sizes', 'R=64 Kc=80 M=14 oracle case')


def test_softmax_cross_entropy_and_softmax(dev):
    rng = np.random.RandomState(2)
    x = (rng.standard_normal((1024, 81)) * 2).astype(np.float32)
    t = rng.randint(-1, 81, 1024).astype(np.int32)
    xt = _t(x, dev, True)
    loss = F.softmax_cross_entropy(xt, _t(t, dev))
    loss.backward()
    l_ref, g_ref = np_ref.softmax_cross_entropy(x, t)
    np.testing.assert_allclose(loss.item(), l_ref, rtol=1e-4)
    np.testing.assert_allclose(xt.grad.cpu().numpy(), g_ref, rtol=1e-4, atol=1e-8)
    l64, g64, l_tol, g_tol = L.softmax_ce(xt.detach().to(F64), _t(t, dev))
    _within('softmax CE sizes', loss, l64, l_tol, 'loss oracle case')
    _within('softmax CE sizes', xt.grad, g64, g_tol, 'gx oracle case')
    # strided view (fused head output)
    big = np.zeros((1024, 408), np.float32)
    big[:, 324:405] = x
    p = F.softmax(_t(big, dev)[:, 324:405])
    e = np.exp(x - x.max(1, keepdims=True))
    np.testing.assert_allclose(p.cpu().numpy(), e / e.sum(1, keepdims=True), rtol=1e-4, atol=1e-7)
    y64, y_tol = L.softmax(_t(x, dev).to(F64))
    _within('softmax sizes', p, y64, y_tol, 'y strided oracle case')


def _sl1(dev, pred, gt, label, sigma, group, cls=None, what=''):
    """smooth L1 through the wrapper against the reference; returns (loss, gx)."""
    pt = _t(np.asarray(pred, np.float32), dev, True)
    gt_t, lab_t = _t(np.asarray(gt, np.float32), dev), _t(np.asarray(label, np.int32), dev)
    cls_t = None if cls is None else _t(np.asarray(cls, np.int32), dev)
    loss = F.fast_rcnn_loc_loss(pt, gt_t, lab_t, sigma, cls=cls_t)
    loss.backward()
    l_ref, g_ref, l_tol, g_tol = L.smooth_l1(pt.detach().to(F64), cls_t, gt_t.to(F64), lab_t, sigma)
    _within(group, loss, l_ref, l_tol, 'loss ' + what)
    _within(group, pt.grad, g_ref, g_tol, 'gx ' + what)
    return loss.detach(), pt.grad


def _sl1_input(n, seed):
    """Labels in {-1, 0, 1, 2}; the first and the last row are foreground with |d| = 3 in every
    coordinate (several times the mean element)."""
    rng = np.random.RandomState(seed)
    pred = rng.standard_normal((n, 4)).astype(np.float32)
    gt = rng.standard_normal((n, 4)).astype(np.float32)
    label = rng.randint(-1, 3, n).astype(np.int32)
    if n:
        label[0] = label[-1] = 1
        pred[0] = gt[0] + 3.
        pred[-1] = gt[-1] - 3.
    return pred, gt, label


@pytest.mark.parametrize('sigma', [1., 3.])
def test_fast_rcnn_loc_loss(dev, sigma):
    n = 5000
    pred, gt, label = _sl1_input(n, 3)
    pt = _t(pred, dev, True)
    loss = F.fast_rcnn_loc_loss(pt, _t(gt, dev), _t(label, dev), sigma)
    loss.backward()
    l_ref, g_ref = np_ref.fast_rcnn_loc_loss(pred, gt, label, sigma)
    np.testing.assert_allclose(loss.item(), l_ref, rtol=1e-4)
    np.testing.assert_allclose(pt.grad.cpu().numpy(), g_ref, rtol=1e-4, atol=1e-8)
    l64, g64, l_tol, g_tol = L.smooth_l1(pt.detach().to(F64), None, _t(gt, dev).to(F64),
                                         _t(label, dev), sigma)
    _within('smooth L1 sizes', loss, l64, l_tol, 'loss n=%d sigma=%g' % (n, sigma))
    _within('smooth L1 sizes', pt.grad, g64, g_tol, 'gx n=%d sigma=%g' % (n, sigma))


def test_fast_rcnn_loc_loss_class_select(dev):
    rng = np.random.RandomState(4)
    n, ncls = 512, 81
    pred = rng.standard_normal((n, ncls * 4)).astype(np.float32)
    gt = rng.standard_normal((n, 4)).astype(np.float32)
    label = rng.randint(0, ncls, n).astype(np.int32)
    pt = _t(pred, dev, True)
    loss = F.fast_rcnn_loc_loss(pt, _t(gt, dev), _t(label, dev), 1., cls=_t(label, dev))
    loss.backward()
    sel = pred.reshape(n, ncls, 4)[np.arange(n), label]
    l_ref, g_sel = np_ref.fast_rcnn_loc_loss(sel, gt, label, 1.)
    g_ref = np.zeros((n, ncls, 4), np.float32)
    g_ref[np.arange(n), label] = g_sel
    np.testing.assert_allclose(loss.item(), l_ref, rtol=1e-4)
    np.testing.assert_allclose(pt.grad.cpu().numpy(), g_ref.reshape(n, -1), rtol=1e-4, atol=1e-8)
    l64, g64, l_tol, g_tol = L.smooth_l1(pt.detach().to(F64), _t(label, dev), _t(gt, dev).to(F64),
                                         _t(label, dev), 1.)
    _within('smooth L1 class select', loss, l64, l_tol, 'loss oracle case')
    _within('smooth L1 class select', pt.grad, g64, g_tol, 'gx oracle case')


def test_sgd_momentum_wd(dev):
    rng = np.random.RandomState(5)
    n = 1000003
    p = rng.standard_normal(n).astype(np.float32)
    g = rng.standard_normal(n).astype(np.float32)
    v = rng.standard_normal(n).astype(np.float32)
    pt, gt, vt = _t(p, dev), _t(g, dev), _t(v, dev)
    _lib.call('mrcnn_sgd_momentum_wd', _lib.ptr(pt), _lib.ptr(gt), _lib.ptr(vt), n,
              0.02, 0.9, 1e-4, 1.0, _lib.stream_ptr())
    p2, v2 = np_ref.momentum_sgd_wd(p, g, v, 0.02)
    np.testing.assert_allclose(pt.cpu().numpy(), p2, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(vt.cpu().numpy(), v2, rtol=1e-5, atol=1e-6)


def test_loc_loss_matches_reference_function_fixture(dev, golden_dir):
    import os
    d = np.load(os.path.join(golden_dir, 'loc_loss.npz'))
    for sigma, key in ((3., 'loss_sigma3'), (1., 'loss_sigma1')):
        loss = F.fast_rcnn_loc_loss(_t(d['pred'], dev), _t(d['gt'], dev), _t(d['label'], dev), sigma)
        np.testing.assert_allclose(loss.item(), float(d[key]), rtol=1e-5)


# ---- the edge matrix ---------------------------------------------------------------------------

# every logit where a naive log(1 + exp(x)) or 1 / (1 + exp(-x)) breaks: products with denormal
# results, the fp32 saturation of sigmoid (17), of sigmoid - 1 (20), expf's overflow threshold
# (88.72) from both sides, the flush of expf(-x) to zero (104), and far beyond
SCE_LOGITS = [0., 1e-30, 1e-4, 17., 20., 88., 89., 104., 1e4]


def _sce_value_input(seed):
    """Every +-logit of SCE_LOGITS with every target in {0, 1, -1}, spread among ordinary logits."""
    x, t = _sce_input(600, seed)
    special = [(sg * v, tt) for v in SCE_LOGITS for sg in (1., -1.) for tt in (0, 1, -1)]
    pos = np.random.RandomState(seed + 1).choice(np.arange(1, 599), len(special), replace=False)
    for p, (v, tt) in zip(pos, special):
        x[p], t[p] = v, tt
    return x, t


def test_sigmoid_cross_entropy_extreme_logits(dev):
    x, t = _sce_value_input(40)
    loss, gx = _sce(dev, x, t, 'sigmoid CE values', 'mixed to 1e4')
    assert torch.isfinite(loss) and torch.isfinite(gx).all()
    # sigmoidf saturates: the gradient of a confident, correct element is exactly 0 or tiny, never NaN
    assert float(gx.abs().max()) <= (1. + 2 * L.U) / int((t != -1).sum())


@pytest.mark.parametrize('n', [1, 301])
@pytest.mark.parametrize('x0,t0', [(FLT_MAX, 0), (-FLT_MAX, 1), (FLT_MAX, 1), (-FLT_MAX, 0),
                                   (FLT_MAX, -1), (-FLT_MAX, -1)])
def test_sigmoid_cross_entropy_flt_max(dev, n, x0, t0):
    """One element at +-FLT_MAX: an element loss of FLT_MAX (wrong side) or 0 (right side, or
    ignored).  The expected loss is the float64 reference rounded to fp32 (tol_ratio accepts it)."""
    x, t = _sce_input(n, 41)
    x[n // 2], t[n // 2] = x0, t0
    loss, gx = _sce(dev, x, t, 'sigmoid CE values', 'n=%d x=%g t=%d' % (n, x0, t0))
    assert torch.isfinite(loss) and torch.isfinite(gx).all()
    if t0 != -1:
        want = (1. if x0 > 0 else 0.) - t0                 # sigmoid is exactly 0 or 1 there
        count = int((t != -1).sum())
        assert abs(float(gx[n // 2]) * count - want) <= 4 * L.U


def test_sigmoid_cross_entropy_permutation(dev):
    """The partials are reduced in a fixed order, so a permutation of (x, t) changes the roundings
    only: it stays inside the loss bound of the same reference."""
    x, t = _sce_input(128520, 42)
    l0, _ = _sce(dev, x, t, 'sigmoid CE paths', 'identity order')
    perm = np.random.RandomState(43).permutation(len(x))
    l1, _ = _sce(dev, x[perm], t[perm], 'sigmoid CE paths', 'permuted')
    l_ref, _, l_tol, _ = L.sigmoid_ce(_t(x, dev).to(F64), _t(t, dev))
    _within('sigmoid CE paths', l1, l_ref, l_tol, 'permuted loss vs the unpermuted reference')


def test_rpn_label_distribution(dev):
    """The RPN's real shape: 128 520 anchors, 256 sampled (128 foreground), the rest ignored."""
    rng = np.random.RandomState(44)
    n = 128520
    label = np.full(n, -1, np.int32)
    pick = rng.choice(np.arange(1, n - 1), 254, replace=False)
    label[pick[:126]] = 1
    label[pick[126:]] = 0
    label[0] = label[-1] = 1
    x = (rng.standard_normal(n) * 3).astype(np.float32)
    x[0] = x[-1] = -4.
    _sce(dev, x, label, 'RPN label distribution', 'sigmoid CE 256 of 128520')
    pred, gt, _ = _sl1_input(n, 45)
    _sl1(dev, pred, gt, label, 3., 'RPN label distribution', what='smooth L1 256 of 128520')


# ---- softmax CE / softmax ------------------------------------------------------------------------

ROW_SIZES = [(R, 81) for R in (0, 1, 3, 4, 5, 1023, 1024, 1025, 4099)] + \
            [(1025, c) for c in (1, 2, 21, 63, 64, 65, 128, 129, 1000)]


def _rows_input(R, ncls, seed):
    """N(0, 2) logits, targets in -1 .. ncls - 1; the first and the last row are valid and target
    their least likely class (more than the mean row loss)."""
    rng = np.random.RandomState(seed)
    x = (rng.standard_normal((R, ncls)) * 2).astype(np.float32)
    t = rng.randint(-1, ncls, R).astype(np.int32)
    if R:
        t[0], t[-1] = x[0].argmin(), x[-1].argmin()
    return x, t


def _smce(dev, x, t, group, what=''):
    xt = _t(np.asarray(x, np.float32), dev, True)
    tt = _t(np.asarray(t, np.int32), dev)
    loss = F.softmax_cross_entropy(xt, tt)
    loss.backward()
    l_ref, g_ref, l_tol, g_tol = L.softmax_ce(xt.detach().to(F64), tt)
    _within(group, loss, l_ref, l_tol, 'loss ' + what)
    _within(group, xt.grad, g_ref, g_tol, 'gx ' + what)
    return loss.detach(), xt.grad


def _softmax(dev, x, group, what=''):
    xt = _t(np.asarray(x, np.float32), dev)
    y = F.softmax(xt)
    y_ref, y_tol = L.softmax(xt.to(F64))
    _within(group, y, y_ref, y_tol, 'y ' + what)
    return y


@pytest.mark.parametrize('R,ncls', ROW_SIZES)
def test_softmax_cross_entropy_sizes(dev, R, ncls):
    """R > 1024 runs the row grid-stride loop of the first pass; ncls around 64 and 128 the lane
    loop's tail."""
    x, t = _rows_input(R, ncls, 50 + R + ncls)
    loss, gx = _smce(dev, x, t, 'softmax CE sizes', 'R=%d ncls=%d' % (R, ncls))
    assert torch.isfinite(loss) and tuple(gx.shape) == (R, ncls)


@pytest.mark.parametrize('R,ncls', ROW_SIZES + [(8192, 81), (8193, 81), (20001, 81)])
def test_softmax_sizes(dev, R, ncls):
    """R > 8192 runs softmax_kernel's row grid-stride loop."""
    x, _ = _rows_input(R, ncls, 60 + R + ncls)
    y = _softmax(dev, x, 'softmax sizes', 'R=%d ncls=%d' % (R, ncls))
    assert tuple(y.shape) == (R, ncls)
    if R:
        assert float((y.sum(1) - 1).abs().max()) < 1e-5


def _row_value_inputs(ncls, seed):
    """name -> (x, t): 64 rows each."""
    rng = np.random.RandomState(seed)
    R = 64
    base = (rng.standard_normal((R, ncls)) * 2).astype(np.float32)
    t = rng.randint(-1, ncls, R).astype(np.int32)
    t[0], t[-1], t[1], t[2] = base[0].argmin(), base[-1].argmin(), 0, ncls - 1
    out = collections.OrderedDict()
    for off in (1e4, -1e4, 3e38, -3e38):
        out['offset %g' % off] = (base + np.float32(off), t)          # added in fp32: quantised
    dom = base.copy()
    hot = rng.randint(0, ncls, R)
    dom[np.arange(R), hot] = dom.max(1) + 200.                       # the others underflow to 0
    td = t.copy()
    td[::2] = hot[::2]                                               # half the rows target it
    out['dominant logit'] = (dom, td)
    eq = np.repeat((rng.standard_normal((R, 1)) * 5).astype(np.float32), ncls, 1)
    out['all-equal rows'] = (eq, t)
    ninf = base.copy()
    tv = np.where(t < 0, 0, t)
    for r in range(R):
        k = rng.choice(np.setdiff1d(np.arange(ncls), [tv[r]]), ncls // 3, replace=False)
        ninf[r, k] = -np.inf
    out['-inf off the target'] = (ninf, t)
    return out


@pytest.mark.parametrize('ncls', [81, 21])
def test_softmax_cross_entropy_extreme_logits(dev, ncls):
    for name, (x, t) in _row_value_inputs(ncls, 70 + ncls).items():
        assert not np.isnan(x).any() and not np.isposinf(x).any()
        loss, gx = _smce(dev, x, t, 'softmax CE values', '%s ncls=%d' % (name, ncls))
        assert torch.isfinite(loss) and torch.isfinite(gx).all(), name
        y = _softmax(dev, x, 'softmax values', '%s ncls=%d' % (name, ncls))
        assert torch.isfinite(y).all(), name
        if name == 'dominant logit':
            # a row that targets its dominant logit costs exactly nothing and has zero gradient
            xt = _t(x[::2], dev, True)
            l_dom = F.softmax_cross_entropy(xt, _t(t[::2], dev))
            l_dom.backward()
            assert l_dom.item() == 0. and float(xt.grad.abs().max()) == 0.
        if name == '-inf off the target':
            assert float(y[torch.tensor(np.isinf(x), device=dev)].abs().max()) == 0.
            assert float(gx[torch.tensor(np.isinf(x), device=dev)].abs().max()) == 0.
        if name == 'all-equal rows':
            assert float((y - 1. / ncls).abs().max()) <= 4 * L.U


@pytest.mark.parametrize('off', [324, 1])
def test_softmax_cross_entropy_strided_view_with_gradient(dev, off):
    """The class scores as the fused cls_loc / score layer leaves them: columns off .. off + 81 of
    408-wide rows (off = 1: a base address that is not 16-byte aligned)."""
    x, t = _rows_input(1024, 81, 80 + off)
    buf = np.random.RandomState(81).standard_normal((1024, 408)).astype(np.float32)
    buf[:, off:off + 81] = x
    bt = _t(buf, dev, True)
    view = bt[:, off:off + 81]
    assert view.stride(0) == 408
    loss = F.softmax_cross_entropy(view, _t(t, dev))
    loss.backward()
    l_ref, g_ref, l_tol, g_tol = L.softmax_ce(_t(x, dev).to(F64), _t(t, dev))
    _within('softmax CE paths', loss, l_ref, l_tol, 'loss strided off=%d' % off)
    _within('softmax CE paths', bt.grad[:, off:off + 81], g_ref, g_tol, 'gx strided off=%d' % off)
    outside = bt.grad.clone()
    outside[:, off:off + 81] = 0
    assert float(outside.abs().max()) == 0.
    # the same numbers as the contiguous copy, bit for bit
    xt = _t(x, dev, True)
    l2 = F.softmax_cross_entropy(xt, _t(t, dev))
    l2.backward()
    assert torch.equal(l2, loss) and torch.equal(xt.grad, bt.grad[:, off:off + 81])


def test_softmax_padded_outputs_direct(dev, monkeypatch):
    """ldg / ldy wider than ncls through the library entry points: the padding columns keep their
    contents, the values match the contiguous call bit for bit.  Run under the launch checker, whose
    own padding comparison no wrapper call reaches."""
    chk = L.LaunchChecker()
    chk.install(monkeypatch)
    R, ncls, ld = 1025, 81, 96
    x, t = _rows_input(R, ncls, 82)
    xt, tt = _t(x, dev), _t(t, dev)
    lib = _lib.load()
    ws = _lib.workspace(lib.mrcnn_loss_workspace_bytes(R), dev, 'loss')
    loss = torch.empty((), device=dev)
    gx = torch.full((R, ld), 7., device=dev)
    _lib.call('mrcnn_softmax_ce', _lib.ptr(xt), ncls, _lib.ptr(tt), R, ncls, _lib.ptr(loss),
              _lib.ptr(gx), ld, _lib.ptr(ws), _lib.stream_ptr())
    l_ref, g_ref, l_tol, g_tol = L.softmax_ce(xt.to(F64), tt)
    _within('softmax CE paths', loss, l_ref, l_tol, 'loss ldg=96')
    _within('softmax CE paths', gx[:, :ncls], g_ref, g_tol, 'gx ldg=96')
    assert bool((gx[:, ncls:] == 7.).all())
    y = torch.full((R, ld), 7., device=dev)
    _lib.call('mrcnn_softmax', _lib.ptr(xt), ncls, _lib.ptr(y), ld, R, ncls, _lib.stream_ptr())
    y_ref, y_tol = L.softmax(xt.to(F64))
    _within('softmax sizes', y[:, :ncls], y_ref, y_tol, 'y ldy=96')
    assert bool((y[:, ncls:] == 7.).all())
    assert torch.equal(y[:, :ncls], F.softmax(xt))
    # gx = NULL: the same loss, bit for bit
    loss0 = torch.empty((), device=dev)
    _lib.call('mrcnn_softmax_ce', _lib.ptr(xt), ncls, _lib.ptr(tt), R, ncls, _lib.ptr(loss0),
              None, ncls, _lib.ptr(ws), _lib.stream_ptr())
    assert torch.equal(loss0, loss)
    chk.assert_clean()
    assert chk.stats['mrcnn_softmax_ce'][0] == 4 and chk.stats['mrcnn_softmax'][0] == 3, chk.table()


# ---- mask loss -----------------------------------------------------------------------------------

def _mask_input(R, Kc, M, seed):
    """Labels cover 1, Kc and 0; background rows (label 0) keep non-ignored targets on odd rows, so
    the wrap of label - 1 to channel Kc - 1 is observed; the first and the last RoI are foreground,
    wrong everywhere by a logit of 4."""
    rng = np.random.RandomState(seed)
    x = rng.standard_normal((R, Kc, M, M)).astype(np.float32)
    label = rng.randint(0, Kc + 1, R).astype(np.int32)
    t = rng.randint(0, 2, (R, M, M)).astype(np.int32)
    if R >= 4:
        label[1], label[2], label[3] = 1, Kc, 0
    bg = np.nonzero(label == 0)[0]
    t[bg[bg % 2 == 0]] = -1
    t[rng.random_sample(t.shape) < 0.1] = -1
    if R:
        label[0], label[-1] = Kc, 1
        for r in (0, -1):
            x[r, label[r] - 1] = -4.
            t[r] = 1
    return x, label, t


@pytest.mark.parametrize('layout', ['nchw', 'channels_last'])
@pytest.mark.parametrize('R,Kc,M', [(0, 80, 14), (1, 1, 14), (64, 80, 14), (37, 20, 28),
                                    (1024, 80, 14)])
def test_mask_sigmoid_cross_entropy_sizes(dev, R, Kc, M, layout):
    x, label, t = _mask_input(R, Kc, M, 90 + R)
    xt = torch.tensor(x, device=dev)
    if layout == 'channels_last':
        xt = xt.contiguous(memory_format=torch.channels_last)
    xt.requires_grad_(True)
    lt, tt = _t(label, dev), _t(t, dev)
    loss = F.mask_sigmoid_cross_entropy(xt, lt, tt)
    loss.backward()
    what = 'R=%d Kc=%d M=%d %s' % (R, Kc, M, layout)
    _mask_check(xt, lt, tt, loss, 'mask CE sizes', what)
    # NumPy's own indexing, negative index included, picks the same channels
    if R:
        sel = x[np.arange(R), label - 1]
        l_np, g_sel = np_ref.sigmoid_cross_entropy(sel, t)
        np.testing.assert_allclose(loss.item(), l_np, rtol=1e-5)
        g = xt.grad.cpu().numpy()
        nz = np.zeros((R, Kc), bool)
        nz[np.arange(R), label - 1] = True
        assert not g[~nz].any()
        bg = np.nonzero((label == 0) & (t.reshape(R, -1) != -1).any(1))[0]
        if Kc > 1 and R >= 4:
            assert len(bg) and all(np.abs(g[r, Kc - 1]).max() > 0 for r in bg)


def test_mask_sigmoid_cross_entropy_background_row_uses_last_channel(dev):
    """label 0 with non-ignored targets: channel Kc - 1, as roi_masks[arange(n), labels - 1]."""
    R, Kc, M = 3, 5, 14
    rng = np.random.RandomState(95)
    x = rng.standard_normal((R, Kc, M, M)).astype(np.float32)
    t = rng.randint(0, 2, (R, M, M)).astype(np.int32)
    label = np.zeros(R, np.int32)
    xt = _t(x, dev, True)
    loss = F.mask_sigmoid_cross_entropy(xt, _t(label, dev), _t(t, dev))
    loss.backward()
    # the same loss as a plain sigmoid CE on the last channel, bit for bit in value order
    last = _t(np.ascontiguousarray(x[:, Kc - 1]), dev, True)
    l2 = F.sigmoid_cross_entropy(last, _t(t, dev))
    l2.backward()
    assert torch.equal(loss, l2)
    assert torch.equal(xt.grad[:, Kc - 1], last.grad)
    assert float(xt.grad[:, :Kc - 1].abs().max()) == 0.
    _mask_check(xt, _t(label, dev), _t(t, dev), loss, 'mask CE sizes', 'all background, Kc=5')


def test_mask_sigmoid_cross_entropy_extreme_logits(dev):
    xs, ts = _sce_value_input(96)                          # 600 elements
    R, Kc, M = 4, 3, 14
    rng = np.random.RandomState(97)
    x = rng.standard_normal((R, Kc, M, M)).astype(np.float32)
    label = np.array([1, 3, 0, 2], np.int32)
    t = rng.randint(-1, 2, (R, M, M)).astype(np.int32)
    sel = x[np.arange(R), label - 1].reshape(-1)
    sel[:600] = xs
    t.reshape(-1)[:600] = ts
    x[np.arange(R), label - 1] = sel.reshape(R, M, M)
    xt = _t(x, dev, True)
    loss = F.mask_sigmoid_cross_entropy(xt, _t(label, dev), _t(t, dev))
    loss.backward()
    assert torch.isfinite(loss) and torch.isfinite(xt.grad).all()
    _mask_check(xt, _t(label, dev), _t(t, dev), loss, 'mask CE values', 'mixed to 1e4')
    for x0, t0 in ((FLT_MAX, 0), (-FLT_MAX, 1), (FLT_MAX, 1), (-FLT_MAX, 0)):
        x1 = rng.standard_normal((R, Kc, M, M)).astype(np.float32)
        t1 = rng.randint(-1, 2, (R, M, M)).astype(np.int32)
        x1[1, label[1] - 1, 3, 5], t1[1, 3, 5] = x0, t0
        xt = _t(x1, dev, True)
        loss = F.mask_sigmoid_cross_entropy(xt, _t(label, dev), _t(t1, dev))
        loss.backward()
        assert torch.isfinite(loss) and torch.isfinite(xt.grad).all()
        _mask_check(xt, _t(label, dev), _t(t1, dev), loss, 'mask CE values', 'x=%g t=%d' % (x0, t0))


def test_mask_sigmoid_cross_entropy_foreground_subset(dev):
    """The train chain's foreground-only form (index_select of labels and targets by mask_rows, the
    mask branch run on those rows only) against the full form, whose background rows are ignored:
    the same loss and the same gradient rows, bit for bit; 34 foreground RoIs of 1024."""
    R, Kc, M = 1024, 80, 14
    rng = np.random.RandomState(98)
    x = rng.standard_normal((R, Kc, M, M)).astype(np.float32)
    label = np.zeros(R, np.int32)
    fg = np.sort(rng.choice(R, 34, replace=False))
    label[fg] = rng.randint(1, Kc + 1, 34)
    t = rng.randint(0, 2, (R, M, M)).astype(np.int32)
    t[label == 0] = -1
    lt, tt = _t(label, dev), _t(t, dev)
    rows = _t(fg.astype(np.int64), dev)
    full = _t(x, dev, True)
    l_full = F.mask_sigmoid_cross_entropy(full, lt, tt)
    l_full.backward()
    sub = _t(x[fg], dev, True)
    l_sub = F.mask_sigmoid_cross_entropy(sub, lt.index_select(0, rows), tt.index_select(0, rows))
    l_sub.backward()
    _mask_check(sub, lt.index_select(0, rows), tt.index_select(0, rows), l_sub, 'mask CE paths',
                '34 foreground rows')
    _mask_check(full, lt, tt, l_full, 'mask CE paths', '1024 rows, 34 foreground')
    assert torch.equal(full.grad[rows], sub.grad)
    bg = torch.ones(R, dtype=torch.bool, device=dev)
    bg[rows] = False
    assert float(full.grad[bg].abs().max()) == 0.
    # the two reduce different partial layouts, so the losses agree within their bounds of the
    # same float64 value rather than bit for bit
    l64, _, l_tol, _ = L.mask_sigmoid_ce(sub.detach().permute(0, 2, 3, 1).reshape(34, M * M, Kc).to(F64),
                                         lt.index_select(0, rows), tt.index_select(0, rows).reshape(34, -1))
    _within('mask CE paths', l_full, l64, l_tol, 'full-form loss vs the subset reference')


# ---- smooth L1 -----------------------------------------------------------------------------------

@pytest.mark.parametrize('n', [s for s in FLAT_SIZES if s != 300])
def test_fast_rcnn_loc_loss_sizes(dev, n):
    pred, gt, label = _sl1_input(n, 100 + n % 1000)
    sigma = 3. if n % 2 else 1.
    if n == 0:
        # nothing counted: 0 / 0, as the original's unguarded division (see the all-ignored test)
        loss = F.fast_rcnn_loc_loss(_t(pred, dev, True), _t(gt, dev), _t(label, dev), sigma)
        assert torch.isnan(loss)
        return
    loss, gx = _sl1(dev, pred, gt, label, sigma, 'smooth L1 sizes', what='n=%d sigma=%g' % (n, sigma))
    assert torch.isfinite(loss)
    assert float(gx[_t(label, dev) <= 0].abs().sum()) == 0.


@pytest.mark.parametrize('sigma', [1., 3.])
def test_fast_rcnn_loc_loss_switch_and_labels(dev, sigma):
    """Differences of exactly 0, exactly +-1 / sigma^2 and the two fp32 neighbours on each side, in
    rows of every label kind.  Value and gradient are continuous across the switch, so every
    element is compared."""
    thr = np.float32(1) / np.float32(sigma * sigma)
    near = [thr]
    for _ in range(2):
        near = [np.nextafter(near[0], np.float32(0))] + near + [np.nextafter(near[-1], np.float32(2))]
    d = np.array([0.] + [s * v for v in near for s in (1, -1)] + [0.5 * thr], np.float32)   # 12
    assert len(d) % 4 == 0
    block = d.reshape(-1, 4)
    labels = [1, 80, 0, -1, 1]
    pred = np.concatenate([block] * len(labels))
    label = np.repeat(np.array(labels, np.int32), len(block))
    gt = np.zeros_like(pred)                                # pred - gt is exactly d
    loss, gx = _sl1(dev, pred, gt, label, sigma, 'smooth L1 values', what='switch sigma=%g' % sigma)
    g = gx.cpu().numpy()
    count = int((label >= 0).sum())
    assert count == 4 * len(block)                          # label 0 counts, label -1 does not
    assert not g[label <= 0].any()
    fgd = label > 0
    assert not g[fgd][pred[fgd] == 0].any()                 # sign(0) = 0
    assert np.all(np.sign(g[fgd]) == np.sign(pred[fgd]))
    # with gt offset so that the difference is formed by a rounding subtraction
    gt2 = np.random.RandomState(110).standard_normal(pred.shape).astype(np.float32)
    _sl1(dev, pred + gt2, gt2, label, sigma, 'smooth L1 values', what='offset switch sigma=%g' % sigma)


@pytest.mark.parametrize('ncls', [81, 21])
def test_fast_rcnn_loc_loss_class_select_widths(dev, ncls):
    """4 x ncls wide rows, cls = 0 on background rows, labels in {-1, 0, 1 .. ncls - 1}: the columns
    outside the selected 4-vector are exactly zero (the reference's bound is 0 there)."""
    rng = np.random.RandomState(120 + ncls)
    n = 1025
    pred = rng.standard_normal((n, 4 * ncls)).astype(np.float32)
    gt = rng.standard_normal((n, 4)).astype(np.float32)
    label = rng.randint(-1, ncls, n).astype(np.int32)
    label[0], label[-1] = ncls - 1, 1
    cls = np.maximum(label, 0)
    for sigma in (1., 3.):
        loss, gx = _sl1(dev, pred, gt, label, sigma, 'smooth L1 class select', cls=cls,
                        what='ncls=%d sigma=%g' % (ncls, sigma))
        g = gx.cpu().numpy().reshape(n, ncls, 4)
        keep = np.zeros((n, ncls), bool)
        keep[np.arange(n), cls] = True
        assert not g[~keep].any() and not g[label <= 0].any()
        assert np.abs(g[label > 0][keep[label > 0]]).max() > 0


# ---- nothing counted -----------------------------------------------------------------------------

def test_softmax_cross_entropy_all_ignored(dev):
    xt = _t(np.random.RandomState(130).standard_normal((10, 81)).astype(np.float32), dev, True)
    loss = F.softmax_cross_entropy(xt, _t(np.full(10, -1, np.int32), dev))
    loss.backward()
    assert loss.item() == 0. and float(xt.grad.abs().sum()) == 0.


def test_mask_sigmoid_cross_entropy_all_ignored(dev):
    xt = _t(np.random.RandomState(131).standard_normal((6, 80, 14, 14)).astype(np.float32), dev, True)
    label = np.array([0, 3, 80, 0, 1, 7], np.int32)
    loss = F.mask_sigmoid_cross_entropy(xt, _t(label, dev), _t(np.full((6, 14, 14), -1, np.int32), dev))
    loss.backward()
    assert loss.item() == 0. and float(xt.grad.abs().sum()) == 0.


def test_fast_rcnn_loc_loss_all_ignored_is_nan(dev):
    """Every label -1: the normaliser #(label >= 0) is 0 and the original divides by it unguarded;
    the kernel keeps that (include/mrcnn_hip.h), unlike the two cross entropies above."""
    pred, gt, _ = _sl1_input(10, 132)
    label = np.full(10, -1, np.int32)
    pt = _t(pred, dev, True)
    loss = F.fast_rcnn_loc_loss(pt, _t(gt, dev), _t(label, dev), 3.)
    loss.backward()
    with np.errstate(invalid='ignore', divide='ignore'):
        l_np, _ = np_ref.fast_rcnn_loc_loss(pred, gt, label, 3.)
    assert np.isnan(l_np) and torch.isnan(loss)
    assert float(pt.grad.abs().sum()) == 0.
    l64 = L.smooth_l1(pt.detach().to(F64), None, _t(gt, dev).to(F64), _t(label, dev), 3.)[0]
    assert torch.isnan(l64)


# ---- paths: no gradient, upstream gradient, shared scratch, repeatability, streams --------------

def _five(dev, seed=140):
    """The five losses of the train chain at its sizes."""
    rng = np.random.RandomState(seed)
    xs, ts = _sce_input(128520, seed)
    pr, gr, lr = _sl1_input(128520, seed + 1)
    xc, tc = _rows_input(1024, 81, seed + 2)
    pc = rng.standard_normal((1024, 324)).astype(np.float32)
    gc = rng.standard_normal((1024, 4)).astype(np.float32)
    lc = np.maximum(tc, 0)
    xm, lm, tm = _mask_input(34, 80, 14, seed + 3)
    d = lambda a: _t(a, dev)
    ts_, gr_, lr_, tc_, gc_, lc_, lm_, tm_ = map(d, (ts, gr, lr, tc, gc, lc, lm, tm))
    def mask_ref(x):
        R, Kc, M, _ = x.shape
        l, g, lt, gt_ = L.mask_sigmoid_ce(x.permute(0, 2, 3, 1).reshape(R, M * M, Kc), lm_,
                                          tm_.reshape(R, M * M))
        back = lambda v: v.view(R, M, M, Kc).permute(0, 3, 1, 2)
        return l, back(g), lt, back(gt_)

    # name -> (the loss of the leaf, the leaf's array, the float64 reference of the leaf)
    return collections.OrderedDict([
        ('rpn_loc', (lambda p: F.fast_rcnn_loc_loss(p, gr_, lr_, 3.), pr,
                     lambda p: L.smooth_l1(p, None, gr_.to(F64), lr_, 3.))),
        ('rpn_cls', (lambda x: F.sigmoid_cross_entropy(x, ts_), xs,
                     lambda x: L.sigmoid_ce(x, ts_))),
        ('roi_loc', (lambda p: F.fast_rcnn_loc_loss(p, gc_, lc_, 1., cls=lc_), pc,
                     lambda p: L.smooth_l1(p, lc_, gc_.to(F64), lc_, 1.))),
        ('roi_cls', (lambda x: F.softmax_cross_entropy(x, tc_), xc,
                     lambda x: L.softmax_ce(x, tc_))),
        ('roi_mask', (lambda x: F.mask_sigmoid_cross_entropy(x, lm_, tm_), xm, mask_ref)),
    ])


def _alone(dev, fn, a, scale=None):
    leaf = _t(a, dev, True)
    loss = fn(leaf)
    (loss if scale is None else scale * loss).backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), leaf.grad.clone()


def test_losses_repeat_bit_identically_and_without_gradient(dev):
    for name, (fn, a, _) in _five(dev).items():
        l1, g1 = _alone(dev, fn, a)
        l2, g2 = _alone(dev, fn, a)
        assert torch.equal(l1, l2) and torch.equal(g1, g2), name
        with torch.no_grad():
            l0 = fn(_t(a, dev))                      # gx = NULL
        assert torch.equal(l0, l1), name
        assert bool(torch.isfinite(l1)), name


def test_losses_scale_the_upstream_gradient(dev):
    for name, (fn, a, _) in _five(dev).items():
        l1, g1 = _alone(dev, fn, a)
        l2, g2 = _alone(dev, fn, a, scale=0.25)
        assert torch.equal(l1, l2) and torch.equal(g2, g1 * 0.25), name


def test_five_losses_share_one_workspace(dev):
    """The train chain's sum: the five run back to back on one stream and one scratch buffer; each
    value and each gradient equals its result when run alone, bit for bit."""
    five = _five(dev)
    alone = {k: _alone(dev, fn, a) for k, (fn, a, _) in five.items()}
    leaves = {k: _t(a, dev, True) for k, (fn, a, _) in five.items()}
    losses = {k: five[k][0](leaves[k]) for k in five}
    total = sum(losses.values())
    total.backward()
    torch.cuda.synchronize()
    for k in five:
        assert torch.equal(losses[k].detach(), alone[k][0]), k
        assert torch.equal(leaves[k].grad, alone[k][1]), k
    want = sum(float(alone[k][0]) for k in five)
    assert abs(total.item() - want) <= 8 * L.U * abs(want)


def test_losses_on_two_streams(dev):
    """_lib.workspace keys its scratch by stream: the same losses issued on two side streams in
    turn, each compared with the float64 reference and, bit for bit, with the default stream's
    result.  One pass, synchronised between."""
    five = _five(dev, 150)
    base = {k: _alone(dev, fn, a) for k, (fn, a, _) in five.items()}
    torch.cuda.synchronize()
    for i, s in enumerate((torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev))):
        for k, (fn, a, ref) in five.items():
            leaf = _t(a, dev, True)
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                loss = fn(leaf)
                loss.backward()
            s.synchronize()
            torch.cuda.synchronize()
            l_ref, g_ref, l_tol, g_tol = ref(leaf.detach().to(F64))
            _within('streams', loss, l_ref, l_tol, '%s loss, side stream %d' % (k, i))
            _within('streams', leaf.grad, g_ref, g_tol, '%s gx, side stream %d' % (k, i))
            assert torch.equal(loss.detach(), base[k][0]), k
            assert torch.equal(leaf.grad, base[k][1]), k
