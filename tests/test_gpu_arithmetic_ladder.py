"""'split_bf16x2' and 'bf16x1' (functions.conv.set_gemm_arithmetic; NP = 2, 1 of conv_gemm_kernel) on the
device, over the cases of tests/arithmetic_ladder.py — shapes of tests/gemm_edge_cases.py that reach
every branch of the launch policy, every geometry instantiation on both tile sizes, W8, strided, stem and
deconvolution launches and the 128x128 weight gradient with a K-split workspace.

Per case, for every output (y, gx, gw) that a split-operand launch produces (r1, r2, tie_free and the
constants: tests/arithmetic_ladder.py; "equals" is ``==`` on the numbers, a sum of signed zeros may
differ in sign):

1. 'bf16x1' on (x, w, gy) equals 'split_bf16x3' on (r1 x, r1 w, r1 gy): the five products it drops are exact
   zeros there and the K order is the same.  The bias is not rounded.
2. 'split_bf16x2' equals 'split_bf16x3' on r2 of the one operand where the other operand is bf16-exact, in
   both roles, on tie-free operands.  That pins hi mid and mid hi and the absence of the lo terms.
3. Both differ from 'split_bf16x3' on the same operands (the knob is not ignored); an output of an fp32-MFMA
   launch is the same bits under all three.
4. |got - float64| <= c S + 1e-5 max|ref| per element, c = 2u + u^2 (one plane), 3u^2 + 6u^3 + 4u^4 (two);
   tests/test_arithmetic_ladder_cpu.py shows on a float64 model that the same operands meet c S.
6. The Winograd entry points are bit-identical for split_planes = 1, 2, 3, and 'bf16x1' sends a routed 3x3
   layer to the direct kernels, where statement 1 holds.
Then the operand-range statement of set_gemm_arithmetic's docstring at one small case, and one train step
and one predict of the small model per new arithmetic: finite, and bit-identical run to run."""
import numpy as np
import pytest
import torch

import arithmetic_ladder as A
import gemm_edge_cases as G
import test_gpu_model as TM
from chainer_mask_rcnn_amd import _lib
from chainer_mask_rcnn_amd import functions as F
from chainer_mask_rcnn_amd.functions import conv as C
from chainer_mask_rcnn_amd.functions._layout import nhwc

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def defaults(dev):
    yield
    C.set_gemm_arithmetic(C.DEFAULT_GEMM_ARITHMETIC)
    for k, v in G.DEFAULT_KNOBS.items():
        _lib.set_tuning(k, v)
    _lib.set_tuning('split_planes', 3)


def _run(dev, case, name, x, w, gy, b):
    """The case's operation under arithmetic ``name`` (None: leave it) -> {'y', 'gx', 'gw'} on the host."""
    if name is not None:
        C.set_gemm_arithmetic(name)
    for k, v in case.knobs.items():
        _lib.set_tuning(k, v)
    t = lambda a, g=False: torch.tensor(a, device=dev).requires_grad_(g)       # noqa: E731
    bt = t(b)
    if case.kind == 'stem':
        from chainer_mask_rcnn_amd.models.resnet_extractor import pack_stem_filter, pad_image_nhwc4
        out = {'y': F.stem_conv(pad_image_nhwc4(t(x)), pack_stem_filter(t(w)), bt, None, None)}
    else:
        xt, wt = t(x, case.backward), t(w, case.backward)
        with torch.set_grad_enabled(case.backward):
            if case.kind == 'deconv':
                y = F.deconv2x2s2(xt, wt, bt)
            else:
                y = F.conv2d(xt, wt, bt, stride=case.d.stride, pad=case.d.pad)
        out = {'y': y.detach()}
        if case.backward:
            y.backward(t(gy))
            out['gx'], out['gw'] = xt.grad, wt.grad
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in out.items()}
    assert all(bool(torch.isfinite(v).all()) for v in out.values())
    return out


def _same(a, b):
    return bool((a == b).all())


def _opt(f, a):
    return None if a is None else f(a)


@pytest.mark.parametrize('case', A.cases(), ids=[c.id for c in A.cases()])
def test_planes_are_the_products_they_claim(dev, case):
    x, w, gy, b = A.operands(case)
    split = A.split_outputs(case)
    assert split['y'], 'every case has a split-operand forward'
    full = _run(dev, case, 'split_bf16x3', x, w, gy, b)
    one = _run(dev, case, 'bf16x1', x, w, gy, b)
    two = _run(dev, case, 'split_bf16x2', x, w, gy, b)
    for k, on in split.items():                                       # statement 3
        if on:
            assert not _same(one[k], full[k]) and not _same(two[k], full[k]) and not _same(one[k], two[k]), k
        else:
            assert torch.equal(one[k], full[k]) and torch.equal(two[k], full[k]), k
    # statement 1
    want = _run(dev, case, 'split_bf16x3', A.r1(x), A.r1(w), _opt(A.r1, gy), b)
    for k in (k for k, on in split.items() if on):
        assert _same(one[k], want[k]), 'one plane, %s: %d elements differ' % (k, int((one[k] != want[k]).sum()))
    # statement 2: the filter bf16-exact (y: x general; gx: gy general), then the input (y: w general; gw: gy general)
    xs, ws, gs = A.tie_free(x), A.tie_free(w), _opt(A.tie_free, gy)
    for exact, outs in (('w', ('y', 'gx')), ('x', ('y', 'gw'))):
        xa, wa = (xs, A.r1(w)) if exact == 'w' else (A.r1(x), ws)
        got = _run(dev, case, 'split_bf16x2', xa, wa, gs, b)
        want = _run(dev, case, 'split_bf16x3', A.r2(xa), A.r2(wa), _opt(A.r2, gs), b)
        for k in (k for k in outs if split.get(k)):
            assert _same(got[k], want[k]), 'two planes, %s bf16-exact, %s: %d elements differ' % (
                exact, k, int((got[k] != want[k]).sum()))
    # statement 4
    ref, S = A.reference(case, x, w, gy)
    ref['y'] = ref['y'] + b.astype(np.float64).reshape((1, -1, 1, 1))
    if case.kind == 'stem':                      # the stem entry point always ends in ReLU (1-Lipschitz: same bound)
        ref['y'] = np.maximum(ref['y'], 0)
    for name, got in (('bf16x1', one), ('split_bf16x2', two)):
        for k in ref:
            err = np.abs(got[k].numpy().astype(np.float64) - ref[k])
            bound = A.BOUND[name] * S[k] + A.T3 * np.abs(ref[k]).max()
            worst = float((err / bound).max())
            print('%-14s %-3s worst error / bound %.3f, max error %.2e of max|ref|' % (
                name, k, worst, err.max() / np.abs(ref[k]).max()))
            assert worst <= 1.0, (name, k, worst)


def test_a_rejected_knob_value_keeps_the_setting(dev):
    case = A.cases()[0]
    x, w, gy, b = A.operands(case)
    one = _run(dev, case, 'bf16x1', x, w, gy, b)
    for bad in (0, 4):
        with pytest.raises(_lib.MrcnnHipError):
            _lib.set_tuning('split_planes', bad)
        again = _run(dev, case, None, x, w, gy, b)
        assert all(torch.equal(again[k], one[k]) for k in one)
    _lib.set_tuning('split_planes', 2)                                  # the knob alone, without the Python name
    two = _run(dev, case, None, x, w, gy, b)
    want = _run(dev, case, 'split_bf16x2', x, w, gy, b)
    assert all(torch.equal(two[k], want[k]) for k in two) and not torch.equal(two['y'], one['y'])


# ---- Winograd --------------------------------------------------------------------------------------------
# (N, C, H, W, K): the tiny maps of the edge lists, one whose 36 GEMMs run as W8 launches (88 x 64 = 5632 tiles
# of 4x4 = 22 x 256 rows, 128 columns, 256 deep: 36 x 22 >= 768 workgroups) and one on 128x128 tiles
WINO_SHAPES = G.WINOGRAD + [(88, 256, 32, 32, 128), (3, 64, 32, 36, 132)]


@pytest.mark.parametrize('shape', WINO_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_winograd_entry_points_run_three_planes_whatever_the_knob(dev, shape):
    N, Cc, H, W, K = shape
    d = G.desc(N, Cc, H, W, K, 3, 3, 1, 1)
    x, w, gy = G.operands(d)
    xt, wt, gt = (nhwc(torch.tensor(a, device=dev)) for a in (x, w, gy))
    dd = C.make_desc(xt.shape, wt.shape, 1, 1)
    outs = {}
    for planes in (3, 2, 1):
        _lib.set_tuning('split_planes', planes)
        y, _ = C.wino_fwd(xt, wt, dd, None, None, False)
        gx = C.wino_dgrad(dd, gt, wt)
        gw = torch.empty_like(wt)
        C.wino_wgrad_into(dd, xt, None, gt, gw)
        with torch.no_grad():
            direct = C._fwd_raw(xt, wt, dd, None, None, None, False)
        torch.cuda.synchronize()
        outs[planes] = (y, gx, gw, direct)
    for planes in (2, 1):
        for k in range(3):
            assert torch.equal(outs[planes][k], outs[3][k]), (planes, 'y gx gw'.split()[k])
        assert not torch.equal(outs[planes][3], outs[3][3]), 'the direct kernel ignored the knob'


def test_bf16x1_sends_a_routed_layer_to_the_direct_kernels(dev, monkeypatch):
    """4 x 256 x 32 x 32 -> 256, 3x3 / pad 1: on the Winograd route under the other names (at the suite's work
    threshold), direct under 'bf16x1', where statement 1 holds against the direct three-plane kernels."""
    case = A.Case('routed 3x3', 'conv', G.desc(4, 256, 32, 32, 256, 3, 3, 1, 1), {}, True)
    dd = C.make_desc((4, 256, 32, 32), (256, 256, 3, 3), 1, 1)
    x, w, gy, b = A.operands(case)
    calls = []
    orig = _lib.call
    monkeypatch.setattr(_lib, 'call', lambda name, *a: (calls.append(name), orig(name, *a))[1])
    for name in ('split_bf16x3', 'split_bf16x2'):
        C.set_gemm_arithmetic(name)
        assert C.uses_winograd(dd)
        del calls[:]
        _run(dev, case, None, x, w, gy, b)
        assert any(c.startswith('mrcnn_conv3x3_wino') for c in calls), calls
    C.set_gemm_arithmetic('bf16x1')
    assert not C.uses_winograd(dd)
    del calls[:]
    one = _run(dev, case, None, x, w, gy, b)
    assert 'mrcnn_conv2d_fwd' in calls and 'mrcnn_conv2d_dgrad_wt' in calls and \
        not any(c.startswith('mrcnn_conv3x3_wino') for c in calls), calls
    monkeypatch.setattr(C, 'USE_WINOGRAD', False)
    want = _run(dev, case, 'split_bf16x3', A.r1(x), A.r1(w), A.r1(gy), b)
    full = _run(dev, case, 'split_bf16x3', x, w, gy, b)
    for k, on in A.split_outputs(case).items():
        assert on and _same(one[k], want[k]) and not _same(one[k], full[k]), k


# ---- operand range ----------------------------------------------------------------------------------------

def test_infinite_operands_as_documented(dev):
    """set_gemm_arithmetic's docstring: an infinite operand (or a finite one beyond bf16's range) makes the
    outputs that read it NaN under 'split_bf16x2' as under 'split_bf16x3' (mid = inf - inf), and +-inf with the
    sign IEEE multiplication gives under 'bf16x1', where hi is the only plane; NaN stays NaN; rows that do not
    read the element keep their bits."""
    rng = np.random.RandomState(13)
    M, K, Cc = 130, 192, 256
    x = rng.standard_normal((1, Cc, 1, M)).astype(np.float32)
    w = (rng.standard_normal((K, Cc, 1, 1)) / 16.).astype(np.float32)
    b = np.zeros(K, np.float32)
    bad = {5: np.inf, 64: -np.inf, 65: np.float32(3.4e38), 129: np.nan}
    xb = x.copy()
    for r, v in bad.items():
        xb[0, 17, 0, r] = v
    rest = np.setdiff1d(np.arange(M), sorted(bad))

    def run(name, xin):                       # (rows, K); non-finite values are the point here
        C.set_gemm_arithmetic(name)
        y = F.conv2d(torch.tensor(xin, device=dev), torch.tensor(w, device=dev), None)
        return y.cpu().numpy()[0, :, 0, :].T
    for name in ('split_bf16x3', 'split_bf16x2'):
        got, clean = run(name, xb), run(name, x)
        assert np.all(np.isnan(got[sorted(bad)])), name
        assert np.array_equal(got[rest], clean[rest]), name
    got, clean = run('bf16x1', xb), run('bf16x1', x)
    assert np.array_equal(got[rest], clean[rest])
    w17 = A.r1(w[:, 17, 0, 0])
    assert np.all(w17 != 0)
    for r in (5, 64, 65):
        sign = np.sign(xb[0, 17, 0, r]) * np.sign(w17)
        assert np.array_equal(got[r], np.where(sign > 0, np.inf, -np.inf).astype(np.float32)), r
    assert np.all(np.isnan(got[129]))


# ---- the model ----------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def small_model(dev):
    return TM._build(dev, 50)


def _host(v):
    return v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)


@pytest.mark.parametrize('name', ['split_bf16x2', 'bf16x1'])
def test_train_step_and_predict(dev, small_model, name):
    model, chain, imgs, bboxes, labels, masks = small_model
    C.set_gemm_arithmetic(name)
    steps = []
    for _ in range(2):
        for p in chain.parameters():
            p.grad = None
        np.random.seed(321)
        loss = chain(torch.tensor(imgs, device=dev), bboxes, labels, masks, [1., 1.])
        loss.backward()
        torch.cuda.synchronize()
        steps.append(({k: float(v) for k, v in chain.report.items()},
                      {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}))
    assert steps[0][0] and all(np.isfinite(v) for v in steps[0][0].values()), steps[0][0]
    assert steps[0][0] == steps[1][0]
    assert steps[0][1] and all(bool(torch.isfinite(g).all()) for g in steps[0][1].values())
    assert all(torch.equal(g, steps[1][1][n]) for n, g in steps[0][1].items())
    preds = []
    for _ in range(2):
        preds.append(model.predict_prepared(torch.tensor(imgs, device=dev), [1., 1.], [(TM.H, TM.W)] * 2))
    for a, b in zip(preds[0], preds[1]):                 # bboxes, masks, labels, scores: one entry per image
        assert len(a) == len(b) == 2
        for u, v in zip(a, b):
            u, v = _host(u), _host(v)
            assert np.all(np.isfinite(u.astype(np.float64))) and np.array_equal(u, v)
