"""mrcnn_grad_sumsq / mrcnn_grad_control / mrcnn_sgd_momentum_wd_ctl through the C ABI against the
float64 reference of tests/grad_control_ref.py: every element counted once, a derived error bound,
repeatable bits, no stale partial, the control word case by case, and the guarded SGD launch bit
for bit against mrcnn_sgd_momentum_wd_ex at the factor the device computed."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import grad_control_ref as R
from chainer_mask_rcnn_amd import _lib, optimizers

pytestmark = pytest.mark.gpu

P = optimizers.SUMSQ_PARTIALS
SIZES = [0, 1, 3, 4, 5, 255, 4 * P - 1, 4 * P, 4 * P + 1, 2 ** 20 + 3]


def _partials(g, n, dev, poison=float('nan')):
    """partials of g[:n], from a buffer filled with ``poison`` before the call."""
    out = torch.full((P,), poison, dtype=torch.float64, device=dev)
    _lib.call('mrcnn_grad_sumsq', _lib.ptr(g), n, _lib.ptr(out), _lib.stream_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _device(a, dev):
    """``a`` on the device in a buffer of at least one 16-byte group (n == 0 included)."""
    buf = torch.zeros(max(len(a), 4), dtype=torch.float32, device=dev)
    buf[:len(a)] = torch.tensor(a)
    return buf


@functools.lru_cache(maxsize=None)
def _randn(n):
    g = np.random.RandomState(n % 9973).standard_normal(n).astype(np.float32)
    g.setflags(write=False)
    return g, R.exact_sumsq(g)


@pytest.mark.parametrize('n', SIZES)
def test_sumsq_counts_every_element_once(dev, n):
    got = _partials(torch.ones(max(n, 4), dtype=torch.float32, device=dev), n, dev)
    assert float(got.sum()) == float(n)           # integers below 2^53: exact in any order
    assert np.all(got >= 0) and np.all(got == np.floor(got))


@pytest.mark.parametrize('n', SIZES)
def test_sumsq_within_the_worst_case_bound_and_repeatable(dev, n):
    g, ref = _randn(n)
    buf = _device(g, dev)
    a = _partials(buf, n, dev, poison=float('nan'))
    b = _partials(buf, n, dev, poison=1e300)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))     # bits, whatever was there before
    assert np.isfinite(a).all()                                      # no stale value survives
    got = math.fsum(a.tolist())        # the test's own sum of the partials adds no rounding
    err, bound = abs(got - ref), n * 2.0 ** -53 * ref
    print('n %d: |got - fsum| = %.3e, bound n 2^-53 fsum = %.3e' % (n, err, bound))
    # non-negative float64 terms (the squares are exact): any summation order is within
    # (n - 1) u sum to first order
    assert err <= bound
    # and in index order in float64, as mrcnn_grad_control sums them
    seq = 0.
    for x in a.tolist():
        seq += x
    assert abs(seq - ref) <= (n + P) * 2.0 ** -53 * ref


@pytest.mark.parametrize('n', [s for s in SIZES if s > 0])
@pytest.mark.parametrize('where', ['last', 'first'])
def test_sumsq_finds_a_single_large_element(dev, n, where):
    g = np.zeros(n, np.float32)
    g[n - 1 if where == 'last' else 0] = 1e10
    got = _partials(_device(g, dev), n, dev)
    assert float(got.sum()) == float(np.float32(1e10)) ** 2
    assert np.count_nonzero(got) == 1


def test_sumsq_refuses_bad_arguments(dev):
    g = torch.zeros(8, dtype=torch.float32, device=dev)
    out = torch.zeros(P, dtype=torch.float64, device=dev)
    with pytest.raises(_lib.MrcnnHipError, match='16-byte'):
        _lib.call('mrcnn_grad_sumsq', _lib.ptr(g[1:]), 4, _lib.ptr(out), _lib.stream_ptr())
    with pytest.raises(_lib.MrcnnHipError):
        _lib.call('mrcnn_grad_sumsq', _lib.ptr(g), -1, _lib.ptr(out), _lib.stream_ptr())
    with pytest.raises(_lib.MrcnnHipError):
        _lib.call('mrcnn_grad_sumsq', _lib.ptr(g), 8, None, _lib.stream_ptr())


# ---- control word ------------------------------------------------------------------------------
N_CTL, GRAD_SCALE = 4099, 0.5


@functools.lru_cache(maxsize=None)
def _ctl_base():
    g, ss = _randn(N_CTL)
    return g, math.sqrt(ss) * GRAD_SCALE


def _control(g, dev, clip, guard, grad_scale=GRAD_SCALE, runs=1):
    n = len(g)
    buf = _device(g, dev)
    parts = torch.full((runs * P,), float('nan'), dtype=torch.float64, device=dev)
    # ``runs`` > 1: the slice cut into that many 16-byte aligned runs, one slab of partials each
    cuts = [0] + [(n * k // runs) // 4 * 4 for k in range(1, runs)] + [n]
    for k in range(runs):
        _lib.call('mrcnn_grad_sumsq', _lib.ptr(buf[cuts[k]:]), cuts[k + 1] - cuts[k],
                  _lib.ptr(parts[k * P:]), _lib.stream_ptr())
    ctl = torch.full((4,), float('nan'), dtype=torch.float32, device=dev)
    _lib.call('mrcnn_grad_control', _lib.ptr(parts), runs * P, ctypes.c_float(grad_scale),
              ctypes.c_float(clip), 1 if guard else 0, _lib.ptr(ctl), _lib.stream_ptr())
    torch.cuda.synchronize()
    return ctl.cpu().numpy()


def _poisoned(kind):
    g = _ctl_base()[0].copy()
    if kind == 'inf-last':
        g[-1] = np.inf
    elif kind == 'nan-first':
        g[0] = np.nan
    elif kind == 'eight-3e38':
        g[100:108] = 3e38
    return g


CASES = [  # (name, gradient, clip as a multiple of the clean norm, guard)
    ('no-clip', 'clean', 0., False),
    ('clip-2x', 'clean', 2., False),
    ('clip-half', 'clean', 0.5, False),
    ('clip-half-guard', 'clean', 0.5, True),
    ('inf-guard-on', 'inf-last', 0., True),
    ('inf-guard-off', 'inf-last', 0., False),
    ('inf-guard-off-clip', 'inf-last', 0.5, False),
    ('nan-guard-on', 'nan-first', 0., True),
    ('nan-guard-on-clip', 'nan-first', 0.5, True),
    ('3e38-guard-on', 'eight-3e38', 0., True),
]


@pytest.mark.parametrize('name,kind,clip_mult,guard', CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize('runs', [1, 3])
def test_control_word(dev, name, kind, clip_mult, guard, runs):
    g = _poisoned(kind)
    clip = float(np.float32(clip_mult * _ctl_base()[1]))
    got = _control(g, dev, clip, guard, runs=runs)
    ref = R.control_word(R.exact_sumsq(g), GRAD_SCALE, clip, guard)
    print(name, 'device', got.tolist(), 'reference', ref)
    norm, factor, skipped, reported = (got[i] for i in (R.CTL_NORM, R.CTL_FACTOR, R.CTL_SKIPPED,
                                                        R.CTL_NORM_REPORTED))
    with np.errstate(over='ignore'):          # 4.2e38 saturates to inf in float, as on the device
        ref_norm32 = np.float32(ref['norm'])
    if math.isnan(ref['norm']):
        assert np.isnan(norm)
    elif np.isinf(ref_norm32):               # infinite, or finite in float64 and saturated in float
        assert norm == ref_norm32
    else:
        assert abs(float(norm) - ref['norm']) <= 2.0 ** -23 * ref['norm']
    if ref['clipping']:
        want = np.float32(ref['factor'])
        assert abs(float(factor) - float(want)) <= R.ulp32(want)
        assert float(factor) < GRAD_SCALE
    else:
        assert np.float32(factor).view(np.uint32) == np.float32(GRAD_SCALE).view(np.uint32)
    assert float(skipped) == ref['skipped']
    if math.isfinite(R.exact_sumsq(g)):      # NORM itself, saturated or not
        assert np.float32(reported).view(np.uint32) == np.float32(norm).view(np.uint32)
    else:
        assert float(reported) == 0.
    # the cases as the interface states them
    expect = {'no-clip': (0., False), 'clip-2x': (0., False), 'clip-half': (0., True),
              'clip-half-guard': (0., True), 'inf-guard-on': (1., False), 'inf-guard-off': (0., False),
              'inf-guard-off-clip': (0., True), 'nan-guard-on': (1., False),
              'nan-guard-on-clip': (1., False), '3e38-guard-on': (0., False)}[name]
    assert (float(skipped), bool(ref['clipping'])) == expect
    if kind in ('inf-last', 'nan-first'):
        assert float(reported) == 0.
    if kind == 'eight-3e38':
        assert np.isinf(norm) and np.isinf(reported) and float(skipped) == 0.
    if name == 'inf-guard-off-clip':
        assert float(factor) == 0.          # grad_scale * clip / inf: no special case


def test_control_of_no_partials_is_a_zero_norm(dev):
    ctl = torch.full((4,), float('nan'), dtype=torch.float32, device=dev)
    _lib.call('mrcnn_grad_control', None, 0, ctypes.c_float(0.25), ctypes.c_float(1.), 1,
              _lib.ptr(ctl), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert ctl.cpu().tolist() == [0., 0.25, 0., 0.]


# ---- guarded SGD ---------------------------------------------------------------------------------
LR, MOMENTUM, WD = 0.02, 0.9, 1e-4


def _state(n, dev, seed):
    gen = torch.Generator(device='cpu').manual_seed(seed)
    return [torch.randn(max(n, 4), generator=gen).to(dev) for _ in range(3)]


def _bits(t, n):
    return t[:n].cpu().numpy().view(np.uint32)


@pytest.mark.parametrize('n', [1, 5, 4099])
@pytest.mark.parametrize('zero_grad', [0, 1])
def test_guarded_sgd_equals_the_plain_launch_at_the_device_factor(dev, n, zero_grad):
    p, g, v = _state(n, dev, 100 + n)
    host_g = g[:n].cpu().numpy()
    norm = math.sqrt(R.exact_sumsq(host_g)) * GRAD_SCALE
    for clip in (0., 0.5 * norm):
        parts = torch.empty(P, dtype=torch.float64, device=dev)
        ctl = torch.empty(4, dtype=torch.float32, device=dev)
        _lib.call('mrcnn_grad_sumsq', _lib.ptr(g), n, _lib.ptr(parts), _lib.stream_ptr())
        _lib.call('mrcnn_grad_control', _lib.ptr(parts), P, ctypes.c_float(GRAD_SCALE),
                  ctypes.c_float(clip), 1, _lib.ptr(ctl), _lib.stream_ptr())
        factor = float(ctl.cpu()[R.CTL_FACTOR])
        assert (factor == GRAD_SCALE) == (clip == 0.) and float(ctl.cpu()[R.CTL_SKIPPED]) == 0.
        p1, g1, v1 = p.clone(), g.clone(), v.clone()
        p2, g2, v2 = p.clone(), g.clone(), v.clone()
        _lib.call('mrcnn_sgd_momentum_wd_ctl', _lib.ptr(p1), _lib.ptr(g1), _lib.ptr(v1), n,
                  ctypes.c_float(LR), ctypes.c_float(MOMENTUM), ctypes.c_float(WD), _lib.ptr(ctl),
                  zero_grad, _lib.stream_ptr())
        _lib.call('mrcnn_sgd_momentum_wd_ex', _lib.ptr(p2), _lib.ptr(g2), _lib.ptr(v2), n,
                  ctypes.c_float(LR), ctypes.c_float(MOMENTUM), ctypes.c_float(WD),
                  ctypes.c_float(factor), zero_grad, _lib.stream_ptr())
        torch.cuda.synchronize()
        for a, b, what in ((p1, p2, 'p'), (g1, g2, 'g'), (v1, v2, 'v')):
            assert np.array_equal(_bits(a, n), _bits(b, n)), (what, clip)
        assert not np.array_equal(_bits(p1, n), _bits(p, n))           # it did update
        assert bool((g1[:n] == 0).all()) == bool(zero_grad)
        # nothing past n is touched
        for a, b in ((p1, p), (g1, g), (v1, v)):
            assert torch.equal(a[n:], b[n:])


@pytest.mark.parametrize('n', [1, 5, 4099])
@pytest.mark.parametrize('zero_grad', [0, 1])
def test_guarded_sgd_skips(dev, n, zero_grad):
    p, g, v = _state(n, dev, 200 + n)
    ctl = torch.tensor([float('nan'), 0.5, 1., 0.], dtype=torch.float32, device=dev)
    p1, g1, v1 = p.clone(), g.clone(), v.clone()
    _lib.call('mrcnn_sgd_momentum_wd_ctl', _lib.ptr(p1), _lib.ptr(g1), _lib.ptr(v1), n,
              ctypes.c_float(LR), ctypes.c_float(MOMENTUM), ctypes.c_float(WD), _lib.ptr(ctl),
              zero_grad, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(_bits(p1, n), _bits(p, n)) and np.array_equal(_bits(v1, n), _bits(v, n))
    if zero_grad:
        assert bool((g1[:n] == 0).all())
    else:
        assert np.array_equal(_bits(g1, n), _bits(g, n))
    for a, b in ((p1, p), (g1, g), (v1, v)):
        assert torch.equal(a[n:], b[n:])
