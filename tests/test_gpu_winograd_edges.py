"""The Winograd F(4x4,3x3) route (csrc/conv_winograd.h) on every branch of its launch policy, every
epilogue and the sign fix-up: the Winograd lists of tests/gemm_edge_cases.py on the device.

The harness is tests/test_gpu_gemm_edges.py's Session: launch_ref.LaunchChecker compares every
mrcnn_conv3x3_wino_* call with its float64 restatement under the suite's convolution bound
|got - ref| <= 1e-4 |ref| + 1e-5 max|ref|, outputs that the host code allocates are NaN-prefilled,
and the profiler's GEMM launch counts per kind (the W8 kernel included) must equal what
gemm_edge_cases.route() predicts from plan_wino_gemm / plan_wino_wgrad.  The GEMMs read and write
through buffer descriptors, so a wrong row range, m_lo or tail mask does not fault: it drops a term or
reads a neighbour, and only the value comparison on the right shape finds it.

Beside the bound, the plain passes are held to the level the project pins for this route (max error
<= 1e-5 of the tensor scale, WINO_LEVEL), gradients from a kept v and from raw x are bit-equal, and a
second run of every pass is bit-identical (the ordered slab sum at 1, 2, 7 and 8 slabs).

The fix-up kernel's VALUES are checked by raising wino_ambiguity_ppb to 2e9: the bound is then
2 |A^T||M||A|, every output without a shift lies inside it, and the ordinary bound checks
wino_fixup_kernel's taps, padding and channel loop instead of the Winograd arithmetic.
"""
import ctypes

import numpy as np
import pytest
import torch

import gemm_edge_cases as G
import launch_ref as L
from chainer_mask_rcnn_amd import _lib
from chainer_mask_rcnn_amd.functions import conv as C
from chainer_mask_rcnn_amd.functions._layout import nhwc
from chainer_mask_rcnn_amd._lib import EPI_AFFINE, EPI_RELU, EPI_EXACT_SIGNS
from test_gpu_gemm_edges import NAN, Session, _cdesc, _dev_nhwc, _guard_ok, _krsc, _rel_to_scale, _t

pytestmark = pytest.mark.gpu

# max error of a plain pass against float64, relative to the tensor's scale: the level
# tests/test_gpu_winograd.py pins.  No case of the lists needs more: the worst measured is 8.1e-6 (the
# weight gradient over 511 tiles in one slab), the W8 cases reach 7.0e-6 (forward, 252 channels deep)
WINO_LEVEL = 1e-5


def _ops(dev, d, seed=None):
    x, w, gy = G.operands(d, seed)
    return (x, w, gy), (nhwc(_t(x, dev)), nhwc(_t(w, dev)), nhwc(_t(gy, dev)))


def _passes(d, xt, wt, gt):
    """forward (v kept), data gradient, weight gradient from v and from x."""
    dd = C.make_desc(xt.shape, wt.shape, 1, 1)
    y, v = C.wino_fwd(xt, wt, dd, None, None, False, keep_v=True)
    gx = C.wino_dgrad(dd, gt, wt)
    gW, gW2 = torch.full_like(wt, NAN), torch.full_like(wt, NAN)
    C.wino_wgrad_into(dd, None, v, gt, gW)
    C.wino_wgrad_into(dd, xt, None, gt, gW2)
    return y, gx, gW, gW2


def _expected_labels(d, knobs):
    return [('mrcnn_' + e, G.route(e, d, 0, True, knobs).label)
            for e in G.WINO_ENTRIES + G.WINO_ENTRIES[2:]]


def _policy_and_thresholds(w8):
    seen, out = set(), []
    cases = [(i, d) for i, _, d, _ in G.wino_policy_cases()] + \
        [('threshold %s' % (c,), G.wino_desc(*c)) for c, _, _, _ in G.WINO_THRESHOLDS]
    for cid, d in cases:
        if d in seen or G.is_w8_case(d) != w8:
            continue
        seen.add(d)
        for sb in (3,) if w8 else (3, 0):
            out.append(pytest.param(d, sb, id='%s%s' % (cid, '' if sb == 3 else ' fp32')))
    return out


def _run_policy_case(dev, monkeypatch, d, split_bf16, cid):
    (x, w, gy), (xt, wt, gt) = _ops(dev, d)
    with Session(monkeypatch, 'winograd policy', dict(split_bf16=split_bf16)) as s:
        with s.case(cid):
            first = _passes(d, xt, wt, gt)
            assert s.labels == _expected_labels(d, s.knobs), s.labels
            assert all(bool(torch.isfinite(t).all()) for t in first), 'a NaN of the prefill was left'
        print('winograd case: %s -> %s' % (cid, [lb for _, lb in s.labels[:3]]))
        with s.unchecked():
            again = _passes(d, xt, wt, gt)
        for what, a, b in zip(('forward', 'dgrad', 'wgrad(v)', 'wgrad(x)'), first, again):
            assert torch.equal(a, b), '[%s] %s is not repeatable' % (cid, what)
        assert torch.equal(first[2], first[3]), '[%s] wgrad from v and from x differ' % cid
        X, Wt, Gy = (torch.tensor(a, device=dev, dtype=torch.float64) for a in (x, w, gy))
        for what, got, ref in (('forward', first[0], L.conv_fwd(X, Wt, 1, 1)),
                               ('dgrad', first[1], L.conv_dgrad(Gy, Wt, d.H, d.W, 1, 1)),
                               ('wgrad', first[2], L.conv_wgrad(X, Gy, 3, 3, 1, 1))):
            level = _rel_to_scale(got, ref)
            print('winograd level: %s %s split_bf16=%d: %.3g of the tensor scale' % (cid, what, split_bf16, level))
            assert level <= WINO_LEVEL, (cid, what, level)
        s.assert_clean()


@pytest.mark.parametrize('d,split_bf16', _policy_and_thresholds(False))
def test_policy_branches_and_thresholds(dev, monkeypatch, d, split_bf16, request):
    """Every label of plan_wino_gemm / plan_wino_wgrad at its smallest ragged problem, and both sides of
    every comparison of the two plans, on the split-operand and the fp32 arithmetic."""
    _run_policy_case(dev, monkeypatch, d, split_bf16, request.node.callspec.id)


@pytest.mark.parametrize('d,split_bf16', _policy_and_thresholds(True))
def test_w8_branch(dev, monkeypatch, d, split_bf16, request):
    """The W8 kernel through the batch of 36: whole row tiles, a ragged last row tile (T >= 4096), three
    column tiles with 4 ragged columns, a depth of 8 slices + 4; the forward alone (depth 252) or both."""
    _run_policy_case(dev, monkeypatch, d, split_bf16, request.node.callspec.id)
    assert 'wino/w8' in [G.wino_plan(e, d).label for e in G.WINO_ENTRIES[:2]]


# ---- epilogues ------------------------------------------------------------------------------------------

def _epilogue_operands(dev, d):
    rng = np.random.RandomState(G.seed_of(*d) + 3)
    sc = _t(rng.uniform(.5, 1.5, d.K).astype(np.float32) * np.where(np.arange(d.K) % 3 == 0, -1, 1).astype(np.float32), dev)
    sh = _t(rng.standard_normal(d.K).astype(np.float32), dev)
    fold = _t(rng.uniform(.5, 1.5, d.K).astype(np.float32), dev)
    osc = _t(rng.uniform(.5, 1.5, d.C).astype(np.float32), dev)
    mask = rng.standard_normal((d.N, d.C, d.H, d.W)).astype(np.float32)
    mask[rng.random_sample(mask.shape) < 0.25] = 0.                     # exact zeros: masked out, like negatives
    rs = _t(rng.uniform(.5, 1.5, d.K).astype(np.float32), dev)
    assert (mask > 0).any() and (mask < 0).any() and (mask == 0).any()
    return sc, sh, fold, osc, nhwc(_t(mask, dev)), rs


@pytest.mark.parametrize('c', G.WINO_EPILOGUE_SHAPES + [G.WINO_EPILOGUE_W8], ids=str)
def test_epilogues_on_ragged_and_one_tile_maps(dev, monkeypatch, c):
    """Every epilogue of the three passes on a one-pixel map, maps smaller than a tile in one axis, 7x7
    and 5x9, channels that are no multiple of 32, on 64x64, 128x128, main128+tail64 and W8 launches."""
    d = G.wino_desc(*c)
    _, (xt, wt, gt) = _ops(dev, d)
    sc, sh, fold, osc, mask, rs = _epilogue_operands(dev, d)
    dd = C.make_desc(xt.shape, wt.shape, 1, 1)
    lib = _lib.load()
    with Session(monkeypatch, 'winograd epilogues') as s:
        with s.case('%s forward' % (c,)):
            ys = {}
            for what, scale, shift, relu in (('none', None, None, False), ('AFFINE', sc, sh, False),
                                             ('AFFINE+RELU', sc, sh, True), ('BIAS', None, sh, False),
                                             ('BIAS+RELU', None, sh, True), ('RELU', None, None, True)):
                y_keep, v = C.wino_fwd(xt, wt, dd, scale, shift, relu, keep_v=True)
                y, _ = C.wino_fwd(xt, wt, dd, scale, shift, relu)
                assert bool(torch.isfinite(y).all()), what
                assert torch.equal(y, y_keep), '%s: y with a kept v differs from y with the scratch v' % what
                ys[what] = y
            assert bool((ys['RELU'] == ys['none'].clamp_min(0)).all())
            # a precomputed u and w = NULL: the same bits as the per-call filter transform
            u = torch.full((lib.mrcnn_conv3x3_wino_u_bytes(C.ctx_desc(dd)) // 4,), NAN, device=dev)
            _lib.call('mrcnn_conv3x3_wino_filter', C.ctx_desc(dd), _lib.ptr(wt), _lib.ptr(u), _lib.stream_ptr())
            for what, flags, scale, shift in (('none', 0, None, None), ('AFFINE+RELU', EPI_AFFINE | EPI_RELU, sc, sh)):
                y = torch.full((d.N, d.H, d.W, d.K), NAN, device=dev)
                _lib.call('mrcnn_conv3x3_wino_fwd', C.ctx_desc(dd), _lib.ptr(xt), None, _lib.ptr(u), _lib.ptr(scale),
                          _lib.ptr(shift), _lib.ptr(y), flags, None, _lib.ptr(C._wino_ws(dd, dev)), _lib.stream_ptr())
                assert torch.equal(y.permute(0, 3, 1, 2), ys[what]), 'precomputed u changes the bits (%s)' % what
        with s.case('%s data gradient' % (c,)):
            for kw in ({}, dict(fold_scale=fold), dict(out_scale=osc), dict(out_mask_y=mask),
                       dict(fold_scale=fold, out_scale=osc, out_mask_y=mask)):
                gx = C.wino_dgrad(dd, gt, wt, **kw)
                assert bool(torch.isfinite(gx).all()), sorted(kw)
                if 'out_mask_y' in kw:
                    assert bool((gx[mask <= 0] == 0).all()), 'masked elements are not exact zeros'
        with s.case('%s weight gradient' % (c,), own_outputs=True):
            for row_scale in (None, rs):
                gW = torch.full_like(wt, NAN)
                C.wino_wgrad_into(dd, xt, None, gt, gW, row_scale=row_scale)
                assert bool(torch.isfinite(gW).all())
        s.assert_clean()
        assert s.chk.stats['mrcnn_conv3x3_wino_fwd'][0] == 14 and s.chk.stats['mrcnn_conv3x3_wino_dgrad'][0] == 5


# ---- nothing written outside ------------------------------------------------------------------------------

def _bands_ok(g, cid):
    """The guard bands alone (a workspace defines no value per element)."""
    bits = g.buf
    ok = bool((bits[:G.GUARD] == G.NAN_BITS).all()) and bool((bits[G.GUARD + g.n:] == G.NAN_BITS).all())
    assert ok, '[%s] guard band written' % cid


def _guarded_passes(dev, s, cid, d, exact_signs_flags=EPI_RELU):
    """fwd (plain, then EXACT_SIGNS), filter, dgrad, wgrad through the C ABI into guarded buffers; the
    workspace is exactly mrcnn_conv3x3_wino_workspace_bytes.  Returns (workspace, descriptor)."""
    lib = _lib.load()
    x, w, gy = G.operands(d)
    xt, wt, gt = _dev_nhwc(x, dev), _krsc(w, dev), _dev_nhwc(gy, dev)
    dd = _cdesc(d)
    dp = C.ctx_desc(dd)
    nbytes = lib.mrcnn_conv3x3_wino_workspace_bytes(dp)
    assert nbytes % 4 == 0
    ws = G.Guarded(nbytes // 4, dev)
    y, gx, gw = (G.Guarded(n, dev) for n in (d.N * d.H * d.W * d.K, d.N * d.H * d.W * d.C, d.K * 9 * d.C))
    v = G.Guarded(lib.mrcnn_conv3x3_wino_v_bytes(dp) // 4, dev)
    u = G.Guarded(lib.mrcnn_conv3x3_wino_u_bytes(dp) // 4, dev)
    every = (ws, y, gx, gw, v, u)

    def after(what, *defined):
        torch.cuda.synchronize()
        for g in every:
            _bands_ok(g, '%s after %s' % (cid, what))
        for g in defined:
            _guard_ok(g, '%s after %s' % (cid, what))

    with s.case(cid, own_outputs=True):
        _lib.call('mrcnn_conv3x3_wino_fwd', dp, _lib.ptr(xt), _lib.ptr(wt), None, None, None, _lib.ptr(y.out), 0,
                  _lib.ptr(v.out), _lib.ptr(ws.out), _lib.stream_ptr())
        after('fwd', y, v)
        y.out.view(torch.int32).fill_(G.NAN_BITS)
        _lib.call('mrcnn_conv3x3_wino_fwd', dp, _lib.ptr(xt), _lib.ptr(wt), None, None, None, _lib.ptr(y.out),
                  exact_signs_flags | EPI_EXACT_SIGNS, None, _lib.ptr(ws.out), _lib.stream_ptr())
        after('fwd with EXACT_SIGNS', y)
        _lib.call('mrcnn_conv3x3_wino_filter', dp, _lib.ptr(wt), _lib.ptr(u.out), _lib.stream_ptr())
        after('filter', u)
        _lib.call('mrcnn_conv3x3_wino_dgrad', dp, _lib.ptr(gt), _lib.ptr(wt), None, _lib.ptr(gx.out), None, None,
                  _lib.ptr(ws.out), _lib.stream_ptr())
        after('dgrad', gx)
        _lib.call('mrcnn_conv3x3_wino_wgrad', dp, None, _lib.ptr(v.out), _lib.ptr(gt), _lib.ptr(gw.out), None,
                  _lib.ptr(ws.out), _lib.stream_ptr())
        after('wgrad', gw)
    return ws, dd


GUARDED_SHAPES = [(3, 36, 2, 7, 40), (33, 68, 7, 7, 132), (47, 68, 5, 9, 132), (4100, 260, 2, 2, 260)]


@pytest.mark.parametrize('c', GUARDED_SHAPES, ids=str)
def test_nothing_is_written_outside(dev, monkeypatch, c):
    """y, gx, gw, v, u and a workspace of exactly the advertised size inside guard bands, per GEMM tile
    family (64x64, 128x128, main128+tail64 on the ragged 5x9 maps, W8 with a ragged last row tile)."""
    with Session(monkeypatch, 'winograd guard bands') as s:
        _guarded_passes(dev, s, 'guarded %s' % (c,), G.wino_desc(*c))
        s.assert_clean()


# ---- the values the sign fix-up writes -----------------------------------------------------------------------

AMBIGUITY_ALL = 2000000000         # parts per 1e9: a bound of 2.0 |A^T||M||A|
AMBIGUITY_DEFAULT = 4000


def _fixup_count(dd, ws_ptr):
    cnt = ctypes.c_int(-1)
    _lib.check(_lib.load().mrcnn_conv3x3_wino_fixup_count(C.ctx_desc(dd), ws_ptr, _lib.stream_ptr(),
                                                          ctypes.byref(cnt)), 'fixup_count')
    return cnt.value


@pytest.mark.parametrize('c', G.WINO_FIXUP_SHAPES, ids=str)
def test_fixup_values(dev, monkeypatch, c):
    """With every output inside the ambiguity bound the forward's result IS wino_fixup_kernel's: its taps
    at the borders of 1x1, 2x7 and 7x7 maps, its channel loop at C = 4, 36, 256 (one pass of the wave) and
    260 (a second pass of one lane), its scale and its shift."""
    d = G.wino_desc(*c)
    outputs = d.N * d.H * d.W * d.K
    assert outputs <= G.wino_fix_cap(d)
    _, (xt, wt, gt) = _ops(dev, d)
    dd = C.make_desc(xt.shape, wt.shape, 1, 1)
    with Session(monkeypatch, 'winograd fix-up values') as s:
        try:
            _lib.set_tuning('wino_ambiguity_ppb', AMBIGUITY_ALL)
            with s.case('%s: every output recomputed' % (c,)):
                sc0, sh0 = (_t(a, dev) for a in G.wino_fixup_epilogue(d, 'affine0'))
                for what, scale, shift, relu in (('plain', None, None, False), ('RELU', None, None, True),
                                                 ('AFFINE, mixed-sign scale, zero shift', sc0, sh0, False)):
                    y, _ = C.wino_fwd(xt, wt, dd, scale, shift, relu, exact_signs=True)
                    assert bool(torch.isfinite(y).all()), what
                    assert _fixup_count(dd, _lib.ptr(C._wino_ws(dd, dev))) == outputs, what
            with s.case('%s: a shift' % (c,)):
                for kind in ('bias', 'affine'):
                    sc, sh = G.wino_fixup_epilogue(d, kind)
                    y, _ = C.wino_fwd(xt, wt, dd, None if sc is None else _t(sc, dev), _t(sh, dev), False,
                                      exact_signs=True)
                    n = _fixup_count(dd, _lib.ptr(C._wino_ws(dd, dev)))
                    print('fix-up with a shift: %s %s: %d of %d outputs recomputed' % (c, kind, n, outputs))
                    assert 2 * n >= outputs, (kind, n, outputs)
        finally:
            _lib.set_tuning('wino_ambiguity_ppb', AMBIGUITY_DEFAULT)
        s.assert_clean()


def test_fix_list_overflow(dev, monkeypatch):
    """73 800 candidates against a list of 4606 that ends flush with the workspace: the call succeeds, the
    first 4606 are recomputed, the rest keep their Winograd value (all inside the bound), nothing is
    written behind the workspace, and the count reads 73 800."""
    d = G.wino_desc(*G.WINO_FIXUP_OVERFLOW)
    with Session(monkeypatch, 'winograd fix-list overflow') as s:
        try:
            _lib.set_tuning('wino_ambiguity_ppb', AMBIGUITY_ALL)
            ws, dd = _guarded_passes(dev, s, 'fix-list overflow', d, exact_signs_flags=0)
            # (the data gradient and the weight gradient ran on the workspace since: once more for the count)
            x, w, _ = G.operands(d)
            y = G.Guarded(d.N * d.H * d.W * d.K, dev)
            with s.case('fix-list overflow: the count', own_outputs=True):
                _lib.call('mrcnn_conv3x3_wino_fwd', C.ctx_desc(dd), _lib.ptr(_dev_nhwc(x, dev)), _lib.ptr(_krsc(w, dev)),
                          None, None, None, _lib.ptr(y.out), EPI_EXACT_SIGNS, None, _lib.ptr(ws.out), _lib.stream_ptr())
                assert _fixup_count(dd, _lib.ptr(ws.out)) == d.N * d.H * d.W * d.K == 73800
                assert G.wino_fix_cap(d) == 4606
                _guard_ok(y, 'fix-list overflow')
                _bands_ok(ws, 'fix-list overflow')
        finally:
            _lib.set_tuning('wino_ambiguity_ppb', AMBIGUITY_DEFAULT)
        s.assert_clean()


# ---- rejected by design ------------------------------------------------------------------------------------------

def test_rejections_name_the_descriptor_and_leave_the_library_usable(dev, monkeypatch):
    """What wino_check refuses raises from each of the four entry points before any pointer is looked at
    (all data pointers NULL: the message is the descriptor's), and a valid call afterwards is correct."""
    ok = G.wino_desc(2, 8, 5, 6, 8)
    (_, _, _), (xt, wt, gt) = _ops(dev, ok)
    with Session(monkeypatch, 'winograd rejections') as s:
        for cid, d, why in G.WINO_REJECTED:
            dp = C.ctx_desc(_cdesc(d))
            sp = _lib.stream_ptr()
            calls = (('mrcnn_conv3x3_wino_filter', (dp, None, None, sp)),
                     ('mrcnn_conv3x3_wino_fwd', (dp, None, None, None, None, None, None, 0, None, None, sp)),
                     ('mrcnn_conv3x3_wino_dgrad', (dp, None, None, None, None, None, None, None, sp)),
                     ('mrcnn_conv3x3_wino_wgrad', (dp, None, None, None, None, None, None, sp)))
            for name, args in calls:
                with s.unchecked(), pytest.raises(_lib.MrcnnHipError) as err:
                    _lib.call(name, *args)
                assert why in str(err.value) and 'null pointer' not in str(err.value), (cid, name, str(err.value))
            with s.case(cid + ': a valid call afterwards'):
                _passes(ok, xt, wt, gt)
        dd = C.make_desc(xt.shape, wt.shape, 1, 1)
        _, v = C.wino_fwd(xt, wt, dd, None, None, False, keep_v=True)
        gW = torch.empty_like(wt)
        for x_, v_ in ((xt, v), (None, None)):
            with s.unchecked(), pytest.raises(_lib.MrcnnHipError) as err:
                C.wino_wgrad_into(dd, x_, v_, gt, gW)
            assert 'exactly one of x / v' in str(err.value)
        with s.case('a valid call after the x / v rejections'):
            _passes(ok, xt, wt, gt)
        s.assert_clean()
