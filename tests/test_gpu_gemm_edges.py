"""The convolution GEMM family (csrc/conv_gemm.hip) at degenerate and tile-edge shapes: the case
lists of tests/gemm_edge_cases.py on the device.

Every library call of every case is compared with its float64 restatement by
launch_ref.LaunchChecker under the suite's convolution bound |got - ref| <= 1e-4 |ref| +
1e-5 max|ref|.  All global accesses of the GEMM kernel go through buffer descriptors, so a wrong
tail mask does not fault: it reads a neighbour row or drops a term, and only a value comparison
finds it.  Two more things are held:

* what is never written.  Outputs that the host code allocates (functions/_conv_launch.py, and the
  fresh gradient tensors of functions/_wgrad.py) are prefilled with a NaN (an element the kernel
  skips would otherwise show the allocator's previous, identical result); outputs of the direct
  C-ABI calls live inside a larger NaN-prefilled buffer whose 256-byte guard bands must come back
  bit-identical (gemm_edge_cases.Guarded).  The harness proves that the prefill is live: a ``case``
  during which the NaN allocator was never called fails, unless it declares that all its outputs
  are buffers of its own (``own_outputs=True``) — and then the allocator must not have been called.
* the launch policy.  Around every case the profiler counts launches per kind; the GEMM counts must
  equal what gemm_edge_cases.route() predicts for the calls the case made.  That holds the Python
  restatement of the launch policy (csrc/conv_gemm_plan.h: plan_gemm / plan_wgrad) to what the
  library launches.  The Winograd entry points have a policy of their own (plan_wino_gemm /
  plan_wino_wgrad), restated and predicted the same way; tests/test_gpu_winograd_edges.py runs its
  branches on this harness.  The W8 kernel (256x128 tiles), which a plain GEMM reaches only from
  768 tiles on, is reached there through the Winograd route's batch of 36.

Tiny cases are grouped into loops, one test per family and axis, with the case id in the message.
"""
import collections
import contextlib
import ctypes
import math

import numpy as np
import pytest
import torch

import gemm_edge_cases as G
import launch_ref as L
from chainer_mask_rcnn_amd import _lib
from chainer_mask_rcnn_amd import functions as F
from chainer_mask_rcnn_amd.functions import conv as C
from chainer_mask_rcnn_amd.functions import _conv_launch, _wgrad, stage
from chainer_mask_rcnn_amd.functions._layout import nhwc
from chainer_mask_rcnn_amd._lib import EPI_BIAS, EPI_RELU

pytestmark = pytest.mark.gpu

NAN = float(np.array([G.NAN_BITS], np.int32).view(np.float32)[0])


def _t(a, dev, grad=False):
    t = torch.tensor(a, device=dev)
    if grad:
        t.requires_grad_(True)
    return t


def _nan_empty_nhwc(shape, device, dtype=torch.float32):
    n, c, h, w = shape
    return torch.full((n, h, w, c), NAN, dtype=dtype, device=device).permute(0, 3, 1, 2)


# The host modules of the convolution family (functions/conv.py's layering): the NaN allocator
# replaces ``empty_nhwc`` in every one of them that allocates with it.
_HOST_MODULES = (_conv_launch, _wgrad, C, stage)


def _gemm_kinds():
    lib = _lib.load()
    seen = {}
    for k in range(lib.mrcnn_profile_num_kinds()):
        ms, fl, by, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
        _lib.check(lib.mrcnn_profile_summary(k, ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by),
                                             ctypes.byref(n)), 'profile_summary')
        name = lib.mrcnn_profile_kind_name(k).decode()
        if n.value and name.startswith('conv_gemm_kernel'):
            seen[name] = n.value
    return seen


def _desc_of(dp):
    d = L._d(dp)
    return G.Desc(d.N, d.H, d.W, d.C, d.K, d.R, d.S, d.stride, d.pad)


# entry point -> (descriptor, has_ws) of a call's arguments
_DECODE = {
    'mrcnn_conv2d_fwd': lambda a: (_desc_of(a[0]), bool(L._addr(a[9]))),
    'mrcnn_conv2d_dgrad': lambda a: (_desc_of(a[0]), False),
    'mrcnn_conv2d_dgrad_ex': lambda a: (_desc_of(a[0]), bool(L._addr(a[9]))),
    'mrcnn_conv2d_dgrad_wt': lambda a: (_desc_of(a[0]), bool(L._addr(a[9]))),
    'mrcnn_conv2d_wgrad': lambda a: (_desc_of(a[0]), bool(L._addr(a[4]))),
    'mrcnn_conv2d_wgrad_ex': lambda a: (_desc_of(a[0]), bool(L._addr(a[4]))),
    'mrcnn_conv_stem_fwd': lambda a: (G.stem_desc(a[6], a[7], a[8], a[9]), False),
    'mrcnn_deconv2x2s2_fwd': lambda a: (G.Desc(a[4], a[5], a[6], a[7], a[8], 2, 2, 2, 0), False),
    'mrcnn_deconv2x2s2_fwd_wt': lambda a: (G.Desc(a[4], a[5], a[6], a[7], a[8], 2, 2, 2, 0), False),
    'mrcnn_deconv2x2s2_dgrad': lambda a: (G.Desc(a[3], a[4], a[5], a[6], a[7], 2, 2, 2, 0), False),
    'mrcnn_deconv2x2s2_wgrad': lambda a: (G.Desc(a[3], a[4], a[5], a[6], a[7], 2, 2, 2, 0), bool(L._addr(a[8]))),
    'mrcnn_conv3x3_wino_fwd': lambda a: (_desc_of(a[0]), True),
    'mrcnn_conv3x3_wino_dgrad': lambda a: (_desc_of(a[0]), True),
    'mrcnn_conv3x3_wino_wgrad': lambda a: (_desc_of(a[0]), True),
}


class Session(object):
    """One test's harness: the knobs (restored to the library defaults on exit), a LaunchChecker under
    every ``_lib.call``, NaN-prefilled outputs of the host code (``nan_allocs`` counts them), and per
    ``case`` the profiler's GEMM launch counts against route()'s prediction for the calls made."""

    def __init__(self, monkeypatch, family, knobs=None, predict=True):
        self.mp, self.family, self.predict = monkeypatch, family, predict
        self.knobs = dict(G.DEFAULT_KNOBS)
        self.knobs.update(knobs or {})
        self.chk = L.LaunchChecker()
        self.predicted = collections.Counter()
        self.labels = []
        self.nan_allocs = 0
        self.lib = _lib.load()

    def set(self, **knobs):
        for k, v in knobs.items():
            _lib.set_tuning(k, v)
            self.knobs[k] = v

    def __enter__(self):
        self.set(**self.knobs)
        self.chk.install(self.mp)
        checked = _lib.call

        def call(name, *args):
            checked(name, *args)
            dec = _DECODE.get(name)
            if dec is not None:
                d, ws = dec(args)
                r = G.route(name[len('mrcnn_'):], d, 0, ws, self.knobs)
                self.predicted.update(r.record)
                self.labels.append((name, r.label))
        self._call = call
        self.mp.setattr(_lib, 'call', call)

        def nan_alloc(*args, **kwargs):
            self.nan_allocs += 1
            return _nan_empty_nhwc(*args, **kwargs)
        allocating = [m for m in _HOST_MODULES if hasattr(m, 'empty_nhwc')]
        assert _conv_launch in allocating
        for m in allocating:
            self.mp.setattr(m, 'empty_nhwc', nan_alloc)
        return self

    def __exit__(self, *exc):
        self.lib.mrcnn_profile_enable(0)
        for k, v in G.DEFAULT_KNOBS.items():
            _lib.set_tuning(k, v)
        print('\n== %s ==\n%s' % (self.family, self.chk.table()))
        return False

    @contextlib.contextmanager
    def unchecked(self):
        """Library calls inside go straight to the library: no reference, no prediction."""
        _lib.call = self.chk._orig
        try:
            yield
        finally:
            _lib.call = self._call

    def case(self, cid, own_outputs=False):
        """``own_outputs``: every output of the case is a buffer of the test's own (guarded or
        NaN-filled), none comes from the host code's allocator."""
        return _Case(self, cid, own_outputs)

    def assert_clean(self):
        self.chk.assert_clean()


class _Case(object):
    def __init__(self, sess, cid, own_outputs):
        self.s, self.cid, self.own_outputs = sess, cid, own_outputs

    def __enter__(self):
        s = self.s
        s.predicted.clear()
        del s.labels[:]
        self.fails = len(s.chk.fails)
        self.allocs = s.nan_allocs
        _lib.check(s.lib.mrcnn_profile_enable(3), 'profile_enable')
        return self

    def __exit__(self, et, ev, tb):
        s = self.s
        try:
            torch.cuda.synchronize()
            kinds = _gemm_kinds()
        finally:
            s.lib.mrcnn_profile_enable(0)
        if et is not None:
            if issubclass(et, AssertionError) or issubclass(et, _lib.MrcnnHipError):
                raise et('[%s] %s' % (self.cid, ev)).with_traceback(tb)
            return False
        new = s.chk.fails[self.fails:]
        assert not new, '[%s] over the bound: %s' % (self.cid, ['%s %s: %.4g' % f for f in new[:8]])
        if s.predict:
            assert kinds == dict(s.predicted), '[%s] GEMM launches %s, route() predicted %s via %s' % (
                self.cid, kinds, dict(s.predicted), s.labels)
        allocs = s.nan_allocs - self.allocs
        if self.own_outputs:
            assert allocs == 0, '[%s] declares its own outputs, but the host code allocated %d' % (self.cid, allocs)
        else:
            assert allocs > 0, '[%s] the NaN-prefilling allocator was never called: nothing would show ' \
                'an output element that a kernel leaves unwritten' % self.cid
        return False


def _conv_case(dev, d, bias=True, fused=False, seed=None):
    """F.conv2d forward + backward of descriptor ``d``; returns (y, gx, gW) for bit comparisons."""
    x, w, gy = G.operands(d, seed)
    rng = np.random.RandomState(G.seed_of(*d) + 1)
    xt, wt = _t(x, dev, True), _t(w, dev, True)
    kw = {}
    bt = None
    if fused:
        kw = dict(scale=_t(rng.uniform(.5, 1.5, d.K).astype(np.float32), dev),
                  shift=_t(rng.standard_normal(d.K).astype(np.float32), dev),
                  residual=_t(rng.standard_normal((d.N, d.K, d.P, d.Q)).astype(np.float32), dev, True),
                  relu=True)
    elif bias:
        bt = _t(rng.standard_normal(d.K).astype(np.float32), dev, True)
    y = F.conv2d(xt, wt, bt, stride=d.stride, pad=d.pad, **kw)
    y.backward(_t(gy, dev))
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(xt.grad).all()) and \
        bool(torch.isfinite(wt.grad).all()), 'a NaN of the prefill was left in an output'
    return y.detach(), xt.grad, wt.grad


# ---- tile-boundary grid, pointwise ----------------------------------------------------------------

@pytest.mark.parametrize('M', G.PW_M)
def test_pointwise_grid(dev, monkeypatch, M):
    """(1, Cin, 1, M) under a 1x1 filter with bias, forward and backward: rows, columns and depth one
    below, at and one above 32 / 64 / 128."""
    with Session(monkeypatch, 'pointwise grid') as s:
        for cid, c in G.PW_GRID:
            if c[0] == M:
                with s.case(cid):
                    _conv_case(dev, G.pw_desc(*c))
        s.assert_clean()
        assert set(s.chk.stats) == {'mrcnn_conv2d_fwd', 'mrcnn_filter_flip_transpose', 'mrcnn_conv2d_dgrad_wt',
                                    'mrcnn_conv2d_wgrad', 'mrcnn_colsum'}


@pytest.mark.parametrize('split_bf16', [3, 0], ids=['split_bf16x3', 'fp32'])
def test_pointwise_grid_128x128_tiles(dev, monkeypatch, split_bf16):
    """The sub-grid with more than 64 rows and columns on 128x128 tiles (big_min_tiles = 1), both
    arithmetics."""
    with Session(monkeypatch, 'pointwise grid 128x128 %d' % split_bf16,
                 dict(big_min_tiles=1, split_bf16=split_bf16)) as s:
        for cid, c in G.PW_BIG_GRID:
            with s.case(cid):
                _conv_case(dev, G.pw_desc(*c))
                assert s.labels[0] == ('mrcnn_conv2d_fwd', 'big/all_rows'), s.labels
        s.assert_clean()


def test_pointwise_diagonal_fused_epilogue_and_pw_knob(dev, monkeypatch):
    """A diagonal of the grid with affine + residual + ReLU; pw = 0 / 1 / 2 / 3 select instantiations
    of the same arithmetic: bit-identical."""
    with Session(monkeypatch, 'pointwise diagonal') as s:
        for cid, c in G.PW_DIAGONAL:
            outs = []
            for pw in (3, 0, 1, 2):
                s.set(pw=pw)
                with s.case('%s pw=%d' % (cid, pw)):
                    outs.append(_conv_case(dev, G.pw_desc(*c), fused=True))
            for o in outs[1:]:
                assert all(torch.equal(a, b) for a, b in zip(o, outs[0])), '[%s] pw changes the bits' % cid
        s.assert_clean()


# ---- small maps under real filters ------------------------------------------------------------------

@pytest.mark.parametrize('geom', G.SMALL_MAP_GEOMS, ids=[g[0] for g in G.SMALL_MAP_GEOMS])
def test_small_maps(dev, monkeypatch, geom):
    """Filters larger than the map, 1 .. 129 images across choose_perm's 64 and kPermBlock = 128, in
    natural and position-major order: each within the bound of float64, each bit-repeatable."""
    with Session(monkeypatch, 'small maps') as s:
        for cid, d in G.small_map_cases(geom):
            outs = {}
            for pm in (1, 0) if d.N >= 64 else (1,):
                s.set(position_major_rows=pm)
                with s.case('%s position_major_rows=%d' % (cid, pm)):
                    outs[pm] = _conv_case(dev, d)
                with s.unchecked():                                  # the repeat: same bits
                    again = _conv_case(dev, d)
                assert all(torch.equal(a, b) for a, b in zip(again, outs[pm])), '[%s] not repeatable' % cid
            if len(outs) == 2:
                for a, b in zip(outs[0], outs[1]):
                    L._close(a.cpu().numpy(), b.double().cpu().numpy())
        s.assert_clean()


def test_position_threshold_of_choose_perm(dev, monkeypatch):
    with Session(monkeypatch, 'small maps') as s:
        for cid, d in G.PERM_POSITIONS:
            with s.case(cid):
                _conv_case(dev, d)
        s.assert_clean()


# ---- direct C-ABI calls with guard bands --------------------------------------------------------------

def _dev_nhwc(a, dev):
    """NCHW array -> dense NHWC device tensor (flat buffer the kernels read)."""
    return None if a is None else torch.tensor(np.ascontiguousarray(a.transpose(0, 2, 3, 1)), device=dev)


def _krsc(w, dev):
    return torch.tensor(np.ascontiguousarray(w.transpose(0, 2, 3, 1)), device=dev)


def _cdesc(d):
    return _lib.ConvDesc(d.N, d.H, d.W, d.C, d.K, d.R, d.S, d.stride, d.pad, d.P, d.Q)


def _guard_ok(g, cid, defined=None):
    why = g.check(defined)
    assert why is None, '[%s] %s' % (cid, why)


def _dgrad_direct(dev, cid, d, entry, variant, ws, wT=None):
    """One call of conv2d_dgrad / _ex / _wt into a guarded gx."""
    x, w, gy = G.operands(d)
    rng = np.random.RandomState(G.seed_of(*d) + 7)
    flags, rg, ry, mk, sc, prev = G.dgrad_flags_operands(variant, d, rng)
    g = G.Guarded(d.N * d.H * d.W * d.C, dev)
    if prev is not None:
        g.out.copy_(_dev_nhwc(prev, dev).reshape(-1))
    gyt, wt = _dev_nhwc(gy, dev), _krsc(w, dev)
    rg, ry, mk = (_dev_nhwc(a, dev) for a in (rg, ry, mk))
    sct = None if sc is None else torch.tensor(sc, device=dev)
    dd = _cdesc(d)
    if entry == 'conv2d_dgrad':
        _lib.call('mrcnn_conv2d_dgrad', C.ctx_desc(dd), _lib.ptr(gyt), _lib.ptr(wt), _lib.ptr(g.out), flags,
                  _lib.stream_ptr())
    else:
        if entry == 'conv2d_dgrad_wt':
            wT = torch.empty_like(wt)
            _lib.call('mrcnn_filter_flip_transpose', _lib.ptr(wt), _lib.ptr(wT), d.K, d.R, d.S, d.C, None,
                      _lib.stream_ptr())
        _lib.call('mrcnn_' + entry, C.ctx_desc(dd), _lib.ptr(gyt), _lib.ptr(wT if wT is not None else wt),
                  _lib.ptr(g.out), flags, _lib.ptr(rg), _lib.ptr(ry), _lib.ptr(mk), _lib.ptr(sct),
                  _lib.ptr(C.split_ws(dev)) if ws else None, _lib.stream_ptr())
    torch.cuda.synchronize()
    _guard_ok(g, cid)
    return g.out.view(d.N, d.H, d.W, d.C)


@pytest.mark.parametrize('variant', G.DGRAD_VARIANTS)
def test_k_strided_dgrad_entry_points(dev, monkeypatch, variant):
    """mrcnn_conv2d_dgrad_ex (and mrcnn_conv2d_dgrad for the pieces it has) on a sub-grid of the
    pointwise grid and the 3x3 / pad 1 small maps, with the split workspace and without; the
    64 x 64 x 1024 problem puts the fused pieces through splitk_epilogue_kernel."""
    with Session(monkeypatch, 'K-strided dgrad, direct') as s:
        for cid, d in G.DGRAD_DIRECT:
            for ws in (True, False):
                with s.case('%s %s ws=%d' % (cid, variant, ws), own_outputs=True):
                    _dgrad_direct(dev, cid, d, 'conv2d_dgrad_ex', variant, ws)
            if variant in ('plain', 'accum'):
                with s.case('%s %s plain entry' % (cid, variant), own_outputs=True):
                    _dgrad_direct(dev, cid, d, 'conv2d_dgrad', variant, False)
        cid, d = G.DGRAD_TINY_SPLIT
        for ws, label in ((True, 'small/tiny_split'), (False, 'small/plain')):
            with s.case('%s %s ws=%d' % (cid, variant, ws), own_outputs=True):
                _dgrad_direct(dev, cid, d, 'conv2d_dgrad_ex', variant, ws)
                assert s.labels == [('mrcnn_conv2d_dgrad_ex', label)], s.labels
        s.assert_clean()
        assert s.chk.stats['mrcnn_conv2d_dgrad_ex'][0] >= 2 * len(G.DGRAD_DIRECT)


def test_strided_1x1(dev, monkeypatch):
    """1x1 / stride 2 on 1x1 .. 13x10 maps: forward, then the data gradient on the transposed-filter
    route (conv2d_dgrad_wt) and the K-strided one (conv2d_dgrad_ex), each with and without ACCUM.
    Without ACCUM the pixels between the strided ones are exact zeros."""
    with Session(monkeypatch, 'strided 1x1') as s:
        for cid, d in G.STRIDED:
            x, w, gy = G.operands(d)
            with s.case(cid + ' forward', own_outputs=True):
                y = G.Guarded(d.N * d.P * d.Q * d.K, dev)
                xt, wt = _dev_nhwc(x, dev), _krsc(w, dev)
                _lib.call('mrcnn_conv2d_fwd', C.ctx_desc(_cdesc(d)), _lib.ptr(xt), _lib.ptr(wt), None, None, None,
                          None, _lib.ptr(y.out), 0, _lib.ptr(C.split_ws(dev)), _lib.stream_ptr())
                torch.cuda.synchronize()
                _guard_ok(y, cid)
            between = torch.ones((d.N, d.H, d.W, d.C), dtype=torch.bool, device=dev)
            between[:, ::2, ::2] = False
            for entry in ('conv2d_dgrad_wt', 'conv2d_dgrad_ex'):
                for variant in ('plain', 'accum'):
                    with s.case('%s %s %s' % (cid, entry, variant), own_outputs=True):
                        gx = _dgrad_direct(dev, cid, d, entry, variant, True)
                        if variant == 'plain':
                            assert bool((gx[between] == 0).all()), '[%s] %s: not exact zeros between the ' \
                                'strided pixels' % (cid, entry)
        s.assert_clean()


@pytest.mark.parametrize('pixels', G.WGRAD_PIXELS)
def test_wgrad_by_pixel_count(dev, monkeypatch, pixels):
    """conv2d_wgrad / _ex direct: fewer pixels than one K slice, just off multiples of 32, 8 slices and
    beyond (where splits begin), with the workspace and with NULL, with and without out_row_scale."""
    with Session(monkeypatch, 'wgrad by pixel count') as s:
        for cid, d in G.WGRAD_BY_PIXELS:
            if d.W != pixels:
                continue
            x, w, gy = G.operands(d)
            xt, gyt = _dev_nhwc(x, dev), _dev_nhwc(gy, dev)
            rs = torch.tensor(np.random.RandomState(pixels).uniform(.5, 1.5, d.K).astype(np.float32), device=dev)
            ws = _lib.workspace(_lib.load().mrcnn_conv2d_wgrad_workspace_bytes(C.ctx_desc(_cdesc(d))), dev, 'wgrad')
            for has_ws in (True, False):
                for scale in (None, rs):
                    with s.case('%s ws=%d scale=%d' % (cid, has_ws, scale is not None), own_outputs=True):
                        g = G.Guarded(d.K * d.C, dev)
                        args = (C.ctx_desc(_cdesc(d)), _lib.ptr(xt), _lib.ptr(gyt), _lib.ptr(g.out),
                                _lib.ptr(ws) if has_ws else None)
                        if scale is None:
                            _lib.call('mrcnn_conv2d_wgrad', *(args + (_lib.stream_ptr(),)))
                        else:
                            _lib.call('mrcnn_conv2d_wgrad_ex', *(args + (_lib.ptr(scale), _lib.stream_ptr())))
                        torch.cuda.synchronize()
                        _guard_ok(g, cid)
                        want = 'wgrad/no_ws' if not has_ws else (
                            'wgrad64/one_slab' if pixels < 512 else 'wgrad64/split+reduce')
                        assert s.labels[-1][1] == want, (cid, s.labels)
        s.assert_clean()


def test_wgrad_wperm_gates(dev, monkeypatch):
    """The position-major weight gradient's gate: C % 64 on 64x64 tiles, C % 128 on 128x128 tiles, 64
    images; both sides of each."""
    with Session(monkeypatch, 'wgrad WPERM gates') as s:
        for cid, d, kn, label in G.WGRAD_WPERM:
            s.set(**dict(G.DEFAULT_KNOBS, **kn))
            x, w, gy = G.operands(d)
            xt, gyt = _dev_nhwc(x, dev), _dev_nhwc(gy, dev)
            ws = _lib.workspace(_lib.load().mrcnn_conv2d_wgrad_workspace_bytes(C.ctx_desc(_cdesc(d))), dev, 'wgrad')
            with s.case(cid, own_outputs=True):
                g = G.Guarded(d.K * 9 * d.C, dev)
                _lib.call('mrcnn_conv2d_wgrad_ex', C.ctx_desc(_cdesc(d)), _lib.ptr(xt), _lib.ptr(gyt), _lib.ptr(g.out),
                          _lib.ptr(ws), None, _lib.stream_ptr())
                torch.cuda.synchronize()
                _guard_ok(g, cid)
                assert s.labels == [('mrcnn_conv2d_wgrad_ex', label)], s.labels
        s.assert_clean()


# ---- deconvolution, linear, stem ----------------------------------------------------------------------

@pytest.mark.parametrize('forward_form', [True, False], ids=['forward form', 'K-strided form'])
def test_deconv_column_groups(dev, monkeypatch, forward_form):
    """Deconvolution 2x2 / 2 + bias + ReLU and its three gradients with 4K in {16, 80, 144, 256} (a
    column group (a, b, o) straddles a tile unless 4K is a multiple of 64), ragged C, 1 .. 196 pixels."""
    monkeypatch.setattr(C, 'DECONV_FORWARD_FORM', forward_form)
    with Session(monkeypatch, 'deconvolution') as s:
        for cid, d in G.DECONV:
            rng = np.random.RandomState(G.seed_of(*d))
            x = rng.standard_normal((d.N, d.C, d.H, d.W)).astype(np.float32)
            w = (rng.standard_normal((d.C, d.K, 2, 2)) / math.sqrt(d.C)).astype(np.float32)
            b = rng.standard_normal(d.K).astype(np.float32)
            gy = rng.standard_normal((d.N, d.K, 2 * d.H, 2 * d.W)).astype(np.float32)
            with s.case(cid):
                xt, wt, bt = _t(x, dev, True), _t(w, dev, True), _t(b, dev, True)
                y = F.deconv2x2s2(xt, wt, bt, relu=True)
                y.backward(_t(gy, dev))
                assert all(bool(torch.isfinite(t).all()) for t in (y, xt.grad, wt.grad, bt.grad))
        s.assert_clean()
        want = 'mrcnn_deconv2x2s2_fwd_wt' if forward_form else 'mrcnn_deconv2x2s2_fwd'
        assert want in s.chk.stats and 'mrcnn_deconv2x2s2_dgrad' in s.chk.stats and \
            'mrcnn_deconv2x2s2_wgrad' in s.chk.stats


def test_linear(dev, monkeypatch):
    """F.linear at 1, 2, 64, 65 rows; one row 2048 deep must take small/tiny_split."""
    with Session(monkeypatch, 'linear') as s:
        for cid, (R, Cin, Cout) in G.LINEAR:
            rng = np.random.RandomState(G.seed_of(R, Cin, Cout))
            x = rng.standard_normal((R, Cin)).astype(np.float32)
            w = (rng.standard_normal((Cout, Cin)) / math.sqrt(Cin)).astype(np.float32)
            b = rng.standard_normal(Cout).astype(np.float32)
            with s.case(cid):
                xt, wt, bt = _t(x, dev, True), _t(w, dev, True), _t(b, dev, True)
                y = F.linear(xt, wt, bt)
                y.backward(_t(rng.standard_normal((R, Cout)).astype(np.float32), dev))
                assert all(bool(torch.isfinite(t).all()) for t in (y, xt.grad, wt.grad, bt.grad))
                if R == 1 and Cin == 2048:
                    assert s.labels[0] == ('mrcnn_conv2d_fwd', 'small/tiny_split'), s.labels
        s.assert_clean()


def test_stem_on_tiny_images(dev, monkeypatch):
    """The stem's 7x7 / 2 on images smaller than the filter, through pad_image_nhwc4 / pack_stem_filter."""
    from chainer_mask_rcnn_amd.models.resnet_extractor import pack_stem_filter, pad_image_nhwc4
    with Session(monkeypatch, 'stem') as s:
        for cid, (N, H, W, K, aff) in G.STEM:
            rng = np.random.RandomState(G.seed_of(N, H, W, K))
            x = rng.uniform(-120, 130, (N, 3, H, W)).astype(np.float32)
            w = (rng.standard_normal((K, 3, 7, 7)) / 12.).astype(np.float32)
            b = _t(rng.standard_normal(K).astype(np.float32), dev)
            sc = _t(rng.uniform(.5, 1.5, K).astype(np.float32), dev) if aff else None
            sh = _t(rng.standard_normal(K).astype(np.float32), dev) if aff else None
            with s.case(cid):
                y = F.stem_conv(pad_image_nhwc4(_t(x, dev)), pack_stem_filter(_t(w, dev)), b, sc, sh)
                assert bool(torch.isfinite(y).all()) and tuple(y.shape) == (N, K, (H - 1) // 2 + 1, (W - 1) // 2 + 1)
        s.assert_clean()


# ---- policy branches with ragged last tiles -------------------------------------------------------------

def _policy_params():
    out = []
    for cid, entry, d, kn, label in G.policy_cases():
        for sb in ((3, 0) if entry == 'conv2d_fwd' else (3,)):
            out.append(pytest.param(entry, d, dict(kn, split_bf16=sb), label,
                                    id='%s%s' % (cid, '' if sb == 3 else ' fp32')))
    return out


@pytest.mark.parametrize('entry,d,knobs,label', _policy_params())
def test_policy_branch_with_ragged_tiles(dev, monkeypatch, entry, d, knobs, label, request):
    """One problem per branch of launch<MODE>: a partial last tile in the rows, 4 mod 64 columns."""
    cid = request.node.callspec.id
    with Session(monkeypatch, 'policy branches', knobs) as s:
        x, w, gy = G.operands(d, seed=G.seed_of(d.W, d.C, d.K))
        with s.case(cid, own_outputs=True):
            if entry == 'conv2d_fwd':
                rng = np.random.RandomState(1)
                b = torch.tensor(rng.standard_normal(d.K).astype(np.float32), device=dev)
                y = G.Guarded(d.N * d.P * d.Q * d.K, dev)
                xt, wt = _dev_nhwc(x, dev), _krsc(w, dev)
                _lib.call('mrcnn_conv2d_fwd', C.ctx_desc(_cdesc(d)), _lib.ptr(xt), _lib.ptr(wt), _lib.ptr(b), None,
                          None, None, _lib.ptr(y.out), EPI_BIAS | EPI_RELU, _lib.ptr(C.split_ws(dev)),
                          _lib.stream_ptr())
                torch.cuda.synchronize()
                _guard_ok(y, cid)
            else:
                _dgrad_direct(dev, cid, d, 'conv2d_dgrad_ex', 'all', True)
            assert [lb for _, lb in s.labels] == [label], s.labels
        print('policy case: %s -> %s' % (cid, label))
        s.assert_clean()


# ---- Winograd at tiny maps ------------------------------------------------------------------------------

def _rel_to_scale(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize('case', G.WINOGRAD)
def test_winograd_tiny_maps(dev, monkeypatch, case):
    """wino_fwd / wino_dgrad / wino_wgrad_into on maps of one partial tile: the bound, and the level
    test_gpu_winograd.py pins (max error <= 1e-5 of the tensor scale)."""
    N, Cc, H, W, K = case
    d = G.desc(N, Cc, H, W, K, 3, 3, 1, 1)
    x, w, gy = G.operands(d)
    with Session(monkeypatch, 'winograd tiny maps') as s:
        with s.case('winograd %s' % (case,)):
            xt, wt, gt = nhwc(_t(x, dev)), nhwc(_t(w, dev)), nhwc(_t(gy, dev))
            dd = C.make_desc(xt.shape, wt.shape, 1, 1)
            y, v = C.wino_fwd(xt, wt, dd, None, None, False, keep_v=True)
            gx = C.wino_dgrad(dd, gt, wt)
            gW = torch.full_like(wt, NAN)
            C.wino_wgrad_into(dd, None, v, gt, gW)
            gW2 = torch.full_like(wt, NAN)
            C.wino_wgrad_into(dd, xt, None, gt, gW2)
            torch.cuda.synchronize()
            X, Wt, Gy = (torch.tensor(a, device=dev, dtype=torch.float64) for a in (x, w, gy))
            for what, got, ref in (('forward', y, L.conv_fwd(X, Wt, 1, 1)),
                                   ('dgrad', gx, L.conv_dgrad(Gy, Wt, H, W, 1, 1)),
                                   ('wgrad', gW, L.conv_wgrad(X, Gy, 3, 3, 1, 1))):
                assert L.ratio(got, ref) <= 1., what
                assert _rel_to_scale(got, ref) <= 1e-5, what
            assert torch.equal(gW, gW2)
        s.assert_clean()


# ---- rejected by design ---------------------------------------------------------------------------------

def test_rejected_shapes_raise_and_leave_the_library_usable(dev, monkeypatch):
    """A shape an entry point rejects by design raises MrcnnHipError; a valid call right after it is
    correct."""
    with Session(monkeypatch, 'rejected') as s:
        for cid, entry, d in G.REJECTED:
            entry, _, extra = entry.partition('+')
            buf = torch.zeros((1 << 16,), device=dev)
            dd = _cdesc(d)
            rg = _lib.ptr(buf) if extra == 'res_g' else None
            with s.unchecked(), pytest.raises(_lib.MrcnnHipError):
                if entry == 'conv2d_fwd':
                    _lib.call('mrcnn_conv2d_fwd', C.ctx_desc(dd), _lib.ptr(buf), _lib.ptr(buf), None, None, None, None,
                              _lib.ptr(buf), 0, None, _lib.stream_ptr())
                elif entry == 'conv2d_wgrad':
                    _lib.call('mrcnn_conv2d_wgrad', C.ctx_desc(dd), _lib.ptr(buf), _lib.ptr(buf), _lib.ptr(buf), None,
                              _lib.stream_ptr())
                else:
                    _lib.call('mrcnn_' + entry, C.ctx_desc(dd), _lib.ptr(buf), _lib.ptr(buf), _lib.ptr(buf), 0, rg,
                              None, None, None, None, _lib.stream_ptr())
            with s.case(cid + ': a valid call afterwards'):
                _conv_case(dev, G.desc(2, 8, 3, 3, 8, 3, 3, 1, 1))
        s.assert_clean()
