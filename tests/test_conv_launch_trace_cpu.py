"""Launch trace of the convolution host code (functions/conv.py, functions/stage.py and the two
modules below them) without a device.

The host side of the convolutions decides WHICH entry point of libmrcnn_hip.so runs with WHICH
arguments: the routes (implicit GEMM / Winograd / row-sparse / transposed-filter data gradient),
the fused epilogue pieces, who owns a weight gradient (arena slot, fresh tensor, defer queue).  None
of that needs a GPU: with ``_lib.call`` replaced by a recorder, the ``*_bytes`` queries by constants
and the device check switched off, ``building_block`` / ``conv2d`` / ``deconv2x2s2`` / ``linear`` and
their backward run on CPU tensors (the kernels' outputs stay uninitialised; nothing reads them on the
host) and yield the list of launches.

One line per launch: the entry point, every scalar, the fields of a descriptor, and for every pointer
WHAT it points to where that is one of the case's named tensors (a parameter, its ``.grad`` when the
gradient is arena-backed, an affine vector, the input, a table) or a cached workspace (``ws:<tag>``);
any other buffer is ``ptr``, a null pointer ``null``.

tests/golden/conv_launch_trace.txt is the record of the tree BEFORE the stage node's bookkeeping was
given names (the host code was refactored against it): it is not regenerated when this file's cases
pass or fail, only — case by case, with the reason in the commit — when a launch is changed on
purpose.  ``python tests/test_conv_launch_trace_cpu.py`` prints the current trace in the golden
file's format.  The weight-gradient side stream needs a real stream and stays with the GPU tests.
"""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from chainer_mask_rcnn_amd import _lib, optimizers                     # noqa: E402
from chainer_mask_rcnn_amd import functions as F                        # noqa: E402
from chainer_mask_rcnn_amd.functions import conv as C                   # noqa: E402
from chainer_mask_rcnn_amd.models.resnet_extractor import Bottleneck    # noqa: E402

GOLDEN_FILE = os.path.join(ROOT, 'tests', 'golden', 'conv_launch_trace.txt')
_DESC_FIELDS = [k for k, _ in _lib.ConvDesc._fields_]


class _FakeLib(object):
    """Stands in for the loaded library: every ``*_bytes`` query answers 1024."""

    def __getattr__(self, name):
        if not name.endswith('_bytes'):
            raise AttributeError(name)
        return lambda *args: 1024


class Recorder(object):
    """Replaces the four ``_lib`` functions that need a device or the library; ``lines`` is the trace."""

    def __init__(self):
        self.lines = []
        self.tensors = []          # (label, tensor)
        self.params = []           # (label, parameter): its .grad is labelled '<label>.grad'
        self.ws_cache = {}

    def install(self, monkeypatch):
        fake = _FakeLib()
        monkeypatch.setattr(_lib, 'call', self.call)
        monkeypatch.setattr(_lib, 'load', lambda: fake)
        monkeypatch.setattr(_lib, 'stream_ptr', lambda: 'stream')
        monkeypatch.setattr(_lib, 'require_device', lambda *tensors: None)
        monkeypatch.setattr(_lib, '_ws_cache', self.ws_cache)

    def name(self, label, t):
        self.tensors.append((label, t))
        return t

    def name_module(self, prefix, module):
        for n, p in module.named_parameters():
            self.params.append((prefix + n, p))

    def mark(self, text):
        self.lines.append('# ' + text)

    def _labels(self):
        out = {}
        for (_, _, tag), buf in self.ws_cache.items():
            out[buf.data_ptr()] = 'ws:' + tag
        for label, t in self.tensors:
            out[t.data_ptr()] = label
        for label, p in self.params:
            out[p.data_ptr()] = label
            if p.grad is not None:
                out[p.grad.data_ptr()] = label + '.grad'
        return out

    def _fmt(self, a, labels):
        if a is None:
            return 'null'
        if isinstance(a, str):
            return a
        if isinstance(a, bool):
            return repr(int(a))
        if isinstance(a, (int, float)):
            return repr(a)
        if isinstance(a, ctypes.c_void_p):
            return self._fmt_ptr(a.value, labels)
        if isinstance(a, ctypes.Array):
            if a._type_ is ctypes.c_void_p:
                return '[' + ','.join(self._fmt_ptr(v, labels) for v in a) + ']'
            return '[' + ','.join(repr(int(v)) for v in a) + ']'
        obj = getattr(a, '_obj', None)           # ctypes.byref(ConvDesc)
        if isinstance(obj, _lib.ConvDesc):
            return 'desc(' + ' '.join('%s=%d' % (k, getattr(obj, k)) for k in _DESC_FIELDS) + ')'
        raise TypeError('launch argument of unexpected type: %r' % (a,))

    @staticmethod
    def _fmt_ptr(value, labels):
        if not value:
            return 'null'
        return labels.get(value, 'ptr')

    def call(self, name, *args):
        labels = self._labels()
        self.lines.append(' '.join([name] + [self._fmt(a, labels) for a in args]))


# ---- the cases -------------------------------------------------------------------------------------

def _freeze_affine(block):
    for bn in ('bn1', 'bn2', 'bn3', 'bn4'):
        if hasattr(block, bn):
            optimizers.disable_update(getattr(block, bn))


def _stage(rec, in_ch, mid_ch, out_ch, stride, n_blocks):
    torch.manual_seed(0)
    blocks = [Bottleneck(in_ch, mid_ch, out_ch, stride, projection=True)]
    blocks += [Bottleneck(out_ch, mid_ch, out_ch) for _ in range(n_blocks - 1)]
    for name, b in zip(['a'] + ['b%d' % i for i in range(1, n_blocks)], blocks):
        _freeze_affine(b)
        rec.name_module(name + '.', b)
    return blocks


def _input(rec, shape, requires_grad, label='x'):
    n, c, h, w = shape
    x = torch.randn((n, h, w, c)).permute(0, 3, 1, 2)
    x.requires_grad_(requires_grad)
    return rec.name(label, x)


def _backbone(rec, mp, x_grad):
    """res3-like: a strided projection block and two identity blocks; one filter of an inner block is
    frozen, so every needs_input_grad index must land on its own filter."""
    mp.setattr(C, 'SMALL_WGRAD_MAX_PIXELS', -1)
    blocks = _stage(rec, 16, 8, 32, 2, 3)
    blocks[1].conv3.W.requires_grad_(False)
    x = _input(rec, (2, 16, 8, 12), x_grad)
    y = F.building_block(x, blocks)
    rec.mark('backward')
    y.backward(torch.ones_like(y))


def _head_pieces(rec, mp):
    mp.setattr(C, 'SMALL_WGRAD_MAX_PIXELS', -1)
    mp.setattr(C, 'WINOGRAD_MIN_CHANNELS', 8)
    mp.setattr(C, 'WINOGRAD_MIN_WORK', 0)
    blocks = _stage(rec, 32, 16, 64, 2, 3)
    rois = rec.name('rois', torch.tensor([[0, 1, 1, 40, 30], [0, 8, 4, 60, 50], [1, 0, 0, 90, 70],
                                          [1, 20, 10, 100, 60], [1, 5, 5, 25, 45]], dtype=torch.float32))
    order = rec.name('order', torch.tensor([2, 0, 1, 4, 3], dtype=torch.int32))
    tail = torch.tensor([0, 2, 3], dtype=torch.int64)
    return blocks, rois, order, tail


def _head_backward(rec, blocks, x, rois, order, tail):
    spec = C.RoiSpec(rois, 6, 6, 1. / 16, bin_stride=2, order=order)
    pooled, sub = F.building_block(x, blocks, first_stride=1, tail_rows=tail, roi=spec)
    assert tuple(pooled.shape) == (5, 64, 1, 1) and tuple(sub.shape) == (3, 64, 3, 3)
    rec.mark('backward')
    (pooled.sum() + sub.sum()).backward()


def _head(rec, mp, train_forward):
    """res5-like RoI head stage: pooled behind block a's projections, conv2 on the Winograd route,
    the two-output tail."""
    mp.setattr(C, 'WINOGRAD_TRAIN_FORWARD', train_forward)
    blocks, rois, order, tail = _head_pieces(rec, mp)
    x = _input(rec, (2, 32, 6, 8), True)
    _head_backward(rec, blocks, x, rois, order, tail)


def _head_no_grad(rec, mp):
    blocks, rois, order, tail = _head_pieces(rec, mp)
    x = _input(rec, (2, 32, 6, 8), True)
    with torch.no_grad():
        proj = C.projected_map(x, blocks[0].conv1.W, blocks[0].conv4.W)
        rec.mark('stage')
        spec = C.RoiSpec(rois, 6, 6, 1. / 16, bin_stride=2, order=order, proj=proj)
        F.building_block(x, blocks, first_stride=1, tail_rows=tail, roi=spec)
        rec.mark('again: cached transformed filters')
        F.building_block(x, blocks, first_stride=1, tail_rows=tail, roi=spec)
    with pytest.raises(ValueError):
        F.building_block(x, blocks, first_stride=1, tail_rows=tail, roi=spec)


def _head_pooled_first(rec, mp, tail):
    """The same stage with ``roi=None``: its input is the already pooled map (the reference order)."""
    blocks, _, _, tail_rows = _head_pieces(rec, mp)
    x = _input(rec, (5, 32, 3, 3), True)
    if tail:
        pooled, sub = F.building_block(x, blocks, first_stride=1, tail_rows=tail_rows)
        assert tuple(pooled.shape) == (5, 64, 1, 1) and tuple(sub.shape) == (3, 64, 3, 3)
        out = pooled.sum() + sub.sum()
    else:
        y = F.building_block(x, blocks, first_stride=1)
        assert tuple(y.shape) == (5, 64, 3, 3)
        out = y.sum()
    rec.mark('backward')
    out.backward()


def _head_arena(rec, mp):
    """Arena-backed parameters: gradients written in place; some held back in a DeferQueue."""
    blocks, rois, order, tail = _head_pieces(rec, mp)
    params = [p for b in blocks for p in b.parameters() if p.requires_grad]
    arena = optimizers.ParamArena(params[::-1])
    held = [blocks[0].conv1.W, blocks[0].conv2.W, blocks[0].conv4.W, blocks[1].conv3.W, blocks[2].conv2.W]
    x = _input(rec, (2, 32, 6, 8), False)
    queue = arena.defer = C.DeferQueue(held)
    _head_backward(rec, blocks, x, rois, order, tail)
    arena.defer = None
    assert len(queue.jobs) == len(held)
    rec.mark('deferred')
    C.run_deferred_wgrads(queue.jobs)
    rec.mark('second backward in the same step: every slot is taken')
    _head_backward(rec, blocks, x, rois, order, tail)
    assert arena.written() == [True] * len(params)


def _conv_layer(rec, in_ch, out_ch, k):
    torch.manual_seed(0)
    W = torch.nn.Parameter(torch.randn((out_ch, k, k, in_ch)).permute(0, 3, 1, 2))
    b = torch.nn.Parameter(torch.randn(out_ch))
    rec.params += [('W', W), ('b', b)]
    return W, b


def _stem(rec, mp):
    """The frozen stem: forward only, bias + affine + ReLU."""
    torch.manual_seed(0)
    x4 = rec.name('x4', torch.randn(2, 6, 8, 4))
    w784 = rec.name('w784', torch.randn(8, 7, 8, 4))
    b, scale, shift = (rec.name(n, torch.randn(8)) for n in ('b', 'scale', 'shift'))
    y = F.stem_conv(x4, w784, b, scale, shift)
    assert tuple(y.shape) == (2, 8, 3, 4)
    rec.mark('no affine')
    F.stem_conv(x4, w784, b, None, None)


def _conv2d_sparse(rec, mp, filled, knob=True, map_size=2 * 5 * 6):
    """``map_size``: what the hint's tables describe (the node's own map has 2 x 5 x 6 positions)."""
    mp.setattr(C, 'SPARSE_CONV_BACKWARD', knob)
    W, b = _conv_layer(rec, 8, 16, 3)
    x = _input(rec, (2, 8, 5, 6), True)
    hint = C.SparseRows()
    y = F.conv2d(x, W, b, stride=1, pad=1, relu=True, grad_rows=hint)
    if filled:
        import numpy as np
        rows, lookup = C.SparseRows.host_tables([3, 17, 40, 41], map_size)
        hint.set(rec.name('rows', torch.from_numpy(np.ascontiguousarray(rows))),
                 rec.name('lookup', torch.from_numpy(np.ascontiguousarray(lookup))), len(rows))
    rec.mark('backward')
    y.backward(torch.ones_like(y))
    # (a hint the backward did not use, for either reason, is left as it was)
    assert hint.n == (0 if knob and map_size == 2 * 5 * 6 else 4) or not filled


def _conv2d_affine_residual(rec, mp):
    W, _ = _conv_layer(rec, 8, 16, 3)
    scale = rec.name('scale', torch.rand(16) + 0.5)
    shift = rec.name('shift', torch.randn(16))
    x = _input(rec, (2, 8, 5, 6), True)
    res = _input(rec, (2, 16, 3, 3), True, 'residual')
    y = F.conv2d(x, W, None, stride=2, pad=1, scale=scale, shift=shift, residual=res, relu=True)
    rec.mark('backward')
    y.backward(torch.ones_like(y))


def _conv2d_winograd(rec, mp, train_forward):
    mp.setattr(C, 'WINOGRAD_MIN_CHANNELS', 8)
    mp.setattr(C, 'WINOGRAD_MIN_WORK', 0)
    mp.setattr(C, 'WINOGRAD_TRAIN_FORWARD', train_forward)
    W, b = _conv_layer(rec, 8, 16, 3)
    x = _input(rec, (2, 8, 5, 6), True)
    y = F.conv2d(x, W, b, stride=1, pad=1, relu=True)
    rec.mark('backward')
    y.backward(torch.ones_like(y))
    rec.mark('no_grad')
    with torch.no_grad():
        F.conv2d(x, W, b, stride=1, pad=1, relu=True)
        F.conv2d(x, W, b, stride=1, pad=1, relu=True)


def _conv2d_winograd_no_filter_cache(rec, mp):
    """Graph-free calls inside ``no_filter_cache()``: the filter is transformed per call, by the
    forward launch itself, and nothing is cached."""
    mp.setattr(C, 'WINOGRAD_MIN_CHANNELS', 8)
    mp.setattr(C, 'WINOGRAD_MIN_WORK', 0)
    W, b = _conv_layer(rec, 8, 16, 3)
    x = _input(rec, (2, 8, 5, 6), False)
    with torch.no_grad():
        with C.no_filter_cache():
            F.conv2d(x, W, b, stride=1, pad=1, relu=True)
            F.conv2d(x, W, b, stride=1, pad=1, relu=True)
            assert not C._wino_u_cache
        rec.mark('outside: cached')
        F.conv2d(x, W, b, stride=1, pad=1, relu=True)
        assert len(C._wino_u_cache) == 1


def _conv2d_winograd_bf16x1(rec, mp):
    """A Winograd-sized layer under 'bf16x1' takes the direct kernel, forward and backward."""
    mp.setattr(C, 'WINOGRAD_MIN_CHANNELS', 8)
    mp.setattr(C, 'WINOGRAD_MIN_WORK', 0)
    mp.setattr(C, 'GEMM_ARITHMETIC', 'bf16x1')
    W, b = _conv_layer(rec, 8, 16, 3)
    x = _input(rec, (2, 8, 5, 6), True)
    assert not C.uses_winograd(C.make_desc(x.shape, W.shape, 1, 1))
    y = F.conv2d(x, W, b, stride=1, pad=1, relu=True)
    rec.mark('backward')
    y.backward(torch.ones_like(y))
    rec.mark('no_grad')
    with torch.no_grad():
        F.conv2d(x, W, b, stride=1, pad=1, relu=True)


def _conv2d_arena(rec, mp, winograd):
    """In-place gradients of F.conv2d; W is named in a DeferQueue, which only the Winograd route of
    this node consults."""
    if winograd:
        mp.setattr(C, 'WINOGRAD_MIN_CHANNELS', 8)
        mp.setattr(C, 'WINOGRAD_MIN_WORK', 0)
    W, b = _conv_layer(rec, 8, 16, 3)
    arena = optimizers.ParamArena([b, W])
    x = _input(rec, (2, 8, 5, 6), False)
    queue = arena.defer = C.DeferQueue([W])
    for _ in range(2):
        y = F.conv2d(x, W, b, stride=1, pad=1, relu=True)
        rec.mark('backward')
        y.backward(torch.ones_like(y))
    arena.defer = None
    assert len(queue.jobs) == int(winograd)
    rec.mark('deferred')
    C.run_deferred_wgrads(queue.jobs)


def _deconv(rec, mp, arithmetic, arena=False):
    mp.setattr(C, 'GEMM_ARITHMETIC', arithmetic)
    torch.manual_seed(0)
    W = torch.nn.Parameter(torch.randn((8, 2, 2, 4)).permute(0, 3, 1, 2))       # (in, out, 2, 2)
    b = torch.nn.Parameter(torch.randn(4))
    rec.params += [('W', W), ('b', b)]
    if arena:
        optimizers.ParamArena([b, W])
    x = _input(rec, (3, 8, 4, 5), True)
    y = F.deconv2x2s2(x, W, b, relu=True)
    rec.mark('backward')
    y.backward(torch.ones_like(y))


def _linear(rec, mp):
    torch.manual_seed(0)
    W = torch.nn.Parameter(torch.randn(10, 24))
    b = torch.nn.Parameter(torch.randn(10))
    rec.params += [('W', W), ('b', b)]
    x = rec.name('x', torch.randn(4, 24, 1, 1).requires_grad_(True))
    y = F.linear(x, W, b)
    rec.mark('backward')
    y.backward(torch.ones_like(y))


CASES = [
    ('backbone stage, input gradient', lambda r, m: _backbone(r, m, True)),
    ('backbone stage, no input gradient', lambda r, m: _backbone(r, m, False)),
    ('head stage, WINOGRAD_TRAIN_FORWARD=True', lambda r, m: _head(r, m, True)),
    ("head stage, WINOGRAD_TRAIN_FORWARD='conv2d'", lambda r, m: _head(r, m, 'conv2d')),
    ('head stage, no_grad with RoiSpec(proj=)', _head_no_grad),
    ('head stage, arena and defer queue', _head_arena),
    ('conv2d bias relu, sparse hint filled', lambda r, m: _conv2d_sparse(r, m, True)),
    ('conv2d bias relu, sparse hint empty', lambda r, m: _conv2d_sparse(r, m, False)),
    ('conv2d affine residual relu', _conv2d_affine_residual),
    ('conv2d winograd, WINOGRAD_TRAIN_FORWARD=True', lambda r, m: _conv2d_winograd(r, m, True)),
    ("conv2d winograd, WINOGRAD_TRAIN_FORWARD='stage'", lambda r, m: _conv2d_winograd(r, m, 'stage')),
    ('conv2d arena', lambda r, m: _conv2d_arena(r, m, False)),
    ('conv2d arena, winograd', lambda r, m: _conv2d_arena(r, m, True)),
    ('deconv2x2s2 split_bf16x3', lambda r, m: _deconv(r, m, 'split_bf16x3')),
    ('deconv2x2s2 fp32', lambda r, m: _deconv(r, m, 'fp32')),
    ('deconv2x2s2 arena', lambda r, m: _deconv(r, m, 'split_bf16x3', arena=True)),
    ('linear', _linear),
    ('stem_conv', _stem),
    ('head stage, roi=None, tail_rows', lambda r, m: _head_pooled_first(r, m, True)),
    ('head stage, roi=None', lambda r, m: _head_pooled_first(r, m, False)),
    ('conv2d winograd, no_filter_cache', _conv2d_winograd_no_filter_cache),
    ('conv2d winograd-sized, bf16x1: direct kernel', _conv2d_winograd_bf16x1),
    ('conv2d bias relu, sparse hint filled, SPARSE_CONV_BACKWARD=False',
     lambda r, m: _conv2d_sparse(r, m, True, knob=False)),
    ('conv2d bias relu, sparse hint for another map size', lambda r, m: _conv2d_sparse(r, m, True, map_size=2 * 5 * 7)),
]


def trace(case, monkeypatch):
    rec = Recorder()
    rec.install(monkeypatch)
    C.weights_changed()
    try:
        case(rec, monkeypatch)
    finally:
        C.weights_changed()
    return rec.lines


def read_golden():
    cases, name = {}, None
    with open(GOLDEN_FILE) as f:
        for line in f:
            line = line.rstrip('\n')
            if line.startswith('== '):
                name = line[3:]
                cases[name] = []
            elif line:
                cases[name].append(line)
    return cases


def test_golden_file_has_exactly_the_cases():
    assert sorted(read_golden()) == sorted(name for name, _ in CASES)


@pytest.mark.parametrize('name,case', CASES, ids=[n for n, _ in CASES])
def test_launch_trace(name, case, monkeypatch):
    got = trace(case, monkeypatch)
    want = read_golden()[name]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, 'launch %d of %r differs' % (i, name)
    assert len(got) == len(want)


def test_backbone_stage_launch_count(monkeypatch):
    """A strided projection block plus two identity blocks: 10 forward launches, and per block three
    (four) data and weight gradients less the frozen filter's, the batched filter transposes and the
    stage's entry mask."""
    lines = trace(CASES[0][1], monkeypatch)
    assert len([l for l in lines if not l.startswith('#')]) == 32 - 1      # b1.conv3.W is frozen


if __name__ == '__main__':
    mp = pytest.MonkeyPatch()
    for case_name, fn in CASES:
        print('== ' + case_name)
        try:
            print('\n'.join(trace(fn, mp)))
        finally:
            mp.undo()
        print()
