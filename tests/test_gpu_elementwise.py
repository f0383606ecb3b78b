"""csrc/elementwise.hip through the C ABI at its edges, against the checks of
tests/elementwise_cases.py: the float4 and the scalar body of every entry point (C % 4, pointers
offset by one float), one / some / 128 colsum slabs with and without empty ones, grids past the
4096-workgroup cap (a second pass of the stride loop), every optional argument null and non-null.
Every operand lives inside a buffer filled with a NaN pattern and every output's surroundings are
compared with it after the launch."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import elementwise_cases as EC
from chainer_mask_rcnn_amd import _lib

pytestmark = pytest.mark.gpu
f32 = np.float32


_LIVE = []          # every Buf up to the end of the launch that may read it (see _call)


class Buf:
    """A device array inside a buffer of POISON words: GUARD words, `off` more (off = 1: the array
    is not 16-byte aligned), the array, GUARD words.  A Buf built inside an argument list stays
    alive until _call has synchronised: its block must not be handed to the next allocation."""

    def __init__(self, dev, shape, data=None, off=0):
        self.shape = tuple(shape)
        n = int(np.prod(self.shape))
        self.lo = EC.GUARD + off
        self.hi = self.lo + n
        self.words = torch.full((self.hi + EC.GUARD,), EC.POISON, dtype=torch.int32, device=dev)
        assert self.words.data_ptr() % 16 == 0
        if data is not None:
            data = np.ascontiguousarray(data)
            assert data.shape == self.shape and data.dtype == f32
            self.words[self.lo:self.hi] = torch.from_numpy(data.reshape(-1).view(np.int32)).to(dev)
        assert self.ptr.value % 16 == (4 * off) % 16
        _LIVE.append(self)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.words.data_ptr() + 4 * self.lo)

    def get(self, what='output'):
        """The array, after checking that the words around it are untouched."""
        host = self.words.cpu().numpy()
        EC.check_guard(host, self.lo, self.hi, what)
        return host[self.lo:self.hi].view(f32).reshape(self.shape).copy()

    def untouched(self):
        return bool((self.words == EC.POISON).all())


def _ptr(b):
    return None if b is None else b.ptr


def _call(name, *args):
    try:
        _lib.call(name, *args, _lib.stream_ptr())
    finally:
        torch.cuda.synchronize()
        del _LIVE[:]


def _workspace(dev, C):
    """A colsum workspace holding NaNs: a stale slab that is read shows."""
    n = _lib.load().mrcnn_colsum_workspace_bytes(C) // 4
    return torch.full((max(n, 1),), float('nan'), dtype=torch.float32, device=dev)


def _i32(a, dev):
    return torch.tensor(np.asarray(a, np.int32), dtype=torch.int32, device=dev)


DATA = (('integer', EC.ints), ('normal', EC.normal))


# ---- colsum / affine --------------------------------------------------------------------------------

def test_colsum_workspace_size(dev):
    assert _lib.load().mrcnn_colsum_workspace_bytes(132) == 128 * 132 * 4


@pytest.mark.parametrize('M', EC.COLSUM_M)
def test_colsum(dev, M):
    for C in EC.COLSUM_C:
        ws = _workspace(dev, C)
        for kind, data in DATA:
            a = data((M, C), M, C)
            out = Buf(dev, (C,))
            _call('mrcnn_colsum', Buf(dev, (M, C), a).ptr, out.ptr, M, C, _lib.ptr(ws))
            EC.check_colsum(a, out.get(), None, kind, 'colsum M%d C%d %s' % (M, C, kind))
            ws.fill_(float('nan'))
        for where in ('first', 'last') if M else ():
            a = EC.single_large(M, C, where)
            out = Buf(dev, (C,))
            _call('mrcnn_colsum', Buf(dev, (M, C), a).ptr, out.ptr, M, C, _lib.ptr(ws))
            EC.check_colsum(a, out.get(), None, 'single', 'colsum M%d C%d %s' % (M, C, where))


@pytest.mark.parametrize('M', EC.COLSUM_M)
def test_affine_bwd_every_output_combination(dev, M):
    for C in EC.COLSUM_C:
        ws = _workspace(dev, C)
        W = EC.signed_scale(C, M)
        for kind, data in DATA:
            x, gy = data((M, C), M, C, 0), data((M, C), M, C, 1)
            xb, gyb, Wb = Buf(dev, (M, C), x), Buf(dev, (M, C), gy), Buf(dev, (C,), W)
            for want in itertools.product((0, 1), repeat=3):
                gx, gW, gb = (Buf(dev, s) if w else None
                              for w, s in zip(want, ((M, C), (C,), (C,))))
                ws.fill_(float('nan'))
                _call('mrcnn_affine_bwd', xb.ptr, Wb.ptr, gyb.ptr, _ptr(gx), _ptr(gW), _ptr(gb), M,
                      C, _lib.ptr(ws))
                EC.check_affine_bwd(x, W, gy, *(None if b is None else b.get() for b in (gx, gW, gb)),
                                    kind=kind, what='affine_bwd M%d C%d %s %s' % (M, C, kind, want))


@pytest.mark.parametrize('M', [5, 129, 8128])
def test_colsum_second_call_on_a_shared_workspace_sees_no_stale_slab(dev, M):
    """128 slabs of a 20001-row call stay in the workspace; a later call with fewer slabs (and
    affine_bwd's gW followed by gb) must not add them."""
    C, big = 65, 20001
    ws = _workspace(dev, C)
    a, x = EC.ints((big, C), 0), EC.ints((M, C), 1)
    gy = EC.ints((M, C), 2)
    out = Buf(dev, (C,))
    _call('mrcnn_colsum', Buf(dev, (big, C), a).ptr, out.ptr, big, C, _lib.ptr(ws))
    EC.check_colsum(a, out.get(), None, 'integer')
    assert EC.colsum_splits(M)[0] < 128
    out = Buf(dev, (C,))
    _call('mrcnn_colsum', Buf(dev, (M, C), gy).ptr, out.ptr, M, C, _lib.ptr(ws))
    EC.check_colsum(gy, out.get(), None, 'integer')
    _call('mrcnn_colsum', Buf(dev, (big, C), a).ptr, Buf(dev, (C,)).ptr, big, C, _lib.ptr(ws))
    gW, gb = Buf(dev, (C,)), Buf(dev, (C,))
    W = EC.signed_scale(C, 0)
    _call('mrcnn_affine_bwd', Buf(dev, (M, C), x).ptr, Buf(dev, (C,), W).ptr, Buf(dev, (M, C), gy).ptr,
          None, gW.ptr, gb.ptr, M, C, _lib.ptr(ws))
    EC.check_affine_bwd(x, W, gy, None, gW.get(), gb.get(), 'integer')


@pytest.mark.parametrize('which', ['gy', 'W', 'gx'])
@pytest.mark.parametrize('C', [64, 132])
def test_affine_bwd_misaligned(dev, C, which):
    M = 65
    x, gy, W = EC.normal((M, C), 0), EC.normal((M, C), 1), EC.signed_scale(C, 0)
    off = lambda name: 1 if name == which else 0
    gx, gW, gb = Buf(dev, (M, C), off=off('gx')), Buf(dev, (C,)), Buf(dev, (C,))
    _call('mrcnn_affine_bwd', Buf(dev, (M, C), x).ptr, Buf(dev, (C,), W, off('W')).ptr,
          Buf(dev, (M, C), gy, off('gy')).ptr, gx.ptr, gW.ptr, gb.ptr, M, C,
          _lib.ptr(_workspace(dev, C)))
    EC.check_affine_bwd(x, W, gy, gx.get(), gW.get(), gb.get())


@pytest.mark.parametrize('M,C', [(7, C) for C in EC.CHANNELS] + [(0, 4), EC.EPILOGUE_BIG[0]])
def test_affine_fwd(dev, M, C):
    x, W, b = EC.normal((M, C), M, C), EC.signed_scale(C, 0), EC.signed_scale(C, 1)
    for off in ((0, 0), (1, 0), (0, 1)) if M == 7 else ((0, 0),):
        y = Buf(dev, (M, C), off=off[1])
        _call('mrcnn_affine_fwd', Buf(dev, (M, C), x, off[0]).ptr, Buf(dev, (C,), W).ptr,
              Buf(dev, (C,), b).ptr, y.ptr, M, C)
        EC.check_affine_fwd(x, W, b, y.get())


# ---- epilogue_bwd ---------------------------------------------------------------------------------------

def _epilogue(dev, M, C, with_y, with_scale, off=()):
    gy = EC.normal((M, C), M, C)
    y = EC.mask_operand((M, C), M, C) if with_y else None
    scale = EC.signed_scale(C, M) if with_scale else None
    o = lambda name: 1 if name in off else 0
    g = Buf(dev, (M, C), off=o('g'))
    _call('mrcnn_epilogue_bwd', Buf(dev, (M, C), gy, o('gy')).ptr,
          None if y is None else Buf(dev, (M, C), y, o('y')).ptr,
          None if scale is None else Buf(dev, (C,), scale, o('scale')).ptr, g.ptr, M, C)
    EC.check_epilogue_bwd(gy, y, scale, g.get(),
                          'epilogue_bwd M%d C%d y%d scale%d off %s' % (M, C, with_y, with_scale, off))


@pytest.mark.parametrize('C', EC.CHANNELS)
def test_epilogue_bwd(dev, C):
    for with_y, with_scale in itertools.product((0, 1), repeat=2):
        _epilogue(dev, 7, C, with_y, with_scale)
    if C % 4 == 0:
        for name in ('gy', 'y', 'scale', 'g'):
            _epilogue(dev, 7, C, 1, 1, off=(name,))
    _epilogue(dev, 0, C, 1, 1)


@pytest.mark.parametrize('M,C', EC.EPILOGUE_BIG)
def test_epilogue_bwd_past_the_grid_cap(dev, M, C):
    assert M * C // (4 if C % 4 == 0 else 1) > EC.GRID_CAP
    _epilogue(dev, M, C, 1, 1)


# ---- pooling ----------------------------------------------------------------------------------------------

def _maxpool(dev, shape, kind, off=(0, 0)):
    N, H, W, C = shape
    P, Q = EC.cover_all(H), EC.cover_all(W)
    x = EC.maxpool_input(shape, kind, H, W, C)
    y = Buf(dev, (N, P, Q, C), off=off[1])
    _call('mrcnn_maxpool3x3s2p1_fwd', Buf(dev, shape, x, off[0]).ptr, y.ptr, N, H, W, C, P, Q)
    EC.check_maxpool(x, y.get(), 'maxpool %s %s off %s' % (shape, kind, off))


@pytest.mark.parametrize('N,H,W', EC.MAXPOOL_MAPS)
def test_maxpool(dev, N, H, W):
    for C in EC.MAXPOOL_C:
        for kind in EC.MAXPOOL_KINDS:
            _maxpool(dev, (N, H, W, C), kind)
        if C % 4 == 0:
            _maxpool(dev, (N, H, W, C), 'negative', (1, 0))
            _maxpool(dev, (N, H, W, C), 'neginf', (0, 1))


def test_maxpool_scalar_body_past_the_grid_cap(dev):
    N, H, W, C = EC.MAXPOOL_BIG
    assert C % 4 and N * EC.cover_all(H) * EC.cover_all(W) * C > EC.GRID_CAP
    _maxpool(dev, EC.MAXPOOL_BIG, 'negative')


@pytest.mark.parametrize('dP,dQ', [(1, 0), (0, 1), (-1, 0), (0, -1)])
def test_maxpool_refuses_a_wrong_output_size(dev, dP, dQ):
    N, H, W, C = 2, 5, 8, 4
    P, Q = EC.cover_all(H) + dP, EC.cover_all(W) + dQ
    x = EC.maxpool_input((N, H, W, C), 'negative', 0)
    y = Buf(dev, (N, max(P, 3), max(Q, 5), C))
    with pytest.raises(_lib.MrcnnHipError, match='cover_all'):
        _call('mrcnn_maxpool3x3s2p1_fwd', Buf(dev, x.shape, x).ptr, y.ptr, N, H, W, C, P, Q)
    torch.cuda.synchronize()
    assert y.untouched()


@pytest.mark.parametrize('R,HW,C', EC.AVGPOOL_SHAPES)
def test_avgpool(dev, R, HW, C):
    offs = ((0, 0), (1, 0), (0, 1)) if C % 4 == 0 else ((0, 0),)
    for off in offs:
        for kind, data in DATA:
            x = data((R, HW, C), R, HW, C)
            y = Buf(dev, (R, C), off=off[1])
            _call('mrcnn_avgpool_fwd', Buf(dev, x.shape, x, off[0]).ptr, y.ptr, R, HW, C)
            EC.check_avgpool_fwd(x, y.get(), kind, 'avgpool_fwd %s %s off %s' % (x.shape, kind, off))
        gy, prior = EC.normal((R, C), R, HW, C, 1), EC.normal((R, HW, C), R, HW, C, 2)
        for acc in (0, 1):
            gx = Buf(dev, prior.shape, prior, off[1])
            _call('mrcnn_avgpool_bwd', Buf(dev, gy.shape, gy, off[0]).ptr, gx.ptr, R, HW, C, acc)
            EC.check_avgpool_bwd(gy, HW, gx.get(), prior, acc,
                                 'avgpool_bwd %s acc %d off %s' % (prior.shape, acc, off))


def _head_tail_operands(R, HW, C, kind):
    slot, n = EC.slots(R, kind, HW)
    g_pool, y = EC.normal((R, C), R, 0), EC.mask_operand((R, HW, C), R, HW)
    g_rows = EC.normal((n, HW, C), R, 1) if slot is not None else None
    return g_pool, g_rows, slot, y


@pytest.mark.parametrize('R,HW,C', EC.HEAD_TAIL_SHAPES)
@pytest.mark.parametrize('kind', EC.SLOT_KINDS)
def test_head_tail_bwd(dev, R, HW, C, kind):
    g_pool, g_rows, slot, y = _head_tail_operands(R, HW, C, kind)
    g = Buf(dev, y.shape)
    slot_d = None if slot is None else _i32(np.concatenate([slot, [0]]), dev)   # never empty
    _call('mrcnn_head_tail_bwd', Buf(dev, g_pool.shape, g_pool).ptr,
          None if g_rows is None else Buf(dev, g_rows.shape, g_rows).ptr, _lib.ptr(slot_d),
          Buf(dev, y.shape, y).ptr, g.ptr, R, HW, C)
    EC.check_head_tail_bwd(g_pool, g_rows, slot, y, g.get())


def test_head_tail_bwd_refusals_leave_the_output_untouched(dev):
    R, HW = 3, 49
    for C, off, kind, drop_slot in ((6, (), 'perm', False), (5, (), 'perm', False),
                                    (8, ('g_pool',), 'perm', False), (8, ('g_rows',), 'perm', False),
                                    (8, ('y',), 'perm', False), (8, ('g',), 'perm', False),
                                    (8, (), 'perm', True)):
        g_pool, g_rows, slot, y = _head_tail_operands(R, HW, C, kind)
        o = lambda name: 1 if name in off else 0
        g = Buf(dev, y.shape, off=o('g'))
        slot_d = None if drop_slot else _i32(slot, dev)
        with pytest.raises(_lib.MrcnnHipError):
            _call('mrcnn_head_tail_bwd', Buf(dev, g_pool.shape, g_pool, o('g_pool')).ptr,
                  Buf(dev, g_rows.shape, g_rows, o('g_rows')).ptr, _lib.ptr(slot_d),
                  Buf(dev, y.shape, y, o('y')).ptr, g.ptr, R, HW, C)
        torch.cuda.synchronize()
        assert g.untouched(), (C, off, drop_slot)


# ---- sparse 3x3 ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('N,H,W,C,K', EC.SPARSE_SHAPES)
@pytest.mark.parametrize('kind', EC.ROW_KINDS)
def test_sparse3x3_gather_and_scatter(dev, N, H, W, C, K, kind):
    rows = EC.sparse_rows(N, H, W, kind)
    n = len(rows)
    lookup = EC.lookup_of(rows, N, H, W)
    x, g = EC.normal((N, H, W, C), H, W, 0), EC.normal((N, H, W, K), H, W, 1)
    xb, gb = Buf(dev, x.shape, x), Buf(dev, g.shape, g)
    rows_d = _i32(np.concatenate([rows, [0]]), dev)                      # never empty
    first = None
    for _ in range(2 if kind == 'all' else 1):
        patches, g_rows = Buf(dev, (n, 3, 3, C)), Buf(dev, (n, K))
        _call('mrcnn_sparse3x3_gather', xb.ptr, gb.ptr, _lib.ptr(rows_d), n, N, H, W, C, K,
              patches.ptr, g_rows.ptr)
        got = patches.get(), g_rows.get()
        EC.check_sparse3x3_gather(x, g, rows, *got)
        if first is not None:
            EC.bits_equal(got[0], first[0], 'gather repeats')
        first = got
    lookup_d = _i32(lookup, dev)
    for data_kind, data in DATA:
        gp = data((n, 3, 3, C), H, W, C)
        gpb = Buf(dev, gp.shape, gp)
        first = None
        for _ in range(2 if kind == 'all' else 1):
            gx = Buf(dev, (N, H, W, C))
            _call('mrcnn_sparse3x3_scatter', gpb.ptr, _lib.ptr(lookup_d), N, H, W, C, gx.ptr)
            got = gx.get()
            EC.check_sparse3x3_scatter(gp, lookup, got, data_kind,
                                       'scatter %s %s %s' % ((N, H, W, C), kind, data_kind))
            if first is not None:
                EC.bits_equal(got, first, 'scatter repeats')
            first = got


# ---- SGD --------------------------------------------------------------------------------------------------------

SGD_ENTRIES = (('mrcnn_sgd_momentum_wd', None), ('mrcnn_sgd_momentum_wd_ex', 0),
               ('mrcnn_sgd_momentum_wd_ex', 1))


@pytest.mark.parametrize('n', EC.SGD_N)
@pytest.mark.parametrize('entry,zero_grad', SGD_ENTRIES, ids=['plain', 'ex', 'ex-zero-grad'])
def test_sgd(dev, n, entry, zero_grad):
    h = EC.SGD_HYPER
    assert h['wd'] != 0 and h['grad_scale'] != 1
    if n > EC.GRID_CAP:
        assert n // 4 + 1 > EC.GRID_CAP and n % 4 == 3
    p, g, v = (EC.normal((n,), n, k) for k in range(3))
    pb, gb, vb = (Buf(dev, (n,), a) for a in (p, g, v))
    args = [pb.ptr, gb.ptr, vb.ptr, n, h['lr'], h['momentum'], h['wd'], h['grad_scale']]
    _call(entry, *(args if zero_grad is None else args + [zero_grad]))
    EC.check_sgd(p, g, v, zero_grad=zero_grad or 0, p2=pb.get('p'), g2=gb.get('g'), v2=vb.get('v'),
                 what='%s n%d' % (entry, n), **h)


@pytest.mark.parametrize('which', [0, 1, 2])
def test_sgd_refuses_a_misaligned_arena(dev, which):
    n = 8
    bufs = [Buf(dev, (n,), EC.normal((n,), k), off=int(k == which)) for k in range(3)]
    with pytest.raises(_lib.MrcnnHipError, match='16-byte'):
        _call('mrcnn_sgd_momentum_wd_ex', *(b.ptr for b in bufs), n, 0.02, 0.9, 1e-4, 0.5, 1)
    torch.cuda.synchronize()
    for k, b in enumerate(bufs):
        EC.bits_equal(b.get(), EC.normal((n,), k), 'arena %d' % k)
