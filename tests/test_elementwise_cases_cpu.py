"""The checks of tests/elementwise_cases.py on NumPy emulations of csrc/elementwise.hip and
csrc/image.hip: every check passes on a plain restatement of the operation and fails on a
deliberately wrong one, and the cases satisfy the conditions that make them worth running (the
integer data stays below 2^24, the pasted reference masks reach past x = 256)."""
import numpy as np
import pytest

import elementwise_cases as EC
from oracle import np_infer, np_ref

f32 = np.float32


def _fails(fn, *args, **kw):
    with pytest.raises(AssertionError):
        fn(*args, **kw)


# ---- emulations -----------------------------------------------------------------------------------

def emu_colsum(a, b=None, drop_last_row=False, drop_last_slab=False, stale=None):
    """mrcnn_colsum: fp32 slab sums, then the slabs.  stale: a (128, C) workspace left by an earlier
    call whose every slab a wrong final pass would add."""
    M, C = a.shape
    prod = a if b is None else (a * b).astype(f32)
    if drop_last_row:
        prod = prod[:M - 1]
    splits, per, _ = EC.colsum_splits(M)
    ws = np.zeros((128, C), f32) if stale is None else stale.copy()
    for s in range(splits):
        ws[s] = prod[s * per:min(M, (s + 1) * per)].sum(0, dtype=f32)
    used = 128 if stale is not None else splits - (1 if drop_last_slab else 0)
    return ws[:used].sum(0, dtype=f32), ws


def emu_epilogue(gy, y, scale, ge=False):
    v = gy
    if y is not None:
        v = np.where((y >= 0) if ge else (y > 0), v, f32(0))
    if scale is not None:
        v = (v * scale[None, :]).astype(f32)
    return v.astype(f32)


def emu_maxpool(x, pad=-np.inf, window=3):
    """`window` 2 drops the last row and column of every window."""
    N, H, W, C = x.shape
    P, Q = EC.cover_all(H), EC.cover_all(W)
    xp = np.full((N, 2 * P + 1, 2 * Q + 1, C), pad, f32)
    xp[:, 1:H + 1, 1:W + 1] = x
    y = np.full((N, P, Q, C), -np.inf, f32)
    for r in range(window):
        for s in range(window):
            y = np.maximum(y, xp[:, r:r + 2 * P:2, s:s + 2 * Q:2])
    return y


def emu_avgpool_fwd(x, div=None):
    HW = x.shape[1]
    return (x.sum(1, dtype=f32) * (f32(1) / f32(div or HW))).astype(f32)


def emu_avgpool_bwd(gy, HW, prior, accumulate):
    g = np.repeat((gy * (f32(1) / f32(HW))).astype(f32)[:, None, :], HW, 1)
    return (g + prior).astype(f32) if accumulate else g


def emu_head_tail(g_pool, g_rows, slot, y, by_r=False):
    R, HW, C = y.shape
    v = np.repeat((g_pool * (f32(1) / f32(HW))).astype(f32)[:, None, :], HW, 1)
    if slot is not None:
        for r in range(R):
            if slot[r] >= 0:
                v[r] = v[r] + g_rows[r if by_r else slot[r]]
    return np.where(y > 0, v, f32(0)).astype(f32)


def emu_gather(x, g, rows, wrap=False):
    """wrap: a neighbour outside the map is read at its flat address (the next or previous row, or
    image) instead of as zero."""
    N, H, W, C = x.shape
    flat = x.reshape(-1, C)
    patches = np.zeros((len(rows), 3, 3, C), f32)
    for i, p in enumerate(rows):
        n, py, px = p // (H * W), (p // W) % H, p % W
        for r in range(3):
            for s in range(3):
                yy, xx = py + r - 1, px + s - 1
                if 0 <= yy < H and 0 <= xx < W:
                    patches[i, r, s] = x[n, yy, xx]
                elif wrap:
                    patches[i, r, s] = flat[(p + (r - 1) * W + (s - 1)) % len(flat)]
    return patches, g.reshape(-1, g.shape[3])[rows]


def emu_scatter(gp, lookup, mirror=False):
    N, H, W = lookup.shape
    gx = np.zeros((N, H, W, gp.shape[3]), f32)
    for n, qy, qx in np.ndindex(N, H, W):
        for t in range(9):
            yy, xx = qy - (t // 3 - 1), qx - (t % 3 - 1)
            if 0 <= yy < H and 0 <= xx < W and lookup[n, yy, xx] >= 0:
                tap = 8 - t if mirror else t
                gx[n, qy, qx] += gp[lookup[n, yy, xx], tap // 3, tap % 3]
    return gx


def emu_sgd(p, g, v, lr, momentum, wd, grad_scale, zero_grad, skip_tail=False):
    lr, momentum, wd, grad_scale = f32(lr), f32(momentum), f32(wd), f32(grad_scale)
    n = len(p) // 4 * 4 if skip_tail else len(p)
    p2, g2, v2 = p.copy(), g.copy(), v.copy()
    v2[:n] = momentum * v[:n] - lr * (g[:n] * grad_scale + wd * p[:n])
    p2[:n] = p[:n] + v2[:n]
    if zero_grad:
        g2[:n] = 0
    return p2, g2, v2


# ---- colsum / affine ------------------------------------------------------------------------------

def test_integer_cases_stay_exact():
    """The largest reduction of the GPU tests, in the worst case of the data's range."""
    M = max(EC.COLSUM_M)
    assert M == EC.MAX_TERMS and M * EC.INT_LIMIT ** 2 < 2 ** 24
    a, b = EC.ints((M, 3), 0), EC.ints((M, 3), 1)
    EC.integer_data(M, a, b)
    assert a.min() == -8 and a.max() == 8
    _fails(EC.integer_data, M, a * f32(2))
    _fails(EC.integer_data, M, a + f32(0.5))
    _fails(EC.integer_data, M + 1, a)
    # fp32 sums in two different orders equal the int64 sum
    ref = (a.astype(np.int64) * b.astype(np.int64)).sum(0)
    prod = (a * b).astype(f32)
    assert np.array_equal(prod.sum(0, dtype=f32), ref)
    assert np.array_equal(prod[::-1].cumsum(0, dtype=f32)[-1], ref)


def test_colsum_split_plan():
    assert EC.colsum_splits(0) == (1, 0, 0) and EC.colsum_splits(1) == (1, 1, 1)
    assert EC.colsum_splits(64) == (1, 64, 1) and EC.colsum_splits(65) == (2, 33, 2)
    assert EC.colsum_splits(8128) == (127, 64, 127) and EC.colsum_splits(8129) == (128, 64, 128)
    assert EC.colsum_splits(8193) == (128, 65, 127)          # the last slab is empty
    assert EC.colsum_splits(20001) == (128, 157, 128)


@pytest.mark.parametrize('M', EC.COLSUM_M)
def test_colsum_check_accepts_right_and_rejects_wrong(M):
    for C in (1, 65):
        for kind, data in (('integer', EC.ints), ('normal', EC.normal)):
            a, b = data((M, C), M, C, 0), data((M, C), M, C, 1)
            EC.check_colsum(a, emu_colsum(a)[0], None, kind)
            EC.check_colsum(a, emu_colsum(a, b)[0], b, kind)
        if M == 0:
            _fails(EC.check_colsum, a, np.full((C,), np.nan, f32))
            _fails(EC.check_colsum, a, np.ones((C,), f32), None, 'integer')
            continue
        a = EC.ints((M, C), M, C, 2)
        a[M - 1] = np.where(a[M - 1] == 0, 1, a[M - 1])          # the last row counts everywhere
        _fails(EC.check_colsum, a, emu_colsum(a, drop_last_row=True)[0], None, 'integer')
        if EC.colsum_splits(M)[2] == EC.colsum_splits(M)[0]:    # the last slab holds rows
            _fails(EC.check_colsum, a, emu_colsum(a, drop_last_slab=True)[0], None, 'integer')
        # a second call with fewer rows on the first call's workspace
        big = EC.ints((20001, C), C, 3)
        stale = emu_colsum(big)[1]
        if EC.colsum_splits(M)[0] < 128:
            _fails(EC.check_colsum, a, emu_colsum(a, stale=stale)[0], None, 'integer')
        for where in ('first', 'last'):
            s = EC.single_large(M, C, where)
            EC.check_colsum(s, emu_colsum(s)[0], None, 'single')
            _fails(EC.check_colsum, s, np.zeros((C,), f32), None, 'single')     # that row lost


def test_suite_bound_misses_a_lost_row_that_integer_data_finds():
    """A same-sign column at M = 20001: one lost row is about 1 / M of the sum, inside rel 1e-4."""
    M = 20001
    a = np.abs(EC.normal((M, 2), 7)) + f32(0.5)
    EC.check_colsum(a, emu_colsum(a, drop_last_row=True)[0])           # not noticed
    i = np.abs(EC.ints((M, 2), 7)) + f32(0)
    i[M - 1] = 1
    _fails(EC.check_colsum, i, emu_colsum(i, drop_last_row=True)[0], None, 'integer')


def test_affine_checks():
    M, C = 129, 5
    x, gy = EC.normal((M, C), 0), EC.normal((M, C), 1)
    W, b = EC.signed_scale(C, 0), EC.signed_scale(C, 1)
    y = (W[None] * x + b[None]).astype(f32)
    EC.check_affine_fwd(x, W, b, y)
    fused = (W[None].astype(np.float64) * x + b[None]).astype(f32)      # one rounding
    EC.check_affine_fwd(x, W, b, fused)
    _fails(EC.check_affine_fwd, x, W, b, (W[None] * x + np.roll(b, 1)[None]).astype(f32))
    _fails(EC.check_affine_fwd, x, W, b, y * (1 + f32(2. ** -21)))
    gx = (gy * W[None]).astype(f32)
    EC.check_affine_bwd(x, W, gy, gx, emu_colsum(gy, x)[0], emu_colsum(gy)[0])
    EC.check_affine_bwd(x, W, gy)
    _fails(EC.check_affine_bwd, x, W, gy, gx=(gy * np.roll(W, 1)[None]).astype(f32))
    _fails(EC.check_affine_bwd, x, W, gy, gW=emu_colsum(gy)[0])
    _fails(EC.check_affine_bwd, x, W, gy, gb=emu_colsum(gy, x)[0])
    xi, gi = EC.ints((M, C), 2), EC.ints((M, C), 3)
    EC.check_affine_bwd(xi, W, gi, None, emu_colsum(gi, xi)[0], emu_colsum(gi)[0], 'integer')
    _fails(EC.check_affine_bwd, xi, W, gi, None, emu_colsum(gi, xi)[0] + f32(1), None, 'integer')


def test_epilogue_check():
    M, C = 7, 5
    gy, y, scale = EC.normal((M, C), 0), EC.mask_operand((M, C), 0), EC.signed_scale(C, 2)
    assert ((y == 0) & ~np.signbit(y)).any() and ((y == 0) & np.signbit(y)).any()
    assert (scale < 0).any() and (scale > 0).any()
    for yy in (None, y):
        for sc in (None, scale):
            EC.check_epilogue_bwd(gy, yy, sc, emu_epilogue(gy, yy, sc))
    for sc in (None, scale):
        _fails(EC.check_epilogue_bwd, gy, y, sc, emu_epilogue(gy, y, sc, ge=True))
    out = emu_epilogue(gy, y, None)
    assert not np.signbit(out[y <= 0]).any()                  # +0, not -0
    neg = out.copy()
    neg[y <= 0] = -0.
    _fails(EC.check_epilogue_bwd, gy, y, None, neg)


# ---- pooling ----------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', EC.MAXPOOL_KINDS)
def test_maxpool_check(kind):
    for N, H, W in EC.MAXPOOL_MAPS:
        for C in (1, 4):
            x = EC.maxpool_input((N, H, W, C), kind, H, W, C)
            y = emu_maxpool(x)
            assert np.array_equal(y.transpose(0, 3, 1, 2),
                                  np_ref.max_pooling_2d(x.transpose(0, 3, 1, 2)))
            EC.check_maxpool(x, y)
            if kind == 'negative':
                _fails(EC.check_maxpool, x, emu_maxpool(x, pad=0.))
            if kind == 'negative' and (H > 1 or W > 1):
                _fails(EC.check_maxpool, x, emu_maxpool(x, window=2))


def test_maxpool_cover_all_window_reaches_the_last_row_and_column():
    """H = W = 8: the fifth window starts at the last row; missing it leaves -inf."""
    x = EC.maxpool_input((1, 8, 8, 3), 'negative', 0)
    y = emu_maxpool(x)
    assert y.shape == (1, 5, 5, 3) and np.isfinite(y).all()
    short = y.copy()
    short[:, -1] = y[:, -2]
    _fails(EC.check_maxpool, x, short)


@pytest.mark.parametrize('R,HW,C', EC.AVGPOOL_SHAPES)
def test_avgpool_checks(R, HW, C):
    for kind, data in (('integer', EC.ints), ('normal', EC.normal)):
        x = data((R, HW, C), R, HW, C)
        EC.check_avgpool_fwd(x, emu_avgpool_fwd(x), kind)
        EC.check_avgpool_fwd(x, (x.astype(np.float64).sum(1) / HW).astype(f32), kind)
        if R and HW > 1:
            x1 = x + f32(1) if kind == 'integer' else x
            if kind == 'integer':
                x1 = np.clip(x1, 1, 8)                    # no zero sums: every output moves
            _fails(EC.check_avgpool_fwd, x1, emu_avgpool_fwd(x1, div=HW - 1), kind)
            lost = emu_avgpool_fwd(x1) - x1[:, -1] * (f32(1) / f32(HW))
            if kind == 'integer':
                _fails(EC.check_avgpool_fwd, x1, lost.astype(f32), kind)
    gy, prior = EC.normal((R, C), R, HW, C, 1), EC.normal((R, HW, C), R, HW, C, 2)
    for acc in (0, 1):
        out = emu_avgpool_bwd(gy, HW, prior, acc)
        EC.check_avgpool_bwd(gy, HW, out, prior, acc)
        if R:
            _fails(EC.check_avgpool_bwd, gy, HW, emu_avgpool_bwd(gy, HW, prior, 1 - acc), prior, acc)
    if R:
        fused = (gy.astype(np.float64)[:, None] * np.float64(f32(1) / f32(HW)) + prior).astype(f32)
        EC.check_avgpool_bwd(gy, HW, fused, prior, 1)


@pytest.mark.parametrize('R,HW,C', EC.HEAD_TAIL_SHAPES)
@pytest.mark.parametrize('kind', EC.SLOT_KINDS)
def test_head_tail_check(R, HW, C, kind):
    slot, n = EC.slots(R, kind, HW)
    g_pool, y = EC.normal((R, C), R, 0), EC.mask_operand((R, HW, C), R, HW)
    g_rows = EC.normal((n, HW, C), R, 1) if slot is not None else None
    out = emu_head_tail(g_pool, g_rows, slot, y)
    EC.check_head_tail_bwd(g_pool, g_rows, slot, y, out)
    if R == 0:
        return
    leak = out.copy()
    leak[y <= 0] = -0.
    _fails(EC.check_head_tail_bwd, g_pool, g_rows, slot, y, leak)
    if kind == 'perm' and n >= 2:
        assert (np.diff(slot[slot >= 0]) < 0).any()           # not monotone
        wide = np.concatenate([g_rows, EC.normal((R, HW, C), R, 2)])[:R]
        _fails(EC.check_head_tail_bwd, g_pool, wide, slot, y,
               emu_head_tail(g_pool, wide, slot, y, by_r=True))
        _fails(EC.check_head_tail_bwd, g_pool, g_rows, slot, y,
               emu_head_tail(g_pool, None, None, y))


# ---- sparse 3x3 -------------------------------------------------------------------------------------

@pytest.mark.parametrize('N,H,W,C,K', EC.SPARSE_SHAPES[:3])
@pytest.mark.parametrize('kind', EC.ROW_KINDS)
def test_sparse3x3_checks(N, H, W, C, K, kind):
    C = min(C, 8)                                             # the loops above are per element
    rows = EC.sparse_rows(N, H, W, kind)
    lookup = EC.lookup_of(rows, N, H, W)
    assert sorted(lookup[lookup >= 0].tolist()) == list(range(len(rows)))
    x, g = EC.normal((N, H, W, C), 0) + f32(3), EC.normal((N, H, W, K), 1)
    patches, g_rows = emu_gather(x, g, rows)
    EC.check_sparse3x3_gather(x, g, rows, patches, g_rows)
    if kind in ('corners', 'all') and H * W > 1:              # rows at a map border
        _fails(EC.check_sparse3x3_gather, x, g, rows, *emu_gather(x, g, rows, wrap=True))
    if len(rows) > 1:
        _fails(EC.check_sparse3x3_gather, x, g, rows, patches, g_rows[::-1].copy())
    for data_kind, data in (('integer', EC.ints), ('normal', EC.normal)):
        gp = data((len(rows), 3, 3, C), H, W, 2)
        gx = emu_scatter(gp, lookup)
        EC.check_sparse3x3_scatter(gp, lookup, gx, data_kind)
        if len(rows) and H * W > 1:
            gp1 = np.where(gp == gp[:, ::-1, ::-1], gp + f32(1), gp) if data_kind == 'integer' else gp
            gp1 = np.clip(gp1, -8, 8) if data_kind == 'integer' else gp1
            bad = emu_scatter(gp1, lookup, mirror=True)
            if not np.array_equal(bad, emu_scatter(gp1, lookup)):
                _fails(EC.check_sparse3x3_scatter, gp1, lookup, bad, data_kind)
    if kind == 'all' and H * W > 1:
        gp = EC.ints((len(rows), 3, 3, C), 5)
        bad = emu_scatter(gp, lookup, mirror=True)
        assert not np.array_equal(bad, emu_scatter(gp, lookup))
        _fails(EC.check_sparse3x3_scatter, gp, lookup, bad, 'integer')


# ---- SGD ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', [n for n in EC.SGD_N if n < 10 ** 5])
@pytest.mark.parametrize('zero_grad', [0, 1])
def test_sgd_check(n, zero_grad):
    p, g, v = (EC.normal((n,), n, k) for k in range(3))
    h = EC.SGD_HYPER
    EC.check_sgd(p, g, v, zero_grad=zero_grad, **h, **dict(zip(('p2', 'g2', 'v2'),
                                                              emu_sgd(p, g, v, zero_grad=zero_grad, **h))))
    p_np, v_np = np_ref.momentum_sgd_wd(p, (g * f32(h['grad_scale'])).astype(f32), v, h['lr'],
                                        h['momentum'], h['wd'])
    EC.check_sgd(p, g, v, zero_grad=0, p2=p_np.astype(f32), g2=g, v2=v_np.astype(f32), **h)
    if n % 4:
        p2, g2, v2 = emu_sgd(p, g, v, zero_grad=zero_grad, skip_tail=True, **h)
        _fails(EC.check_sgd, p, g, v, zero_grad=zero_grad, p2=p2, g2=g2, v2=v2, **h)
    if n:
        p2, g2, v2 = emu_sgd(p, g, v, zero_grad=zero_grad, **h)
        _fails(EC.check_sgd, p, g, v, zero_grad=1 - zero_grad, p2=p2, g2=g2, v2=v2, **h)
        p2, g2, v2 = emu_sgd(p, g, v, zero_grad=zero_grad, **dict(h, grad_scale=1.))
        _fails(EC.check_sgd, p, g, v, zero_grad=zero_grad, p2=p2, g2=g2, v2=v2, **h)


# ---- guard band -----------------------------------------------------------------------------------------

def test_guard_check():
    n = 13
    buf = np.full(EC.GUARD + 1 + n + EC.GUARD, EC.POISON, np.uint32)
    assert np.isnan(buf.view(f32)).all()
    lo = EC.GUARD + 1
    buf[lo:lo + n] = np.arange(n, dtype=f32).view(np.uint32)
    EC.check_guard(buf, lo, lo + n)
    EC.check_guard(buf.view(np.int32), lo, lo + n)
    for k in (lo + n, lo - 1, 0, len(buf) - 1):                # a float4 store rounded up, and others
        bad = buf.copy()
        bad[k] = 0
        _fails(EC.check_guard, bad, lo, lo + n)


# ---- image kernels ----------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', [c[0] for c in EC.PREPARE_CASES])
def test_prepare_cases_and_check(name):
    case = EC.prepare_case(name)
    ref = case['ref']
    assert ref.shape[2] > 256
    EC.check_prepare(name, ref.copy())
    EC.check_prepare(name, ref[:, :, ::-1].copy(), flip=True)
    _fails(EC.check_prepare, name, ref.copy(), flip=True)                 # left unflipped
    shifted = ref.copy()
    shifted[:, :, 256:] = ref[:, :, 255:-1]
    _fails(EC.check_prepare, name, shifted)
    if case['img'].dtype == np.uint8:                                      # integers minus the mean
        assert np.array_equal(ref + np.asarray(EC.MEAN, f32).reshape(3, 1, 1),
                              np.rint(ref + np.asarray(EC.MEAN, f32).reshape(3, 1, 1)))


def test_prepare_cases_cover_what_the_issue_lists():
    widths = {n: EC.prepare_case(n)['ref'].shape[2] for n, *_ in EC.PREPARE_CASES}
    scales = {n: EC.prepare_case(n)['scale'] for n, *_ in EC.PREPARE_CASES}
    assert any(256 < w <= 512 for w in widths.values()) and any(w > 512 for w in widths.values())
    assert all(w % 256 for w in widths.values())                           # a partial last block
    assert any(s > 1 for s in scales.values()) and any(s < 0.5 for s in scales.values())
    kinds = {EC.prepare_case(n)['img'].dtype for n, *_ in EC.PREPARE_CASES}
    assert kinds == {np.dtype(np.uint8), np.dtype(np.float32)}


@pytest.mark.parametrize('im_w', EC.PASTE_WIDTHS)
def test_paste_cases_and_checks(im_w):
    case = EC.paste_case(im_w)
    EC.paste_conditions(case)
    ref, tags = case['ref'], case['tags']
    for t in ('out-left', 'out-right', 'out-top', 'out-bottom', 'inverted'):
        assert not ref[tags.index(t)].any(), t
    assert ref[tags.index('zero-height')].any(0).sum() > 0
    assert ref[tags.index('zero-height')].any(1).sum() == 1                 # one row
    EC.check_paste(case, ref.astype(np.uint8))
    shifted = ref.copy()
    shifted[:, :, 256:] = ref[:, :, 255:-1]
    _fails(EC.check_paste, case, shifted.astype(np.uint8))
    # the packed format, from the oracle's masks
    D, H, W = ref.shape
    Wq = (W + 63) // 64
    padded = np.zeros((D, H, Wq * 64), np.uint8)
    padded[:, :, :W] = ref
    packed = np.packbits(padded, axis=-1, bitorder='little').view('<u8').reshape(D, H, Wq)
    area = ref.sum((1, 2)).astype(np.int32)
    extent = np.zeros((D, 4), np.int32)
    for d, (x_0, x_1, y_0, y_1) in enumerate(case['clip']):
        if x_0 < x_1 and y_0 < y_1:
            extent[d] = (y_0, y_1, x_0 // 64, (x_1 + 63) // 64)
    EC.check_paste_packed(case, packed.view(np.int64), area, extent)
    assert (extent.any(1) == (case['clip'][:, 0] < case['clip'][:, 1])
            & (case['clip'][:, 2] < case['clip'][:, 3])).all()
    # every set bit lies inside its extent
    for d in range(D):
        ys, xs = np.where(ref[d])
        if len(ys):
            assert extent[d, 0] <= ys.min() and ys.max() < extent[d, 1]
            assert extent[d, 2] * 64 <= xs.min() and xs.max() < extent[d, 3] * 64
    bad = area.copy()
    bad[int(np.argmax(area))] -= 1
    _fails(EC.check_paste_packed, case, packed, bad, extent)
    bad = extent.copy()
    bad[tags.index('larger'), 3] -= 1
    _fails(EC.check_paste_packed, case, packed, area, bad)
    bad = packed.copy()
    bad[tags.index('larger'), 0, Wq - 1] |= np.uint64(1) << np.uint64(63)  # past the image width
    _fails(EC.check_paste_packed, case, bad, area, extent)
    shifted_p = np.zeros_like(padded)
    shifted_p[:, :, :W] = shifted
    _fails(EC.check_paste_packed, case,
           np.packbits(shifted_p, axis=-1, bitorder='little').view('<u8').reshape(D, H, Wq),
           area, extent)


def test_paste_clip_follows_the_oracle():
    """paste_clip restates the clip of np_infer.segm_results: set pixels stay inside it."""
    for im_w in EC.PASTE_WIDTHS:
        case = EC.paste_case(im_w)
        for d, (x_0, x_1, y_0, y_1) in enumerate(case['clip']):
            outside = case['ref'][d].copy()
            if x_0 < x_1 and y_0 < y_1:
                outside[y_0:y_1, x_0:x_1] = False
            assert not outside.any()
    assert np_infer.segm_results(np.zeros((0, 4), f32), np.zeros(0, np.int32),
                                 np.zeros((0, 5, 14, 14), f32), 40, 300).shape == (0, 40, 300)
