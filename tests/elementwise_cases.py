"""Edge inputs and pure checks of the elementwise / pooling / optimizer kernels (csrc/elementwise.hip)
and of the two image kernels (csrc/image.hip), shared by tests/test_gpu_elementwise.py and
tests/test_gpu_image_edges.py (the kernels) and by tests/test_elementwise_cases_cpu.py (the same
checks on NumPy emulations, right and wrong).  No device work and no library call: every check_*
takes the operands and the outputs as NumPy arrays and raises AssertionError on a mismatch.  The
references are those of tests/launch_ref.py and the oracle (oracle/np_ref.py, oracle/np_infer.py).

Two kinds of data.

Integer data: integers in [-8, 8] stored as fp32.  A sum of `terms` <= 20001 of them, or of
products of two of them (|.| <= 64), stays below 20001 * 64 < 2^24 in magnitude, so every partial
sum of every fp32 summation order is exact and a lost, doubled or misplaced element moves the
result by at least 1.  The reductions (colsum, the gW / gb of affine_bwd, sparse3x3_scatter) must
then equal the int64 result; `integer_data` asserts the condition on the operands.

Normal data: seeded N(0, 1).  Reductions are held to the suite's bound (launch_ref._close:
rel 1e-4, floor 1e-5 of the largest reference value).  Element-wise results are held to bounds
counted from the kernels' roundings in units of u = 2^-24 (a correctly rounded operation is within
u of its exact result, relative); elementwise.hip is compiled with FMA contraction allowed, so a
multiply-add is one rounding or two, and every bound below holds for both:
  affine_fwd    y = W x + b:  the product u |W x|, the sum u |y|
  avgpool_bwd   inv = 1 / HW (u), g inv (u), + the prior gx (u of the result):
                u (2 |g / HW| + |result|); the same for head_tail_bwd's  g_pool inv + g_rows
  avgpool_fwd   on integer data the sum is exact: inv and the product, 2 u |sum / HW|, while a lost
                element moves the result by at least 1 / HW
Each derived bound carries a factor 1.01 for the second-order terms.  Selects (the ReLU masks),
max-pooling, the gather and epilogue_bwd's single multiply have no rounding freedom and are compared
bit for bit.

epilogue_bwd  g = (y > 0 ? gy : +0) * scale[c]:  the fp32 product of the selected value and the
scale, bit for bit.  A masked element is therefore +0 without a scale or under a non-negative one,
and 0 * scale = -0 under a negative one; it compares equal to 0 in every case.

Guard bands: the GPU tests place every output inside a larger buffer filled with POISON (a NaN bit
pattern) and pass the whole buffer to check_guard, which demands that every word before and after
the output still holds it: a float4 store that overruns, or a scalar one off by one, shows.
"""
import functools

import numpy as np
import torch

import launch_ref as L
from oracle import np_infer

f32 = np.float32
U = 2. ** -24
SLACK = 1.01
POISON = 0x7fc0beef                 # a quiet NaN; as int32 it is positive
GUARD = 8                           # words on either side of an output (32 bytes: keeps alignment)
INT_LIMIT = 8
MAX_TERMS = 20001

CHANNELS = (1, 3, 4, 5, 63, 64, 65, 68, 132)
COLSUM_M = (0, 1, 5, 63, 64, 65, 129, 8128, 8129, 8193, 20001)
COLSUM_C = (1, 63, 64, 65, 132)
EPILOGUE_BIG = ((4099, 257), (16400, 260))          # scalar / vector body past the grid cap
MAXPOOL_MAPS = ((1, 1, 1), (1, 2, 2), (2, 1, 7), (2, 7, 1), (2, 5, 8), (1, 8, 5), (3, 13, 17))
MAXPOOL_C = (1, 3, 4, 68)
MAXPOOL_BIG = (1, 65, 65, 965)
MAXPOOL_KINDS = ('negative', 'neginf', 'fltmax')
AVGPOOL_SHAPES = ((0, 49, 8), (1, 1, 1), (3, 2, 5), (257, 49, 4), (2, 196, 68), (65, 49, 132))
HEAD_TAIL_SHAPES = ((0, 49, 4), (1, 1, 4), (3, 49, 8), (130, 49, 68), (5, 196, 260))
SLOT_KINDS = ('null', 'none', 'perm')
SPARSE_SHAPES = ((1, 1, 1, 4, 4), (2, 3, 5, 8, 4), (1, 7, 9, 260, 12), (1, 4, 4, 1028, 4))
ROW_KINDS = ('none', 'one', 'corners', 'all')
SGD_N = (0, 1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4099, 4194311)
SGD_HYPER = dict(lr=0.02, momentum=0.9, wd=1e-4, grad_scale=0.37)
GRID_CAP = 4096 * 256               # threads of the largest grid: more work needs a second pass


def cover_all(size):
    """chainer get_conv_outsize(size, 3, 2, 1, cover_all=True)."""
    return (size + 2 - 3 + 2 - 1) // 2 + 1


def colsum_splits(M):
    """(slabs, rows per slab, non-empty slabs) of mrcnn_colsum."""
    splits = max(1, min(128, -(-M // 64)))
    per = -(-M // splits)
    return splits, per, (-(-M // per) if per else 0)


# ---- data -----------------------------------------------------------------------------------------

def _rng(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 17) % (2 ** 31 - 1)
    return np.random.RandomState(seed)


def ints(shape, *key):
    return _rng(1, *key).randint(-INT_LIMIT, INT_LIMIT + 1, shape).astype(f32)


def normal(shape, *key):
    return _rng(2, *key).standard_normal(shape).astype(f32)


def mask_operand(shape, *key):
    """A ReLU output to mask by: N(0, 1) with +0 at every 7th and -0 at every 11th position (+3)."""
    y = normal(shape, 3, *key)
    flat = y.reshape(-1)
    flat[::7] = 0.
    flat[3::11] = -0.
    return y


def signed_scale(C, *key):
    """Per-channel scale of both signs."""
    return normal((C,), 4, *key)


def single_large(M, C, where, *key):
    """Zeros with one 1e10 per call in row 0 ('first') or M - 1 ('last'), column from the seed."""
    a = np.zeros((M, C), f32)
    a[0 if where == 'first' else M - 1, _rng(5, M, C, *key).randint(0, C)] = 1e10
    return a


def maxpool_input(shape, kind, *key):
    """(N, H, W, C): 'negative' is below -0.5 everywhere (a border padded by 0 instead of -inf
    shows in every border window); 'neginf' has -inf at a fifth of the positions and one whole
    image row of it; 'fltmax' the same with -FLT_MAX."""
    rng = _rng(6, *key)
    x = (-np.abs(rng.standard_normal(shape)) - 0.5).astype(f32)
    if kind == 'negative':
        return x
    x = rng.standard_normal(shape).astype(f32)
    v = -np.inf if kind == 'neginf' else np.finfo(f32).min
    x[rng.rand(*shape) < 0.2] = v
    x[:, 0] = v
    return x


def slots(R, kind, *key):
    """(slot (R,) int32 or None, rows of g_rows): 'null' no slot array; 'none' all -1; 'perm' the
    even rows carry a permutation of 0 .. n - 1 that is not monotone for n >= 2, the rest -1."""
    if kind == 'null':
        return None, 0
    slot = np.full((R,), -1, np.int32)
    if kind == 'none':
        return slot, 0
    on = np.arange(0, R, 2)
    perm = _rng(7, R, *key).permutation(len(on)).astype(np.int32)
    if len(on) >= 2 and (np.diff(perm) > 0).all():
        perm = perm[::-1].copy()
    slot[on] = perm
    return slot, len(on)


def sparse_rows(N, H, W, kind, *key):
    """Positions (indices into N * H * W), int32: 'none'; 'one' (the middle of the last image);
    'corners' (the distinct corners of every image); 'all' (every position, shuffled)."""
    if kind == 'none':
        rows = []
    elif kind == 'one':
        rows = [(N - 1) * H * W + (H // 2) * W + W // 2]
    elif kind == 'corners':
        rows = []
        for n in range(N):
            for p in (0, W - 1, (H - 1) * W, H * W - 1):
                if n * H * W + p not in rows:
                    rows.append(n * H * W + p)
    else:
        rows = _rng(8, N, H, W, *key).permutation(N * H * W)
    return np.asarray(rows, np.int32)


def lookup_of(rows, N, H, W):
    """position -> row or -1, (N, H, W) int32."""
    lookup = np.full((N * H * W,), -1, np.int32)
    lookup[rows] = np.arange(len(rows), dtype=np.int32)
    return lookup.reshape(N, H, W)


# ---- comparison helpers -----------------------------------------------------------------------------

def integer_data(terms, *arrays):
    """The condition of the module comment on integer operands summed over `terms` terms."""
    assert 0 <= terms <= MAX_TERMS and MAX_TERMS * INT_LIMIT * INT_LIMIT < 2 ** 24
    for a in arrays:
        if a is None:
            continue
        a = np.asarray(a)
        assert a.dtype == f32 and np.array_equal(a, np.rint(a)) and (np.abs(a) <= INT_LIMIT).all(), \
            'not integers in [-%d, %d]' % (INT_LIMIT, INT_LIMIT)
        assert terms * float(np.abs(a).max(initial=0)) ** 2 < 2 ** 24


def _f32(a, what):
    a = np.asarray(a)
    assert a.dtype == f32, '%s: dtype %s' % (what, a.dtype)
    return a


def bits_equal(got, ref, what):
    got, ref = np.ascontiguousarray(_f32(got, what)), np.ascontiguousarray(ref, f32)
    assert got.shape == ref.shape, '%s: shape %s, expected %s' % (what, got.shape, ref.shape)
    bad = got.view(np.uint32) != ref.view(np.uint32)
    if bad.any():
        i = np.unravel_index(bad.argmax(), bad.shape)
        raise AssertionError('%s: %d of %d elements differ in bits, first at %s: got %r, expected %r'
                             % (what, bad.sum(), bad.size, i, got[i], ref[i]))


def equal_exact(got, ref, what):
    """got (fp32) equals the int64 / float64 reference as a number."""
    got = _f32(got, what).astype(np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, '%s: shape %s, expected %s' % (what, got.shape, ref.shape)
    bad = ~(got == ref)
    if bad.any():
        i = np.unravel_index(bad.argmax(), bad.shape)
        raise AssertionError('%s: %d of %d elements differ, first at %s: got %r, expected %r'
                             % (what, bad.sum(), bad.size, i, got[i], ref[i]))


def within(got, ref, tol, what):
    """|got - ref| <= tol element for element (a NaN fails)."""
    got = _f32(got, what).astype(np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, '%s: shape %s, expected %s' % (what, got.shape, ref.shape)
    err = np.abs(got - ref)
    bad = ~(err <= tol)
    if bad.any():
        tol = np.broadcast_to(tol, ref.shape)
        i = np.unravel_index(bad.argmax(), bad.shape)
        raise AssertionError('%s: %d of %d elements over the bound, first at %s: got %.9g, '
                             'reference %.9g, error %.3g u, bound %.3g u'
                             % (what, bad.sum(), bad.size, i, got[i], ref[i], err[i] / U, tol[i] / U))


def close(got, ref, what):
    """The suite's reduction bound (launch_ref._close)."""
    got, ref = _f32(got, what), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, '%s: shape %s, expected %s' % (what, got.shape, ref.shape)
    if ref.size:
        assert np.isfinite(got).all(), what + ': not finite'
        try:
            L._close(got, ref)
        except AssertionError as e:
            raise AssertionError('%s: %s' % (what, e))


def check_guard(words, lo, hi, what='guard'):
    """`words`: a whole buffer as 32-bit words, the output at [lo, hi): all the rest is POISON."""
    w = np.asarray(words).view(np.uint32).reshape(-1)
    assert 0 <= lo <= hi <= len(w)
    for name, part, base in (('before', w[:lo], 0), ('after', w[hi:], hi)):
        bad = part != np.uint32(POISON)
        if bad.any():
            raise AssertionError('%s: word %d %s the output [%d, %d) was overwritten with 0x%08x'
                                 % (what, base + int(bad.argmax()), name, lo, hi,
                                    int(part[bad.argmax()])))


def _t(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype)))


# ---- checks, one per entry point ------------------------------------------------------------------

def check_colsum(a, out, b=None, kind='normal', what='colsum'):
    """out (C,) = sum over the rows of a (M, C) [* b (M, C)].  kind 'integer': equal to the int64
    sum; 'single': at most one non-zero term per column, every order is exact; 'normal': the
    suite's bound.  M = 0 gives zeros."""
    a = _f32(a, what)
    M, C = a.shape
    prod = a.astype(np.float64) * (1. if b is None else _f32(b, what).astype(np.float64))
    if kind == 'integer':
        integer_data(M, a, b)
        ref = np.rint(prod).astype(np.int64).sum(0)
        equal_exact(out, ref, what)
    elif kind == 'single':
        assert ((prod != 0).sum(0) <= 1).all()
        equal_exact(out, prod.sum(0).astype(f32), what)
    else:
        close(out, prod.sum(0), what)
    if M == 0:
        bits_equal(out, np.zeros((C,), f32), what + ' M = 0')


def check_epilogue_bwd(gy, y, scale, g, what='epilogue_bwd'):
    """g = (y > 0 ? gy : +0) * scale[c] in fp32, bit for bit (y None: no mask; scale None: 1)."""
    v = _f32(gy, what)
    if y is not None:
        v = np.where(_f32(y, what) > 0, v, f32(0))
    if scale is not None:
        v = (v * _f32(scale, what)[None, :]).astype(f32)
    bits_equal(g, v, what)
    if y is not None:
        assert (np.asarray(g)[y <= 0] == 0).all(), what + ': gradient where y <= 0'


def check_affine_fwd(x, W, b, y, what='affine_fwd'):
    wx = _f32(W, what).astype(np.float64)[None, :] * _f32(x, what).astype(np.float64)
    ref = wx + _f32(b, what).astype(np.float64)[None, :]
    within(y, ref, U * (np.abs(wx) + np.abs(ref)) * SLACK, what)


def check_affine_bwd(x, W, gy, gx=None, gW=None, gb=None, kind='normal', what='affine_bwd'):
    """gx = gy W[c] (one multiply: bit for bit), gW = colsum(gy x), gb = colsum(gy); each checked
    where given."""
    if gx is not None:
        check_epilogue_bwd(gy, None, W, gx, what + ' gx')
    if gW is not None:
        check_colsum(gy, gW, x, kind, what + ' gW')
    if gb is not None:
        check_colsum(gy, gb, None, kind, what + ' gb')


def check_maxpool(x, y, what='maxpool'):
    """x (N, H, W, C) -> y (N, P, Q, C): max_pooling_2d(3, 2, 1, cover_all) with -inf padding."""
    x = _f32(x, what)
    ref = L.maxpool3x3s2p1(_t(x).permute(0, 3, 1, 2)).permute(0, 2, 3, 1).contiguous().numpy()
    assert ref.shape[1:3] == (cover_all(x.shape[1]), cover_all(x.shape[2]))
    bits_equal(y, ref, what)


def check_avgpool_fwd(x, y, kind='normal', what='avgpool_fwd'):
    """x (R, HW, C) -> y (R, C) = mean over HW."""
    x = _f32(x, what)
    R, HW, C = x.shape
    ref = x.astype(np.float64).sum(1) / HW
    if kind == 'integer':
        integer_data(HW, x)
        within(y, ref, 2 * U * np.abs(ref) * SLACK, what)
    else:
        close(y, ref, what)


def check_avgpool_bwd(gy, HW, gx, prior=None, accumulate=0, what='avgpool_bwd'):
    """gx (R, HW, C) = gy (R, C) / HW  [+ prior, with accumulate]."""
    q = np.repeat((_f32(gy, what).astype(np.float64) / HW)[:, None, :], HW, 1)
    ref = q + _f32(prior, what).astype(np.float64) if accumulate else q
    within(gx, ref, U * (2 * np.abs(q) + np.abs(ref)) * SLACK, what)


def check_head_tail_bwd(g_pool, g_rows, slot, y, g, what='head_tail_bwd'):
    """g (R, HW, C) = (g_pool[r] / HW + (slot[r] >= 0 ? g_rows[slot[r]] : 0)) where y > 0, else +0."""
    y = _f32(y, what)
    R, HW, C = y.shape
    q = np.repeat((_f32(g_pool, what).astype(np.float64) / HW)[:, None, :], HW, 1)
    ref = q.copy()
    if slot is not None:
        on = np.asarray(slot) >= 0
        ref[on] += _f32(g_rows, what).astype(np.float64)[np.asarray(slot)[on]]
    keep = y > 0
    g = _f32(g, what)
    assert g.shape == y.shape
    bits_equal(g[~keep], np.zeros(int((~keep).sum()), f32), what + ' masked')
    within(g[keep], ref[keep], (U * (2 * np.abs(q) + np.abs(ref)) * SLACK)[keep], what)


def check_sparse3x3_gather(x, g, rows, patches, g_rows, what='sparse3x3_gather'):
    """patches (n, 3, 3, C): the 3x3 neighbourhood of every listed position, zero outside the map;
    g_rows (n, K) = g at the position.  Data movement: bit for bit."""
    x, g = _f32(x, what), _f32(g, what)
    n = len(rows)
    assert np.asarray(patches).shape == (n, 3, 3, x.shape[3])
    assert np.asarray(g_rows).shape == (n, g.shape[3])
    if n:
        p_ref, g_ref = L.sparse3x3_gather(_t(x), _t(g), _t(rows, np.int64))
        bits_equal(patches, p_ref.numpy(), what + ' patches')
        bits_equal(g_rows, g_ref.numpy(), what + ' g_rows')


def check_sparse3x3_scatter(g_patches, lookup, gx, kind='normal', what='sparse3x3_scatter'):
    """gx (N, H, W, C): every pixel sums the patch gradients whose window covers it."""
    gp = _f32(g_patches, what)
    N, H, W = lookup.shape
    C = gp.shape[3]
    ref = L.sparse3x3_scatter(_t(gp, np.float64), _t(lookup), N, H, W, C).numpy()
    if kind == 'integer':
        integer_data(9, gp)
        equal_exact(gx, ref, what)
    else:
        close(gx, ref, what)


def check_sgd(p, g, v, lr, momentum, wd, grad_scale, zero_grad, p2, g2, v2, what='sgd'):
    """launch_ref.sgd on the hyper-parameters as the kernel receives them (C floats)."""
    lr, momentum, wd, grad_scale = (float(f32(h)) for h in (lr, momentum, wd, grad_scale))
    rp, rv, tp, tv = L.sgd(_t(p, np.float64), _t(g, np.float64), _t(v, np.float64), lr, momentum,
                           wd, grad_scale)
    within(v2, rv.numpy(), tv.numpy(), what + ' v')
    within(p2, rp.numpy(), tp.numpy(), what + ' p')
    bits_equal(g2, np.zeros_like(g) if zero_grad else g, what + ' g')


# ---- image kernels ---------------------------------------------------------------------------------

MEAN = (122.7717, 115.9465, 102.9801)
# (name, source (H, W), dtype, min_size, max_size): the scale follows MaskRCNN.prepare's rule
PREPARE_CASES = (
    ('up-u8-3blocks', (40, 300), np.uint8, 100, 0),          # x 2.5: 100 x 750, 2 * 256 + 238
    ('up-f32-2blocks', (40, 300), np.float32, 60, 0),        # x 1.5: 60 x 450
    ('down-u8-2blocks', (90, 700), np.uint8, 36, 0),         # x 0.4: 36 x 280
    ('down-f32-3blocks', (90, 1400), np.float32, 36, 0),     # x 0.4: 36 x 560
    ('maxsize-u8-3blocks', (90, 700), np.uint8, 120, 600),   # max_size rule, x 6 / 7: 77 x 600
)


@functools.lru_cache(None)
def prepare_case(name):
    """dict(img (3, H, W), min_size, max_size, ref (3, h, w) f32, scale) — the oracle's result."""
    _, (H, W), dtype, min_size, max_size = next(c for c in PREPARE_CASES if c[0] == name)
    rng = _rng(9, H, W, min_size)
    if dtype == np.uint8:
        img = rng.randint(0, 256, (3, H, W)).astype(np.uint8)
    else:
        img = rng.uniform(0, 255, (3, H, W)).astype(np.float32)
    ref, scale = np_infer.prepare(img, MEAN, min_size, max_size)
    img.setflags(write=False)
    ref.setflags(write=False)
    return dict(img=img, min_size=min_size, max_size=max_size, ref=ref, scale=scale)


def check_prepare(name, got, flip=False, what='prepare'):
    """got (3, h, w): the prepared image, mirrored left-right when a flip was asked."""
    ref = prepare_case(name)['ref']
    if flip:
        ref = ref[:, :, ::-1]
    got = _f32(got, what)
    assert got.shape == ref.shape, '%s: shape %s, expected %s' % (what, got.shape, ref.shape)
    np.testing.assert_allclose(got, ref, rtol=0, atol=2e-4, err_msg=what)


PASTE_WIDTHS = (257, 300, 600)
PASTE_H, PASTE_M, PASTE_NFG = 40, 14, 5


@functools.lru_cache(None)
def paste_case(im_w):
    """dict(bbox (D, 4) yx f32, label (D,), logits (D, n_fg, M, M), im_h, im_w, tags, ref (D, im_h,
    im_w) bool — the oracle's result, inside (D,) bool — the ordinary boxes (tags 'in-...') whose
    expanded box lies inside the image, clip (D, 4) of paste_clip)."""
    im_h = PASTE_H
    rows = [('in-left', (3, 10, 30, 120)),
            ('span256', (4, 200, 33, 300)),
            ('larger', (-20, -30, im_h + 15, im_w + 40)),
            ('touch-right-bottom', (12, im_w - 60, im_h, im_w)),
            ('tall-right', (-5, im_w - 30, im_h + 5, im_w + 10)),
            ('out-left', (5, -60, 30, -20)), ('out-right', (5, im_w + 20, 30, im_w + 60)),
            ('out-top', (-50, 50, -15, 120)), ('out-bottom', (im_h + 10, 50, im_h + 40, 120)),
            ('zero-height', (12, 236, 12, 256.5 if im_w == 257 else 284)),
            ('inverted', (25, 240, 15, 256.5 if im_w == 257 else 290)),
            ('inverted-one-row', (10.6, 240, 10.2, 256.5 if im_w == 257 else 280))]
    if im_w == 257:
        rows += [('sub-pixel', (3.2, 256.1, 3.9, 256.6))]
    else:
        rows += [('sub-pixel', (3.2, 260.3, 3.9, 260.8)),
                 ('in-span256', (5, 200, 35, 290)),
                 ('in-right', (8, im_w - 36, 30, im_w - 10))]
    if im_w > 512:
        rows += [('in-span512', (4, 470, 34, 560)), ('in-far', (6, 520, 33, 590)),
                 ('span-both', (2, 180, 37, 585))]
    tags = tuple(t for t, _ in rows)
    bbox = np.asarray([b for _, b in rows], f32)
    D = len(bbox)
    rng = _rng(10, im_w)
    logits = (rng.standard_normal((D, PASTE_NFG, PASTE_M, PASTE_M)) * 3).astype(f32)
    label = rng.randint(0, PASTE_NFG, D).astype(np.int32)
    ref = np_infer.segm_results(bbox, label, logits, im_h, im_w)
    clip, rb = paste_clip(bbox, PASTE_M, im_h, im_w)
    inside = np.asarray([t.startswith('in-') for t in tags])
    assert ((rb[inside, 0] >= 0) & (rb[inside, 1] >= 0) & (rb[inside, 2] < im_w)
            & (rb[inside, 3] < im_h)).all()
    for a in (bbox, logits, label, ref, inside):
        a.setflags(write=False)
    return dict(bbox=bbox, label=label, logits=logits, im_h=im_h, im_w=im_w, tags=tags, ref=ref,
                inside=inside, clip=clip)


def paste_clip(bbox, M, im_h, im_w):
    """The oracle's expanded integer boxes rb (D, 4) = (x1, y1, x2, y2) and their clip to the image
    (x_0, x_1, y_0, y_1), half-open (np_infer.segm_results)."""
    rb = np_infer.expand_boxes(np.asarray(bbox, f32)[:, [1, 0, 3, 2]], (M + 2.0) / M).astype(np.int32)
    clip = np.stack([np.maximum(rb[:, 0], 0), np.minimum(rb[:, 2] + 1, im_w),
                     np.maximum(rb[:, 1], 0), np.minimum(rb[:, 3] + 1, im_h)], 1)
    return clip, rb


def paste_conditions(case):
    """What makes a paste case worth running, on the oracle alone: at least three masks with set
    pixels at x >= 256, and every in-image box neither empty nor full inside its clip."""
    ref, clip = case['ref'], case['clip']
    assert int(ref[:, :, 256:].any((1, 2)).sum()) >= 3
    assert case['inside'].sum() >= 1
    for d in np.where(case['inside'])[0]:
        x_0, x_1, y_0, y_1 = clip[d]
        box = ref[d, y_0:y_1, x_0:x_1]
        assert box.size and box.any() and not box.all(), case['tags'][d]
        assert ref[d].sum() == box.sum()


def check_paste(case, dense, what='paste_masks'):
    """dense (D, im_h, im_w) uint8 / bool = np_infer.segm_results."""
    dense = np.asarray(dense)
    assert dense.shape == case['ref'].shape and dense.dtype in (np.uint8, np.bool_)
    assert (dense.view(np.uint8) <= 1).all(), what + ': values other than 0 and 1'
    if not np.array_equal(dense.astype(bool), case['ref']):
        bad = dense.astype(bool) != case['ref']
        d, y, x = (int(i[0]) for i in np.where(bad))
        raise AssertionError('%s: %d pixels differ, first at detection %d (%s) y %d x %d'
                             % (what, bad.sum(), d, case['tags'][d], y, x))


def unpack_words(packed, W):
    """(D, H, Wq) 64-bit words (bit l of word w = pixel 64 w + l) -> (D, H, W) bool, and the bits
    past W of the last word (must be clear)."""
    p = np.ascontiguousarray(packed).view(np.uint64)
    D, H, Wq = p.shape
    assert Wq == (W + 63) // 64
    bits = np.unpackbits(p.astype('<u8').view(np.uint8).reshape(D, H, Wq * 8), axis=2,
                         bitorder='little')
    return bits[:, :, :W].astype(bool), bits[:, :, W:]


def check_paste_packed(case, packed, area, extent, what='paste_masks_packed'):
    """The packed paste: the bits equal the oracle's masks, nothing set past the image width, area
    is the popcount, extent is all zero for an empty clip and else (y_0, y_1, x_0 >> 6,
    ((x_1 - 1) >> 6) + 1): the clipped expanded box with its columns widened to whole words."""
    ref = case['ref']
    D, im_h, im_w = ref.shape
    dense, tail = unpack_words(packed, im_w)
    assert not tail.any(), what + ': bits set past the image width'
    check_paste(case, dense, what)
    assert np.array_equal(np.asarray(area, np.int64), ref.sum((1, 2))), what + ': area'
    expect = np.zeros((D, 4), np.int32)
    for d, (x_0, x_1, y_0, y_1) in enumerate(case['clip']):
        if x_0 < x_1 and y_0 < y_1:
            expect[d] = (y_0, y_1, x_0 >> 6, ((x_1 - 1) >> 6) + 1)
    assert np.array_equal(np.asarray(extent), expect), \
        '%s: extent\n%s\nexpected\n%s' % (what, np.asarray(extent), expect)
