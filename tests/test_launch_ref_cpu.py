"""The float64 references of tests/launch_ref.py against the NumPy / C oracle on the CPU, and a
self-test of the comparison: it must flag a single dropped term at realistic reduction lengths."""
import itertools

import numpy as np
import pytest
import torch

import launch_ref as L
from chainer_mask_rcnn_amd._lib import EPI_ACCUM, EPI_AFFINE, EPI_BIAS, EPI_RELU, EPI_RESIDUAL
from oracle import np_ref

F64 = torch.float64


def _t(a):
    return torch.tensor(np.asarray(a, np.float64))


@pytest.mark.parametrize('R,stride,pad,H,W', [(1, 1, 0, 9, 11), (1, 2, 0, 9, 11), (3, 1, 1, 8, 7),
                                              (3, 2, 1, 9, 10), (7, 2, 3, 13, 12)])
def test_conv_references_match_oracle(R, stride, pad, H, W):
    rng = np.random.RandomState(R * 10 + stride)
    N, C, K = 2, 5, 6
    x = rng.standard_normal((N, C, H, W))
    w = rng.standard_normal((K, C, R, R))
    y = L.conv_fwd(_t(x), _t(w), stride, pad)
    y_np = np_ref.conv2d_fwd(x, w, None, stride, pad)
    L._close(y.numpy(), y_np, rel=1e-12, floor=1e-12)
    gy = rng.standard_normal(y_np.shape)
    gx_np, gw_np, _ = np_ref.conv2d_bwd(x, w, gy, stride, pad)
    L._close(L.conv_dgrad(_t(gy), _t(w), H, W, stride, pad).numpy(), gx_np, rel=1e-12, floor=1e-12)
    L._close(L.conv_wgrad(_t(x), _t(gy), R, R, stride, pad).numpy(), gw_np, rel=1e-12, floor=1e-12)


def test_conv_references_chunk_over_the_batch(monkeypatch):
    """The chunked loops give the unchunked result."""
    rng = np.random.RandomState(1)
    x, w = _t(rng.standard_normal((5, 4, 6, 7))), _t(rng.standard_normal((3, 4, 3, 3)))
    gy = _t(rng.standard_normal((5, 3, 6, 7)))
    full = (L.conv_fwd(x, w, 1, 1), L.conv_dgrad(gy, w, 6, 7, 1, 1), L.conv_wgrad(x, gy, 3, 3, 1, 1))
    monkeypatch.setattr(L, '_CHUNK', 1)
    part = (L.conv_fwd(x, w, 1, 1), L.conv_dgrad(gy, w, 6, 7, 1, 1), L.conv_wgrad(x, gy, 3, 3, 1, 1))
    for a, b in zip(full, part):
        assert torch.allclose(a, b, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize('flags', [sum(c) for n in range(5)
                                   for c in itertools.combinations(
                                       (EPI_BIAS, EPI_AFFINE, EPI_RESIDUAL, EPI_RELU), n)])
def test_forward_epilogue_every_flag_combination(flags):
    """y = relu?(affine?(conv + bias?) + residual?), a direct per-element loop."""
    rng = np.random.RandomState(flags)
    y = rng.standard_normal((2, 3, 2, 2))
    b, s, t, r = (rng.standard_normal(3), rng.standard_normal(3), rng.standard_normal(3),
                  rng.standard_normal(y.shape))
    ref = np.empty_like(y)
    for i in np.ndindex(*y.shape):
        v = y[i]
        c = i[1]
        if flags & EPI_BIAS:
            v += b[c]
        if flags & EPI_AFFINE:
            v = v * s[c] + t[c]
        if flags & EPI_RESIDUAL:
            v += r[i]
        if flags & EPI_RELU:
            v = max(v, 0.)
        ref[i] = v
    got = L.fwd_epilogue(_t(y), flags, _t(b), _t(s), _t(t), _t(r))
    np.testing.assert_allclose(got.numpy(), ref, rtol=1e-14, atol=1e-14)


@pytest.mark.parametrize('accum,res,res_y,mask,scale', list(itertools.product((0, 1), repeat=5)))
def test_dgrad_epilogue_every_combination(accum, res, res_y, mask, scale):
    """gx = (acc * out_scale[c] + res_g * (res_y > 0) + prev) * (out_mask_y > 0), per element."""
    rng = np.random.RandomState(accum + 2 * res + 4 * res_y + 8 * mask + 16 * scale)
    shape = (2, 3, 2, 2)
    acc, prev, rg, ry, my = (rng.standard_normal(shape) for _ in range(5))
    sc = rng.standard_normal(3)
    ref = np.empty(shape)
    for i in np.ndindex(*shape):
        v = acc[i] * (sc[i[1]] if scale else 1.)
        if res:
            v += rg[i] * (ry[i] > 0 if res_y else 1.)
        if accum:
            v += prev[i]
        if mask:
            v *= my[i] > 0
        ref[i] = v
    got = L.dgrad_epilogue(_t(acc), EPI_ACCUM if accum else 0, _t(prev), _t(rg) if res else None,
                           _t(ry) if res and res_y else None, _t(my) if mask else None,
                           _t(sc) if scale else None)
    np.testing.assert_allclose(got.numpy(), ref, rtol=1e-14, atol=1e-14)


def test_deconv_references_match_oracle():
    rng = np.random.RandomState(4)
    x, w = rng.standard_normal((2, 5, 3, 4)), rng.standard_normal((5, 6, 2, 2))
    y_np = np_ref.deconv2x2s2_fwd(x, w)
    L._close(L.deconv_fwd(_t(x), _t(w)).numpy(), y_np)
    gy = rng.standard_normal(y_np.shape)
    gx_np, gw_np, _ = np_ref.deconv2x2s2_bwd(x.astype(np.float32), w.astype(np.float32),
                                             gy.astype(np.float32))
    L._close(L.deconv_dgrad(_t(gy), _t(w)).numpy(), gx_np)
    L._close(L.deconv_wgrad(_t(x), _t(gy)).numpy(), gw_np)


def test_pool_affine_sgd_references_match_oracle():
    rng = np.random.RandomState(5)
    x = rng.standard_normal((2, 3, 9, 8)).astype(np.float32)
    got = L.maxpool3x3s2p1(torch.tensor(x))
    assert np.array_equal(got.numpy(), np_ref.max_pooling_2d(x))
    r = rng.standard_normal((4, 3, 7, 7)).astype(np.float32)
    avg = _t(r).permute(0, 2, 3, 1).reshape(4, 49, 3).mean(1)
    L._close(avg.numpy(), np_ref.average_pooling_2d(r, 7, 7).reshape(4, 3))
    W_, b_ = rng.standard_normal(3), rng.standard_normal(3)
    L._close((_t(x) * _t(W_).view(1, -1, 1, 1) + _t(b_).view(1, -1, 1, 1)).numpy(),
             np_ref.affine_channel_2d_fwd(x.astype(np.float64), W_, b_))
    p, g, v = (rng.standard_normal(1000).astype(np.float32) for _ in range(3))
    p2, v2, tp, tv = L.sgd(_t(p), _t(g), _t(v), 0.02, 0.9, 1e-4, 1.0)
    p_np, v_np = np_ref.momentum_sgd_wd(p, g, v, 0.02, 0.9, 1e-4)
    assert ((v2 - _t(v_np)).abs() <= tv).all() and ((p2 - _t(p_np)).abs() <= tp).all()


@pytest.mark.parametrize('sampling_ratio', [0, 2])
def test_roi_align_references_match_oracle(sampling_ratio):
    import oracle
    rng = np.random.RandomState(6 + sampling_ratio)
    N, C, H, W = 2, 3, 20, 30
    x = rng.standard_normal((N, C, H, W)).astype(np.float32)
    rois = np.array([[0, 3.5, 2.0, 200.0, 150.0], [1, 0, 0, 479, 319], [1, 100.2, 50.7, 101.0, 51.1],
                     [0, -40, -30, 60, 50], [1, 430, 300, 520, 400]], np.float32)
    y_or = oracle.roi_align_fwd(x, rois, 7, 7, 1 / 16., sampling_ratio)
    xn = torch.tensor(x).permute(0, 2, 3, 1).to(F64)
    y = L.roi_align_fwd(xn, torch.tensor(rois), 7, 7, 1 / 16., sampling_ratio, chunk=2)
    L._close(y.permute(0, 3, 1, 2).numpy(), y_or)
    # strided bins: the even bins of the full grid
    y2 = L.roi_align_fwd(xn, torch.tensor(rois), 7, 7, 1 / 16., sampling_ratio, bin_stride=2)
    assert torch.equal(y2, y[:, ::2, ::2])
    gy = rng.standard_normal(y_or.shape).astype(np.float32)
    gx_or = oracle.roi_align_bwd(gy, rois, x.shape, 1 / 16., sampling_ratio)
    gx = L.roi_align_bwd(torch.tensor(gy).permute(0, 2, 3, 1).to(F64), torch.tensor(rois),
                         (N, H, W, C), 1 / 16., sampling_ratio, chunk=2)
    L._close(gx.permute(0, 3, 1, 2).numpy(), gx_or)


def test_sparse3x3_references_match_loops():
    rng = np.random.RandomState(7)
    N, H, W, C, K = 2, 4, 5, 3, 2
    x = torch.tensor(rng.standard_normal((N, H, W, C)).astype(np.float32))
    g = torch.tensor(rng.standard_normal((N, H, W, K)).astype(np.float32))
    rows = torch.tensor(sorted(rng.choice(N * H * W, 9, replace=False)))
    patches, g_rows = L.sparse3x3_gather(x, g, rows)
    for j, r in enumerate(rows.tolist()):
        n, h, w = r // (H * W), (r // W) % H, r % W
        for dy in range(3):
            for dx in range(3):
                yy, xx = h + dy - 1, w + dx - 1
                want = x[n, yy, xx] if 0 <= yy < H and 0 <= xx < W else torch.zeros(C)
                assert torch.equal(patches[j, dy, dx], want)
        assert torch.equal(g_rows[j], g.view(-1, K)[r])
    gp = torch.tensor(rng.standard_normal((9, 3, 3, C)))
    lookup = torch.full((N * H * W,), -1, dtype=torch.int32)
    lookup[rows] = torch.arange(9, dtype=torch.int32)
    gx = L.sparse3x3_scatter(gp, lookup.view(N, H, W), N, H, W, C)
    ref = torch.zeros((N, H, W, C), dtype=F64)
    for j, r in enumerate(rows.tolist()):
        n, h, w = r // (H * W), (r // W) % H, r % W
        for dy in range(3):
            for dx in range(3):
                yy, xx = h + dy - 1, w + dx - 1
                if 0 <= yy < H and 0 <= xx < W:
                    ref[n, yy, xx] += gp[j, dy, dx]
    assert torch.allclose(gx, ref, rtol=1e-14, atol=1e-14)


def test_comparison_flags_one_dropped_term():
    """At realistic scale — a 4608-long dot product (res5 3x3: 512 x 9) and a 50176-long weight-
    gradient reduction (1024 RoIs x 49) — dropping one term of one output element, or zeroing the
    last ragged row of a tile, exceeds the bound; the fp32 result of the same sums does not."""
    rng = np.random.RandomState(8)
    for n, cols in ((4608, 256), (50176, 64)):
        a = torch.tensor(np.maximum(rng.standard_normal((n,)), 0) if n == 4608
                         else rng.standard_normal((n,)))
        b = torch.tensor(rng.standard_normal((n, cols)) / np.sqrt(n))
        ref = a @ b
        fp32 = (a.float() @ b.float()).double()
        assert L.ratio(fp32, ref) <= 1.
        # the largest term of output 3 dropped
        k = int(torch.argmax((a[:, None] * b[:, 3:4]).abs()))
        got = fp32.clone()
        got[3] -= a[k] * b[k, 3]
        assert L.ratio(got, ref) > 1., (n, L.ratio(got, ref))
    # a tile's last ragged row left at zero (1000 rows, 128-row tiles: row 999)
    y = torch.tensor(rng.standard_normal((1000, 64)))
    got = y.float().double()
    got[999] = 0
    assert L.ratio(got, y) > 1.
    assert L.exact(got.float(), y.float()) > 1.


# ---- losses: the references against the oracle, and the bounds against the kernels' reduction -----

def _f32(a):
    return np.asarray(a, np.float32)


def _ti(a):
    return torch.tensor(np.asarray(a, np.int32))


def test_sigmoid_ce_reference_matches_oracle():
    rng = np.random.RandomState(20)
    x = _f32(rng.standard_normal(3001) * 3)
    t = rng.randint(-1, 2, 3001).astype(np.int32)
    loss, gx, l_tol, g_tol = L.sigmoid_ce(_t(x), _ti(t))
    l_np, g_np = np_ref.sigmoid_cross_entropy(x, t)
    np.testing.assert_allclose(float(loss), l_np, rtol=3e-7)        # the oracle's element is fp32
    np.testing.assert_allclose(gx.numpy(), g_np, rtol=2e-7, atol=1e-12)
    assert (g_tol[torch.tensor(t == -1)] == 0).all() and (g_tol[torch.tensor(t != -1)] > 0).all()
    assert 0 < float(l_tol) < 1e-5 * float(loss)
    # nothing valid: 0 with zero gradients and zero tolerance
    loss, gx, l_tol, g_tol = L.sigmoid_ce(_t(x[:7]), _ti([-1] * 7))
    assert float(loss) == 0 and float(l_tol) == 0 and not gx.any() and not g_tol.any()


def test_mask_sigmoid_ce_reference_matches_oracle():
    rng = np.random.RandomState(21)
    R, Kc, M = 9, 5, 4
    x = _f32(rng.standard_normal((R, Kc, M, M)) * 2)
    label = np.array([0, 1, 5, 3, 0, 2, 5, 1, 4], np.int32)
    t = rng.randint(-1, 2, (R, M, M)).astype(np.int32)            # background rows keep targets
    sel = x[np.arange(R), label - 1]                               # label 0 -> channel Kc - 1
    l_np, g_sel = np_ref.sigmoid_cross_entropy(sel, t)
    g_np = np.zeros_like(x)
    g_np[np.arange(R), label - 1] = g_sel
    xr = _t(x).permute(0, 2, 3, 1).reshape(R, M * M, Kc)
    loss, gx, l_tol, g_tol = L.mask_sigmoid_ce(xr, _ti(label), _ti(t.reshape(R, -1)))
    np.testing.assert_allclose(float(loss), l_np, rtol=3e-7)
    got = gx.view(R, M, M, Kc).permute(0, 3, 1, 2).numpy()
    np.testing.assert_allclose(got, g_np, rtol=2e-7, atol=1e-12)
    assert (g_tol[gx == 0] == 0).all() and (g_tol[gx != 0] > 0).all()
    assert ((g_tol > 0).sum(2) <= 1).all()                          # one channel per pixel at most


def test_softmax_references_match_oracle():
    rng = np.random.RandomState(22)
    x = _f32(rng.standard_normal((257, 81)) * 2)
    t = rng.randint(-1, 81, 257).astype(np.int32)
    loss, gx, l_tol, g_tol = L.softmax_ce(_t(x), _ti(t))
    l_np, g_np = np_ref.softmax_cross_entropy(x, t)
    np.testing.assert_allclose(float(loss), l_np, rtol=2e-7)
    np.testing.assert_allclose(gx.numpy(), g_np, rtol=2e-7, atol=1e-12)
    assert (g_tol[torch.tensor(t == -1)] == 0).all()
    y, y_tol = L.softmax(_t(x))
    e = np.exp(x.astype(np.float64) - x.max(1, keepdims=True))
    np.testing.assert_allclose(y.numpy(), e / e.sum(1, keepdims=True), rtol=1e-13)
    assert (y_tol > 0).all() and float(y_tol.max()) < 1e-4
    # -inf logits off the target: probability 0, finite loss, finite bound
    x[:, 3] = -np.inf
    t[t == 3] = 4
    loss, gx, l_tol, g_tol = L.softmax_ce(_t(x), _ti(t))
    assert np.isfinite(float(loss)) and torch.isfinite(gx).all() and torch.isfinite(g_tol).all()
    assert (gx[:, 3] == 0).all()


@pytest.mark.parametrize('sigma', [1., 3.])
def test_smooth_l1_reference_matches_oracle_and_fixture(sigma, golden_dir):
    import os
    rng = np.random.RandomState(23)
    n = 1500
    pred, gt = _f32(rng.standard_normal((n, 4))), _f32(rng.standard_normal((n, 4)))
    label = rng.randint(-1, 3, n).astype(np.int32)
    loss, gx, l_tol, g_tol = L.smooth_l1(_t(pred), None, _t(gt), _ti(label), sigma)
    l_np, g_np = np_ref.fast_rcnn_loc_loss(pred.astype(np.float64), gt.astype(np.float64), label,
                                           sigma)
    np.testing.assert_allclose(float(loss), l_np, rtol=2e-7)
    np.testing.assert_allclose(gx.numpy(), g_np, rtol=2e-7, atol=1e-12)
    assert (g_tol[torch.tensor(label <= 0)] == 0).all() and (g_tol[torch.tensor(label > 0)] > 0).all()
    # class-selected form: the same numbers in the selected columns, exact zeros elsewhere
    ncls = 21
    cls = np.where(label > 0, rng.randint(1, ncls, n), 0).astype(np.int32)
    wide = _f32(rng.standard_normal((n, 4 * ncls)))
    wide.reshape(n, ncls, 4)[np.arange(n), cls] = pred
    loss2, gx2, l_tol2, g_tol2 = L.smooth_l1(_t(wide), _ti(cls), _t(gt), _ti(label), sigma)
    assert float(loss2) == float(loss) and float(l_tol2) == float(l_tol)
    g3 = gx2.view(n, ncls, 4)
    assert torch.equal(g3[torch.arange(n), torch.tensor(cls).long()], gx)
    assert int((gx2 != 0).sum()) == int((gx != 0).sum())
    assert int((g_tol2 != 0).sum()) == int((g_tol != 0).sum())
    # the fixture the original function body produced
    d = np.load(os.path.join(golden_dir, 'loc_loss.npz'))
    loss, _, l_tol, _ = L.smooth_l1(_t(d['pred']), None, _t(d['gt']), _ti(d['label']), sigma)
    want = float(d['loss_sigma%d' % sigma])                          # computed in float32
    np.testing.assert_allclose(float(loss), want, rtol=1e-6)
    # nothing counted: the unguarded 0 / 0 of the original
    loss, gx, _, _ = L.smooth_l1(_t(pred[:5]), None, _t(gt[:5]), _ti([-1] * 5), sigma)
    with np.errstate(invalid='ignore', divide='ignore'):
        l_np, _ = np_ref.fast_rcnn_loc_loss(pred[:5], gt[:5], np.full(5, -1, np.int32), sigma)
    assert np.isnan(float(loss)) and np.isnan(l_np) and not gx.any()


def test_tol_ratio():
    ref = torch.tensor([1., 0., float('nan'), 1e39])
    tol = torch.tensor([1e-6, 0., 0., 0.])
    ok = torch.tensor([1. + 5e-7, 0., float('nan'), float('inf')])
    assert L.tol_ratio(ok, ref, tol) <= 1.
    assert L.tol_ratio(torch.tensor([1. + 2e-6, 0., float('nan'), float('inf')]), ref, tol) > 1.
    assert L.tol_ratio(torch.tensor([1., 1e-30, float('nan'), float('inf')]), ref, tol) == np.inf
    assert L.tol_ratio(torch.tensor([1., 0., 0., float('inf')]), ref, tol) == np.inf
    assert L.tol_ratio(torch.tensor([float('nan'), 0., float('nan'), float('inf')]), ref, tol) == np.inf
    assert L.tol_ratio(torch.tensor([1., 0., float('nan'), 3e38]), ref, tol) == np.inf
    assert L.tol_ratio(torch.zeros(0), torch.zeros(0), 0.) == 0.


def _emulate_sum(el, parts, lanes_used=64):
    """The first pass of csrc/loss.hip on fp32 terms `el` (flat order): `parts` workgroups of 256
    threads; with lanes_used = 64 thread j adds elements j, j + T, j + 2 T, ... (T = 256 parts) in
    fp32, with lanes_used = 1 only lane 0 of each wave does (wave w takes terms w, w + 4 parts, ...:
    softmax CE); a 64-lane fp32 butterfly; the four wave sums pairwise and the partials serially in
    double.  Returns the double total."""
    slots = parts * 256 if lanes_used == 64 else parts * 4
    per = -(-len(el) // slots)
    a = np.zeros(per * slots, np.float32)
    a[:len(el)] = el
    a = a.reshape(per, slots)
    s = np.zeros(slots, np.float32)
    for j in range(per):
        s = s + a[j]                                   # fp32 adds in thread order
    if lanes_used == 64:
        v = s.reshape(-1, 64)
    else:
        v = np.zeros((slots, 64), np.float32)
        v[:, 0] = s
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ o]
    assert v.dtype == np.float32
    w = v[:, 0].astype(np.float64).reshape(parts, 4)
    partial = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])
    total = 0.
    for p in partial:
        total += p
    return total


def _sce_el32(x, t):
    x = x.astype(np.float32)
    ind = (x >= 0).astype(np.float32)
    return -(x * (t.astype(np.float32) - ind) - np.log1p(np.exp(-np.abs(x)))).astype(np.float32)


def _loss_cases():
    """(name, fp32 terms, count, parts, lanes, float64 loss, bound) at the three project sizes."""
    rng = np.random.RandomState(30)
    # RPN class loss: n = 128 520, 126 workgroups
    n = 128520
    x, t = _f32(rng.standard_normal(n) * 3), rng.randint(0, 2, n).astype(np.int32)
    loss, _, tol, _ = L.sigmoid_ce(_t(x), _ti(t))
    assert L.flat_parts(n) == 126
    yield 'rpn', _sce_el32(x, t), n, 126, 64, float(loss), float(tol)
    # mask loss: 1024 RoIs x 14 x 14, channel selection does not enter the reduction (Kc = 3 here)
    R, HW, Kc = 1024, 196, 3
    x = _f32(rng.standard_normal((R, HW, Kc)))
    label = rng.randint(1, Kc + 1, R).astype(np.int32)
    t = rng.randint(0, 2, (R, HW)).astype(np.int32)
    loss, _, tol, _ = L.mask_sigmoid_ce(_t(x), _ti(label), _ti(t))
    sel = x[np.arange(R), :, label - 1]
    yield 'mask', _sce_el32(sel.reshape(-1), t.reshape(-1)), R * HW, L.flat_parts(R * HW), 64, \
        float(loss), float(tol)
    # RoI class loss: 1024 rows of 81, one row per wave
    x = _f32(rng.standard_normal((1024, 81)) * 2)
    t = rng.randint(0, 81, 1024).astype(np.int32)
    loss, _, tol, _ = L.softmax_ce(_t(x), _ti(t))
    m = x.max(1)
    lse = (m + np.log(np.exp(x - m[:, None]).sum(1, dtype=np.float32))).astype(np.float32)
    yield 'softmax', (lse - x[np.arange(1024), t]).astype(np.float32), 1024, L.row_parts(1024), 1, \
        float(loss), float(tol)


def test_loss_bound_passes_the_kernels_reduction_and_flags_one_element():
    """The analogue of test_comparison_flags_one_dropped_term for the losses: fp32 element terms
    reduced in the kernels' order pass the bound; the same with one element of at least mean
    magnitude dropped, or with the valid count off by one, do not."""
    for name, el, count, parts, lanes, ref, tol in _loss_cases():
        assert el.dtype == np.float32 and (el >= 0).all()
        total = _emulate_sum(el, parts, lanes)
        good = float(np.float32(total / count))
        assert abs(good - ref) <= tol, (name, abs(good - ref) / tol)
        mean = total / count
        k = int(np.argmin(np.where(el >= mean, el, np.inf)))        # the smallest such element
        assert mean <= el[k] < 1.5 * mean, (name, el[k], mean)
        dropped = el.copy()
        dropped[k] = 0
        bad = float(np.float32(_emulate_sum(dropped, parts, lanes) / count))
        assert abs(bad - ref) > tol, (name, 'dropped', abs(bad - ref) / tol)
        for c in (count - 1, count + 1):
            bad = float(np.float32(total / c))
            assert abs(bad - ref) > tol, (name, 'count', c, abs(bad - ref) / tol)
        print('%s: emulation %.3f of the bound (%.2f u of the loss), dropped %.1f, count+1 %.1f'
              % (name, abs(good - ref) / tol, abs(good - ref) / (ref * L.U),
                 abs(float(np.float32(_emulate_sum(dropped, parts, lanes) / count)) - ref) / tol,
                 abs(float(np.float32(total / (count + 1))) - ref) / tol))


def test_gradient_bound_flags_a_count_off_by_one():
    """Every gradient element moves by 1 / count relative when the count is off by one: fp32
    gradients with the right count pass, with count + 1 they do not."""
    rng = np.random.RandomState(31)
    n = 128520
    x, t = _f32(rng.standard_normal(n) * 3), rng.randint(0, 2, n).astype(np.int32)
    _, gx, _, g_tol = L.sigmoid_ce(_t(x), _ti(t))
    sig = (np.float32(1) / (np.float32(1) + np.exp(-x))).astype(np.float32)
    for c, ok in ((n, True), (n + 1, False), (n - 1, False)):
        g32 = ((sig - t.astype(np.float32)) * (np.float32(1) / np.float32(c))).astype(np.float32)
        assert (L.tol_ratio(torch.tensor(g32), gx, g_tol) <= 1.) == ok, c
    # mask loss at 1024 x 196 (same kernel arithmetic, count = 200 704)
    n = 1024 * 196
    xs, ts = np.resize(x, n), np.resize(t, n)
    _, gx, _, g_tol = L.sigmoid_ce(_t(xs), _ti(ts))
    sig = (np.float32(1) / (np.float32(1) + np.exp(-xs))).astype(np.float32)
    for c, ok in ((n, True), (n + 1, False)):
        g32 = ((sig - ts.astype(np.float32)) * (np.float32(1) / np.float32(c))).astype(np.float32)
        assert (L.tol_ratio(torch.tensor(g32), gx, g_tol) <= 1.) == ok, c
    # softmax CE, 1024 x 81
    x = _f32(rng.standard_normal((1024, 81)) * 2)
    t = rng.randint(0, 81, 1024).astype(np.int32)
    _, gx, _, g_tol = L.softmax_ce(_t(x), _ti(t))
    m = x.max(1, keepdims=True)
    lse = (m + np.log(np.exp(x - m).sum(1, keepdims=True, dtype=np.float32))).astype(np.float32)
    p = np.exp(x - lse).astype(np.float32)
    p[np.arange(1024), t] -= np.float32(1)
    for c, ok in ((1024, True), (1025, False)):
        g32 = (p * (np.float32(1) / np.float32(c))).astype(np.float32)
        assert (L.tol_ratio(torch.tensor(g32), gx, g_tol) <= 1.) == ok, c
    # smooth L1 at the RPN size, 256 counted anchors of which 128 are foreground
    n = 128520
    label = np.full(n, -1, np.int32)
    pick = rng.choice(n, 256, replace=False)
    label[pick[:128]] = 1
    label[pick[128:]] = 0
    label[0] = label[-1] = 1
    pred, gt = _f32(rng.standard_normal((n, 4))), _f32(rng.standard_normal((n, 4)))
    _, gx, _, g_tol = L.smooth_l1(_t(pred), None, _t(gt), _ti(label), 3.)
    count = int((label >= 0).sum())
    d = pred - gt
    g = np.where(np.abs(d) < np.float32(1) / np.float32(9), np.float32(9) * d, np.sign(d))
    g = np.where(label[:, None] > 0, g, 0).astype(np.float32)
    for c, ok in ((count, True), (count + 1, False)):
        g32 = (g * (np.float32(1) / np.float32(c))).astype(np.float32)
        assert (L.tol_ratio(torch.tensor(g32), gx, g_tol) <= 1.) == ok, c
