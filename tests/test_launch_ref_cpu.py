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


# ---- target creators: the references on NumPy emulations of csrc/targets.hip -------------------

import target_cases as TC
from oracle import np_targets
from test_targets_cpu import _scene


def _worst(checks):
    return max([r for r, _ in checks] + [0.])


def _emu_iou_argmax(a, b, last_argmax=False, col_skip_last=False):
    """iou_argmax_kernel / iou_colmax_kernel: fp32 in the reference's order, first argmax."""
    iou = L.bbox_iou_f32(a, b)
    arg = iou.argmax(1) if not last_argmax else iou.shape[1] - 1 - iou[:, ::-1].argmax(1)
    col = (iou[:-1] if col_skip_last else iou).max(0)
    return iou.max(1), arg.astype(np.int32), iou, col


def _emu_anchor_labels(iou, mx, gt_max, neg, pos, order='neg,gt,pos'):
    label = np.full(len(iou), -1, np.int32)
    with np.errstate(invalid='ignore'):
        for rule in order.split(','):
            if rule == 'neg':
                label[mx < np.float32(neg)] = 0
            elif rule == 'gt':
                label[(iou == gt_max[None]).any(1)] = 1
            else:
                label[mx >= np.float32(pos)] = 1
    return label


def _emu_mask_targets(masks, roi, gt_index, n_fg, M, half_away=False, ge=False, force_t=True):
    """mask_targets_kernel line by line (rintf, clamp, mask_axis, fp32 blend, prob > 0.5)."""
    Hh, Ww = masks.shape[1:]
    out = -np.ones((len(roi), M, M), np.int32)
    rnd = TC.round_half_away if half_away else np.round
    f32 = np.float32

    def axis(n_in, start, limit):
        n = float(max(n_in, 1))
        pos = (np.arange(M, dtype=np.float64) + 0.5) * (n / float(M)) - 0.5
        i0 = np.floor(pos).astype(np.int64)
        t = (pos - i0).astype(f32)
        last = int(n) - 1
        if force_t:
            t[(i0 < 0) | (i0 >= last)] = 0
        i0 = np.clip(i0, 0, last)
        i1 = np.minimum(i0 + 1, last)
        return np.clip(i0 + start, 0, limit - 1), np.clip(i1 + start, 0, limit - 1), t

    for r in range(n_fg):
        y0, x0, y1, x1 = (int(v) for v in rnd(roi[r].astype(np.float64)))
        y0, y1 = min(max(y0, 0), Hh), min(max(y1, 0), Hh)
        x0, x1 = min(max(x0, 0), Ww), min(max(x1, 0), Ww)
        h, w = max(y1 - y0, 0), max(x1 - x0, 0)
        if h == 0 or w == 0:
            out[r] = 0
            continue
        ya, yb, ty = axis(h, y0, Hh)
        xa, xb, tx = axis(w, x0, Ww)
        m = (masks[gt_index[r]] > 0).astype(f32)
        tx_, ty_ = tx[None, :], ty[:, None]
        top = m[ya][:, xa] * (f32(1) - tx_) + m[ya][:, xb] * tx_
        bot = m[yb][:, xa] * (f32(1) - tx_) + m[yb][:, xb] * tx_
        prob = top * (f32(1) - ty_) + bot * ty_
        out[r] = (prob >= f32(0.5)) if ge else (prob > f32(0.5))
    return out


@pytest.mark.parametrize('na,g,degenerate', [(1, 1, False), (255, 2, False), (257, 9, True),
                                             (2008, 100, True), (21000, 9, False)])
def test_bbox_iou_reference_accepts_right_and_rejects_wrong(na, g, degenerate):
    a, b = TC.iou_boxes(na, g, degenerate=degenerate)
    mx, arg, iou, col = _emu_iou_argmax(a, b)
    assert np.array_equal(iou, np_ref.bbox_iou(a, b), equal_nan=True)
    if degenerate:
        # every zero-area row against the zero-area box is 0 / 0
        assert np.isnan(iou).sum() == 2 and np.isnan(mx).sum() == 2 and np.isnan(col).sum() == 1
    assert _worst(L.check_bbox_iou_argmax(a, b, mx, arg, iou, col)) <= 1.
    assert _worst(L.check_bbox_iou_argmax(a, b, mx, arg)) <= 1.
    if g >= 3 and na > 8:                       # b[1] = b[0], a[0] = b[0]: a tied row
        _, arg_last, _, _ = _emu_iou_argmax(a, b, last_argmax=True)
        assert _worst(L.check_bbox_iou_argmax(a, b, mx, arg_last, iou, col)) > 1.
        assert _worst(L.check_bbox_iou_argmax(a, b, mx, arg_last)) > 1.
    if na > 1:                                  # the last row holds its column's only IoU 1
        _, _, _, col_bad = _emu_iou_argmax(a, b, col_skip_last=True)
        assert _worst(L.check_bbox_iou_argmax(a, b, mx, arg, iou, col_bad)) > 1.
    # arithmetic: one ulp-scale slip passes, a dropped "- inter" does not
    bad = iou.copy()
    k = np.nanargmax(np.where(iou < 1, iou, 0))
    bad.flat[k] = np.float32(bad.flat[k] * (1 + 64 * L.U))
    assert _worst(L.check_bbox_iou_argmax(a, b, bad.max(1), bad.argmax(1).astype(np.int32), bad,
                                          bad.max(0))) > 1.


def test_bbox_iou_bound_holds_on_scene_and_golden(golden_dir):
    import os
    d = np.load(os.path.join(golden_dir, 'proposal_target_creator.npz'))
    for roi, bbox in [(_scene(s)[0], _scene(s)[1]) for s in (0, 1, 2)] + [(d['roi'], d['bbox'])]:
        cand = np.concatenate([roi, bbox], 0)
        mx, arg, iou, col = _emu_iou_argmax(cand, bbox)
        checks = list(L.check_bbox_iou_argmax(cand, bbox, mx, arg, iou, col))
        assert _worst(checks) <= 1., checks
        print('iou vs float64: %.3f of the bound' % checks[0][0])


def _label_scenes():
    """(anchors, boxes, neg, pos): IoU exactly 0.25 and 0.5 at the thresholds; an anchor below neg
    that is a column maximum; a box no anchor overlaps; a NaN column."""
    A = np.array([[0, 0, 10, 10], [100, 100, 110, 110], [100, 100, 105, 105],
                  [200, 200, 240, 240], [300, 300, 310, 310], [7, 7, 7, 7]], np.float32)
    base = np.array([[0, 0, 10, 5], [100, 100, 105, 105], [200, 200, 210, 210]], np.float32)
    yield A[:5], base, 0.25, 0.5
    yield A[:5], np.concatenate([base, [[600, 600, 650, 650]]]).astype(np.float32), 0.25, 0.5
    yield A, np.concatenate([base, [[7, 7, 7, 7]]]).astype(np.float32), 0.25, 0.5
    yield A[:5], base, 0.3, 0.7


def test_anchor_labels_reference_follows_the_oracle_and_rejects_wrong_orders():
    expected_first = [1, -1, 1, 1, 0]            # 0.5 >= pos; 0.25 is not < neg; max; col max; none
    for n, (a, b, neg, pos) in enumerate(_label_scenes()):
        mx, arg, iou, col = _emu_iou_argmax(a, b)
        good = _emu_anchor_labels(iou, mx, col, neg, pos)
        # chainercv's _create_label without its draws (n_sample large enough)
        atc = np_ref.AnchorTargetCreator(n_sample=4 * len(a), neg_iou_thresh=neg,
                                         pos_iou_thresh=pos, pos_ratio=1.)
        with np.errstate(invalid='ignore', divide='ignore'):
            _, ref = atc._create_label(np.arange(len(a)), a, b)
        assert np.array_equal(good, ref), (n, good, ref)
        if n == 0:
            assert good.tolist() == expected_first
        if n == 1:
            assert (good == 1).all()            # gt_max = 0: every zero-IoU anchor is positive
        assert _worst(L.check_anchor_labels(iou, mx, col, neg, pos, good)) <= 1.
        harmless = _emu_anchor_labels(iou, mx, col, neg, pos, 'neg,pos,gt')
        assert np.array_equal(harmless, good)
        if n in (0, 3):
            bad = _emu_anchor_labels(iou, mx, col, neg, pos, 'gt,pos,neg')
            assert _worst(L.check_anchor_labels(iou, mx, col, neg, pos, bad)) > 1.
    # >= instead of > / < at equality
    a, b, neg, pos = next(_label_scenes())
    mx, arg, iou, col = _emu_iou_argmax(a, b)
    lt = _emu_anchor_labels(iou, mx, col, np.nextafter(np.float32(neg), np.float32(1)), pos)
    assert _worst(L.check_anchor_labels(iou, mx, col, neg, pos, lt)) > 1.


@pytest.mark.parametrize('seed', [0, 1])
def test_anchor_targets_finish_reference(seed):
    _, bbox, _, _, size = _scene(seed)
    ab = np_ref.generate_anchor_base(16, (0.5, 1, 2), (2, 4, 8, 16, 32))
    anchor = np_ref.enumerate_shifted_anchor(ab, 16, 30, 40).astype(np.float32)
    np.random.seed(5)
    loc_ref, label_ref = np_ref.AnchorTargetCreator()(bbox, anchor, size)
    inside = np.where((anchor[:, 0] >= 0) & (anchor[:, 1] >= 0) & (anchor[:, 2] <= size[0])
                      & (anchor[:, 3] <= size[1]))[0].astype(np.int32)
    a = anchor[inside]
    mx, arg, iou, col = _emu_iou_argmax(a, bbox)
    before = _emu_anchor_labels(iou, mx, col, 0.3, 0.7)
    after = label_ref[inside]
    disabled = np.where(before != after)[0].astype(np.int32)
    assert len(disabled) and (after[disabled] == -1).all()
    args = (a, inside, before, arg, bbox, disabled, len(anchor), after)
    assert _worst(L.check_anchor_targets_finish(*args, loc_ref, label_ref)) <= 1.
    bad = label_ref.copy()
    bad[np.setdiff1d(np.arange(len(anchor)), inside)[0]] = 0          # a write outside
    assert _worst(L.check_anchor_targets_finish(*args, loc_ref, bad)) > 1.
    bad = loc_ref.copy()
    bad[inside[3], 2] = np.float32(bad[inside[3], 2] * (1 + 2e-6) + 2e-6)
    assert _worst(L.check_anchor_targets_finish(*args, bad, label_ref)) > 1.
    bad = after.copy()
    bad[np.where(before == after)[0][0]] ^= 1                          # label_inside elsewhere
    assert _worst(L.check_anchor_targets_finish(*args[:-1], bad, loc_ref, label_ref)) > 1.


def test_proposal_gather_and_mask_references_match_the_oracle(golden_dir):
    import os
    d = np.load(os.path.join(golden_dir, 'proposal_target_creator.npz'))
    cases = [_scene(s)[:4] for s in (0, 1, 2)] + [(d['roi'], d['bbox'], d['label'],
                                                   d['mask'].astype(np.int32))]
    for roi, bbox, label, mask in cases:
        np.random.seed(7)
        s_roi, loc, lab, gt_mask = np_targets.ProposalTargetCreator(n_sample=128)(
            roi, bbox, label, mask)
        cand = np.concatenate([roi, bbox], 0)
        iou = np_ref.bbox_iou(cand, bbox)
        assigned = iou.argmax(1).astype(np.int32)
        # recover the draws from the sampled boxes (candidates are distinct)
        chosen = np.array([np.where((cand == r).all(1))[0][0] for r in s_roi], np.int32)
        n_fg = int((lab > 0).sum())
        gi = assigned[chosen]
        mean, std = (0., 0., 0., 0.), (0.1, 0.1, 0.2, 0.2)
        args = (cand, bbox, label.astype(np.int32), assigned, chosen, n_fg, mean, std)
        checks = list(L.check_proposal_targets_gather(*args, s_roi, loc, lab, gi))
        assert _worst(checks) <= 1., checks
        bad = loc.copy()
        bad[0, 0] = np.float32(bad[0, 0] + 1e-4 * max(abs(bad[0, 0]), 1))
        assert _worst(L.check_proposal_targets_gather(*args, s_roi, bad, lab, gi)) > 1.
        bad = lab.copy()
        bad[n_fg] = 1
        assert _worst(L.check_proposal_targets_gather(*args, s_roi, loc, bad, gi)) > 1.
        m8 = (mask != 0).astype(np.uint8)
        assert np.array_equal(L.mask_targets_ref(m8, s_roi, gi, n_fg, 14), gt_mask)
        assert np.array_equal(_emu_mask_targets(m8, s_roi, gi, n_fg, 14), gt_mask)


def test_proposal_gather_reference_non_finite_positions():
    cand = np.array([[10, 10, 10, 30], [10, 10, 50, 30], [5, 5, 25, 45]], np.float32)
    bbox = np.array([[10, 10, 40, 30], [20, 20, 20, 60]], np.float32)     # second: zero height
    assigned, chosen = np.array([0, 1, 1], np.int32), np.array([0, 1, 2, 2], np.int32)
    label = np.array([3, 7], np.int32)
    mean, std = (0.1, -0.2, 0.3, 0.05), (0.1, 0.3, 0.2, 0.7)
    from chainer_mask_rcnn_amd.utils.bbox import bbox2loc
    with np.errstate(divide='ignore'):
        loc = ((bbox2loc(cand[chosen], bbox[assigned[chosen]]) - np.array(mean, np.float32))
               / np.array(std, np.float32)).astype(np.float32)
    assert np.isneginf(loc[1:, 2]).all() and np.isfinite(loc[0]).all()
    args = (cand, bbox, label, assigned, chosen, 2, mean, std, cand[chosen])
    lab, gi = np.array([4, 8, 0, 0], np.int32), assigned[chosen]
    assert _worst(L.check_proposal_targets_gather(*args, loc, lab, gi)) <= 1.
    for v in (0., np.inf, np.nan):
        bad = loc.copy()
        bad[1, 2] = v
        assert _worst(L.check_proposal_targets_gather(*args, bad, lab, gi)) > 1.


def test_mask_reference_on_the_edge_crops_rejects_wrong_kernels():
    """The crop set of tests/target_cases.py on 800 x 1333 masks: the literal one-hot / resize /
    argmax reference equals the emulated kernel on every row, and differs from round-half-away,
    from prob >= 0.5 and from an unclamped border weight."""
    G = 12
    masks = TC.mask_patterns(G)
    roi, gt = TC.mask_rows(G)
    n = len(roi)
    prob, valid = TC.tie_stats(masks, roi, gt)
    ties = (prob == 392) & valid[:, None, None]
    ref = L.mask_targets_ref(masks, roi, gt, n, 14)
    assert np.array_equal(ref[valid], (prob[valid] > 392).astype(np.int32)) and (ref[~valid] == 0).all()
    mixed = np.array([len(np.unique(r)) == 2 for r in ref])
    print('rows %d, half-way rows %d, tie pixels %d, tie pixels in mixed rows %d'
          % (n, TC.halfway_rows(roi).sum(), ties.sum(), ties[mixed].sum()))
    assert TC.halfway_rows(roi).sum() >= 100 and ties.sum() >= 1000 and ties[mixed].sum() > 0
    good = _emu_mask_targets(masks, roi, gt, n, 14)
    assert _worst(L.check_mask_targets(masks, roi, gt, n, 14, good)) <= 1.
    for kw in (dict(half_away=True), dict(ge=True), dict(force_t=False)):
        bad = _emu_mask_targets(masks, roi, gt, n, 14, **kw)
        rows = int((bad != good).any((1, 2)).sum())
        print('%s: %d rows differ' % (kw, rows))
        assert rows > 0 and _worst(L.check_mask_targets(masks, roi, gt, n, 14, bad)) > 1.
    for M in (7, 28):
        sub = slice(0, n, 5)
        good = _emu_mask_targets(masks, roi[sub], gt[sub], len(roi[sub]), M)
        assert _worst(L.check_mask_targets(masks, roi[sub], gt[sub], len(roi[sub]), M, good)) <= 1.
    half = _emu_mask_targets(masks, roi, gt, n // 2, 14)
    assert (half[n // 2:] == -1).all()
    assert _worst(L.check_mask_targets(masks, roi, gt, n // 2, 14, half)) <= 1.
    full = _emu_mask_targets(masks, roi, gt, n, 14)
    assert _worst(L.check_mask_targets(masks, roi, gt, n // 2, 14, full)) > 1.
