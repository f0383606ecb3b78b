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
