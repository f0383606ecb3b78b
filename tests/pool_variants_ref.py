"""NumPy restatements of the two RoI feature extractors beside ROIAlign — ``roi_pooling_2d``
(chainer's F.roi_pooling_2d GPU kernel, Caffe's Fast R-CNN ROIPooling) and ``crop_and_resize``
(the reference's functions/crop_and_resize.py:7-41 with F.resize_images) — and their gradients,
written from the semantics DESIGN.md section 2.1 states.  Test infrastructure: chainer is not
available here, so these are the yardstick of tests/test_*pool_variants*.py.

Arrays are NCHW NumPy; rois (R, 5) rows (batch, x1, y1, x2, y2)."""
import numpy as np


def _round_half_away(v):
    """roundf: half away from zero (v float32, evaluated exactly in float64)."""
    v = np.float64(v)
    return int(np.sign(v) * np.floor(np.abs(v) + 0.5))


def pool_windows(roi, outh, outw, spatial_scale, H, W):
    """[(hstart, hend)] * outh, [(wstart, wend)] * outw of one RoI (fp32 arithmetic)."""
    s = np.float32(spatial_scale)
    r = np.asarray(roi, np.float32)
    start_w = _round_half_away(r[1] * s)
    start_h = _round_half_away(r[2] * s)
    end_w = _round_half_away(r[3] * s)
    end_h = _round_half_away(r[4] * s)
    roi_w = max(end_w - start_w + 1, 1)
    roi_h = max(end_h - start_h + 1, 1)
    bin_h = np.float32(roi_h) / np.float32(outh)
    bin_w = np.float32(roi_w) / np.float32(outw)

    def win(p, b, start, size):
        lo = int(np.floor(np.float32(p) * b))
        hi = int(np.ceil(np.float32(p + 1) * b))
        return min(max(lo + start, 0), size), min(max(hi + start, 0), size)

    return ([win(p, bin_h, start_h, H) for p in range(outh)],
            [win(p, bin_w, start_w, W) for p in range(outw)])


def roi_pooling_2d_fwd(x, rois, outh, outw, spatial_scale):
    """-> y (R, C, outh, outw) float32, argmax (R, C, outh, outw) int32 (h * W + w or -1)."""
    x = np.asarray(x, np.float32)
    N, C, H, W = x.shape
    R = len(rois)
    y = np.zeros((R, C, outh, outw), np.float32)
    am = np.full((R, C, outh, outw), -1, np.int32)
    for r in range(R):
        b = int(np.float32(rois[r][0]))
        hw, ww = pool_windows(rois[r], outh, outw, spatial_scale, H, W)
        for ph, (hs, he) in enumerate(hw):
            for pw, (ws, we) in enumerate(ww):
                if he <= hs or we <= ws:
                    continue
                m = np.full(C, np.float32(-1e37), np.float32)
                a = np.full(C, -1, np.int32)
                for h in range(hs, he):
                    for w in range(ws, we):
                        v = x[b, :, h, w]
                        upd = v > m              # strict: the first maximum stays; NaN never wins
                        m = np.where(upd, v, m)
                        a = np.where(upd, h * W + w, a)
                y[r, :, ph, pw] = m
                am[r, :, ph, pw] = a
    return y, am


def roi_pooling_2d_bwd(gy, argmax, rois, x_shape):
    """gx (N, C, H, W) float32: gy summed into the argmax pixels in (r, ph, pw) order, fp32."""
    N, C, H, W = x_shape
    gx = np.zeros((N, C, H * W), np.float32)
    gy = np.asarray(gy, np.float32)
    R, _, PH, PW = gy.shape
    cc = np.arange(C)
    for r in range(R):
        b = int(np.float32(rois[r][0]))
        for ph in range(PH):
            for pw in range(PW):
                a = argmax[r, :, ph, pw]
                ok = a >= 0
                # one pixel per channel: the fp32 sums run in the kernel's order
                gx[b, cc[ok], a[ok]] = gx[b, cc[ok], a[ok]] + gy[r, ok, ph, pw]
    return gx.reshape(N, C, H, W)


def crop_box(roi, spatial_scale, H, W):
    """(y1', x1', hc, wc): the integer crop (float64, Python's round = half to even), the start
    clamped into the map (extension), the end truncated as a slice."""
    s = float(spatial_scale)

    def axis(v1, v2, size):
        a = min(max(int(round(float(v1) * s)), 0), size - 1)
        b = max(int(round(float(v2) * s)), a + 1)
        return a, min(b, size) - a

    r = [float(np.float32(v)) for v in roi]
    y1, hc = axis(r[2], r[4], H)
    x1, wc = axis(r[1], r[3], W)
    return y1, x1, hc, wc


def lin_taps(n, m):
    """Taps of linspace(0, m - 1, n) (F.resize_images, aligned corners): i0, i1 (int arrays),
    w0, w1 (float32, rounded once from float64)."""
    v = np.linspace(0, m - 1, n) if n > 1 else np.zeros(1)
    if m == 1:
        z = np.zeros(n, np.int64)
        return z, z, np.ones(n, np.float32), np.zeros(n, np.float32)
    i0 = np.clip(np.floor(v).astype(np.int64), 0, m - 2)
    d = v - i0
    return i0, i0 + 1, (1.0 - d).astype(np.float32), d.astype(np.float32)


def output_rows(rois):
    """Output row of every RoI: the stable sort by batch index (the reference's per-image concat)."""
    b = np.array([int(np.float32(r[0])) for r in rois], np.int64)
    rows = np.empty(len(b), np.int64)
    rows[np.argsort(b, kind='stable')] = np.arange(len(b))
    return rows


def crop_and_resize_fwd(x, rois, outh, outw, spatial_scale):
    """-> y (R, C, outh, outw) float32 in the reference's (batch-sorted) row order."""
    x = np.asarray(x, np.float32)
    N, C, H, W = x.shape
    R = len(rois)
    y = np.zeros((R, C, outh, outw), np.float32)
    rows = output_rows(rois)
    for r in range(R):
        b = int(np.float32(rois[r][0]))
        y1, x1, hc, wc = crop_box(rois[r], spatial_scale, H, W)
        vi0, vi1, vw0, vw1 = lin_taps(outh, hc)
        ui0, ui1, uw0, uw1 = lin_taps(outw, wc)
        for ph in range(outh):
            r0 = x[b, :, y1 + vi0[ph]]
            r1 = x[b, :, y1 + vi1[ph]]
            for pw in range(outw):
                c0, c1 = x1 + ui0[pw], x1 + ui1[pw]
                w00, w01 = vw0[ph] * uw0[pw], vw0[ph] * uw1[pw]        # fp32 products
                w10, w11 = vw1[ph] * uw0[pw], vw1[ph] * uw1[pw]
                y[rows[r], :, ph, pw] = ((w00 * r0[:, c0] + w01 * r0[:, c1]) + w10 * r1[:, c0]) + \
                    w11 * r1[:, c1]
    return y


def crop_and_resize_bwd(gy, rois, x_shape, spatial_scale, dtype=np.float64):
    """gx (N, C, H, W): the adjoint of the four taps (accumulated in ``dtype``)."""
    N, C, H, W = x_shape
    gy = np.asarray(gy, dtype)
    R, _, PH, PW = gy.shape
    gx = np.zeros((N, C, H, W), dtype)
    rows = output_rows(rois)
    for r in range(R):
        b = int(np.float32(rois[r][0]))
        y1, x1, hc, wc = crop_box(rois[r], spatial_scale, H, W)
        vi0, vi1, vw0, vw1 = lin_taps(PH, hc)
        ui0, ui1, uw0, uw1 = lin_taps(PW, wc)
        for ph in range(PH):
            for pw in range(PW):
                g = gy[rows[r], :, ph, pw]
                for yy, wy in ((vi0[ph], vw0[ph]), (vi1[ph], vw1[ph])):
                    for xx, wx in ((ui0[pw], uw0[pw]), (ui1[pw], uw1[pw])):
                        gx[b, :, y1 + yy, x1 + xx] += dtype(wy) * dtype(wx) * g
    return gx


def strided(a, s):
    return a[:, :, ::s, ::s]
