"""Exact cases for the three RoI feature extractors, and the list geometry of their pixel-owner
backwards restated on the host.  Test infrastructure: no device is touched here.

Why exact.  With spatial scale 1, integer RoI corners and a RoI side of ``bins * g`` pixels with
g in {1, 2, 4}, every ROIAlign sample position (start + p g + (i + .5) g / grid), bilinear weight,
``1 / count`` (count = grid^2 in {1, 4, 16}), and — with integer gy — every product and partial
sum is a dyadic rational with few bits.  The float64 reference is then representable in fp32, and
so is every partial sum in ANY order of summation, fused or not: each one is a multiple of the
common quantum 2^-k bounded by the sum of the absolute terms, and the builders assert
``sum |terms| * 2^k < 2^24``.  Owner, gather and scatter form must therefore all equal the
reference bit for bit; one lost, doubled or misplaced list entry changes the result.
Crop-and-resize is exact in the same way for output sizes n with n - 1 a power of two (the
linspace step (m - 1) / (n - 1) is dyadic); max pooling sums integers.

Layouts are the kernels': maps (N, H, W, C), gy (R, OH, OW, C), rois (R, 5) rows
(batch, x1, y1, x2, y2).

The counters restate what the owner kernels do with a tile (image n, row y, columns x0 .. x0 + 7):
roi_align.hip scans kOwnScan * nthr RoIs per chunk, keeps those whose extent meets the tile (m) and
walks their m * OH * OW (RoI, bin) candidates in windows of 2 * nthr; roi_pool_variants.hip scans
nthr RoIs per chunk and writes each kept RoI's rectangle of covering bins (ntot entries in all)
in windows of kPvCap.  A GPU case asserts through them that it reaches the branch it is named for.
"""
import collections
import functools
import os
import re

import numpy as np
import torch

import launch_ref as L
import pool_variants_ref as PV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'chainer_mask_rcnn_amd', 'csrc')

# ---- the kernels' constants, restated (tests/test_roi_exact_cases_cpu.py reads the sources) ------
K_OWN_XT = 8          # roi_align.hip kOwnXT: pixels of a row per owner workgroup
K_OWN_SCAN = 4        # kOwnScan: RoIs tested per thread and chunk
K_OWN_THREADS = 256   # kOwnThreads
K_PV_XT = 8           # roi_pool_variants.hip kPvXT
K_PV_CAP = 512        # kPvCap: LDS list entries per window
K_PV_THREADS = 256    # kPvThreads
GATHER_LDS_LIMIT = 48 * 1024
FORM_OWNER, FORM_GATHER, FORM_SCATTER = 0, 1, 2


def own_window(nthr):
    """(RoI, bin) candidates per window of the ROIAlign owner kernel: two per thread."""
    return 2 * nthr


def pick_threads(cv):
    """roi_common.h pick_threads: whole waves for cv channel vectors, at most 256."""
    t = ((cv + 63) // 64) * 64
    return 256 if t > 256 else (64 if t < 64 else t)


def channel_vectors(C, aligned=True):
    """float4 vectors per pixel when C % 4 == 0 and every pointer is 16-byte aligned, else floats."""
    return C // 4 if (C % 4 == 0 and aligned) else C


def owner_threads(C, lanes=0, aligned=True):
    """Workgroup size of the ROIAlign owner kernel under set_tuning('roi_bwd_lanes', lanes)."""
    n = pick_threads(channel_vectors(C, aligned))
    return min(n, lanes) if lanes > 0 else n


def pv_threads(C, aligned=True):
    return pick_threads(channel_vectors(C, aligned))


def gather_lds_bytes(W, PH, PW):
    return 4 * (PH + (W + 4) * PW) + 4 * 2 * (W + 4)


def out_bins(P, bin_stride):
    return (P + bin_stride - 1) // bin_stride


def source_constants():
    """{name: int} of every ``constexpr int k... = <int>;`` of the two kernel files."""
    found = {}
    for name in ('roi_align.hip', 'roi_pool_variants.hip'):
        with open(os.path.join(CSRC, name)) as f:
            for k, v in re.findall(r'constexpr int (k\w+) = (\d+);', f.read()):
                found[k] = int(v)
    return found


def source_text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# ---- exactness -----------------------------------------------------------------------------------
def frac_bits(a, limit=30):
    """Smallest k with a * 2^k integral everywhere (a float64 array of dyadic rationals)."""
    a = np.asarray(a, np.float64)
    for k in range(limit + 1):
        s = a * 2. ** k
        if np.array_equal(s, np.rint(s)):
            return k
    raise AssertionError('not dyadic within %d bits' % limit)


def assert_exact(ref64, abs64, k, what):
    """ref64 (float64) survives the round trip through fp32, and every partial sum does: all are
    multiples of 2^-k bounded by abs64 (the same sums over |terms|)."""
    ref64 = np.asarray(ref64, np.float64)
    assert np.array_equal(ref64.astype(np.float32).astype(np.float64), ref64), \
        '%s: the float64 reference is not representable in fp32' % what
    assert np.array_equal(ref64 * 2. ** k, np.rint(ref64 * 2. ** k)), '%s: quantum 2^-%d' % (what, k)
    assert float(np.max(abs64, initial=0.)) * 2. ** k < 2. ** 24, \
        '%s: partial sums may need more than 24 bits (%g * 2^%d)' % (what, np.max(abs64), k)


def int_values(rng, shape, hi=8):
    """Integers in +-[1, hi], never 0, as float32."""
    return (rng.randint(1, hi + 1, shape) * rng.choice([-1, 1], shape)).astype(np.float32)


# ---- ROIAlign --------------------------------------------------------------------------------------
AlignCase = collections.namedtuple(
    'AlignCase', 'rois gy gx N H W C PH PW bin_stride sampling_ratio')


def align_extent(rois, H, W, PH, PW, sampling_ratio, spatial_scale=1.):
    """roi_align.hip roi_geom + roi_extent in fp32, operation for operation:
    (batch, ylo, yhi, xlo, xhi) int arrays, the patch the owner kernel tests a tile against."""
    f = np.asarray(rois, np.float32)
    s = np.float32(spatial_scale)
    one, half = np.float32(1), np.float32(.5)

    def axis(lo, hi, P, size):
        start = lo * s
        side = np.maximum(hi * s - start, one)
        bin_ = side / np.float32(P)
        grid = (np.full(side.shape, sampling_ratio) if sampling_ratio > 0
                else np.ceil(side / np.float32(P))).astype(np.int64)
        gf = grid.astype(np.float32)
        first = start + half * bin_ / gf
        last = start + np.float32(P - 1) * bin_ + (gf - half) * bin_ / gf
        a = np.floor(np.maximum(first, 0)).astype(np.int64) - 1
        b = np.floor(np.maximum(last, 0)).astype(np.int64) + 2
        return np.clip(a, 0, size - 1), np.clip(b, 0, size - 1)

    ylo, yhi = axis(f[:, 2], f[:, 4], PH, H)
    xlo, xhi = axis(f[:, 1], f[:, 3], PW, W)
    return f[:, 0].astype(np.int64), ylo, yhi, xlo, xhi


def align_meets(rois, H, W, PH, PW, sampling_ratio, tile, spatial_scale=1.):
    """bool (R): the RoIs step A of the owner kernel keeps for tile (n, y, x0)."""
    n, y, x0 = tile
    b, ylo, yhi, xlo, xhi = align_extent(rois, H, W, PH, PW, sampling_ratio, spatial_scale)
    return (b == n) & (y >= ylo) & (y <= yhi) & (xhi >= x0) & (xlo <= x0 + K_OWN_XT - 1)


def align_counters(rois, H, W, PH, PW, bin_stride, sampling_ratio, tile, nthr, spatial_scale=1.):
    """Per scan chunk of kOwnScan * nthr RoIs, for tile (n, y, x0): ``m`` RoIs kept, ``windows`` =
    ceil(m OH OW / (2 nthr)) candidate windows, ``entries`` (RoI, bin) candidates with a non-zero
    weight on the tile (what reaches the LDS list; from launch_ref.roi_tables)."""
    n, y, x0 = tile
    R = len(rois)
    nb = out_bins(PH, bin_stride) * out_bins(PW, bin_stride)
    meets = align_meets(rois, H, W, PH, PW, sampling_ratio, tile, spatial_scale)
    _, Ay, Bx, _ = L.roi_tables(torch.as_tensor(np.asarray(rois, np.float32)), H, W, PH, PW,
                                spatial_scale, sampling_ratio, bin_stride)
    hit_y = (Ay[:, :, y] != 0).numpy()                                   # (R, OH)
    hit_x = (Bx[:, :, x0:x0 + K_OWN_XT] != 0).any(2).numpy()             # (R, OW)
    live = hit_y[:, :, None] & hit_x[:, None, :]                         # (R, OH, OW)
    b = np.asarray(rois, np.float32)[:, 0].astype(np.int64)
    # the extent is a superset of the weights' support: no contribution escapes step A
    assert not (live.any((1, 2)) & (b == n) & ~meets).any()
    ent = live.sum((1, 2)) * meets
    chunk = K_OWN_SCAN * nthr
    m = [int(meets[r0:r0 + chunk].sum()) for r0 in range(0, R, chunk)]
    return dict(m=m, windows=[-(-k * nb // own_window(nthr)) for k in m],
                entries=[int(ent[r0:r0 + chunk].sum()) for r0 in range(0, R, chunk)],
                candidates=[k * nb for k in m])


def align_rois(rng, R, N, H, W, PH, PW, sampling_ratio, gs=(1, 2, 4), off_map=True, pile=None,
               empty_image=None):
    """(R, 5) float32 dyadic RoIs: integer corners, sides PH * gh x PW * gw.  ``pile`` =
    (indices, (n, y, x0), gs): those RoIs start inside the tile's 8 columns and cover row y; no other
    RoI's extent meets the tile.  ``empty_image``: an image index no RoI names."""
    images = [i for i in range(N) if i != empty_image]
    rois = np.zeros((R, 5), np.float32)

    def draw(k):
        gh, gw = rng.choice(gs, k), rng.choice(gs, k)
        sh, sw = PH * gh, PW * gw
        if off_map:
            y1 = rng.randint(-(sh // 2), H - 1, k) if H > 1 else -rng.randint(0, sh // 2 + 1, k)
            x1 = rng.randint(-(sw // 2), W, k)
        else:
            y1 = np.array([rng.randint(0, max(H - a, 0) + 1) for a in sh])
            x1 = np.array([rng.randint(0, max(W - a, 0) + 1) for a in sw])
        return np.stack([rng.choice(images, k), x1, y1, x1 + sw, y1 + sh], 1).astype(np.float32)

    rois[:] = draw(R)
    if pile is not None:
        idx, tile, pgs = pile
        idx = np.asarray(idx)
        n, y, x0 = tile
        for _ in range(200):
            rest = np.setdiff1d(np.arange(R), idx)
            bad = rest[align_meets(rois[rest], H, W, PH, PW, sampling_ratio, tile)]
            if not len(bad):
                break
            rois[bad] = draw(len(bad))
        else:
            raise AssertionError('could not keep the other RoIs off the tile')
        k = len(idx)
        gh, gw = rng.choice(pgs, k), rng.choice(pgs, k)
        sh, sw = PH * gh, PW * gw
        y1 = y - np.array([rng.randint(0, a) for a in sh])
        x1 = x0 + rng.randint(0, min(K_OWN_XT, W - x0), k)
        rois[idx] = np.stack([np.full(k, n), x1, y1, x1 + sw, y1 + sh], 1).astype(np.float32)
    return rois


def align_bwd_ref(rois, gy, shape, PH, PW, bin_stride, sampling_ratio, what='roi_align_bwd'):
    """float32 (N, H, W, C): launch_ref.roi_align_bwd in float64, proven exact."""
    rt = torch.as_tensor(rois)
    g64 = torch.as_tensor(gy).to(torch.float64)
    ref = L.roi_align_bwd(g64, rt, shape, 1., sampling_ratio, bin_stride, PH, PW).numpy()
    mag = L.roi_align_bwd(g64.abs(), rt, shape, 1., sampling_ratio, bin_stride, PH, PW).numpy()
    _, Ay, Bx, count = L.roi_tables(rt, shape[1], shape[2], PH, PW, 1., sampling_ratio, bin_stride)
    k = frac_bits(Ay.numpy()) + frac_bits(Bx.numpy()) + frac_bits(1. / count.numpy())
    assert_exact(ref, mag, k, what)
    return ref.astype(np.float32)


def align_fwd_ref(rois, x, PH, PW, bin_stride, sampling_ratio, what='roi_align_fwd'):
    """float32 (R, OH, OW, C): launch_ref.roi_align_fwd in float64 of an integer map, proven exact."""
    rt = torch.as_tensor(rois)
    x64 = torch.as_tensor(x).to(torch.float64)
    ref = L.roi_align_fwd(x64, rt, PH, PW, 1., sampling_ratio, bin_stride).numpy()
    mag = L.roi_align_fwd(x64.abs(), rt, PH, PW, 1., sampling_ratio, bin_stride).numpy()
    _, Ay, Bx, count = L.roi_tables(rt, x.shape[1], x.shape[2], PH, PW, 1., sampling_ratio, bin_stride)
    k = frac_bits(Ay.numpy()) + frac_bits(Bx.numpy()) + frac_bits(1. / count.numpy())
    assert_exact(ref, mag, k, what)
    return ref.astype(np.float32)


def align_case(seed, N, H, W, C, PH, PW, bin_stride, sampling_ratio, R, gy_hi=8, **kw):
    """An exact ROIAlign backward case (``kw``: align_rois' options)."""
    rng = np.random.RandomState(seed)
    rois = align_rois(rng, R, N, H, W, PH, PW, sampling_ratio, **kw)
    gy = int_values(rng, (R, out_bins(PH, bin_stride), out_bins(PW, bin_stride), C), gy_hi)
    gx = align_bwd_ref(rois, gy, (N, H, W, C), PH, PW, bin_stride, sampling_ratio,
                       'align_case(seed=%d)' % seed)
    return AlignCase(rois, gy, gx, N, H, W, C, PH, PW, bin_stride, sampling_ratio)


def awkward_rois(rng, R, N, H, W, scale):
    """tests/test_gpu_pool_variants._rois, restated for a host module: proposal-like boxes plus
    reversed corners, zero size, wholly before / past the map, .5 ties."""
    Hi, Wi = H / scale, W / scale
    y1 = rng.uniform(-0.1 * Hi, 0.9 * Hi, R)
    x1 = rng.uniform(-0.1 * Wi, 0.9 * Wi, R)
    h = rng.uniform(2, 0.6 * Hi, R)
    w = rng.uniform(2, 0.6 * Wi, R)
    b = rng.randint(0, N, R)
    rois = np.stack([b, x1, y1, x1 + w, y1 + h], 1).astype(np.float32)
    extra = np.array([[N - 1, 40, 40, 72, 72], [N - 1, 24, 8, 24, 8], [N - 1, 90, 90, 10, 10],
                      [0, 4 * Wi, 4 * Hi, 5 * Wi, 5 * Hi],
                      [N - 1, -3 * Wi, -3 * Hi, -2 * Wi, -2 * Hi],
                      [N - 1, -8, -8, 0.5 * Wi, 8], [0, 0, 0, Wi - 1, Hi - 1]], np.float32)
    return np.concatenate([rois, extra])


# ---- max pooling and crop-and-resize -----------------------------------------------------------------
def _pv_tables(kind, rois, N, H, W, PH, PW, bin_stride, out_rows=None):
    """pv_tables_kernel restated at spatial scale 1: per RoI (ok, batch, ylo, yhi, xlo, xhi) and
    the row / column entries as (R, O, 2) int arrays — pooling windows [start, end) or the two tap
    coordinates."""
    R = len(rois)
    OH, OW = out_bins(PH, bin_stride), out_bins(PW, bin_stride)
    rows = np.zeros((R, OH, 2), np.int64)
    cols = np.zeros((R, OW, 2), np.int64)
    ext = np.zeros((R, 6), np.int64)
    for r in range(R):
        b = int(np.float32(rois[r][0]))
        if kind == 'pool':
            hw, ww = PV.pool_windows(rois[r], PH, PW, 1., H, W)
            rows[r] = np.array(hw[::bin_stride])
            cols[r] = np.array(ww[::bin_stride])
            ys = [(a, e - 1) for a, e in rows[r] if e > a]
            xs = [(a, e - 1) for a, e in cols[r] if e > a]
        else:
            y1, x1, hc, wc = PV.crop_box(rois[r], 1., H, W)
            vi0, vi1, _, _ = PV.lin_taps(PH, hc)
            ui0, ui1, _, _ = PV.lin_taps(PW, wc)
            rows[r] = np.stack([y1 + vi0, y1 + vi1], 1)[::bin_stride]
            cols[r] = np.stack([x1 + ui0, x1 + ui1], 1)[::bin_stride]
            ys, xs = [tuple(t) for t in rows[r]], [tuple(t) for t in cols[r]]
        dst = r if out_rows is None else int(out_rows[r])
        ok = 0 <= b < N and 0 <= dst < R and bool(ys) and bool(xs)
        if ok:
            ext[r] = (1, b, min(a for a, _ in ys), max(e for _, e in ys),
                      min(a for a, _ in xs), max(e for _, e in xs))
    return ext, rows, cols


def _pv_hits(kind, t, lo, n):
    if kind == 'pool':
        return (t[:, 1] > lo) & (t[:, 0] < lo + n) & (t[:, 1] > t[:, 0])
    return ((t[:, 0] >= lo) & (t[:, 0] < lo + n)) | ((t[:, 1] >= lo) & (t[:, 1] < lo + n))


def pv_counters(kind, rois, N, H, W, PH, PW, bin_stride, tile, nthr, out_rows=None):
    """pv_bwd_owner_kernel on tile (n, y, x0), per scan chunk of nthr RoIs: ``m`` RoIs kept, ``ntot``
    rectangle entries, ``windows`` = ceil(ntot / kPvCap), and ``straddles``: the rectangles that
    begin in one kPvCap window and end in a later one (clipped by j0 / j1)."""
    n, y, x0 = tile
    ext, rows, cols = _pv_tables(kind, rois, N, H, W, PH, PW, bin_stride, out_rows)
    R = len(rois)
    out = dict(m=[], ntot=[], windows=[], straddles=[])
    for r0 in range(0, R, nthr):
        m = off = straddle = 0
        for r in range(r0, min(r0 + nthr, R)):
            ok, b, ylo, yhi, xlo, xhi = ext[r]
            if not (ok and b == n and ylo <= y <= yhi and xhi >= x0 and xlo <= x0 + K_PV_XT - 1):
                continue
            m += 1
            hy = np.nonzero(_pv_hits(kind, rows[r], y, 1))[0]
            hx = np.nonzero(_pv_hits(kind, cols[r], x0, K_PV_XT))[0]
            cnt = (hy[-1] - hy[0] + 1) * (hx[-1] - hx[0] + 1) if len(hy) and len(hx) else 0
            if cnt and off // K_PV_CAP != (off + cnt - 1) // K_PV_CAP:
                straddle += 1
            off += int(cnt)
        out['m'].append(m)
        out['ntot'].append(off)
        out['windows'].append(-(-off // K_PV_CAP))
        out['straddles'].append(straddle)
    return out


def pv_entries(kind, rois, N, H, W, PH, PW, bin_stride, tile, nthr, out_rows=None):
    """The LDS list of the first scan chunk on tile (n, y, x0), in the kernel's order: (RoI, oh, ow)
    of every rectangle entry — RoIs in index order, each rectangle row-major."""
    n, y, x0 = tile
    ext, rows, cols = _pv_tables(kind, rois, N, H, W, PH, PW, bin_stride, out_rows)
    out = []
    for r in range(min(nthr, len(rois))):
        ok, b, ylo, yhi, xlo, xhi = ext[r]
        if not (ok and b == n and ylo <= y <= yhi and xhi >= x0 and xlo <= x0 + K_PV_XT - 1):
            continue
        hy = np.nonzero(_pv_hits(kind, rows[r], y, 1))[0]
        hx = np.nonzero(_pv_hits(kind, cols[r], x0, K_PV_XT))[0]
        if len(hy) and len(hx):
            out += [(r, oh, ow) for oh in range(hy[0], hy[-1] + 1) for ow in range(hx[0], hx[-1] + 1)]
    return out


def nhwc(a):
    return np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1)))


def nchw(a):
    return np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2)))


CROP_EXACT_OUT = (5, 9, 17)       # n - 1 a power of two: dyadic linspace steps for any crop size
CROP_EXACT_SIZES = (2, 3, 5)


def crop_rois(rng, R, N, H, W, sizes=CROP_EXACT_SIZES, pile=None):
    """Integer crops of ``sizes`` pixels inside the map.  ``pile`` = (indices, (n, y, x0), size):
    those crops start on row y, inside the tile's columns."""
    hc, wc = rng.choice(sizes, R), rng.choice(sizes, R)
    y1 = np.array([rng.randint(0, max(H - a, 0) + 1) for a in hc])
    x1 = np.array([rng.randint(0, max(W - a, 0) + 1) for a in wc])
    rois = np.stack([rng.randint(0, N, R), x1, y1, x1 + wc, y1 + hc], 1).astype(np.float32)
    if pile is not None:
        idx, (n, y, x0), size = pile
        k = len(idx)
        px = x0 + rng.randint(0, max(min(K_PV_XT, W - x0) - size, 0) + 1, k)
        rois[np.asarray(idx)] = np.stack([np.full(k, n), px, np.full(k, y), px + size,
                                          np.full(k, y + size)], 1).astype(np.float32)
    return rois


def crop_bwd_ref(rois, gy, shape, bin_stride=1, out_rows=None, PH=None, PW=None, what='crop_bwd'):
    """float32 (N, H, W, C): pool_variants_ref.crop_and_resize_bwd(dtype=float64) at scale 1,
    proven exact.  gy (R, OH, OW, C) in the kernel's row order: row out_rows[r] holds RoI r (the
    restatement places rows by its own batch sort, so they are permuted to that here)."""
    N, H, W, C = shape
    R, OH, OW, _ = gy.shape
    PH = PH if PH is not None else OH * bin_stride
    PW = PW if PW is not None else OW * bin_stride
    mine = np.arange(R) if out_rows is None else np.asarray(out_rows)
    theirs = PV.output_rows(rois)
    full = np.zeros((R, C, PH, PW), np.float64)
    g = nchw(gy).astype(np.float64)
    for r in range(R):
        full[theirs[r], :, ::bin_stride, ::bin_stride] = g[mine[r]]
    ref = PV.crop_and_resize_bwd(full, rois, (N, C, H, W), 1., dtype=np.float64)
    mag = PV.crop_and_resize_bwd(np.abs(full), rois, (N, C, H, W), 1., dtype=np.float64)
    k = 0
    for m in set(int(v) for r in rois for v in PV.crop_box(r, 1., H, W)[2:]):
        k = max(k, frac_bits(PV.lin_taps(PH, m)[3].astype(np.float64)),
                frac_bits(PV.lin_taps(PW, m)[3].astype(np.float64)))
    assert_exact(ref, mag, 2 * k, what)
    return nhwc(ref).astype(np.float32)


def crop_bwd_close_ref(rois, gy, shape, bin_stride=1, out_rows=None):
    """float64 (N, H, W, C) adjoint without the exactness proof (non-dyadic output sizes)."""
    N, H, W, C = shape
    R, OH, OW, _ = gy.shape
    mine = np.arange(R) if out_rows is None else np.asarray(out_rows)
    theirs = PV.output_rows(rois)
    full = np.zeros((R, C, OH * bin_stride, OW * bin_stride), np.float64)
    g = nchw(gy).astype(np.float64)
    for r in range(R):
        full[theirs[r], :, ::bin_stride, ::bin_stride] = g[mine[r]]
    return nhwc(PV.crop_and_resize_bwd(full, rois, (N, C, H, W), 1., dtype=np.float64))


def pool_rois(rng, R, N, H, W, pile=None, max_side=6):
    """Integer boxes, some over the map's edge.  ``pile`` = (indices, (n, y, x0), side): boxes of
    ``side`` pixels that start on row y inside the tile's columns."""
    h, w = rng.randint(1, max_side + 1, R), rng.randint(1, max_side + 1, R)
    y1, x1 = rng.randint(-1, H, R), rng.randint(-1, W, R)
    rois = np.stack([rng.randint(0, N, R), x1, y1, x1 + w - 1, y1 + h - 1], 1).astype(np.float32)
    if pile is not None:
        idx, (n, y, x0), side = pile
        k = len(idx)
        px = x0 + rng.randint(0, max(min(K_PV_XT, W - x0) - side, 0) + 1, k)
        rois[np.asarray(idx)] = np.stack([np.full(k, n), px, np.full(k, y), px + side - 1,
                                          np.full(k, y + side - 1)], 1).astype(np.float32)
    return rois


def pool_refs(x, rois, gy, PH, PW, bin_stride=1):
    """(y, argmax (R, OH, OW, C) int32, gx (N, H, W, C)) of pool_variants_ref at scale 1 for a map x
    (N, H, W, C) and gy (R, OH, OW, C): the backward is the restatement's fp32 sum in the kernel's
    order, of integers."""
    y, am = PV.roi_pooling_2d_fwd(nchw(x), rois, PH, PW, 1.)
    y, am = PV.strided(y, bin_stride), PV.strided(am, bin_stride)
    gx = PV.roi_pooling_2d_bwd(nchw(gy), am, rois, (x.shape[0], x.shape[3], x.shape[1], x.shape[2]))
    return nhwc(y), nhwc(am), nhwc(gx)


def find_pile(kind, target, N, H, W, PH, PW, bin_stride, tile, nthr, sizes, seed=0, tries=400):
    """Host search over the restated geometry: RoIs piled on ``tile`` whose ntot there is exactly
    ``target``.  Candidate boxes of ``sizes`` pixels at every offset that meets the tile are
    measured one at a time, then a subset-sum over their entry counts picks the pile.  Returns the
    (k, 5) RoIs or None."""
    n, y, x0 = tile
    cand = []
    for s in sizes:
        for dy in range(-s, 1):
            for dx in range(-s, K_PV_XT):
                x1, y1 = x0 + dx, y + dy
                if x1 < 0 or y1 < 0:
                    continue
                roi = np.array([[n, x1, y1, x1 + s - (kind == 'pool'), y1 + s - (kind == 'pool')]],
                               np.float32)
                c = pv_counters(kind, roi, N, H, W, PH, PW, bin_stride, tile, nthr)['ntot'][0]
                if c:
                    cand.append((c, roi[0]))
    if not cand:
        return None
    # unbounded subset sum, fewest RoIs first
    best = {0: []}
    for total in range(1, target + 1):
        for c, roi in cand:
            prev = total - c
            if prev in best and (total not in best or len(best[prev]) + 1 < len(best[total])):
                best[total] = best[prev] + [roi]
    if target not in best or len(best[target]) > nthr:
        return None
    return np.stack(best[target]).astype(np.float32)


# ---- the catalogue: every exact configuration the GPU tests run ---------------------------------------
# tests/test_roi_exact_cases_cpu.py builds each one on the host (the builders prove exactness and the
# counters prove the branch); tests/test_gpu_roi_exact.py runs them.  Built once per process.

BINS = [(7, 7, 1), (3, 5, 1), (14, 14, 1), (14, 14, 2), (14, 14, 3)]
SAMPLING = [0, 1, 2]
LANES = [64, 128, 192, 0]
WINDOW_EDGES = ['2n-1', '2n', '2n+1', '>4n']
ALIGN_TILE = (1, 3, 8)       # image, row, first column of the tile ROIAlign RoIs are piled on
PV_TILE = (1, 2, 0)
# ROIAlign channel cases: (C, byte offset of the misaligned map, float4 kernel?, channel vectors,
# lanes, channel chunks).  260 = 4 * 65 runs the float4 kernel when aligned (one partial chunk)
# and the scalar kernel in two chunks when the map is 4 bytes off.
CHANNELS = [(3, 0, False, 3, 64, 1), (260, 0, True, 65, 128, 1), (260, 4, False, 260, 256, 2),
            (261, 0, False, 261, 256, 2), (1028, 0, True, 257, 256, 2)]
NARROW = [(N, H, W) for W in (1, 7, 8, 9) for N, H in ((1, 1), (2, 3))]
PV_CHUNKS = [(8, 64), (8, 65), (8, 3 * 64 + 5), (1024, 257)]
PV_PILES = [(1, 1, 0), (2, 2, 1), (3, 2, 1), (4, 3, 2), (7, 4, 3)]     # k RoIs, windows, straddles (crop)
PV_FULL = [512, 513, 1024, 1025]


def scatter_width(PH, PW):
    """Smallest W whose gather tables no longer fit 48 KB of LDS."""
    W = 1
    while gather_lds_bytes(W, PH, PW) <= GATHER_LDS_LIMIT:
        W += 1
    return W


@functools.lru_cache(maxsize=None)
def form_cases(PH, PW, bs, sr):
    """[(case, [(workspace mode, form)])]: 600 RoIs on a two-image 11 x 19 map (owner, gather,
    gather through a shifted workspace), then a 2-row map just wide enough for the scatter form, and
    one pixel narrower (gather)."""
    seed = 1000 * sr + 10 * PH + bs
    W = scatter_width(PH, PW)
    assert 2 * W <= 4000
    return [(align_case(seed, 2, 11, 19, 4, PH, PW, bs, sr, 600),
             [('aligned', FORM_OWNER), (None, FORM_GATHER), ('shifted', FORM_GATHER)]),
            (align_case(seed + 1, 1, 2, W, 4, PH, PW, bs, sr, 40),
             [('aligned', FORM_OWNER), (None, FORM_SCATTER)]),
            (align_case(seed + 2, 1, 2, W - 1, 4, PH, PW, bs, sr, 40), [(None, FORM_GATHER)])]


@functools.lru_cache(maxsize=None)
def lds_case(W):
    return align_case(W, 1, 2, W, 4, 14, 14, 1, 0, 24)


@functools.lru_cache(maxsize=None)
def roi_count_case(R):
    """One 1 x 1 bin per RoI on a 2 x 3 map, one channel (g = 1: 2 fraction bits leave room for the
    sum of 65536 terms)."""
    return align_case(R, 1, 2, 3, 1, 1, 1, 1, 0, R, gs=(1,))


def lanes_channels(lanes):
    """Channels for a lanes-wide owner workgroup: two channel chunks, the second of two float4
    lanes (1024 channels fill the default 256 lanes once)."""
    return 4 * lanes + 8 if lanes else 1024


@functools.lru_cache(maxsize=None)
def chunk_edge_case(lanes, extra):
    """(case, nthr, counters on ALIGN_TILE): R = 4 nthr (+ 1) RoIs of 2 x 2 bins; the RoIs next to
    the scan chunk's edge, and the lone one past it, are piled on the tile."""
    C = lanes_channels(lanes)
    nthr = owner_threads(C, lanes)
    assert nthr == (lanes or 256)
    R = K_OWN_SCAN * nthr + extra
    idx = [0, 1, R // 2, 4 * nthr - 2, 4 * nthr - 1] + ([4 * nthr] if extra else [])
    c = align_case(lanes + extra, 2, 6, 19, C, 2, 2, 1, 0, R, gy_hi=4, pile=(idx, ALIGN_TILE, (1, 2, 4)))
    k = align_counters(c.rois, c.H, c.W, 2, 2, 1, 0, ALIGN_TILE, nthr)
    assert k['m'] == ([5, 1] if extra else [5]) and all(e > 0 for e in k['entries']), k
    return c, nthr, k


def bins_for(target):
    """(OH, OW, m) with m * OH * OW == target: the first listed bin grid that divides it."""
    for oh, ow in ((3, 5), (3, 3), (1, 7), (1, 5), (2, 2), (1, 3), (1, 1)):
        if target % (oh * ow) == 0:
            return oh, ow, target // (oh * ow)


@functools.lru_cache(maxsize=None)
def window_edge_case(lanes, where):
    """(case, nthr, counters): m RoIs piled on ALIGN_TILE with m * OH * OW candidates one short of a
    window of 2 nthr, exactly one window, one over, and more than two windows."""
    C = lanes_channels(lanes)
    nthr = owner_threads(C, lanes)
    target = {'2n-1': 2 * nthr - 1, '2n': 2 * nthr, '2n+1': 2 * nthr + 1, '>4n': 4 * nthr + 4}[where]
    PH, PW, m = bins_for(target)
    R = m + 24
    assert R <= K_OWN_SCAN * nthr
    idx = np.sort(np.random.RandomState(target).choice(R, m, replace=False))
    c = align_case(target, 2, 6, 19, C, PH, PW, 1, 0, R, gy_hi=2, pile=(idx, ALIGN_TILE, (1, 2)))
    k = align_counters(c.rois, c.H, c.W, PH, PW, 1, 0, ALIGN_TILE, nthr)
    assert k['m'] == [m] and k['candidates'] == [target], k
    assert k['windows'] == [{'2n-1': 1, '2n': 1, '2n+1': 2, '>4n': 3}[where]], k
    assert k['entries'][0] >= m
    return c, nthr, k


@functools.lru_cache(maxsize=None)
def narrow_case(N, H, W, sr):
    tiles = N * H * ((W + K_OWN_XT - 1) // K_OWN_XT)
    assert (tiles < 8) == (H == 1 or W <= 8)
    return align_case(100 * W + H + sr, N, H, W, 8, 7, 7, 1, sr, 50)


@functools.lru_cache(maxsize=None)
def channel_case(C, off):
    return align_case(C + off, 2, 6, 19, C, 7, 7, 1, 0, 60)


@functools.lru_cache(maxsize=None)
def channel_fwd_cases(C, off):
    """[(rois, x, PH, PW, bin_stride, sampling_ratio, y reference)] on an integer map."""
    rng = np.random.RandomState(C + off)
    out = []
    for PH, PW, bs, sr in ((7, 7, 1, 0), (14, 14, 2, 2), (14, 14, 3, 0)):
        rois = align_rois(rng, 60, 2, 6, 19, PH, PW, sr)
        x = int_values(rng, (2, 6, 19, C))
        out.append((rois, x, PH, PW, bs, sr, align_fwd_ref(rois, x, PH, PW, bs, sr)))
    return out


@functools.lru_cache(maxsize=None)
def nonfinite_case(C):
    """7 x 7 bins of one pixel each, every RoI inside a 2 x 9 x 27 map: bin (3, 4) of RoI 17 has
    one sample with four taps of weight 1/4."""
    return align_case(77 + C, 2, 9, 27, C, 7, 7, 1, 0, 40, off_map=False, gs=(1,))


@functools.lru_cache(maxsize=None)
def empty_image_case():
    """Three images, the middle one without a RoI: the owner form, which never zero-fills, must
    write its zeros."""
    c = align_case(9, 3, 11, 19, 4, 7, 7, 1, 0, 200, empty_image=1)
    assert not c.gx[1].any() and c.gx[0].any() and c.gx[2].any()
    return c


PvCase = collections.namedtuple('PvCase', 'kind rois shape PH PW bin_stride out_rows x gy refs counters')


def _pv_case(kind, rois, shape, PH, PW, bs, seed, tile, out_rows=None, exact=True):
    """gy of integers and the references: pooling (y, argmax, gx) of the restatement's in-order fp32
    sums of integers; crop-and-resize gx proven exact (or, for a non-dyadic output size, the float64
    adjoint, refs[1] False)."""
    rng = np.random.RandomState(seed)
    N, H, W, C = shape
    gy = int_values(rng, (len(rois), out_bins(PH, bs), out_bins(PW, bs), C))
    x = rng.standard_normal(shape).astype(np.float32)
    if kind == 'pool':
        refs = pool_refs(x, rois, gy, PH, PW, bs)
    elif exact:
        refs = (crop_bwd_ref(rois, gy, shape, bs, out_rows, PH, PW), True)
    else:
        refs = (crop_bwd_close_ref(rois, gy, shape, bs, out_rows), False)
    k = pv_counters(kind, rois, N, H, W, PH, PW, bs, tile, pv_threads(C), out_rows)
    return PvCase(kind, rois, shape, PH, PW, bs, out_rows, x, gy, refs, k)


def _pv_rois(kind, rng, R, N, H, W, idx):
    return (pool_rois if kind == 'pool' else crop_rois)(rng, R, N, H, W, pile=(idx, PV_TILE, 3))


@functools.lru_cache(maxsize=None)
def pv_chunk_case(kind, C, R):
    """R = nthr, nthr + 1, 3 nthr + 5 RoIs (nthr = 64 at C = 8, 256 at C = 1024) on a 2 x 6 x 9 map;
    the RoIs on both sides of every scan chunk's edge are piled on PV_TILE."""
    nthr = pv_threads(C)
    assert nthr == (64 if C == 8 else 256)
    chunks = -(-R // nthr)
    assert chunks == {64: 1, 65: 2, 197: 4, 257: 2}[R]
    idx = sorted(set([0] + [e + d for e in range(nthr, R, nthr) for d in (-1, 0)]))
    rois = _pv_rois(kind, np.random.RandomState(R + C), R, 2, 6, 9, idx)
    PH, PW = (7, 7) if kind == 'pool' else (5, 9)
    c = _pv_case(kind, rois, (2, 6, 9, C), PH, PW, 1, R, PV_TILE)
    k = c.counters
    assert len(k['m']) == chunks and min(k['m']) >= 1 and min(k['ntot']) >= 1, k
    return c


@functools.lru_cache(maxsize=None)
def pv_stride_case(kind, bs):
    """14 x 14 (pooling) / 17 x 17 (crop-and-resize) bins read with stride bs, two scan chunks."""
    P = 14 if kind == 'pool' else 17
    rois = _pv_rois(kind, np.random.RandomState(bs), 70, 2, 6, 9, [63, 64])
    c = _pv_case(kind, rois, (2, 6, 9, 8), P, P, bs, bs, PV_TILE)
    assert len(c.counters['m']) == 2 and min(c.counters['m']) >= 1
    return c


def _with_others(kind, pile, H, W, seed, others=6):
    """The piled RoIs (image 0), then a few in image 1."""
    rest = (pool_rois if kind == 'pool' else crop_rois)(np.random.RandomState(seed), others, 1, H, W)
    rest[:, 0] = 1
    return np.concatenate([pile, rest]).astype(np.float32)


PILE_TILE = (0, 1, 0)      # row 1: the LAST entry of a piled RoI's rectangle carries weight there


@functools.lru_cache(maxsize=None)
def pv_pile_case(kind, k):
    """k 2 x 2-pixel RoIs at the map's origin onto 17 x 17 bins, counted on PILE_TILE (row 1): 17 x 17
    = 289 (crop-and-resize: both taps of every bin row lie on rows 0 and 1) or 9 x 17 = 153 (pooling:
    bin rows 8 .. 16 cover row 1) rectangle entries each.  On row 1 a rectangle's last entry (the
    last bin row and column) has weight 1 — on row 0 it would have weight 0 for crop-and-resize and
    a window that lost it would go unnoticed."""
    end = 1 if kind == 'pool' else 2
    rois = _with_others(kind, np.tile(np.array([[0, 0, 0, end, end]], np.float32), (k, 1)), 6, 9, k)
    c = _pv_case(kind, rois, (2, 6, 9, 8), 17, 17, 1, k, PILE_TILE)
    assert c.counters['ntot'] == [k * (153 if kind == 'pool' else 289)], c.counters
    return c


@functools.lru_cache(maxsize=None)
def pv_full_case(kind, target):
    """Exactly ``target`` list entries on PILE_TILE, found by find_pile among 2- and 16-pixel boxes
    onto 16 x 16 bins of a 17 x 24 map (a 2-pixel box over rows 0 and 1 gives 256 / 128 entries, a
    16-pixel box whose first row and last-but-one column meet the tile gives 1).  16 x 16 is not a
    dyadic output size: crop-and-resize is compared under the pool-variant suite's bound there."""
    pile = find_pile(kind, target, 1, 17, 24, 16, 16, 1, PILE_TILE, 64, sizes=(2, 16))
    assert pile is not None, 'no pile of %d entries for %s' % (target, kind)
    c = _pv_case(kind, _with_others(kind, pile, 17, 24, target), (2, 17, 24, 8), 16, 16, 1, target,
                 PILE_TILE, exact=False)
    assert c.counters['ntot'] == [target] and c.counters['windows'] == [-(-target // K_PV_CAP)]
    return c


@functools.lru_cache(maxsize=None)
def pv_out_rows_case(R):
    """Crop-and-resize, 9 x 5 bins, out_rows a random permutation, RoIs piled across the chunk edge."""
    rng = np.random.RandomState(R)
    rois = _pv_rois('crop', rng, R, 2, 6, 9, [0, 63, 64, R - 1])
    out_rows = rng.permutation(R)
    assert not np.array_equal(out_rows, np.arange(R))
    c = _pv_case('crop', rois, (2, 6, 9, 8), 9, 5, 1, R, PV_TILE, out_rows=out_rows)
    k = c.counters
    assert len(k['m']) == -(-R // 64) and k['m'][0] >= 2 and k['m'][1] >= 1
    return c
