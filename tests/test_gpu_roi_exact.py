"""The RoI extractors' backward forms and list boundaries on the device, bit for bit.

Every case here is built by tests/roi_exact_cases.py, whose builders prove on the host that the
float64 reference — and every partial sum, in any order — is representable in fp32.  So the
pixel-owner, gather and scatter forms of the ROIAlign backward, and the pixel-owner backwards of max
pooling and crop-and-resize, must equal the reference with ``array_equal``: a lost, doubled or
misplaced list entry cannot hide inside a tolerance.  Each case asserts, through
``mrcnn_roi_align_bwd_form`` or the restated list counters, that it reaches the branch it is named
for.  Entry points are called directly through the C ABI; the gradient map sits inside a guard band
of NaNs that must come back untouched.
"""
import ctypes

import numpy as np
import pytest
import torch

from chainer_mask_rcnn_amd import _lib

import launch_ref as L
import pool_variants_ref as PV
import roi_exact_cases as X

pytestmark = pytest.mark.gpu

GUARD = 64        # floats on either side of an output: 256 bytes, keeps the 16-byte alignment


# ---- placing arrays at chosen addresses -------------------------------------------------------------
def _place(a, dev, offset=0):
    """The array on the device, its first byte ``offset`` bytes past a 16-byte boundary."""
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a)
    assert offset % t.element_size() == 0
    k = offset // t.element_size()
    flat = torch.zeros(a.size + 8, dtype=t.dtype, device=dev)
    assert flat.data_ptr() % 16 == 0
    v = flat[k:k + a.size].view(a.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == offset % 16
    return v


class _Guarded(object):
    """An output of ``shape`` pre-filled with NaN (int: -7) inside a guard band of the same."""

    def __init__(self, shape, dev, offset=0, dtype=torch.float32):
        n = int(np.prod(shape))
        k = offset // 4
        self.fill = float('nan') if dtype == torch.float32 else -7
        self.whole = torch.full((GUARD + n + GUARD + 8,), self.fill, dtype=dtype, device=dev)
        assert self.whole.data_ptr() % 16 == 0
        self.lo, self.hi = GUARD + k, GUARD + k + n
        self.t = self.whole[self.lo:self.hi].view(shape)

    def result(self):
        torch.cuda.synchronize()
        w = self.whole.cpu().numpy()
        band = np.concatenate([w[:self.lo], w[self.hi:]])
        assert np.isnan(band).all() if w.dtype.kind == 'f' else (band == self.fill).all(), \
            'the kernel wrote outside its output'
        return w[self.lo:self.hi].reshape(tuple(self.t.shape)).copy()


def _ws(nbytes, dev, shift=0):
    buf = torch.empty(nbytes + 16, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    return buf, ctypes.c_void_p(buf.data_ptr() + shift)


# ---- direct calls --------------------------------------------------------------------------------------
def _align_bwd(dev, rois, gy, shape, PH, PW, bs, sr, scale=1., ws='aligned', off=None):
    """mrcnn_roi_align_bwd_ws -> (form reported by mrcnn_roi_align_bwd_form, gx (N, H, W, C)).
    ws: 'aligned', 'shifted' (8 bytes past a 16-byte boundary) or None."""
    off = off or {}
    lib = _lib.load()
    N, H, W, C = shape
    R = len(rois)
    gyd = _place(gy, dev, off.get('gy', 0))
    rd = _place(rois, dev)
    gx = _Guarded(shape, dev, off.get('gx', 0))
    need = lib.mrcnn_roi_align_bwd_workspace_bytes(N, H, W, R, PH, PW, bs)
    buf, wsp, nbytes = None, None, 0
    if ws is not None:
        buf, wsp = _ws(need, dev, 8 if ws == 'shifted' else 0)
        nbytes = need
    form = lib.mrcnn_roi_align_bwd_form(N, H, W, R, PH, PW, bs, int(wsp is not None),
                                        int(wsp is not None and wsp.value % 16 == 0))
    _lib.call('mrcnn_roi_align_bwd_ws', _lib.ptr(gyd), _lib.ptr(rd), _lib.ptr(gx.t), N, H, W, C, R,
              PH, PW, bs, scale, sr, wsp, nbytes, _lib.stream_ptr())
    return form, gx.result()


def _align_fwd(dev, rois, x, PH, PW, bs, sr, scale=1., order=None, off=None):
    off = off or {}
    N, H, W, C = x.shape
    R = len(rois)
    xd = _place(x, dev, off.get('x', 0))
    rd = _place(rois, dev)
    y = _Guarded((R, X.out_bins(PH, bs), X.out_bins(PW, bs), C), dev, off.get('y', 0))
    od = None if order is None else _place(np.asarray(order, np.int32), dev)
    _lib.call('mrcnn_roi_align_fwd_ex', _lib.ptr(xd), _lib.ptr(rd), _lib.ptr(y.t), N, H, W, C, R, PH,
              PW, bs, scale, sr, _lib.ptr(od), _lib.stream_ptr())
    return y.result()


def _pool_fwd(dev, rois, x, PH, PW, bs, off=None):
    off = off or {}
    N, H, W, C = x.shape
    R = len(rois)
    out = (R, X.out_bins(PH, bs), X.out_bins(PW, bs), C)
    xd, rd = _place(x, dev, off.get('x', 0)), _place(rois, dev)
    y = _Guarded(out, dev, off.get('y', 0))
    am = _Guarded(out, dev, off.get('argmax', 0), torch.int32)
    _lib.call('mrcnn_roi_pool_fwd', _lib.ptr(xd), _lib.ptr(rd), _lib.ptr(y.t), _lib.ptr(am.t), N, H, W,
              C, R, PH, PW, bs, 1., None, _lib.stream_ptr())
    return y.result(), am.result()


def _pool_bwd(dev, rois, gy, argmax, shape, PH, PW, bs, off=None):
    off = off or {}
    lib = _lib.load()
    N, H, W, C = shape
    R = len(rois)
    gyd, rd = _place(gy, dev, off.get('gy', 0)), _place(rois, dev)
    amd = _place(np.asarray(argmax, np.int32), dev, off.get('argmax', 0))
    gx = _Guarded(shape, dev, off.get('gx', 0))
    need = lib.mrcnn_roi_pool_bwd_workspace_bytes(N, H, W, R, PH, PW, bs)
    buf, wsp = _ws(need, dev)
    _lib.call('mrcnn_roi_pool_bwd_ws', _lib.ptr(gyd), _lib.ptr(amd), _lib.ptr(rd), _lib.ptr(gx.t), N, H,
              W, C, R, PH, PW, bs, 1., wsp, need, _lib.stream_ptr())
    return gx.result()


def _crop_fwd(dev, rois, x, PH, PW, bs, out_rows=None, off=None):
    off = off or {}
    N, H, W, C = x.shape
    R = len(rois)
    xd, rd = _place(x, dev, off.get('x', 0)), _place(rois, dev)
    od = None if out_rows is None else _place(np.asarray(out_rows, np.int32), dev)
    y = _Guarded((R, X.out_bins(PH, bs), X.out_bins(PW, bs), C), dev, off.get('y', 0))
    _lib.call('mrcnn_crop_resize_fwd', _lib.ptr(xd), _lib.ptr(rd), _lib.ptr(od), _lib.ptr(y.t), N, H, W,
              C, R, PH, PW, bs, 1., None, _lib.stream_ptr())
    return y.result()


def _crop_bwd(dev, rois, gy, shape, PH, PW, bs, out_rows=None, off=None):
    off = off or {}
    lib = _lib.load()
    N, H, W, C = shape
    R = len(rois)
    gyd, rd = _place(gy, dev, off.get('gy', 0)), _place(rois, dev)
    od = None if out_rows is None else _place(np.asarray(out_rows, np.int32), dev)
    gx = _Guarded(shape, dev, off.get('gx', 0))
    need = lib.mrcnn_crop_resize_bwd_workspace_bytes(N, H, W, R, PH, PW, bs)
    buf, wsp = _ws(need, dev)
    _lib.call('mrcnn_crop_resize_bwd_ws', _lib.ptr(gyd), _lib.ptr(rd), _lib.ptr(od), _lib.ptr(gx.t), N,
              H, W, C, R, PH, PW, bs, 1., wsp, need, _lib.stream_ptr())
    return gx.result()


def _bits(got, ref):
    """array_equal on the values, with the first differing element in the message."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype
    if not np.array_equal(got, ref):
        bad = np.argwhere(~(got == ref))
        i = tuple(bad[0])
        raise AssertionError('%d of %d elements differ; first at %s: got %r, reference %r'
                             % (len(bad), got.size, i, got[i], ref[i]))


def _run_case_all_ways(dev, c, ways):
    """Run an exact ROIAlign case in each (workspace mode, expected form): bit equality."""
    for ws, want in ways:
        form, gx = _align_bwd(dev, c.rois, c.gy, (c.N, c.H, c.W, c.C), c.PH, c.PW, c.bin_stride,
                              c.sampling_ratio, ws=ws)
        assert form == want, (ws, form, want)
        _bits(gx, c.gx)


# ---- a. every ROIAlign backward form, exactly --------------------------------------------------------
@pytest.mark.parametrize('sr', X.SAMPLING)
@pytest.mark.parametrize('PH,PW,bs', X.BINS)
def test_align_bwd_every_form_is_exact(dev, PH, PW, bs, sr):
    """Owner and gather (also: owner refused for a workspace 8 bytes off a 16-byte boundary) on a
    two-image 11 x 19 map with 600 dyadic RoIs partly off the map; then owner and scatter on a 2-row
    map just wide enough that the gather form's LDS tables pass 48 KB, and gather one pixel
    narrower.  All equal the float64 reference bit for bit."""
    for c, ways in X.form_cases(PH, PW, bs, sr):
        _run_case_all_ways(dev, c, ways)


@pytest.mark.parametrize('W,lds,form', [(763, 49144, X.FORM_GATHER), (764, 49208, X.FORM_SCATTER)])
def test_align_bwd_gather_scatter_boundary_by_lds(dev, W, lds, form):
    assert X.gather_lds_bytes(W, 14, 14) == lds and (lds <= 49152) == (form == X.FORM_GATHER)
    _run_case_all_ways(dev, X.lds_case(W), [(None, form), ('aligned', X.FORM_OWNER)])


@pytest.mark.parametrize('R,form', [(65535, X.FORM_GATHER), (65536, X.FORM_SCATTER)])
def test_align_bwd_gather_scatter_boundary_by_roi_count(dev, R, form):
    """The gather form carries the RoI in grid.y: 65535 RoIs at most.  One 1 x 1 bin per RoI on a
    2 x 3 map, one channel; the owner form walks the same RoIs in 256 scan chunks."""
    _run_case_all_ways(dev, X.roi_count_case(R), [(None, form), ('aligned', X.FORM_OWNER)])


@pytest.mark.parametrize('sr', [0, 2])
def test_align_bwd_every_form_on_awkward_rois(dev, sr):
    """Random non-dyadic RoIs with reversed corners, zero size, wholly before / past the map: all
    three forms within the suite's bound (launch_ref._close) of the float64 reference."""
    rng = np.random.RandomState(40 + sr)
    own_gather = [('aligned', X.FORM_OWNER), (None, X.FORM_GATHER)]
    for shape, scale, ways in (((2, 13, 19, 8), 1 / 16., own_gather), ((2, 13, 19, 8), 0.3, own_gather),
                               ((2, 2, X.scatter_width(7, 7), 4), 0.3,
                                [('aligned', X.FORM_OWNER), (None, X.FORM_SCATTER)])):
        N, H, W, C = shape
        rois = X.awkward_rois(rng, 30, N, H, W, scale)
        gy = rng.standard_normal((len(rois), 7, 7, C)).astype(np.float32)
        ref = L.roi_align_bwd(torch.from_numpy(gy).double(), torch.from_numpy(rois), shape, scale, sr,
                              1, 7, 7).numpy()
        for ws, want in ways:
            form, gx = _align_bwd(dev, rois, gy, shape, 7, 7, 1, sr, scale=scale, ws=ws)
            assert form == want
            L._close(gx, ref)


# ---- b. ROIAlign owner list boundaries, exactly -----------------------------------------------------
def _owner_with_lanes(dev, c, lanes):
    _lib.set_tuning('roi_bwd_lanes', lanes)
    try:
        form, gx = _align_bwd(dev, c.rois, c.gy, (c.N, c.H, c.W, c.C), c.PH, c.PW, c.bin_stride,
                              c.sampling_ratio)
    finally:
        _lib.set_tuning('roi_bwd_lanes', 0)
    assert form == X.FORM_OWNER
    return gx


@pytest.mark.parametrize('lanes', X.LANES)
@pytest.mark.parametrize('extra', [0, 1])
def test_align_owner_scan_chunk_edge(dev, lanes, extra):
    """R = 4 nthr fills one scan chunk exactly; R = 4 nthr + 1 leaves one RoI for a second chunk.
    The RoIs next to the chunk edge (and the lone one past it) are piled on one tile."""
    c, nthr, k = X.chunk_edge_case(lanes, extra)
    assert len(c.rois) == 4 * nthr + extra and nthr == (lanes or 256)
    assert k['m'] == ([5, 1] if extra else [5]) and min(k['entries']) > 0
    _bits(_owner_with_lanes(dev, c, lanes), c.gx)


@pytest.mark.parametrize('lanes', X.LANES)
@pytest.mark.parametrize('where', X.WINDOW_EDGES)
def test_align_owner_candidate_window_edge(dev, lanes, where):
    """m RoIs piled on one tile with m * OH * OW (RoI, bin) candidates one short of a window of
    2 nthr, exactly one window, one over, and more than two windows."""
    c, nthr, k = X.window_edge_case(lanes, where)
    want = {'2n-1': 2 * nthr - 1, '2n': 2 * nthr, '2n+1': 2 * nthr + 1, '>4n': 4 * nthr + 4}[where]
    assert nthr == (lanes or 256) and k['candidates'] == [want]
    assert k['windows'] == [-(-want // (2 * nthr))] and k['windows'][0] == {'2n-1': 1, '2n': 1, '2n+1': 2, '>4n': 3}[where]
    _bits(_owner_with_lanes(dev, c, lanes), c.gx)


@pytest.mark.parametrize('N,H,W', X.NARROW)
def test_align_owner_narrow_maps_and_few_tiles(dev, N, H, W):
    """Maps narrower than, equal to and one past an 8-pixel tile; one row; fewer than 8 tiles in
    all (every XCD's run of the tile remap is then one tile long)."""
    assert (N * H * ((W + 7) // 8) < 8) == (H == 1 or W <= 8)
    for sr in (0, 2):
        _run_case_all_ways(dev, X.narrow_case(N, H, W, sr),
                           [('aligned', X.FORM_OWNER), (None, X.FORM_GATHER)])


def test_align_bwd_image_without_rois(dev):
    """The owner form never zero-fills: the tiles of an image no RoI names are written as zeros
    over the NaN pre-fill; the atomic forms zero-fill."""
    c = X.empty_image_case()
    assert not c.gx[1].any()
    _run_case_all_ways(dev, c, [('aligned', X.FORM_OWNER), (None, X.FORM_GATHER)])


@pytest.mark.parametrize('C,gx_off,vec,cv,nthr,chunks', X.CHANNELS)
def test_align_channel_chunks_backward(dev, C, gx_off, vec, cv, nthr, chunks):
    """Scalar kernels (by C, and by a gradient map 4 bytes off although C % 4 == 0) and float4
    kernels, one channel chunk and two with a partial last one."""
    assert X.channel_vectors(C, gx_off == 0) == cv and (C % 4 == 0 and gx_off == 0) == vec
    assert X.owner_threads(C, 0, gx_off == 0) == nthr and -(-cv // nthr) == chunks
    c = X.channel_case(C, gx_off)
    for ws, want in (('aligned', X.FORM_OWNER), (None, X.FORM_GATHER)):
        form, gx = _align_bwd(dev, c.rois, c.gy, (c.N, c.H, c.W, C), 7, 7, 1, 0, ws=ws, off=dict(gx=gx_off))
        assert form == want
        _bits(gx, c.gx)


@pytest.mark.parametrize('C,x_off,vec,cv,nthr,chunks', X.CHANNELS)
def test_align_channel_chunks_forward(dev, C, x_off, vec, cv, nthr, chunks):
    """The forward on the same channel cases: bit equality on an integer map with dyadic RoIs,
    the suite's bound on random data and awkward RoIs; `order` changes nothing."""
    assert X.pick_threads(cv) == nthr and -(-cv // nthr) == chunks
    rng = np.random.RandomState(C + x_off)
    for rois, x, PH, PW, bs, sr, ref in X.channel_fwd_cases(C, x_off):
        _bits(_align_fwd(dev, rois, x, PH, PW, bs, sr, off=dict(x=x_off)), ref)
        _bits(_align_fwd(dev, rois, x, PH, PW, bs, sr, order=rng.permutation(len(rois)),
                         off=dict(x=x_off)), ref)
    N, H, W = 2, 6, 19
    rois = X.awkward_rois(rng, 30, N, H, W, 0.3)
    x = rng.standard_normal((N, H, W, C)).astype(np.float32)
    ref = L.roi_align_fwd(torch.from_numpy(x).double(), torch.from_numpy(rois), 7, 7, 0.3, 0).numpy()
    y = _align_fwd(dev, rois, x, 7, 7, 1, 0, scale=0.3, off=dict(x=x_off))
    L._close(y, ref)
    _bits(_align_fwd(dev, rois, x, 7, 7, 1, 0, scale=0.3, order=rng.permutation(len(rois)),
                     off=dict(x=x_off)), y)


# ---- c. pool-variant owner boundaries ----------------------------------------------------------------
def _pv_close(got, want, rtol=1e-4, atol_of_max=1e-5):
    """tests/test_gpu_pool_variants._close: |got - ref| <= 1e-4 |ref| + 1e-5 max|ref|."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    tol = rtol * np.abs(want) + atol_of_max * max(np.abs(want).max(), 1e-30)
    bad = np.abs(got - want) > tol
    assert not bad.any(), 'max err %g (scale %g), %d elements' % (
        np.abs(got - want).max(), np.abs(want).max(), bad.sum())


def _pv_run(dev, c):
    """One pool-variant case against its reference.  Max pooling: forward values and argmax, then
    the backward, bit for bit.  Crop-and-resize: the backward bit for bit on dyadic output sizes,
    under the pool-variant suite's bound otherwise."""
    if c.kind == 'pool':
        y_ref, am_ref, gx_ref = c.refs
        y, am = _pool_fwd(dev, c.rois, c.x, c.PH, c.PW, c.bin_stride)
        _bits(y, y_ref)
        _bits(am, am_ref)
        _bits(_pool_bwd(dev, c.rois, c.gy, am_ref, c.shape, c.PH, c.PW, c.bin_stride), gx_ref)
        return
    gx_ref, exact = c.refs
    gx = _crop_bwd(dev, c.rois, c.gy, c.shape, c.PH, c.PW, c.bin_stride, c.out_rows)
    if exact:
        _bits(gx, gx_ref)
    else:
        _pv_close(gx, gx_ref)


@pytest.mark.parametrize('kind', ['pool', 'crop'])
@pytest.mark.parametrize('C,R', X.PV_CHUNKS)
def test_pv_owner_scan_chunk_edge(dev, kind, C, R):
    """R = nthr, nthr + 1 and 3 nthr + 5 RoIs (nthr = 64 at C = 8; 256 at C = 1024) on a 2 x 6 x 9
    map: the scan loop runs once, twice with a lone RoI, and four times.  The RoIs on both sides
    of every chunk edge are piled on one tile."""
    c = X.pv_chunk_case(kind, C, R)
    nthr = 64 if C == 8 else 256
    assert len(c.counters['m']) == -(-R // nthr) and min(c.counters['m']) >= 1
    _pv_run(dev, c)


@pytest.mark.parametrize('kind', ['pool', 'crop'])
@pytest.mark.parametrize('bs', [1, 2])
def test_pv_owner_strided_bins_across_chunks(dev, kind, bs):
    """14 x 14 (pooling) and 17 x 17 (crop-and-resize) bins read with stride 1 and 2, two chunks."""
    c = X.pv_stride_case(kind, bs)
    assert len(c.counters['m']) == 2 and min(c.counters['m']) >= 1
    _pv_run(dev, c)


@pytest.mark.parametrize('kind', ['pool', 'crop'])
@pytest.mark.parametrize('k,windows,straddles', X.PV_PILES)
def test_pv_owner_list_windows_exact(dev, kind, k, windows, straddles):
    """k 2 x 2-pixel RoIs onto 17 x 17 bins at one tile's origin: 289 (crop-and-resize) or 153
    (pooling) rectangle entries each.  One window; a rectangle that straddles entry 512; more
    than 1024 entries."""
    c = X.pv_pile_case(kind, k)
    cnt, per = c.counters, (289 if kind == 'crop' else 153)
    assert cnt['ntot'] == [k * per] and cnt['windows'] == [-(-k * per // 512)]
    if kind == 'crop':
        assert cnt['windows'] == [windows] and cnt['straddles'] == [straddles]
        assert (k * per <= 512) == (k == 1) and (512 < k * per <= 1024) == (k in (2, 3))
    else:
        assert (k * per <= 512) == (k <= 3) and (512 < k * per <= 1024) == (k == 4)
        assert (cnt['straddles'][0] >= 1) == (k >= 4)
    assert (k * per > 1024) == (k == 7 or (kind == 'crop' and k == 4))
    _pv_run(dev, c)


@pytest.mark.parametrize('kind', ['pool', 'crop'])
@pytest.mark.parametrize('target', X.PV_FULL)
def test_pv_owner_list_exactly_full_windows(dev, kind, target):
    """A host search over the restated geometry piles RoIs (2- and 16-pixel boxes onto 16 x 16 bins)
    on one tile until its list holds exactly 512 / 513 / 1024 / 1025 entries: a window filled to
    its last entry, and one entry left over for the next window."""
    c = X.pv_full_case(kind, target)
    assert c.counters['ntot'] == [target] and c.counters['windows'] == [-(-target // 512)]
    _pv_run(dev, c)


@pytest.mark.parametrize('R', [65, 133])
def test_crop_resize_output_rows_across_a_chunk_edge(dev, R):
    """out_rows a random permutation (not the identity): the RoI found in one scan chunk reads
    the gy row named by out_rows, wherever it lies; the forward writes that row."""
    c = X.pv_out_rows_case(R)
    assert not np.array_equal(c.out_rows, np.arange(R)) and len(c.counters['m']) == -(-R // 64)
    assert c.counters['m'][0] >= 2 and c.counters['m'][1] >= 1
    _pv_run(dev, c)
    x = X.int_values(np.random.RandomState(R), c.shape)
    y = _crop_fwd(dev, c.rois, x, c.PH, c.PW, 1, c.out_rows)
    _bits(y[c.out_rows], _crop_fwd(dev, c.rois, x, c.PH, c.PW, 1, None))


# ---- d. alignment ------------------------------------------------------------------------------------
def _random_case(rng, N, H, W, C):
    rois = X.awkward_rois(rng, 20, N, H, W, 1.)
    x = rng.standard_normal((N, H, W, C)).astype(np.float32)
    return rois, x


def test_align_misaligned_pointers_take_the_scalar_kernels(dev):
    """C % 4 == 0 with x, y, gy or gx four bytes past a 16-byte boundary: the scalar kernels run and
    give the aligned run's bits (forward, owner backward), which is within the suite's bound of
    float64."""
    rng = np.random.RandomState(5)
    N, H, W, C = 2, 6, 19, 8
    rois, x = _random_case(rng, N, H, W, C)
    for PH, PW, bs, sr in ((7, 7, 1, 0), (14, 14, 2, 2)):
        y0 = _align_fwd(dev, rois, x, PH, PW, bs, sr)
        L._close(y0, L.roi_align_fwd(torch.from_numpy(x).double(), torch.from_numpy(rois), PH, PW, 1.,
                                     sr, bs).numpy())
        for name in ('x', 'y'):
            _bits(_align_fwd(dev, rois, x, PH, PW, bs, sr, off={name: 4}), y0)
        gy = rng.standard_normal(y0.shape).astype(np.float32)
        form, g0 = _align_bwd(dev, rois, gy, (N, H, W, C), PH, PW, bs, sr)
        assert form == X.FORM_OWNER
        ref = L.roi_align_bwd(torch.from_numpy(gy).double(), torch.from_numpy(rois), (N, H, W, C), 1.,
                              sr, bs, PH, PW).numpy()
        L._close(g0, ref)
        for name in ('gy', 'gx'):
            form, g = _align_bwd(dev, rois, gy, (N, H, W, C), PH, PW, bs, sr, off={name: 4})
            assert form == X.FORM_OWNER
            _bits(g, g0)
            form, g = _align_bwd(dev, rois, gy, (N, H, W, C), PH, PW, bs, sr, ws=None, off={name: 4})
            assert form == X.FORM_GATHER
            L._close(g, ref)


def test_pool_misaligned_pointers_take_the_scalar_kernels(dev):
    rng = np.random.RandomState(6)
    N, H, W, C = 2, 6, 19, 8
    rois, x = _random_case(rng, N, H, W, C)
    for PH, PW, bs in ((7, 7, 1), (14, 14, 2)):
        y_ref, am_ref = PV.roi_pooling_2d_fwd(X.nchw(x), rois, PH, PW, 1.)
        y_ref, am_ref = X.nhwc(PV.strided(y_ref, bs)), X.nhwc(PV.strided(am_ref, bs))
        for o in ({}, dict(x=4), dict(y=4), dict(argmax=4)):
            y, am = _pool_fwd(dev, rois, x, PH, PW, bs, off=o)
            _bits(y, y_ref)
            _bits(am, am_ref)
        gy = rng.standard_normal(y_ref.shape).astype(np.float32)
        gx_ref = X.nhwc(PV.roi_pooling_2d_bwd(X.nchw(gy), X.nchw(am_ref), rois, (N, C, H, W)))
        for o in ({}, dict(gy=4), dict(gx=4), dict(argmax=4)):
            _bits(_pool_bwd(dev, rois, gy, am_ref, (N, H, W, C), PH, PW, bs, off=o), gx_ref)


def test_crop_misaligned_pointers_take_the_scalar_kernels(dev):
    rng = np.random.RandomState(7)
    N, H, W, C = 2, 6, 19, 8
    rois, x = _random_case(rng, N, H, W, C)
    rows = PV.output_rows(rois)
    for PH, PW, bs in ((7, 7, 1), (14, 14, 2)):
        y_ref = X.nhwc(PV.strided(PV.crop_and_resize_fwd(X.nchw(x), rois, PH, PW, 1.), bs))
        for o in ({}, dict(x=4), dict(y=4)):
            _bits(_crop_fwd(dev, rois, x, PH, PW, bs, rows, off=o), y_ref)
        gy = rng.standard_normal(y_ref.shape).astype(np.float32)
        g0 = _crop_bwd(dev, rois, gy, (N, H, W, C), PH, PW, bs, rows)
        _pv_close(g0, X.crop_bwd_close_ref(rois, gy, (N, H, W, C), bs, rows))
        for o in (dict(gy=4), dict(gx=4)):
            _bits(_crop_bwd(dev, rois, gy, (N, H, W, C), PH, PW, bs, rows, off=o), g0)


# ---- e. a non-finite gy element in the ROIAlign owner form --------------------------------------------
@pytest.mark.parametrize('C', [8, 6])
def test_owner_nonfinite_gy_stays_in_its_channel_and_tiles(dev, C):
    """What the trainer's non-finite step guard relies on.  One +inf at one (RoI, bin, channel):
    every gx element the bin has a non-zero weight on (where the exact gradient is non-finite) is
    non-finite; every other channel, every other image, every row the bin has no weight on and
    every 8-pixel tile it does not touch equal the finite run bit for bit.  Inside a touched tile a
    pixel with zero weight MAY become NaN: owner_consume applies the bin to all 8 pixels of the
    tile, 0 * inf — such pixels are left unconstrained here."""
    N, H, W, PH, PW = 2, 9, 27, 7, 7
    c = X.nonfinite_case(C)
    assert (c.N, c.H, c.W, c.PH, c.PW) == (N, H, W, PH, PW)
    r, oh, ow, ch = 17, 3, 4, C - 3
    form, g0 = _align_bwd(dev, c.rois, c.gy, (N, H, W, C), PH, PW, 1, 0)
    assert form == X.FORM_OWNER
    _bits(g0, c.gx)
    gy = c.gy.copy()
    gy[r, oh, ow, ch] = np.inf
    form, g1 = _align_bwd(dev, c.rois, gy, (N, H, W, C), PH, PW, 1, 0)
    assert form == X.FORM_OWNER
    batch, Ay, Bx, _ = L.roi_tables(torch.from_numpy(c.rois), H, W, PH, PW, 1., 0, 1)
    n = int(batch[r])
    wy, wx = Ay[r, oh].numpy() != 0, Bx[r, ow].numpy() != 0
    assert wy.sum() == 2 and wx.sum() == 2                      # the bin's one sample, four taps
    support = wy[:, None] & wx[None, :]
    assert not np.isfinite(g1[n, :, :, ch][support]).any()
    same = np.ones((N, H, W, C), bool)
    tiles = np.zeros(W, bool)
    for x0 in range(0, W, X.K_OWN_XT):
        tiles[x0:x0 + X.K_OWN_XT] = wx[x0:x0 + X.K_OWN_XT].any()
    assert 0 < tiles.sum() < W
    same[n, :, :, ch] = ~(wy[:, None] & tiles[None, :])
    assert same.sum() == same.size - 2 * tiles.sum()
    assert np.array_equal(g1[same], g0[same])
    assert np.isfinite(g0).all()
