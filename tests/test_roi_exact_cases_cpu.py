"""Host side of tests/test_gpu_roi_exact.py: every exact configuration is proven exact here (a case
that is not fails on the host, not on the device), the fp32 C oracle — which sums in another order —
equals the float64 reference bit for bit on them, the restated constants equal the kernels', and
``mrcnn_roi_align_bwd_form`` reports each form at its thresholds."""
import numpy as np
import pytest

import oracle

import roi_exact_cases as X


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from chainer_mask_rcnn_amd import _lib
    return _lib.load()


# ---- the restated constants -------------------------------------------------------------------------
def test_restated_constants_equal_the_kernels():
    k = X.source_constants()
    assert (k['kOwnXT'], k['kOwnScan'], k['kOwnThreads']) == (X.K_OWN_XT, X.K_OWN_SCAN, X.K_OWN_THREADS)
    assert (k['kPvXT'], k['kPvCap'], k['kPvThreads']) == (X.K_PV_XT, X.K_PV_CAP, X.K_PV_THREADS)
    align, pv, common = (X.source_text(n) for n in ('roi_align.hip', 'roi_pool_variants.hip', 'roi_common.h'))
    # the loops the counters restate
    assert 'for (int r0 = 0; r0 < R; r0 += kOwnScan * nthr)' in align
    assert 'const int cap = 2 * nthr;' in align and 'for (int w0 = 0; w0 < m * nb; w0 += cap)' in align
    assert 'for (int r0 = 0; r0 < R; r0 += nthr)' in pv
    assert 'for (int win = 0; win < ntot; win += kPvCap)' in pv
    assert 'const int j0 = max(0, win - off), j1 = min(cnt, win + kPvCap - off);' in pv
    # pick_threads
    assert 'int t = ((cv + 63) / 64) * 64;' in common
    assert 'return t > 256 ? 256 : (t < 64 ? 64 : t);' in common
    assert [X.pick_threads(c) for c in (1, 64, 65, 128, 129, 192, 193, 256, 257, 5000)] == \
        [64, 64, 128, 128, 192, 192, 256, 256, 256, 256]
    # the gather form's LDS need
    assert 'sizeof(float) * ((size_t)PH + (size_t)(W + 4) * PW) + sizeof(int) * 2 * (W + 4)' in align
    assert '<= 48 * 1024' in align
    assert (X.gather_lds_bytes(763, 14, 14), X.gather_lds_bytes(764, 14, 14)) == (49144, 49208)
    assert X.own_window(64) == 128 and X.own_window(256) == 512


def test_owner_threads_follow_lanes_channels_and_alignment():
    assert [X.owner_threads(1024, l) for l in X.LANES] == [64, 128, 192, 256]
    assert [X.owner_threads(X.lanes_channels(l), l) for l in X.LANES] == [64, 128, 192, 256]
    for C, off, vec, cv, nthr, chunks in X.CHANNELS:
        assert X.channel_vectors(C, off == 0) == cv and X.owner_threads(C, 0, off == 0) == nthr
        assert -(-cv // nthr) == chunks
    assert X.pv_threads(8) == 64 and X.pv_threads(1024) == 256


# ---- the form query -----------------------------------------------------------------------------------
def test_backward_form_query_at_its_thresholds(lib):
    f = lib.mrcnn_roi_align_bwd_form
    O, G, S = X.FORM_OWNER, X.FORM_GATHER, X.FORM_SCATTER
    # (N, H, W, R, PH, PW, bin_stride, has_ws, ws_aligned)
    assert f(2, 11, 19, 600, 7, 7, 1, 1, 1) == O
    assert f(2, 11, 19, 600, 7, 7, 1, 1, 0) == G          # a workspace that is not 16-byte aligned
    assert f(2, 11, 19, 600, 7, 7, 1, 0, 0) == G
    assert f(2, 11, 19, 600, 7, 7, 1, 0, 1) == G          # alignment of no workspace means nothing
    assert f(2, 11, 19, 0, 7, 7, 1, 1, 1) == G            # no RoIs: zero-fill only
    # LDS of the gather form: 49144 <= 49152 < 49208
    assert f(1, 2, 763, 24, 14, 14, 1, 0, 0) == G and f(1, 2, 764, 24, 14, 14, 1, 0, 0) == S
    assert f(1, 2, 764, 24, 14, 14, 1, 1, 1) == O and f(1, 2, 764, 24, 14, 14, 1, 1, 0) == S
    for PH, PW, bs in X.BINS:                              # bin_stride does not enter: PH, PW size the tables
        W = X.scatter_width(PH, PW)
        assert f(1, 2, W - 1, 40, PH, PW, bs, 0, 0) == G and f(1, 2, W, 40, PH, PW, bs, 0, 0) == S
    # RoIs in grid.y
    assert f(1, 2, 3, 65535, 1, 1, 1, 0, 0) == G and f(1, 2, 3, 65536, 1, 1, 1, 0, 0) == S
    assert f(1, 2, 3, 65536, 1, 1, 1, 1, 1) == O
    # 16-bit extents of the owner tables, rows in grid.x of the gather form
    assert f(1, 65535, 8, 4, 1, 1, 1, 1, 1) == O and f(1, 65536, 8, 4, 1, 1, 1, 1, 1) == S
    assert f(1, 65535, 8, 4, 1, 1, 1, 0, 0) == G and f(1, 65536, 8, 4, 1, 1, 1, 0, 0) == S
    assert f(1, 1, 65536, 4, 1, 1, 1, 1, 1) == S          # W > 65535: no owner, and the tables pass 48 KB
    # bad shapes
    assert f(0, 2, 3, 1, 1, 1, 1, 0, 0) == -1 and f(1, 2, 3, 1, 1, 1, 0, 0, 0) == -1
    assert f(1, 2, 3, -1, 1, 1, 1, 0, 0) == -1


# ---- every committed exact configuration ---------------------------------------------------------------
def _oracle_equals(c):
    """oracle.roi_align_bwd (fp32, C, the reference's scatter order) == the float64 reference."""
    R, OH, OW, C = c.gy.shape
    full = np.zeros((R, c.PH, c.PW, C), np.float32)
    full[:, ::c.bin_stride, ::c.bin_stride] = c.gy
    got = oracle.roi_align_bwd(X.nchw(full), c.rois, (c.N, C, c.H, c.W), 1., c.sampling_ratio)
    assert np.array_equal(X.nhwc(got), c.gx)


@pytest.mark.parametrize('sr', X.SAMPLING)
@pytest.mark.parametrize('PH,PW,bs', X.BINS)
def test_form_cases_are_exact(PH, PW, bs, sr):
    cases = X.form_cases(PH, PW, bs, sr)
    assert [len(c.rois) for c, _ in cases] == [600, 40, 40]
    assert {f for _, ways in cases for _, f in ways} == {0, 1, 2}
    for c, _ in cases:
        assert c.gx.dtype == np.float32 and (c.gy != 0).all() and np.abs(c.gy).max() <= 8
        assert np.array_equal(c.gy, np.rint(c.gy)) and np.array_equal(c.rois, np.rint(c.rois))
        _oracle_equals(c)
    big = cases[0][0]
    assert big.gx[0].any() and big.gx[1].any()
    # RoIs partly off the map on every side
    r = big.rois
    assert (r[:, 1] < 0).any() and (r[:, 2] < 0).any() and (r[:, 3] > big.W).any() and (r[:, 4] > big.H).any()
    assert np.abs(big.gx[big.gx != 0]).min() <= 2. ** -2      # small weights: a lost entry is visible, not rounded away


def test_threshold_cases_are_exact():
    for W in (763, 764):
        _oracle_equals(X.lds_case(W))
    for R in (65535, 65536):
        c = X.roi_count_case(R)
        assert len(c.rois) == R
        _oracle_equals(c)


@pytest.mark.parametrize('lanes', X.LANES)
def test_owner_list_cases_are_exact_and_reach_their_branch(lanes):
    for extra in (0, 1):
        c, nthr, k = X.chunk_edge_case(lanes, extra)
        assert len(c.rois) == X.K_OWN_SCAN * nthr + extra and len(k['m']) == 1 + extra
        _oracle_equals(c)
    seen = []
    for where in X.WINDOW_EDGES:
        c, nthr, k = X.window_edge_case(lanes, where)
        seen.append(k['candidates'][0] - 2 * nthr)
        _oracle_equals(c)
    assert seen == [-1, 0, 1, 2 * nthr + 4]


def test_narrow_channel_and_nonfinite_cases_are_exact():
    for N, H, W in X.NARROW:
        for sr in (0, 2):
            _oracle_equals(X.narrow_case(N, H, W, sr))
    for C, off, *_ in X.CHANNELS:
        _oracle_equals(X.channel_case(C, off))
        for rois, x, PH, PW, bs, sr, ref in X.channel_fwd_cases(C, off):
            got = oracle.roi_align_fwd(X.nchw(x), rois, PH, PW, 1., sr)
            assert np.array_equal(X.nhwc(got)[:, ::bs, ::bs], ref)
    for C in (8, 6):
        _oracle_equals(X.nonfinite_case(C))


def test_one_image_without_rois():
    c = X.empty_image_case()
    assert not (c.rois[:, 0] == 1).any() and not c.gx[1].any()
    _oracle_equals(c)


def test_an_inexact_case_fails_on_the_host():
    rng = np.random.RandomState(0)
    rois = X.align_rois(rng, 20, 2, 11, 19, 7, 7, 0)
    gy = X.int_values(rng, (20, 7, 7, 4))
    X.align_bwd_ref(rois, gy, (2, 11, 19, 4), 7, 7, 1, 0)
    bad = rois.copy()
    bad[3, 3] += 1                           # a side of 7 g + 1: bins of (7 g + 1) / 7 pixels
    with pytest.raises(AssertionError):
        X.align_bwd_ref(bad, gy, (2, 11, 19, 4), 7, 7, 1, 0)
    with pytest.raises(AssertionError):      # exact values, but partial sums may pass 24 bits
        X.align_bwd_ref(rois, gy * np.float32(2. ** 20), (2, 11, 19, 4), 7, 7, 1, 0)
    crop = X.crop_rois(rng, 10, 2, 6, 9)
    g = X.int_values(rng, (10, 7, 7, 4))
    with pytest.raises(AssertionError):      # 7 outputs: steps of 1/6
        X.crop_bwd_ref(crop, g, (2, 6, 9, 4))
    X.crop_bwd_ref(crop, X.int_values(rng, (10, 9, 5, 4)), (2, 6, 9, 4))


# ---- pool variants -------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['pool', 'crop'])
def test_pool_variant_cases_reach_their_branches(kind):
    for C, R in X.PV_CHUNKS:
        c = X.pv_chunk_case(kind, C, R)
        assert len(c.rois) == R and len(c.counters['m']) == -(-R // X.pv_threads(C))
    for bs in (1, 2):
        X.pv_stride_case(kind, bs)
    for k, windows, straddles in X.PV_PILES:
        c = X.pv_pile_case(kind, k)
        if kind == 'crop':
            assert (c.counters['windows'], c.counters['straddles']) == ([windows], [straddles])
            assert c.refs[1] is True
    tot = [X.pv_pile_case(kind, k).counters['ntot'][0] for k, _, _ in X.PV_PILES]
    assert min(tot) <= 512 and any(512 < t <= 1024 for t in tot) and max(tot) > 1024
    assert any(X.pv_pile_case(kind, k).counters['straddles'][0] for k, _, _ in X.PV_PILES)
    for target in X.PV_FULL:
        c = X.pv_full_case(kind, target)
        assert c.counters['ntot'] == [target]
    if kind == 'crop':
        for R in (65, 133):
            c = X.pv_out_rows_case(R)
            assert sorted(c.out_rows.tolist()) == list(range(R))


def test_counters_on_hand_counted_tiles():
    """The counters against tiles counted by hand."""
    # ROIAlign, 2 x 2 bins of one pixel at (x, y) = (8, 3): samples at 8.5 / 9.5, rows 3.5 / 4.5
    rois = np.array([[0, 8, 3, 10, 5]], np.float32)
    k = X.align_counters(rois, 8, 24, 2, 2, 1, 0, (0, 3, 8), 64)
    assert k == dict(m=[1], windows=[1], entries=[2], candidates=[4])      # row 3: bin row 0 only
    k = X.align_counters(rois, 8, 24, 2, 2, 1, 0, (0, 4, 8), 64)
    assert k['entries'] == [4]                                             # row 4: both bin rows
    assert X.align_counters(rois, 8, 24, 2, 2, 1, 0, (0, 3, 16), 64)['entries'] == [0]
    assert X.align_counters(rois, 8, 24, 2, 2, 1, 0, (1, 3, 8), 64)['m'] == [0]
    # 300 copies: two scan chunks of 256 RoIs at 64 lanes, 1200 candidates
    k = X.align_counters(np.tile(rois, (300, 1)), 8, 24, 2, 2, 1, 0, (0, 4, 8), 64)
    assert k['m'] == [256, 44] and k['windows'] == [8, 2] and k['entries'] == [1024, 176]
    # max pooling: a 4 x 4 box at (2, 1) onto 2 x 2 bins: windows [1, 3) [3, 5) x [2, 4) [4, 6)
    box = np.array([[0, 2, 1, 5, 4]], np.float32)
    assert X.pv_counters('pool', box, 1, 8, 16, 2, 2, 1, (0, 1, 0), 64)['ntot'] == [2]
    assert X.pv_counters('pool', box, 1, 8, 16, 2, 2, 1, (0, 1, 8), 64)['m'] == [0]
    assert X.pv_counters('pool', box, 1, 8, 16, 2, 2, 1, (0, 5, 0), 64)['m'] == [0]
    # crop-and-resize: a 2 x 2 crop onto 5 x 5 outputs: every bin taps rows 1, 2 and columns 2, 3
    crop = np.array([[0, 2, 1, 4, 3]], np.float32)
    assert X.pv_counters('crop', crop, 1, 8, 16, 5, 5, 1, (0, 1, 0), 64)['ntot'] == [25]
    k = X.pv_counters('crop', np.tile(crop, (70, 1)), 1, 8, 16, 5, 5, 1, (0, 2, 0), 64)
    assert k == dict(m=[64, 6], ntot=[1600, 150], windows=[4, 1], straddles=[3, 0])


@pytest.mark.parametrize('kind', ['pool', 'crop'])
def test_window_edge_entries_of_the_piled_cases_carry_weight(kind):
    """The entries on either side of a kPvCap window edge matter: removing the gy element of list
    entry 511, 512, 1023 or 1024 (where the list has one) changes the reference on the tile, so a
    kernel that lost exactly that entry fails the GPU test.  One exception by construction: bin row
    0 of a crop puts all its weight on the crop's first row, so the first entry of a crop's rectangle
    has weight 0 on PILE_TILE's row (entry 512 of the 1024-entry list)."""
    cases = [X.pv_full_case(kind, t) for t in X.PV_FULL] + [X.pv_pile_case(kind, k) for k in (4, 7)]
    checked, skipped = 0, []
    for c in cases:
        N, H, W, C = c.shape
        n, y, x0 = X.PILE_TILE
        ent = X.pv_entries(kind, c.rois, N, H, W, c.PH, c.PW, c.bin_stride, X.PILE_TILE, 64)
        assert len(ent) == c.counters['ntot'][0]

        def ref(gy):
            if kind == 'pool':
                return X.nhwc(X.PV.roi_pooling_2d_bwd(X.nchw(gy), X.nchw(c.refs[1]), c.rois, (N, C, H, W)))
            return X.crop_bwd_close_ref(c.rois, gy, c.shape, c.bin_stride)

        whole = ref(c.gy)[n, y, x0:x0 + X.K_PV_XT]
        for e in (511, 512, 1023, 1024):
            if e >= len(ent):
                continue
            r, oh, ow = ent[e]
            if kind == 'crop' and oh == 0:
                skipped.append((len(ent), e))
                continue
            gy = c.gy.copy()
            gy[r, oh, ow, :] = 0
            assert not np.array_equal(ref(gy)[n, y, x0:x0 + X.K_PV_XT], whole), (len(ent), e, ent[e])
            checked += 1
    assert checked >= 14 and skipped == ([(1024, 512)] if kind == 'crop' else [])
