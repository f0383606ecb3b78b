"""The case lists and the policy restatement of tests/gemm_edge_cases.py, without a device:
coverage of the launch policy's branches and of the kernel instantiations, the float64 references
of tests/launch_ref.py at the degenerate geometries of the lists, the comparison of
tests/test_gpu_gemm_edges.py on emulated kernels (right, and wrong the way each edge goes wrong),
the size caps, and the library's own launch plan (mrcnn_conv_gemm_plan: no device touched) against
route() on every listed call and on a dense sweep of shapes.  The same for the Winograd route's own
policy (plan_wino_gemm / plan_wino_wgrad), whose plans are compared as whole lines, and a float64 model
of that route (oracle/np_winograd.py) damaged the way its launches, fix-up and transforms can go wrong."""
import collections
import contextlib
import ctypes
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import gemm_edge_cases as G
import launch_ref as L
from oracle import np_ref

F64 = torch.float64


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))


def _calls():
    return list(G.all_calls())


# ---- coverage -----------------------------------------------------------------------------------

# label -> why no accepted shape reaches it in that mode (none so far: every label is reached)
UNREACHABLE_FWD = {}
UNREACHABLE_DGRAD = {}


def test_every_policy_label_is_reached():
    seen = collections.defaultdict(set)
    for fam, i, entry, d, ws, kn in _calls():
        r = G.route(entry, d, 0, ws, kn)
        p = None if 'wgrad' in entry else G.gemm_problem(entry, d, ws, dict(G.DEFAULT_KNOBS, **kn))
        mode = 'wgrad' if p is None else p.mode
        arith = 'fp32' if kn.get('split_bf16', 3) == 0 else 'split'
        seen[(mode, arith)].add(r.label)
        assert r.label != 'w8', i                  # out of scope, and never by accident
        assert sum(r.record.values()) == len(r.launches) >= 1
    assert seen[(G.FWD, 'split')] | set(UNREACHABLE_FWD) == set(G.FWD_LABELS)
    assert seen[(G.FWD, 'fp32')] | set(UNREACHABLE_FWD) == set(G.FWD_LABELS)
    assert seen[(G.DGRAD, 'split')] | set(UNREACHABLE_DGRAD) == set(G.FWD_LABELS)
    assert seen[('wgrad', 'split')] >= set(G.WGRAD_LABELS)
    assert seen[('wgrad', 'split')] - set(G.WGRAD_LABELS) <= set(G.OTHER_LABELS)


def test_every_instantiation_appears():
    tags = collections.Counter()
    per_mode = collections.defaultdict(set)
    for fam, i, entry, d, ws, kn in _calls():
        for kind, t in G.route(entry, d, 0, ws, kn).launches:
            tags.update(t)
            per_mode[t[0]].add(t[1:])
    for want in ('PW', 'K3', 'general', 'perm', 'stem', G.OUT_STRIDED, G.OUT_DECONV, 'WPERM', 'split', 'fp32',
                 '64x64', '128x128'):
        assert tags[want] > 0, want
    # both tile sizes of the three modes; the strided scatter and the pixel shuffle in both forms
    for mode in (G.FWD, G.DGRAD, G.WGRAD):
        assert {t[0] for t in per_mode[mode]} == {'64x64', '128x128'}, mode
    for out in (G.OUT_STRIDED, G.OUT_DECONV):
        assert any(t[1] == out for t in per_mode[G.FWD]) and any(t[1] == out for t in per_mode[G.DGRAD]), out
    # PW and K3 on both tile sizes, the position-major order on the general instantiation only
    for inst in ('PW', 'K3'):
        assert {t[0] for t in per_mode[G.FWD] if inst in t} == {'64x64', '128x128'}, inst


def test_expected_labels_of_the_lists():
    for i, d, kn, label in G.WGRAD_WPERM:
        assert G.route('conv2d_wgrad_ex', d, 0, True, kn).label == label, i
    for i, entry, d, kn, label in G.policy_cases():
        assert G.route(entry, d, 0, True, kn).label == label, i
        rows, cols = d.W, (d.K if entry == 'conv2d_fwd' else d.C)
        assert cols % 64 == 4 and rows % 64 != 0 and rows % 128 != 0, i       # ragged in both
    assert G.route('conv2d_dgrad_ex', G.DGRAD_TINY_SPLIT[1]).label == 'small/tiny_split'
    assert G.route('conv2d_dgrad', G.DGRAD_TINY_SPLIT[1], 0, False).label == 'small/plain'
    for i, (R, Cin, Cout) in G.LINEAR:
        if R == 1 and Cin == 2048:
            assert G.route('conv2d_fwd', G.desc(R, Cin, 1, 1, Cout)).label == 'small/tiny_split', i
    # the thresholds of choose_perm: 63 / 64 images, 256 / 272 positions, the knob
    on = dict(G.DEFAULT_KNOBS)
    assert G.choose_perm(63, 7, 7, 3, 3, 1, 1, on) == 0 and G.choose_perm(64, 7, 7, 3, 3, 1, 1, on) == 64
    assert G.choose_perm(64, 16, 16, 3, 3, 1, 1, on) == 64 and G.choose_perm(64, 16, 17, 3, 3, 1, 1, on) == 0
    assert G.choose_perm(64, 7, 7, 3, 3, 1, 0, on) == 0 and G.choose_perm(64, 7, 7, 1, 1, 1, 1, on) == 0
    assert G.choose_perm(64, 7, 7, 3, 3, 1, 1, dict(on, position_major_rows=0)) == 0
    perm = [G.gemm_problem('conv2d_fwd', d, True, on) for _, d in G.PERM_POSITIONS]
    assert perm[0].perm_n == 64 and perm[0].M == 128 * 256 and perm[1].perm_n == 0
    # 129 images: two blocks of kPermBlock, 127 padding rows per position in the last
    p = G.gemm_problem('conv2d_fwd', G.desc(129, 4, 2, 2, 4, 3, 3, 1, 1), True, on)
    assert p.perm_n == 129 and p.M == 256 * 4


def test_policy_cases_are_the_smallest_that_reach_their_label():
    """One tile row fewer (rows - 64, still ragged) at the same columns and depth takes another branch."""
    for i, entry, d, kn, label in G.policy_cases():
        if d.W <= 64:
            continue
        fewer = d._replace(W=d.W - 64)
        assert G.route(entry, fewer, 0, True, kn).label != label, i


def test_fit_ws_clamp_is_unreachable_at_the_default_knobs():
    """The arithmetic of the comment above gemm_edge_cases.fit_ws, at its worst cases."""
    ws = G.SPLIT_WS_BYTES
    assert 512 * 128 * 128 * 4 <= ws                    # one-round rule: T fit <= 512
    assert 383 * 128 * 128 * 8 * 4 <= ws                # big_split_k > 0 under big_min_tiles = 384
    assert 128 * 64 * 64 * 16 * 4 <= ws                 # tiny split
    assert 154 * 64 * 64 * 16 * 4 <= ws                 # 64x64 fused tail
    assert 1024 * 128 * 128 * 4 <= ws                   # 128x128 fused tail: tiles x slabs < 1024
    for fam, i, entry, d, ws_, kn in _calls():
        if 'wgrad' in entry:
            continue
        p = G.gemm_problem(entry, d, ws_, dict(G.DEFAULT_KNOBS, **kn))
        assert G.fit_ws(16, p.M, p.N) == 16 or p.M * p.N * 4 > (ws >> 4), i


# ---- size caps ------------------------------------------------------------------------------------

def test_size_caps():
    over = set()
    for fam, i, entry, d, ws, kn in _calls():
        b = G.moved_bytes(entry, d)
        assert b <= 256 << 20, i
        if b > 16 << 20:
            assert fam == 'policy', i
            over.add(i)
    by_id = {i: label for i, _, _, _, label in G.policy_cases()}
    for i in over:
        assert by_id[i] in G.POLICY_SIZE_REASON and 'size forced by ' + by_id[i] in i, i
    for N, C, H, W, K in G.WINOGRAD:
        assert 4 * N * H * W * (C + K) <= 16 << 20


def test_operands_have_no_zeros_and_no_repeats():
    for d in (G.pw_desc(129, 132, 100), G.desc(65, 36, 2, 2, 40, 3, 3, 1, 1), G.desc(1, 4, 1, 1, 4)):
        x, w, gy = G.operands(d)
        for a in (x.transpose(0, 2, 3, 1).reshape(-1, d.C), w.reshape(d.K, -1), gy.transpose(0, 2, 3, 1).reshape(-1, d.K)):
            assert np.all(a != 0)
            assert len(np.unique(a, axis=0)) == a.shape[0] and len(np.unique(a.T, axis=0)) == a.shape[1]
        x2, _, _ = G.operands(d)
        assert np.array_equal(x, x2)                 # seeded


# ---- the references at the degenerate geometries ---------------------------------------------------

def _close64(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    assert np.abs(a - b).max() <= 1e-12 * max(1., np.abs(b).max())


def _geometries():
    out = []
    for what, R, S, pad, H, W in G.SMALL_MAP_GEOMS:
        out += [G.desc(N, 4, H, W, 8, R, S, 1, pad) for N in (1, 3)]
    out += [d._replace(C=4, K=8) for _, d in G.STRIDED if d.N == 1]
    out += [G.desc(1, 4, 1, 1, 4), G.desc(1, 8, 1, 5, 4)]                  # one pixel, one image / one row
    out += [G.desc(N, 3, H, W, 4, 7, 7, 2, 3) for _, (N, H, W, K, aff) in G.STEM[::4]]    # the stem's geometry
    return out


@pytest.mark.parametrize('d', _geometries(), ids=lambda d: 'N%d %dx%d R%dS%d s%d p%d' % (
    d.N, d.H, d.W, d.R, d.S, d.stride, d.pad))
def test_conv_references_at_degenerate_geometries(d):
    """launch_ref.conv_fwd / conv_dgrad / conv_wgrad against the NumPy oracle (square filters) and
    torch.nn.functional in float64 (every filter) where H < R, on odd and 1x1 maps under stride 2, for
    a non-square filter, one pixel, one image."""
    x, w, gy = (a.astype(np.float64) for a in G.operands(d))
    y = L.conv_fwd(_t(x), _t(w), d.stride, d.pad)
    gx = L.conv_dgrad(_t(gy), _t(w), d.H, d.W, d.stride, d.pad)
    gw = L.conv_wgrad(_t(x), _t(gy), d.R, d.S, d.stride, d.pad)
    assert tuple(y.shape) == (d.N, d.K, d.P, d.Q)
    xt, wt = _t(x).requires_grad_(True), _t(w).requires_grad_(True)
    yt = TF.conv2d(xt, wt, None, d.stride, d.pad)
    yt.backward(_t(gy))
    _close64(y, yt.detach())
    _close64(gx, xt.grad)
    _close64(gw, wt.grad)
    if d.R == d.S:
        _close64(y, np_ref.conv2d_fwd(x, w, None, d.stride, d.pad))
        ogx, ogw, _ = np_ref.conv2d_bwd(x, w, gy, d.stride, d.pad)
        _close64(gx, ogx)
        _close64(gw, ogw)


def test_stem_reference_through_the_packed_layout():
    """The stem reference of the checker reads x4 (N,H,W,4) and w784 (K,7,8,4): the same slicing on the
    tiny images, against the oracle."""
    for i, (N, H, W, K, aff) in G.STEM[::2]:
        rng = np.random.RandomState(G.seed_of(N, H, W, K))
        x = rng.standard_normal((N, 3, H, W))
        w = rng.standard_normal((K, 3, 7, 7)) / 12.
        b, sc, sh = rng.standard_normal(K), rng.uniform(.5, 1.5, K), rng.standard_normal(K)
        x4 = np.zeros((N, H, W, 4))
        x4[..., :3] = x.transpose(0, 2, 3, 1)
        w784 = np.zeros((K, 7, 8, 4))
        w784[:, :, :7, :3] = w.transpose(0, 2, 3, 1)
        X = _t(x4)[..., :3].permute(0, 3, 1, 2)
        Wt = _t(w784)[:, :, :7, :3].permute(0, 3, 1, 2)
        flags = L.EPI_RELU | L.EPI_BIAS | (L.EPI_AFFINE if aff else 0)
        got = L.fwd_epilogue(L.conv_fwd(X, Wt, 2, 3), flags, _t(b), _t(sc), _t(sh))
        ref = np_ref.conv2d_fwd(x, w, b, 2, 3)
        if aff:
            ref = np_ref.affine_channel_2d_fwd(ref, sc, sh)
        _close64(got, np.maximum(ref, 0))


def test_deconv_references_at_the_list_shapes():
    for i, d in G.DECONV:
        if d.C == 64:
            continue
        rng = np.random.RandomState(G.seed_of(*d))
        x = rng.standard_normal((d.N, d.C, d.H, d.W))
        w = rng.standard_normal((d.C, d.K, 2, 2)) / np.sqrt(d.C)
        gy = rng.standard_normal((d.N, d.K, 2 * d.H, 2 * d.W))
        xt, wt = _t(x).requires_grad_(True), _t(w).requires_grad_(True)
        yt = TF.conv_transpose2d(xt, wt, None, 2)
        yt.backward(_t(gy))
        y, gx, gw = L.deconv_fwd(_t(x), _t(w)), L.deconv_dgrad(_t(gy), _t(w)), L.deconv_wgrad(_t(x), _t(gy))
        _close64(y, yt.detach())
        _close64(gx, xt.grad)
        _close64(gw, wt.grad)
        # the oracle rounds its deconvolution results to fp32: 2^-24 relative
        ogx, ogw, _ = np_ref.deconv2x2s2_bwd(x, w, gy)
        for got, ref in ((y, np_ref.deconv2x2s2_fwd(x, w, None)), (gx, ogx), (gw, ogw)):
            assert got.shape == ref.shape
            assert np.all(np.abs(got.numpy() - ref) <= 2. ** -23 * np.abs(got.numpy()) + 1e-30), i


@pytest.mark.parametrize('variant', G.DGRAD_VARIANTS)
def test_dgrad_epilogue_reference_on_one_pixel_and_tiny_maps(variant):
    for d in (G.desc(1, 4, 1, 1, 4), G.desc(3, 36, 2, 2, 40, 3, 3, 1, 1)):
        rng = np.random.RandomState(3)
        acc = rng.standard_normal((d.N, d.C, d.H, d.W))
        flags, rg, ry, mk, sc, prev = G.dgrad_flags_operands(variant, d, rng)
        ref = acc * (1. if sc is None else sc.astype(np.float64)[None, :, None, None])
        if rg is not None:
            ref = ref + (rg if ry is None else rg * (ry > 0))
        if prev is not None:
            ref = ref + prev
        if mk is not None:
            ref = ref * (mk > 0)
        got = L.dgrad_epilogue(_t(acc), flags, *(None if a is None else _t(a) for a in (prev, rg, ry, mk, sc)))
        _close64(got, ref)
        assert (variant in ('accum', 'all')) == bool(flags & L.EPI_ACCUM)


# ---- the detector catches what it is for ---------------------------------------------------------

def _f32(t):
    """What a correct fp32 kernel may return: the float64 result rounded to fp32."""
    return t.to(torch.float32)


def _accepts(got, ref):
    return L.ratio(got, ref) <= 1.


def _gemm(d):
    """(x rows (M, Kc), w (N, Kc)) float64 of a 1x1 problem and its product."""
    x, w, _ = G.operands(d)
    X = _t(x)[0, :, 0, :].t().contiguous()
    Wm = _t(w)[:, :, 0, 0]
    return X, Wm, X @ Wm.t()


RAGGED = [G.pw_desc(*c) for c in ((65, 68, 36), (129, 132, 100), (1, 4, 4), (63, 60, 28), (200, 132, 100))]


@pytest.mark.parametrize('d', RAGGED, ids=lambda d: G.pw_id(d.W, d.K, d.C))
def test_detector_ragged_k_rows_and_columns(d):
    X, Wm, ref = _gemm(d)
    assert _accepts(_f32(ref), ref)
    if d.C % 32:
        assert not _accepts(_f32(X[:, :-1] @ Wm[:, :-1].t()), ref), 'last K element dropped'
    for what, bad in (('last row dropped', lambda y: y[-1].zero_()),
                      ('last column dropped', lambda y: y[:, -1].zero_()),
                      ('last row taken from its neighbour', lambda y: y[-1].copy_(y[-2] if len(y) > 1 else -y[-1])),
                      ('last column taken from its neighbour', lambda y: y[:, -1].copy_(y[:, -2]))):
        y = _f32(ref).clone()
        bad(y)
        assert not _accepts(y, ref), what


@pytest.mark.parametrize('geom', G.SMALL_MAP_GEOMS[:6], ids=lambda g: g[0])
def test_detector_padding_tap_wrapped(geom):
    what, R, S, pad, H, W = geom
    d = G.desc(3, 4, H, W, 8, R, S, 1, pad)
    x, w, _ = G.operands(d)
    ref = L.conv_fwd(_t(x), _t(w), 1, pad)
    assert _accepts(_f32(ref), ref)
    wrapped = TF.conv2d(TF.pad(_t(x), (pad,) * 4, mode='circular'), _t(w))
    assert not _accepts(_f32(wrapped), ref), 'padding taps read the opposite border'


def test_detector_skipped_k_split_slab():
    cases = [(e, d) for _, e, d, kn, label in G.policy_cases() if label == 'small/tiny_split'] + \
        [('conv2d_dgrad_ex', G.DGRAD_TINY_SPLIT[1])]
    for entry, d in cases:
        depth = d.C if entry == 'conv2d_fwd' else d.K
        rng = np.random.RandomState(5)
        A = _t(rng.standard_normal((d.W, depth)))
        B = _t(rng.standard_normal((68, depth)) / np.sqrt(depth))
        ref = A @ B.t()
        assert _accepts(_f32(ref), ref)
        slices = G.ceil_div(depth, G.BK)
        splits = min(16, slices // 8, 512)
        slab = G.ceil_div(slices, splits) * G.BK
        for s in (0, splits - 1):
            keep = torch.ones(depth, dtype=F64)
            keep[s * slab:(s + 1) * slab] = 0
            assert not _accepts(_f32((A * keep) @ B.t()), ref), 'slab %d of %d skipped' % (s, splits)


def test_detector_deconv_column_groups_shifted():
    for i, d in G.DECONV:
        if (4 * d.K) % 64 == 0 or d.C == 64:
            continue
        rng = np.random.RandomState(G.seed_of(*d))
        x = _t(rng.standard_normal((d.N, d.C, d.H, d.W)))
        w = _t(rng.standard_normal((d.C, d.K, 2, 2)) / np.sqrt(d.C))
        ref = L.deconv_fwd(x, w)
        assert _accepts(_f32(ref), ref), i
        # columns are (a, b, o): the map shifted by one group sends group (a, b) to the next output pixel
        shifted = L.deconv_fwd(x, w.reshape(d.C, d.K, 4).roll(1, 2).reshape(d.C, d.K, 2, 2))
        assert not _accepts(_f32(shifted), ref), i


def test_detector_guard_bands_and_prefill():
    d = G.desc(129, 4, 2, 2, 8, 3, 3, 1, 1)
    x, w, _ = G.operands(d)
    ref = L.conv_fwd(_t(x), _t(w), 1, 1).permute(0, 2, 3, 1).contiguous()          # NHWC, as the kernels write
    n = ref.numel()

    def fresh():
        g = G.Guarded(n, 'cpu')
        g.out.copy_(_f32(ref).reshape(-1))
        return g

    g = fresh()
    assert g.check() is None and _accepts(g.out.view(ref.shape), ref)
    # a padding row of the last kPermBlock block (image 129 of 256) written: it lands behind the output
    g = fresh()
    g.buf[G.GUARD + n:G.GUARD + n + d.K] = 0
    assert 'guard' in g.check()
    # one element written past the end / before the start
    for at in (G.GUARD + n, G.GUARD - 1, n + 2 * G.GUARD - 1):
        g = fresh()
        g.buf[at] = 0x3f800000
        assert 'guard' in g.check()
    # one output element left unwritten: the NaN prefill stays, ratio() is inf and check() names it
    g = fresh()
    g.buf[G.GUARD + n // 2] = G.NAN_BITS
    assert 'never written' in g.check() and not _accepts(g.out.view(ref.shape), ref)
    # ... unless the operation defines no value there
    defined = torch.ones(n, dtype=torch.bool)
    defined[n // 2] = False
    assert g.check(defined) is None
    # the prefill is a NaN with a payload no kernel produces
    assert torch.isnan(G.Guarded(4, 'cpu').out).all()


def test_detector_strided_scatter_needs_exact_zeros():
    """OUT_STRIDED without ACCUM: the positions between the strided pixels are exact zeros; a stale
    value below the bound's floor still fails the exact check the device test makes."""
    d = G.desc(1, 4, 5, 4, 8, 1, 1, 2, 0)
    x, w, gy = G.operands(d)
    ref = L.conv_dgrad(_t(gy), _t(w), d.H, d.W, 2, 0)
    between = torch.ones_like(ref, dtype=torch.bool)
    between[:, :, ::2, ::2] = False
    assert bool((ref[between] == 0).all())
    got = _f32(ref)
    assert _accepts(got, ref) and bool((got[between] == 0).all())
    got[0, 0, 1, 1] = 1e-7 * float(ref.abs().max())
    assert _accepts(got, ref) and not bool((got[between] == 0).all())


# ---- the library's launch plan (csrc/conv_gemm_plan.h) against route() -----------------------------
# mrcnn_conv_gemm_plan prints what an entry point would launch for a descriptor under the knobs set, and
# touches no device: label and instantiations are compared with route(), and every plan is checked for
# what a launch count cannot show: row ranges, grids, slab depths and the workspace.

Plan = collections.namedtuple('Plan', 'label mode M N k launches sum')
PlanLaunch = collections.namedtuple('PlanLaunch', 'kind tags rows grid slab tail')


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from chainer_mask_rcnn_amd import _lib
    return _lib.load()


@contextlib.contextmanager
def _knobs(kn):
    from chainer_mask_rcnn_amd import _lib
    try:
        for k, v in kn.items():
            _lib.set_tuning(k, v)
        yield
    finally:
        for k, v in G.DEFAULT_KNOBS.items():
            _lib.set_tuning(k, v)


def _plan_line(lib, entry, d, has_ws, size=1024):
    from chainer_mask_rcnn_amd._lib import ConvDesc
    buf = ctypes.create_string_buffer(size)
    cd = ConvDesc(d.N, d.H, d.W, d.C, d.K, d.R, d.S, d.stride, d.pad, d.P, d.Q)
    rc = lib.mrcnn_conv_gemm_plan(entry.encode(), ctypes.byref(cd), int(has_ws), buf, size)
    return rc, buf.value.decode()


def _ints(text, sep):
    return tuple(int(v) for v in text.split(sep))


def _plan(lib, entry, d, has_ws):
    rc, line = _plan_line(lib, entry, d, has_ws)
    assert rc == 0, (entry, d, lib.mrcnn_last_error())
    parts = [dict(f.split('=', 1) for f in part.split() if '=' in f) for part in line.split(' | ')]
    head, rest = parts[0], parts[1:]
    total = None
    if rest and 'slabs' in rest[-1]:
        total = (int(rest[-1]['row0']), int(rest[-1]['slabs']))
        rest = rest[:-1]
    launches = [PlanLaunch(f['kind'], tuple(f['tags'].split(',')), _ints(f['rows'], ':'), _ints(f['grid'], 'x'),
                           int(f['slab']), _ints(f['tail'], ',')) for f in rest]
    return Plan(head['label'], head['mode'], int(head['M']), int(head['N']), int(head['k']), launches, total)


def _check_consistent(p, what):
    """Row ranges tile [0, M); grid.x is the tile count of the range (plus the pieces of a fused tail);
    slabs x slab depth cover the K extent with a non-empty last slab; the slabs fit their workspace."""
    at, summed = 0, None
    assert 1 <= len(p.launches) <= 2, what
    for l in p.launches:
        lo, hi = l.rows
        assert lo == at and hi > lo, (what, l)
        at = hi
        bm, bn = (256, 128) if l.tags[1] == '256x128' else (int(l.tags[1].split('x')[0]),) * 2
        tn = G.ceil_div(p.N, bn)
        first, row0, pieces, depth = l.tail
        if pieces:
            assert lo < row0 < hi and (row0 - lo) % bm == 0 and first == (row0 - lo) // bm * tn, (what, l)
            assert l.grid == (first + G.ceil_div(hi - row0, bm) * tn * pieces, 1) and l.slab == 0, (what, l)
            assert pieces >= 2 and (pieces - 1) * depth < p.k <= pieces * depth, (what, l)
            assert pieces * (hi - row0) * p.N * 4 <= G.SPLIT_WS_BYTES, (what, l)
            summed = (row0, pieces)
        else:
            assert l.grid[0] == G.ceil_div(hi - lo, bm) * tn and l.tail == (0, 0, 0, 0), (what, l)
        if l.slab:
            assert (l.grid[1] - 1) * l.slab < p.k <= l.grid[1] * l.slab, (what, l)
            if p.mode == G.WGRAD:
                # the workspace of mrcnn_conv2d_wgrad_workspace_bytes holds 64 slabs of the whole gradient
                assert l.grid[1] <= 64 and l.slab % G.BK == 0, (what, l)
                summed = (0, l.grid[1]) if l.grid[1] > 1 else None
            else:
                assert l.grid[1] * (hi - lo) * p.N * 4 <= G.SPLIT_WS_BYTES, (what, l)
                summed = (lo, l.grid[1])
        else:
            assert l.grid[1] == 1, (what, l)
    assert at == p.M and p.sum == summed, (what, p)


def _check_against_route(lib, entry, d, has_ws, kn, what):
    r = G.route(entry, d, 0, has_ws, kn)
    p = _plan(lib, entry, d, has_ws)
    assert (p.label, [(l.kind, l.tags) for l in p.launches]) == (r.label, r.launches), (what, p, r)
    _check_consistent(p, what)
    return p.label


def test_plan_equals_route_on_every_listed_call(lib):
    for fam, i, entry, d, ws, kn in _calls():
        with _knobs(kn):
            _check_against_route(lib, entry, d, ws, kn, i)
    for i, entry, d, kn, label in G.policy_cases():
        with _knobs(kn):
            assert _check_against_route(lib, entry, d, True, kn, i) == label, i


def test_plan_rejects_what_the_entry_points_reject(lib):
    """The two '+res_g' entries name a call with a residual gradient, which the strided forms refuse."""
    for i, entry, d in G.REJECTED:
        rc, _ = _plan_line(lib, entry, d, True)
        assert rc != 0 and lib.mrcnn_last_error(), i
    ok = G.desc(2, 8, 3, 3, 8, 3, 3, 1, 1)
    for entry in G.ENTRIES:
        assert _plan_line(lib, entry, ok if 'deconv' not in entry else G.DECONV[0][1], True)[0] == 0, entry
    rc, _ = _plan_line(lib, 'conv2d_bwd', ok, True)
    assert rc != 0 and b'unknown entry' in lib.mrcnn_last_error()
    rc, _ = _plan_line(lib, 'conv2d_fwd+res_g', ok, True)
    assert rc != 0 and b'unknown entry' in lib.mrcnn_last_error()
    rc, _ = _plan_line(lib, 'conv2d_fwd', ok, True, size=40)
    assert rc != 0 and b'buffer' in lib.mrcnn_last_error()


# rows 64 k + 1 and 64 k: the policy reads the row count through its tile counts and through M % 256
SWEEP_K = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 134, 135, 153, 154, 255, 256,
           257, 383, 384, 385, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025, 1093)
SWEEP_ENTRIES = ('conv2d_fwd', 'conv2d_dgrad_ex', 'conv2d_dgrad_wt', 'conv2d_wgrad_ex')
# full-size shapes the comments of conv_gemm_plan.h name: the batch-2 res4 3x3 layer and the 1x1 behind it,
# the head's fused cls_loc / score layer (1024 x 408 x 2048), a 50 176-row 1x1 layer of the RoI head (W8)
FULL_SIZE = (G.desc(2, 256, 51, 84, 256, 3, 3, 1, 1), G.desc(2, 1024, 51, 84, 256), G.desc(1024, 2048, 1, 1, 408),
             G.desc(1024, 2048, 7, 7, 512))


def test_plan_equals_route_on_a_dense_sweep_at_the_default_knobs(lib):
    seen = collections.Counter()
    with _knobs({}):
        for entry in SWEEP_ENTRIES:
            for d in FULL_SIZE:
                seen[_check_against_route(lib, entry, d, True, {}, (entry, d))] += 1
            for k, ragged, cols, depth, rs in itertools.product(SWEEP_K, (1, 0), (68, 132, 256, 512, 1024, 2048),
                                                                (32, 256, 1024, 2048), (1, 9)):
                d = G._policy_desc(entry, 64 * k + ragged, cols, depth, rs)
                seen[_check_against_route(lib, entry, d, True, {}, (entry, d))] += 1
    assert seen['w8'] > 0                                  # which no listed call reaches
    assert G.route('conv2d_fwd', FULL_SIZE[3]).label == 'w8'
    for label in ('small/plain', 'small/tiny_split', 'small/fused_tail', 'big/one_round_ksplit', 'big/all_rows',
                  'big/fused_tail', 'wgrad64/one_slab', 'wgrad64/split+reduce', 'wgrad128/split+reduce'):
        assert seen[label] > 0, label


# ---- the Winograd route: plan_wino_gemm / plan_wino_wgrad against wino_plan() ----------------------------

def _wino_line(w, mode):
    """The text mrcnn_conv_gemm_plan prints for WinoPlan ``w``: every field of every launch."""
    out = 'label=%s mode=%s M=%d N=%d k=%d' % (w.label, mode, w.M, w.N, w.k)
    for l in w.launches:
        out += ' | kind=%s tags=%s rows=%d:%d grid=%dx%d batch=%d slab=%d tail=0,0,0,0' % (
            l.kind, ','.join(l.tags), l.rows[0], l.rows[1], l.grid[0], l.grid[1], G.WINO_XI, l.slab)
    if w.slabs > 1:
        out += ' | sum row0=0 slabs=%d' % w.slabs
    return out


def _check_wino(lib, entry, d, kn, what):
    w = G.wino_plan(entry, d, kn)
    rc, line = _plan_line(lib, entry, d, True)
    assert rc == 0, (what, lib.mrcnn_last_error())
    assert line == _wino_line(w, G.WGRAD if entry.endswith('wgrad') else G.FWD), (what, entry, d)
    r = G.route(entry, d, 0, True, kn)
    assert r.label == w.label and sum(r.record.values()) == 1 and len(r.launches) == len(w.launches)
    _check_consistent(_plan(lib, entry, d, True), what)       # (it has no workspace rule for these slabs:
    assert w.slabs <= G.WINO_MAX_SPLITS                       #  the Winograd workspace holds 8)
    return w


def test_wino_plan_equals_route_on_every_listed_call(lib):
    seen = collections.defaultdict(set)
    for fam, i, entry, d, kn in G.wino_calls():
        with _knobs(kn):
            w = _check_wino(lib, entry, d, kn, i)
        seen[(entry, 'fp32' if kn.get('split_bf16', 3) == 0 else 'split')].add(w.label)
        assert G.wino_rejects(d) is None, i
    gemm, wgrad = set(G.WINO_LABELS[:4]), set(G.WINO_LABELS[4:])
    for e in G.WINO_ENTRIES[:2]:                       # every label, forward and data gradient alike
        assert seen[(e, 'split')] == gemm, e
        assert seen[(e, 'fp32')] == gemm - {'wino/w8'}, e
    assert seen[(G.WINO_ENTRIES[2], 'split')] == wgrad and seen[(G.WINO_ENTRIES[2], 'fp32')] == wgrad
    for i, entry, d, label in G.wino_policy_cases():
        assert G.wino_plan(entry, d).label == label, i
    assert {c[3] for c in G.wino_policy_cases()} == set(G.WINO_LABELS)


WINO_SWEEP_T = tuple(range(1, 701)) + (2048, 2049, 2050, 2051, 2052, 2816, 4095, 4096, 4100, 5632)
WINO_SWEEP_CH = (4, 36, 64, 68, 128, 132, 256, 260)


def test_wino_plan_equals_route_on_a_dense_sweep(lib):
    """T tiles (one 4x4 map each) x C x K x both arithmetics x the three entries, as whole lines."""
    from chainer_mask_rcnn_amd._lib import ConvDesc
    buf = ctypes.create_string_buffer(1024)
    for sb in (3, 0):
        kn = dict(G.DEFAULT_KNOBS, split_bf16=sb)
        seen = collections.Counter()
        with _knobs(kn):
            for T in WINO_SWEEP_T:
                gemm = {}
                for C_, K_ in itertools.product(WINO_SWEEP_CH, WINO_SWEEP_CH):
                    cd = ConvDesc(T, 4, 4, C_, K_, 3, 3, 1, 1, 4, 4)
                    for entry, mode, key in (('conv3x3_wino_fwd', G.FWD, (K_, C_)), ('conv3x3_wino_dgrad', G.FWD, (C_, K_)),
                                             ('conv3x3_wino_wgrad', G.WGRAD, None)):
                        if key is None:
                            w = G.wino_wgrad_plan(T, K_, C_, kn)
                            want = _wino_line(w, mode)
                        else:
                            if key not in gemm:
                                w = G.wino_gemm_plan(T, key[0], key[1], kn)
                                gemm[key] = (w.label, _wino_line(w, mode))
                            want = gemm[key][1]
                        assert lib.mrcnn_conv_gemm_plan(entry.encode(), ctypes.byref(cd), 1, buf, 1024) == 0
                        assert buf.value.decode() == want, (entry, T, C_, K_, sb)
                        seen[want.split(' ', 1)[0][len('label='):]] += 1
        want = set(G.WINO_LABELS) - ({'wino/w8'} if sb == 0 else set())
        assert set(seen) == want, (sb, seen)               # on fp32 W8 vanishes


def test_wino_policy_cases_are_the_smallest_that_reach_their_label():
    for i, entry, d, label in G.wino_policy_cases():
        rows = d.N
        assert (d.H, d.W) == (4, 4) and rows % 64 != 0 and rows % G.BK != 0, i
        cols = d.K if entry == 'conv3x3_wino_fwd' else d.C
        assert cols % 64 == 4, i
        if rows > 64:
            assert G.wino_plan(entry, d._replace(N=rows - 64)).label != label, i


# (this side, the other side, the entry that must change its label or its slab count)
WINO_THRESHOLD_PAIRS = [
    ((64, 68, 4, 4, 68), (65, 68, 4, 4, 68), 'conv3x3_wino_fwd'),
    ((64, 68, 4, 4, 68), (65, 68, 4, 4, 68), 'conv3x3_wino_dgrad'),
    ((65, 64, 4, 4, 68), (65, 68, 4, 4, 68), 'conv3x3_wino_dgrad'),
    ((65, 68, 4, 4, 64), (65, 68, 4, 4, 68), 'conv3x3_wino_fwd'),
    ((65, 64, 4, 4, 68), (65, 68, 4, 4, 68), 'conv3x3_wino_wgrad'),
    ((256, 68, 4, 4, 68), (257, 68, 4, 4, 68), 'conv3x3_wino_fwd'),
    ((320, 68, 4, 4, 68), (321, 68, 4, 4, 68), 'conv3x3_wino_fwd'),
    ((320, 68, 4, 4, 68), (321, 68, 4, 4, 68), 'conv3x3_wino_dgrad'),
    ((192, 68, 4, 4, 132), (320, 68, 4, 4, 68), 'conv3x3_wino_fwd'),
    ((511, 64, 4, 4, 64), (512, 64, 4, 4, 64), 'conv3x3_wino_wgrad'),
    ((4095, 260, 2, 2, 260), (4100, 260, 2, 2, 260), 'conv3x3_wino_fwd'),
    ((4095, 260, 2, 2, 260), (4100, 260, 2, 2, 260), 'conv3x3_wino_dgrad'),
    ((2816, 252, 4, 4, 260), (2816, 260, 4, 4, 260), 'conv3x3_wino_fwd'),
    ((2816, 256, 4, 4, 128), (2816, 260, 4, 4, 260), 'conv3x3_wino_fwd'),
]


def test_wino_thresholds_land_where_the_table_says():
    listed = {c for c, _, _, _ in G.WINO_THRESHOLDS}
    for c, fwd, dgrad, (tile, slabs, depth, last) in G.WINO_THRESHOLDS:
        d = G.wino_desc(*c)
        pf, pg, pw = (G.wino_plan(e, d) for e in G.WINO_ENTRIES)
        assert (pf.label, pg.label) == ('wino/' + fwd, 'wino/' + dgrad), c
        l = pw.launches[0]
        assert (int(l.tags[1].split('x')[0]), pw.slabs, l.slab, pw.k - (pw.slabs - 1) * l.slab) == \
            (tile, slabs, depth, last), c
        assert pw.label == 'wino_wgrad%d/%s' % (tile, 'split+sum' if slabs > 1 else 'one_slab'), c
    for a, b, entry in WINO_THRESHOLD_PAIRS:
        assert a in listed and b in listed
        assert G.wino_plan(entry, G.wino_desc(*a)).label != G.wino_plan(entry, G.wino_desc(*b)).label, (a, b, entry)
    # the slab counts the ordered sum is run at, each with a short last slab somewhere
    assert {w[1] for _, _, _, w in G.WINO_THRESHOLDS} >= {1, 2, 7, 8}
    # the tail launch's first row, and a tail of exactly 64 rows
    two = G.wino_plan('conv3x3_wino_fwd', G.wino_desc(320, 68, 4, 4, 68))
    assert [l.rows for l in two.launches] == [(0, 256), (256, 320)] and [l.grid for l in two.launches] == [(2, 1), (2, 1)]


def test_wino_size_caps():
    for fam, i, d in G.wino_cases():
        b = G.wino_moved_bytes(d)
        assert b <= 256 << 20, i
        if b > 16 << 20:
            assert G.is_w8_case(d) or d.N in (2816, 4095), i          # the W8 branch and its two near misses
            assert fam != 'policy' or G.WINO_SIZE_REASON in i, i
    for c in G.WINO_EPILOGUE_SHAPES + G.WINO_FIXUP_SHAPES + [G.WINO_FIXUP_OVERFLOW]:
        assert G.wino_moved_bytes(G.wino_desc(*c)) <= 16 << 20, c
    # the shapes the epilogue list promises
    maps = {(c[2], c[3]) for c in G.WINO_EPILOGUE_SHAPES}
    assert maps >= {(1, 1), (2, 7), (5, 4), (7, 7), (5, 9)}
    chans = {c[1] for c in G.WINO_EPILOGUE_SHAPES} | {c[4] for c in G.WINO_EPILOGUE_SHAPES}
    assert chans >= {4, 36, 40}
    fams = {G.wino_plan('conv3x3_wino_fwd', G.wino_desc(*c)).label for c in G.WINO_EPILOGUE_SHAPES}
    assert fams >= {'wino/small64', 'wino/big128', 'wino/main128+tail64'}
    for c in G.WINO_FIXUP_SHAPES:                      # every output fits the fix list
        d = G.wino_desc(*c)
        assert d.N * d.H * d.W * d.K <= G.wino_fix_cap(d), c
    assert {c[1] for c in G.WINO_FIXUP_SHAPES} >= {4, 36, 256, 260}
    assert {(c[2], c[3]) for c in G.WINO_FIXUP_SHAPES} >= {(1, 1), (2, 7), (7, 7)}
    w8 = G.wino_desc(*G.WINO_EPILOGUE_W8)
    assert [G.wino_plan(e, w8).label for e in G.WINO_ENTRIES[:2]] == ['wino/w8', 'wino/big128']
    assert (w8.H, w8.W) == (7, 7) and G.wino_moved_bytes(w8) <= 64 << 20
    ov = G.wino_desc(*G.WINO_FIXUP_OVERFLOW)
    assert G.wino_fix_cap(ov) == 4606 and ov.N * ov.H * ov.W * ov.K == 73800


def test_wino_plan_rejects_what_wino_check_rejects(lib):
    for i, d, why in G.WINO_REJECTED:
        assert G.wino_rejects(d) is not None, i
        for entry in G.WINO_ENTRIES:
            rc, _ = _plan_line(lib, entry, d, True)
            assert rc != 0 and why.encode() in lib.mrcnn_last_error(), (i, entry, lib.mrcnn_last_error())
    for entry in G.WINO_ENTRIES:
        assert _plan_line(lib, entry, G.wino_desc(2, 8, 7, 7, 8), True)[0] == 0
    rc, _ = _plan_line(lib, 'conv3x3_wino_fwd+res_g', G.wino_desc(2, 8, 7, 7, 8), True)
    assert rc != 0 and b'unknown entry' in lib.mrcnn_last_error()


# ---- detectors on a float64 model of the Winograd route ---------------------------------------------
from oracle import np_winograd as NW      # noqa: E402


def _wino_model(d):
    """float64 operands and the stages of the forward: tiles (N,TH,TW,C,6,6) -> V -> M (a,b,n,y,x,k)."""
    x, w, gy = (a.astype(np.float64) for a in G.operands(d))
    U = np.einsum('ai,kcij,bj->abkc', NW.G, w, NW.G)
    V = np.einsum('ai,nyxcij,bj->abnyxc', NW.BT, NW._tiles(x, 6, 4, -1), NW.BT)
    M = np.einsum('abnyxc,abkc->abnyxk', V, U)
    return x, w, gy, U, V, M


def _wino_out(M, H, W):
    """Y (N,K,4TH,4TW), not yet cropped to the map."""
    Y = np.einsum('ia,abnyxk,jb->nkyixj', NW.AT, M, NW.AT)
    n, k, th, _, tw, _ = Y.shape
    return Y.reshape(n, k, 4 * th, 4 * tw)


def test_wino_model_is_the_convolution():
    d = G.wino_desc(3, 4, 5, 9, 8)
    x, w, gy, U, V, M = _wino_model(d)
    _close64(_wino_out(M, 5, 9)[:, :, :5, :9], L.conv_fwd(_t(x), _t(w), 1, 1))
    _close64(NW.conv3x3_wgrad(x, gy), L.conv_wgrad(_t(x), _t(gy), 3, 3, 1, 1))


def test_detector_wino_wgrad_skips_its_short_last_slab_or_v_is_one_tile_short():
    """(a) and (e): 2050 tiles in 8 slabs of 288 with 34 in the last; 513 tiles in 2 with 225."""
    for c in ((2050, 4, 3, 3, 4), (513, 4, 4, 4, 4)):
        d = G.wino_desc(*c)
        big = G.wino_wgrad_plan(G.wino_tiles(d), 64, 64, dict(G.DEFAULT_KNOBS))      # the slabs of the listed case
        slab, slabs = big.launches[0].slab, big.slabs
        x, w, gy, U, V, M = _wino_model(d)
        Gy = np.einsum('ai,nyxkij,bj->abnyxk', NW.G4, NW._tiles(gy, 4, 4, 0), NW.G4)
        ref = _t(L.conv_wgrad(_t(x), _t(gy), 3, 3, 1, 1))

        def gw(keep):
            dU = np.einsum('abnk,abnc->abkc', Gy.reshape(6, 6, -1, d.K)[:, :, keep], V.reshape(6, 6, -1, d.C)[:, :, keep])
            return _t(np.einsum('ra,abkc,sb->kcrs', NW.WGRAD_AT, dU, NW.WGRAD_AT))
        T = G.wino_tiles(d)
        assert _accepts(_f32(gw(slice(0, T))), ref)
        assert not _accepts(_f32(gw(slice(0, (slabs - 1) * slab))), ref), 'last slab of %d tiles skipped' % (T - (slabs - 1) * slab)
        assert not _accepts(_f32(gw(slice(0, T - 1))), ref), 'v one tile short'


def test_detector_wino_tail_launch_rows():
    """(b): the 64-row tail launch of wino/main128+tail64 started one tile row early, or without its m_lo
    (it then computes rows [0, 64) again and the rows from `full` on keep what the workspace held)."""
    d = G.wino_desc(47, 4, 5, 9, 8)                        # 282 tiles: rows [0, 256) + [256, 282)
    plan = G.wino_gemm_plan(G.wino_tiles(d), 132, 68, dict(G.DEFAULT_KNOBS))
    assert plan.label == 'wino/main128+tail64'
    full = plan.launches[1].rows[0]
    x, w, gy, U, V, M = _wino_model(d)
    ref = L.conv_fwd(_t(x), _t(w), 1, 1)
    shape = M.shape
    rows = M.reshape(6, 6, -1, d.K)
    assert _accepts(_f32(_t(_wino_out(M, 5, 9)[:, :, :5, :9])), ref)
    early = rows.copy()
    early[:, :, full:] = rows[:, :, full - 64:full - 64 + (rows.shape[2] - full)]
    stale = rows.copy()
    stale[:, :, full:] = 0.
    for what, bad in (('tail launch starts at row full - 64', early), ('m_lo dropped', stale)):
        assert not _accepts(_f32(_t(_wino_out(bad.reshape(shape), 5, 9)[:, :, :5, :9])), ref), what


def test_detector_wino_output_transform_ragged_tile():
    """(d): a ragged tile's pixels right of the map written anyway land at the start of the next row."""
    for c in ((3, 4, 5, 9, 8), (2, 4, 2, 7, 4), (2, 4, 7, 7, 4)):
        d = G.wino_desc(*c)
        x, w, gy, U, V, M = _wino_model(d)
        ref = L.conv_fwd(_t(x), _t(w), 1, 1)
        Y = _wino_out(M, d.H, d.W)
        bad = Y[:, :, :d.H, :d.W].copy()
        over = Y.shape[3] - d.W
        bad[:, :, 1:, :over] = Y[:, :, :d.H - 1, d.W:]
        assert over > 0 and not _accepts(_f32(_t(bad)), ref), c


def _abs_bound(M):
    """|A^T| |M| |A| per output (N,K,4TH,4TW): what wino_output_transform_kernel<true> propagates."""
    B = np.einsum('ia,abnyxk,jb->nkyixj', np.abs(NW.AT), np.abs(M), np.abs(NW.AT))
    return B.reshape(M.shape[2], M.shape[5], 4 * M.shape[3], 4 * M.shape[4])


@pytest.mark.parametrize('c', G.WINO_FIXUP_SHAPES, ids=str)
def test_detector_wino_fixup_and_its_one_half_condition(c):
    """(c), and the condition the device test puts on its BIAS / AFFINE-with-shift cases: at an ambiguity of
    2.0 the float64 model of the bound selects every output when the shift is zero and at least half of
    them with the shifts of wino_fixup_epilogue, which stay below 0.1 x rms of the pre-activation."""
    d = G.wino_desc(*c)
    x, w, gy, U, V, M = _wino_model(d)
    conv = _wino_out(M, d.H, d.W)[:, :, :d.H, :d.W]
    bound = 2.0 * _abs_bound(M)[:, :, :d.H, :d.W]
    assert np.all(np.abs(conv) < bound)                                   # (i): every output qualifies
    sc0, _ = G.wino_fixup_epilogue(d, 'affine0')
    assert (sc0 > 0).any() and (sc0 < 0).any()
    wrapped = TF.conv2d(TF.pad(_t(x), (1,) * 4, mode='circular'), _t(w))
    if d.H > 1:       # (a one-pixel map has one real tap: the wrap reads the pixel itself for every other)
        assert not _accepts(_f32(wrapped), _t(conv)), 'padding taps read the wrapped row'
    for kind in ('bias', 'affine'):
        sc, sh = G.wino_fixup_epilogue(d, kind)
        sc = np.ones(d.K) if sc is None else sc.astype(np.float64)
        pre = conv * sc[None, :, None, None]
        ref = pre + sh.astype(np.float64)[None, :, None, None]
        assert np.abs(sh).max() <= 0.1 * np.sqrt((pre ** 2).mean()), kind
        chosen = np.abs(ref) < bound * np.abs(sc)[None, :, None, None]
        assert chosen.mean() >= 0.75, (kind, chosen.mean())              # the model alone, with margin over 1/2
        assert _accepts(_f32(_t(ref)), _t(ref))
        no_shift = np.where(chosen, pre, ref)                             # a fix-up that drops the shift
        assert not _accepts(_f32(_t(no_shift)), _t(ref)), kind
        over = np.abs(no_shift - ref) > 1e-4 * np.abs(ref) + 1e-5 * np.abs(ref).max()
        assert over.mean() >= 0.5, (kind, over.mean())
