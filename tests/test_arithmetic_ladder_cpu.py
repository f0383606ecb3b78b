"""The arithmetic ladder of the convolution GEMMs without a device: the names of
functions.conv.set_gemm_arithmetic, the "split_planes" knob (mrcnn_set_tuning, _lib.set_tuning,
MRCNN_TUNE), the launch plan's independence of it, the Winograd routing under each name, and a
float64 model of the three product sets that holds the error bounds of tests/arithmetic_ladder.py on
the very operands tests/test_gpu_arithmetic_ladder.py gives the kernels."""
import os
import subprocess
import sys

import numpy as np
import pytest

import arithmetic_ladder as A
import gemm_edge_cases as G
from test_gemm_edge_cases_cpu import _plan_line

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from chainer_mask_rcnn_amd import _lib
    return _lib.load()


@pytest.fixture
def conv(lib):
    from chainer_mask_rcnn_amd.functions import conv as C
    yield C
    C.set_gemm_arithmetic(C.DEFAULT_GEMM_ARITHMETIC)
    assert lib.mrcnn_set_tuning(b'split_planes', 3) == 0


def _planes_now(lib):
    """The knob's value, read from the message of a rejected write (there is no getter)."""
    assert lib.mrcnn_set_tuning(b'split_planes', 0) != 0
    msg = lib.mrcnn_last_error().decode()
    assert 'split_planes' in msg and 'stays' in msg, msg
    return int(msg.rsplit('stays', 1)[1].strip(' )'))


def test_names_of_set_gemm_arithmetic(lib, conv):
    assert conv.DEFAULT_GEMM_ARITHMETIC == conv.GEMM_ARITHMETIC == 'split_bf16x3'
    assert set(conv.GEMM_ARITHMETICS) == set(A.NAMES)
    for name in A.NAMES:
        conv.set_gemm_arithmetic(name)
        assert conv.GEMM_ARITHMETIC == name
        assert _planes_now(lib) == A.PLANES.get(name, 3)
        for bad in ('bf16', 'split_bf16', 'bf16x2', 'split_bf16x1', 'tf32', '', None, 3):
            with pytest.raises(ValueError):
                conv.set_gemm_arithmetic(bad)
            assert conv.GEMM_ARITHMETIC == name and _planes_now(lib) == A.PLANES.get(name, 3)
    assert conv.DEFAULT_GEMM_ARITHMETIC == 'split_bf16x3'


def test_split_planes_knob_validation(lib):
    from chainer_mask_rcnn_amd import _lib
    try:
        for good in (1, 2, 3):
            assert lib.mrcnn_set_tuning(b'split_planes', good) == 0
            for bad in (0, 4, -1, 6, 1 << 20):
                assert lib.mrcnn_set_tuning(b'split_planes', bad) != 0
                assert b'split_planes' in lib.mrcnn_last_error()
                with pytest.raises(_lib.MrcnnHipError):
                    _lib.set_tuning('split_planes', bad)
            assert _planes_now(lib) == good                    # a rejected value keeps the setting
            _lib.set_tuning('split_planes', good)
        # independent of the family switch: stays while split_bf16 goes off and on
        _lib.set_tuning('split_planes', 2)
        _lib.set_tuning('split_bf16', 0)
        _lib.set_tuning('split_bf16', 3)
        assert _planes_now(lib) == 2
    finally:
        _lib.set_tuning('split_bf16', 3)
        _lib.set_tuning('split_planes', 3)


_CHILD = """
import sys
sys.path.insert(0, %r)
from chainer_mask_rcnn_amd import _lib
from chainer_mask_rcnn_amd.functions import conv
lib = _lib.load()
assert lib.mrcnn_set_tuning(b'split_planes', 0) != 0
print('MSG', lib.mrcnn_last_error().decode())
print('NAME', conv.GEMM_ARITHMETIC, conv.uses_winograd(conv.make_desc((1024, 512, 7, 7), (512, 512, 3, 3), 1, 1)))
"""


def _child(tune):
    env = dict(os.environ, MRCNN_TUNE=tune)
    return subprocess.run([sys.executable, '-c', _CHILD % ROOT], env=env, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, universal_newlines=True, timeout=300)


def test_mrcnn_tune_sets_the_knob_in_a_child_process(lib):
    for n in (2, 1):
        r = _child('split_planes=%d' % n)
        assert r.returncode == 0, r.stderr
        assert 'stays %d' % n in r.stdout, r.stdout
        # the library knob alone: the Python name and the Winograd route stay as they are
        assert 'NAME split_bf16x3 True' in r.stdout, r.stdout
    r = _child('split_planes=4')
    assert r.returncode != 0 and 'MRCNN_TUNE' in r.stderr and 'split_planes' in r.stderr, r.stderr


def test_the_launch_plan_does_not_depend_on_the_planes(lib):
    """Statement 5: mrcnn_conv_gemm_plan returns the same plan for split_planes = 1, 2, 3 on every call of
    tests/gemm_edge_cases.py, under the knobs the call is listed with."""
    from chainer_mask_rcnn_amd import _lib
    calls = list(G.all_calls())
    assert len(calls) > 1000
    plans = {}
    try:
        for planes in (3, 2, 1):
            _lib.set_tuning('split_planes', planes)
            out = []
            for fam, i, entry, d, ws, kn in calls:
                for k, v in dict(G.DEFAULT_KNOBS, **kn).items():
                    _lib.set_tuning(k, v)
                rc, line = _plan_line(lib, entry, d, ws)
                assert rc == 0, (i, entry, lib.mrcnn_last_error())
                out.append(line)
            plans[planes] = out
    finally:
        for k, v in G.DEFAULT_KNOBS.items():
            _lib.set_tuning(k, v)
        _lib.set_tuning('split_planes', 3)
    assert plans[1] == plans[3] and plans[2] == plans[3]
    assert any('split' in p for p in plans[3]) and any('fp32' in p for p in plans[3])
    # and the cases of the device test, W8 included
    for case in A.cases():
        entry = {'stem': 'conv_stem_fwd', 'deconv': 'deconv2x2s2_fwd_wt'}.get(case.kind, 'conv2d_fwd')
        lines = []
        try:
            for planes in (3, 2, 1):
                for k, v in dict(G.DEFAULT_KNOBS, split_planes=planes, **case.knobs).items():
                    _lib.set_tuning(k, v)
                lines.append(_plan_line(lib, entry, case.d, True))
        finally:
            for k, v in dict(G.DEFAULT_KNOBS, split_planes=3).items():
                _lib.set_tuning(k, v)
        assert lines[0][0] == 0 and lines[0] == lines[1] == lines[2], case.id


def test_the_device_cases_cover_the_branches(lib):
    """What tests/test_gpu_arithmetic_ladder.py runs: every forward label of the policy, W8, both tile sizes in
    the three geometry instantiations, strided / stem / deconvolution launches, and a split 128x128 weight
    gradient that sums slabs."""
    labels, tags = set(), set()
    for case in A.cases():
        entry = {'stem': 'conv_stem_fwd', 'deconv': 'deconv2x2s2_fwd_wt'}.get(case.kind, 'conv2d_fwd')
        r = G.route(entry, case.d, 0, True, case.knobs)
        labels.add(r.label)
        for _, t in r.launches:
            assert 'split' in t, case.id
            tags.add((t[1], [v for v in ('PW', 'K3', 'general', 'W8') if v in t][0]))
            tags.update(v for v in t if v in ('perm', 'stem', G.OUT_STRIDED, G.OUT_DECONV))
    assert labels >= set(G.FWD_LABELS) | {'w8'}, set(G.FWD_LABELS) - labels
    assert tags >= {(tile, v) for tile in ('64x64', '128x128') for v in ('PW', 'K3', 'general')}, tags
    assert tags >= {'perm', 'stem', G.OUT_DECONV}, tags
    strided = [c for c in A.cases() if c.d.stride == 2 and c.kind == 'conv'][0]
    assert G.OUT_STRIDED in G.route('conv2d_dgrad_wt', strided.d, 0, True, strided.knobs).launches[0][1]
    ws = [c for c in A.cases() if c.d == A.WGRAD128_WS[1]][0]
    assert G.route('conv2d_wgrad', ws.d, 0, True, ws.knobs).label == 'wgrad128/split+reduce'
    assert A.split_outputs(ws) == {'y': True, 'gx': True, 'gw': True}
    assert sum(A.split_outputs(c).get('gw', False) for c in A.cases()) >= 4


def test_uses_winograd_under_each_name(lib, conv):
    routed = conv.make_desc((1024, 512, 7, 7), (512, 512, 3, 3), 1, 1)       # res5 of the RoI head
    direct = conv.make_desc((2, 256, 50, 84), (256, 256, 3, 3), 1, 1)        # res4, train batch: too little work
    for name in A.NAMES:
        conv.set_gemm_arithmetic(name)
        assert conv.uses_winograd(routed) == (name != 'bf16x1'), name
        assert not conv.uses_winograd(direct)
    conv.set_gemm_arithmetic('split_bf16x3')
    assert conv.uses_winograd(routed)
    # every switch drops the cached transformed filters
    conv._wino_u_cache['stale'] = None
    conv.set_gemm_arithmetic('split_bf16x2')
    assert not conv._wino_u_cache
    # the forward-form deconvolution belongs to the split family under all three names
    assert set(conv.SPLIT_GEMM_ARITHMETICS) == set(A.PLANES)


# ---- the rounding maps and the bounds ---------------------------------------------------------------------

def test_rounding_maps():
    rng = np.random.RandomState(3)
    a = (rng.standard_normal(1 << 18) * 10.0 ** rng.uniform(-3, 3, 1 << 18)).astype(np.float32)
    hi, mid, lo = A.split3(a)
    assert np.array_equal(A.r1(a), hi) and np.array_equal(A.r2(a).astype(np.float64), hi.astype(np.float64) + mid)
    assert np.array_equal(A.bf16_round(a), hi) and all(np.array_equal(p, q) for p, q in zip(A.hi_mid(a), (hi, mid)))
    assert np.all(np.abs(a - hi) <= A.U * np.abs(a)) and np.all(np.abs(lo) <= A.U ** 2 * np.abs(a))
    # r1 is idempotent and splits into (hi, 0, 0): the premise of statement 1
    h2, m2, l2 = A.split3(hi)
    assert np.array_equal(h2, hi) and not m2.any() and not l2.any()
    # r2 splits back into (hi, mid, 0) except at ties; tie_free removes exactly those
    back = A.split3(A.r2(a))
    ties = back[0] != hi
    assert 0 < ties.mean() < 2.0 ** -8
    t = A.tie_free(a)
    assert np.array_equal(t[~ties], a[~ties]) and np.array_equal(t[ties], hi[ties])
    bh, bm, bl = A.split3(A.r2(t))
    th, tm, _ = A.split3(t)
    assert np.array_equal(bh, th) and np.array_equal(bm, tm) and not bl.any()


def test_bound_constants():
    u = A.U
    assert A.C1 == 2 * u + u * u
    six = (u + u * u) ** 2 + 2 * (1 + u) * u * u + 2 * (u + u * u) * u * u + u ** 4
    assert abs(A.C2 - six) <= 1e-18 and 3 * u * u < A.C2 < 3.1 * u * u
    # per product, on adversarial and random pairs
    rng = np.random.RandomState(4)
    a = np.concatenate([rng.standard_normal(200000), 1 + rng.uniform(0, 1, 200000) * 2.0 ** -7]).astype(np.float32)
    b = np.concatenate([rng.standard_normal(200000), 1 + rng.uniform(0, 1, 200000) * 2.0 ** -7]).astype(np.float32)
    (ah, am, _), (bh, bm, _) = ([p.astype(np.float64) for p in A.split3(v)] for v in (a, b))
    exact = a.astype(np.float64) * b
    assert np.all(np.abs(ah * bh - exact) <= A.C1 * np.abs(exact))
    assert np.all(np.abs(ah * bh + ah * bm + am * bh - exact) <= A.C2 * np.abs(exact))
    assert np.abs(ah * bh - exact).max() > 0.2 * A.C1 * np.abs(exact).min()        # (not vacuous)


@pytest.mark.parametrize('case', A.cases(), ids=[c.id for c in A.cases()])
def test_model_of_the_product_sets_holds_the_bounds(case):
    """Statement 4 before the device sees the operands: per output element of every launch of the case,
    |model - float64| <= c S for the one-plane and the two-plane product set, and the model of the
    three-plane set is at fp32 level (2^-23 S: its three dropped products)."""
    x, w, gy, _ = A.operands(case)
    ref, S = A.reference(case, x, w, gy)
    for planes, c in ((1, A.C1), (2, A.C2), (3, 2.0 ** -23)):
        got = A.model(case, planes, x, w, gy)
        assert set(got) == set(ref) == ({'y', 'gx', 'gw'} if case.backward else {'y'})
        for k in ref:
            err = np.abs(got[k] - ref[k])
            slack = 1e-13 * S[k]                     # float64 rounding of the model itself
            worst = float((err / (c * S[k] + slack + 1e-300)).max())
            assert worst <= 1.0, (planes, k, worst)
            if planes < 3:                           # the reduced sets really differ from float64
                assert float((err / (S[k] + 1e-300)).max()) > 1e-3 * c, (planes, k)
