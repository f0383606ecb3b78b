"""Test-time augmentation without a GPU: the model's view list and its errors, the properties of
the NumPy reference of the two merge rules (tests/test_aug_ref.py), the tools' flags and the
binding table."""
import argparse
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import test_aug_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from chainer_mask_rcnn_amd import _lib
    return _lib.load()


def _model():
    import chainer_mask_rcnn_amd as cmr
    return cmr.models.MaskRCNNResNet(50, n_fg_class=5, min_size=64, max_size=96)


def test_views_default_and_order():
    model = _model()
    assert (model.test_aug_h_flip, tuple(model.test_aug_scales), model.test_aug_max_size,
            model.test_aug_scale_h_flip, model.mask_aug_heur) == (False, (), None, False, 'soft_avg')
    assert model.test_aug_views() == [(64, 96, False)]
    model.test_aug_h_flip = True
    assert model.test_aug_views() == [(64, 96, False), (64, 96, True)]
    model.test_aug_scales = (48, 80)
    assert model.test_aug_views() == [(64, 96, False), (64, 96, True), (48, 96, False),
                                      (80, 96, False)]
    model.test_aug_scale_h_flip, model.test_aug_max_size = True, 120
    assert model.test_aug_views() == [(64, 96, False), (64, 96, True), (48, 120, False),
                                      (48, 120, True), (80, 120, False), (80, 120, True)]
    model.test_aug_h_flip = False
    assert model.test_aug_views() == [(64, 96, False), (48, 120, False), (48, 120, True),
                                      (80, 120, False), (80, 120, True)]
    model.test_aug_scales = (48, 56, 72)                 # 2 + 3 * 2 = 8 views: the most
    model.test_aug_h_flip = True
    assert len(model.test_aug_views()) == 8


@pytest.mark.parametrize('attrs', [
    dict(test_aug_h_flip=True, test_aug_scales=(40, 48, 56, 72), test_aug_scale_h_flip=True),  # 10
    dict(test_aug_scales=(40, 44, 48, 52, 56, 60, 68, 72)),                                    # 9
    dict(test_aug_scales=(48, 0)),
    dict(test_aug_scales=(-48,)),
    dict(test_aug_scales=(48,), test_aug_max_size=0),
    dict(mask_aug_heur='mean'),
    dict(test_aug_h_flip=True, mask_aug_heur=None),
    dict(test_aug_scale_h_flip=True),
    dict(test_aug_h_flip=True, test_aug_scale_h_flip=True),
])
def test_views_errors(attrs):
    model = _model()
    for k, v in attrs.items():
        setattr(model, k, v)
    with pytest.raises(ValueError):
        model.test_aug_views()
    with pytest.raises(ValueError):      # predict_images asks for the views before anything else
        model.predict_images([np.zeros((3, 8, 8), np.uint8)])


def test_prepare_takes_the_views_sizes():
    import inspect
    from chainer_mask_rcnn_amd.models import MaskRCNN
    p = inspect.signature(MaskRCNN.prepare).parameters
    assert list(p)[:3] == ['self', 'imgs', 'x_flips']
    assert p['min_size'].default is None and p['max_size'].default is None
    assert 'n_views' in inspect.signature(MaskRCNN._suppress_queue).parameters


# ---- the reference's own properties ------------------------------------------------------------
def _maps(seed, V, D=3, M=7, Kc=5):
    rng = np.random.RandomState(seed)
    return [rng.uniform(-50, 50, (D, M, M, Kc)).astype(np.float32) for _ in range(V)]


@pytest.mark.parametrize('heur', ['logit_avg', 'soft_max'])
def test_one_unmirrored_view_is_the_identity(heur):
    m = _maps(0, 1)[0]
    m[0, 0, 0, :3] = (0., 300., -300.)
    out = ref.mask_aug_combine([m], [False], heur)
    assert out.dtype == np.float32 and np.array_equal(out.view(np.int32), m.view(np.int32))


@pytest.mark.parametrize('heur', ref.HEURS)
@pytest.mark.parametrize('M', [7, 14])
def test_mirroring_every_view_mirrors_the_result(heur, M):
    maps = _maps(1, 3, M=M)
    plain = ref.mask_aug_combine(maps, [False] * 3, heur)
    mirrored = ref.mask_aug_combine(maps, [True] * 3, heur)
    assert np.array_equal(mirrored.view(np.int32), plain[:, :, ::-1].view(np.int32))
    mixed = ref.mask_aug_combine(maps, [False, True, False], heur)
    again = ref.mask_aug_combine([maps[0], maps[1][:, :, ::-1], maps[2]], [False] * 3, heur)
    assert np.array_equal(mixed.view(np.int32), again.view(np.int32))
    if M % 2:                           # the middle column maps to itself
        assert np.array_equal(mirrored[:, :, M // 2], plain[:, :, M // 2])


@pytest.mark.parametrize('V', [1, 2, 3, 8])
def test_soft_avg_lies_between_the_extreme_logits(V):
    maps = _maps(2 + V, V)
    out = ref.mask_aug_combine(maps, [False] * V, 'soft_avg').astype(np.float64)
    lo, hi = np.min(maps, axis=0).astype(np.float64), np.max(maps, axis=0).astype(np.float64)
    slack = 2.0 ** -23 * np.maximum(np.abs(lo), np.abs(hi))       # the one rounding to fp32
    assert (out >= lo - slack).all() and (out <= hi + slack).all()
    if V == 1:
        assert np.all(np.abs(out - maps[0]) <= 2.0 ** -23 * np.abs(maps[0]) + 2.0 ** -40)


@pytest.mark.parametrize('logits', [
    (-300., -300.), (300., 300., 300.), (-300., 300.), (-300., -290., -300.), (300., 0.),
    (-300., 0., 10.), (300., 295., 299., 300., 300., 298., 300., 300.),
])
def test_soft_avg_stays_accurate_where_the_maps_saturate(logits):
    maps = [np.full((1, 1, 1, 1), l, np.float32) for l in logits]
    got = float(ref.mask_aug_combine(maps, [False] * len(maps), 'soft_avg')[0, 0, 0, 0])
    want = float(ref.soft_avg_analytic(logits))
    assert np.isfinite(got)
    assert abs(got - want) <= 1e-6 * abs(want) + 1e-12, (got, want)


def test_unmirror_is_flip_bbox():
    from chainer_mask_rcnn_amd.datasets.transforms import flip_bbox
    rng = np.random.RandomState(5)
    b = rng.uniform(0, 333, (40, 4)).astype(np.float32)
    b[:, 2:] = np.minimum(b[:, :2] + rng.uniform(0, 90, (40, 2)).astype(np.float32), 333)
    assert np.array_equal(ref.unmirror_boxes(b, 333), flip_bbox(b, (200, 333), x_flip=True))
    u = ref.union_boxes([b[:10].reshape(5, 2, 4), b[10:].reshape(15, 2, 4)], [False, True], 333)
    assert u.shape == (20, 2, 4) and np.array_equal(u[:5].reshape(10, 4), b[:10])
    assert np.array_equal(u[5:].reshape(30, 4), flip_bbox(b[10:], (200, 333), x_flip=True))


# ---- the library and its binding -----------------------------------------------------------------
def test_binding_table_has_both_symbols(lib):
    from chainer_mask_rcnn_amd import _lib
    for name in ('mrcnn_decode_cls_boxes_views', 'mrcnn_mask_aug_combine'):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert ctypes.sizeof(_lib.TestAugView) == 32 and _lib.TEST_AUG_MAX_VIEWS == 8
    assert _lib.MASK_AUG_HEURS == {'soft_avg': 0, 'soft_max': 1, 'logit_avg': 2}


def test_entry_points_validate_arguments_without_device(lib):
    from chainer_mask_rcnn_amd import _lib
    buf = ctypes.cast(ctypes.create_string_buffer(256), ctypes.c_void_p)
    four = (ctypes.c_double * 4)(0, 0, 0, 0)
    views = (_lib.TestAugView * 9)()
    # nothing to do: no launch, no error, no pointer read
    assert lib.mrcnn_decode_cls_boxes_views(views, 0, 81, four, four, 10., 10., None, None) == 0
    assert lib.mrcnn_decode_cls_boxes_views(views, 8, 81, four, four, 10., 10., None, None) == 0
    assert lib.mrcnn_decode_cls_boxes_views(views, 9, 81, four, four, 10., 10., buf, None) != 0
    assert b'n_views' in lib.mrcnn_last_error()
    views[0].R = -1
    assert lib.mrcnn_decode_cls_boxes_views(views, 1, 81, four, four, 10., 10., buf, None) != 0
    views[0] = _lib.TestAugView(buf, buf, 4, 1, 1.0, 0)
    assert lib.mrcnn_decode_cls_boxes_views(views, 1, 2, four, four, 10., 10., buf, None) != 0
    assert b'ld_loc' in lib.mrcnn_last_error()
    maps = (_lib.c_vp * 9)(*([buf.value] * 9))
    flips = (ctypes.c_int32 * 9)()
    out = ctypes.cast(ctypes.create_string_buffer(256), ctypes.c_void_p)
    assert lib.mrcnn_mask_aug_combine(maps, flips, 2, 0, 14, 80, 0, None, None) == 0      # D == 0
    for n_views in (0, 9):
        assert lib.mrcnn_mask_aug_combine(maps, flips, n_views, 1, 14, 80, 0, out, None) != 0
        assert b'n_views' in lib.mrcnn_last_error()
    assert lib.mrcnn_mask_aug_combine(maps, flips, 2, 1, 14, 80, 3, out, None) != 0
    assert b'heuristic' in lib.mrcnn_last_error()
    assert lib.mrcnn_mask_aug_combine(maps, flips, 2, 1, 14, 80, 0, buf, None) != 0
    assert b'aliases' in lib.mrcnn_last_error()


def test_wrappers_check_before_the_device_reads(monkeypatch):
    import torch
    from chainer_mask_rcnn_amd import _lib
    from chainer_mask_rcnn_amd.functions import aug_merge
    monkeypatch.setattr(_lib, 'require_device', lambda *a: None)
    monkeypatch.setattr(_lib, 'call', lambda *a: pytest.fail('reached the library'))
    roi, loc = torch.zeros((5, 4)), torch.zeros((5, 8))
    for views in ([(roi, loc[:, :4], 1., False)], [(roi[:4], loc, 1., False)],
                  [(roi.double(), loc, 1., False)], [(roi, loc.half(), 1., False)],
                  [(roi, loc, 1., False)] * 9, []):
        with pytest.raises(ValueError):
            aug_merge.decode_cls_boxes_views(views, 2, (0,) * 4, (1,) * 4, (10, 10))
    m = torch.zeros((2, 3, 7, 7))
    for maps, flips, heur in (([m], [False], 'mean'), ([m] * 9, [False] * 9, 'soft_avg'),
                              ([], [], 'soft_avg'), ([m, m], [False], 'soft_avg'),
                              ([m, m[:1]], [False, False], 'soft_avg'),
                              ([m.double()], [False], 'soft_avg'),
                              ([torch.zeros((2, 3, 7, 6))], [False], 'soft_avg')):
        with pytest.raises(ValueError):
            aug_merge.mask_aug_combine(maps, flips, heur)


# ---- the tools ---------------------------------------------------------------------------------------
def _tool(name, *args):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'tools', name)] + list(args),
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)


FLAGS = ('--test-aug-h-flip', '--test-aug-scales', '--test-aug-max-size', '--test-aug-scale-h-flip',
         '--mask-aug-heur')


@pytest.mark.parametrize('tool', ['evaluate.py', 'demo.py'])
def test_tools_list_the_flags(tool):
    out = _tool(tool, '--help')
    assert out.returncode == 0, out.stdout
    for flag in FLAGS:
        assert flag in out.stdout


@pytest.mark.parametrize('tool,base', [('evaluate.py', ['--synthetic', '1']),
                                       ('demo.py', ['--img', 'none.jpg', '--snapshot', 'none.npz'])])
@pytest.mark.parametrize('flags,word', [
    (['--test-aug-max-size', '1200'], 'without --test-aug-scales'),
    (['--test-aug-scale-h-flip'], 'without --test-aug-scales'),
    (['--test-aug-h-flip', '--test-aug-scale-h-flip'], 'without --test-aug-scales'),
    (['--mask-aug-heur', 'soft_max'], 'without --test-aug-h-flip'),
    (['--mask-aug-heur', 'mean', '--test-aug-h-flip'], 'mean'),
    (['--test-aug-scales', '500,-3'], 'positive'),
    (['--test-aug-scales', '500,big'], 'positive'),
    (['--test-aug-scales', '500', '--test-aug-max-size', '0'], 'positive'),
    (['--test-aug-h-flip', '--test-aug-scales', '400,500,600,700', '--test-aug-scale-h-flip'],
     'at most 8'),
])
def test_tools_refuse_flags_they_would_ignore(tool, base, flags, word):
    out = _tool(tool, *(base + flags))
    assert out.returncode == 2 and word in out.stdout, out.stdout


def test_evaluate_refuses_the_flags_when_it_scores_a_file():
    out = _tool('evaluate.py', '--results', 'r.json', '--coco-root', 'none', '--test-aug-h-flip')
    assert out.returncode == 2 and 'results file' in out.stdout, out.stdout


def _parsed(*argv):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import evaluate
    finally:
        sys.path.pop(0)
    ap = argparse.ArgumentParser()
    evaluate.add_postprocessing_flags(ap)
    args = ap.parse_args(list(argv))
    evaluate.check_postprocessing_flags(ap, args)
    return evaluate, args


def test_postprocessing_record():
    evaluate, args = _parsed()
    model = _model()
    used = evaluate.apply_postprocessing_flags(model, args)
    assert sorted(used) == ['bbox_vote_thresh', 'nms_thresh', 'score_thresh', 'soft_nms']
    assert model.test_aug_views() == [(64, 96, False)]
    # a caller's own namespace without any of the flags (evaluate_log_dir's callers)
    assert evaluate.apply_postprocessing_flags(_model(), argparse.Namespace()) == used

    evaluate, args = _parsed('--test-aug-h-flip', '--test-aug-scales', '48,80', '--test-aug-max-size',
                             '120', '--test-aug-scale-h-flip', '--mask-aug-heur', 'logit_avg')
    model = _model()
    used = evaluate.apply_postprocessing_flags(model, args)
    assert used['mask_aug_heur'] == 'logit_avg' == model.mask_aug_heur
    assert used['test_aug_views'] == [[64, 96, False], [64, 96, True], [48, 120, False],
                                      [48, 120, True], [80, 120, False], [80, 120, True]]
    assert [tuple(v) for v in used['test_aug_views']] == model.test_aug_views()
    import json
    json.dumps(used)                                     # plain types: the result file takes it
