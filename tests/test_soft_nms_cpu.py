"""Soft-NMS and box voting without a device: the NumPy reference of tests/soft_nms_ref.py against
the hard NMS oracle and against Detectron's loop form, the entry points' argument checks, the
model's attributes and the tools' flags."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import np_ref

import soft_nms_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 63, 64, 65, 129)


def random_sorted(rng, n, canvas=200., lo=4., hi=100.):
    """n boxes with sides lo..hi on a small canvas (frequent overlaps), distinct descending scores."""
    tl = rng.uniform(0, canvas - lo, (n, 2))
    wh = rng.uniform(lo, hi, (n, 2))
    bbox = np.concatenate([tl, np.minimum(tl + wh, canvas)], axis=1).astype(np.float32)
    prob = np.sort(rng.permutation(4 * n)[:n].astype(np.float32) / np.float32(4 * n + 1)
                   * np.float32(0.9) + np.float32(0.06))[::-1].copy()
    assert len(np.unique(prob)) == n
    return bbox, prob


@pytest.mark.parametrize('n', SIZES)
def test_hard_method_is_the_nms_oracle(n):
    bbox, prob = random_sorted(np.random.RandomState(n), n)
    keep, soft = ref.soft_nms(bbox, prob, 'hard', overlap_thresh=0.5)
    assert np.array_equal(keep, np_ref.non_maximum_suppression(bbox, 0.5))
    assert np.array_equal(soft[keep], prob[keep])
    if n >= 63:
        assert len(keep) < n


@pytest.mark.parametrize('method', ['linear', 'gaussian'])
@pytest.mark.parametrize('n', SIZES)
def test_pick_max_form_equals_detectron_loop(n, method):
    bbox, prob = random_sorted(np.random.RandomState(100 + n), n)
    for min_score in (0.001, 0.05):
        keep, soft = ref.soft_nms(bbox, prob, method, min_score=min_score)
        d_keep, d_score = ref.detectron_soft_nms(bbox, prob, method, min_score=min_score)
        assert np.array_equal(keep, d_keep)
        assert np.array_equal(soft[keep], d_score)


@pytest.mark.parametrize('method', ['hard', 'linear', 'gaussian'])
def test_emitted_scores_do_not_increase(method):
    bbox, prob = random_sorted(np.random.RandomState(7), 129)
    keep, soft, margin = ref.soft_nms(bbox, prob, method, min_score=0.05, with_margin=True)
    assert 0 < len(keep) <= 129 and margin >= 0
    assert np.all(np.diff(soft[keep]) <= 0)
    assert np.all(soft[keep] >= np.float32(0.05))
    assert np.all(soft <= prob)


def test_limit_and_empty_input():
    bbox, prob = random_sorted(np.random.RandomState(3), 65)
    full, _ = ref.soft_nms(bbox, prob, 'linear')
    for limit in (1, 64):
        keep, _ = ref.soft_nms(bbox, prob, 'linear', limit=limit)
        assert np.array_equal(keep, full[:limit])
    keep, soft = ref.soft_nms(np.zeros((0, 4)), np.zeros((0,)), 'linear')
    assert keep.shape == (0,) and soft.shape == (0,)


def test_vote_three_boxes_by_hand():
    # box 1 overlaps box 0 with IoU 81 / 119 = 0.68, box 2 overlaps nothing
    bbox = np.array([[0, 0, 10, 10], [1, 1, 11, 11], [50, 50, 60, 60]], np.float32)
    prob = np.array([0.75, 0.25, 0.5], np.float32)
    keep = np.array([0, 2], np.int32)
    voted = ref.box_vote(bbox, prob, keep, vote_thresh=0.5)
    assert np.array_equal(voted[0], np.array([0.25, 0.25, 10.25, 10.25], np.float32))
    assert np.array_equal(voted[1], bbox[2])
    # at 0.8 box 1 no longer votes for box 0
    assert np.array_equal(ref.box_vote(bbox, prob, keep, vote_thresh=0.8), bbox[keep])
    # a zero-area box overlaps nothing, itself included: it comes back unchanged
    flat = np.array([[5, 5, 5, 9], [0, 0, 10, 10]], np.float32)
    assert np.array_equal(ref.box_vote(flat, prob[:2], np.array([0]), 0.8)[0], flat[0])


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from chainer_mask_rcnn_amd import _lib
    return _lib.load()


def _soft_nms_rc(lib, n_max, method, sigma):
    buf = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    return lib.mrcnn_soft_nms_sorted_batched(buf, buf, buf, 1, n_max, method, 0.3, sigma, 0.001, 0,
                                             buf, buf, buf, None)


def test_entry_points_validate_arguments_without_device(lib):
    from chainer_mask_rcnn_amd import _lib
    assert hasattr(lib, 'mrcnn_soft_nms_sorted_batched') and hasattr(lib, 'mrcnn_box_vote')
    assert 'mrcnn_soft_nms_sorted_batched' in _lib.SIGNATURES and 'mrcnn_box_vote' in _lib.SIGNATURES
    assert _soft_nms_rc(lib, 4, 3, 0.5) != 0 and b'method' in lib.mrcnn_last_error()
    assert _soft_nms_rc(lib, 4, -1, 0.5) != 0 and b'method' in lib.mrcnn_last_error()
    assert _soft_nms_rc(lib, 4, 2, -0.5) != 0 and b'sigma' in lib.mrcnn_last_error()
    assert _soft_nms_rc(lib, 4097, 1, 0.5) != 0
    assert b'n_max' in lib.mrcnn_last_error() and b'4096' in lib.mrcnn_last_error()
    buf = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    rc = lib.mrcnn_box_vote(buf, buf, buf, buf, buf, 1, 65535 * 64 + 1, 0.8, buf, None)
    assert rc != 0 and b'n_max' in lib.mrcnn_last_error()
    rc = lib.mrcnn_box_vote(buf, buf, buf, buf, buf, 1, 4, float('nan'), buf, None)
    assert rc != 0 and b'vote_thresh' in lib.mrcnn_last_error()
    rc = lib.mrcnn_box_vote(buf, buf, buf, buf, buf, -1, 4, 0.8, buf, None)
    assert rc != 0 and b'shape' in lib.mrcnn_last_error()


def test_wrapper_rejects_an_unknown_method():
    from chainer_mask_rcnn_amd.functions import proposal_ops as P
    for name, code in (('hard', 0), ('linear', 1), ('gaussian', 2)):
        assert P.soft_nms_method(name) == code and P.soft_nms_method(code) == code
    for bad in ('cubic', 3, None, True):
        with pytest.raises(ValueError):
            P.soft_nms_method(bad)


def test_model_attributes_and_unknown_method():
    import torch
    import chainer_mask_rcnn_amd as cmr
    model = cmr.models.MaskRCNNResNet(50, n_fg_class=5, min_size=64, max_size=96)
    assert model.soft_nms is None and model.bbox_vote_thresh is None
    assert (model.soft_nms_thresh, model.soft_nms_sigma, model.soft_nms_min_score) == (0.3, 0.5, 0.001)
    model.soft_nms = 'cubic'
    with pytest.raises(ValueError):
        model._suppress(torch.zeros((4, 6, 4)), torch.zeros((4, 6)))


def _tool(name, *args):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'tools', name)] + list(args),
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)


@pytest.mark.parametrize('tool', ['evaluate.py', 'demo.py'])
def test_tools_list_the_flags(tool):
    out = _tool(tool, '--help')
    assert out.returncode == 0, out.stdout
    for flag in ('--soft-nms', '--soft-nms-sigma', '--soft-nms-min-score', '--bbox-vote'):
        assert flag in out.stdout
    bad = _tool(tool, '--soft-nms', 'cubic', '--synthetic', '1', '--img', 'none.jpg')
    assert bad.returncode != 0 and 'cubic' in bad.stdout


@pytest.mark.parametrize('flags,word', [
    (['--soft-nms-sigma', '0.4'], 'without --soft-nms'),
    (['--soft-nms-min-score', '0.01', '--bbox-vote', '0.8'], 'without --soft-nms'),
    (['--soft-nms', 'linear', '--soft-nms-sigma', '0.4'], 'gaussian'),
    (['--soft-nms', 'gaussian', '--soft-nms-thresh', '0.4'], 'linear'),
    (['--soft-nms', 'gaussian', '--soft-nms-sigma', '0'], 'positive'),
    (['--results', 'r.json', '--coco-root', 'none', '--bbox-vote', '0.8'], 'results file'),
])
def test_evaluate_refuses_flags_it_would_ignore(flags, word):
    out = _tool('evaluate.py', '--synthetic', '1', *flags)
    assert out.returncode == 2 and word in out.stdout, out.stdout


def test_wrappers_check_dtypes_and_shapes_before_the_device_reads_them(monkeypatch):
    import torch
    from chainer_mask_rcnn_amd import _lib
    from chainer_mask_rcnn_amd.functions import proposal_ops as P
    monkeypatch.setattr(_lib, 'require_device', lambda *a: None)
    monkeypatch.setattr(_lib, 'call', lambda *a: pytest.fail('reached the library'))
    b, p, n = torch.zeros((2, 5, 4)), torch.zeros((2, 5)), torch.zeros((2,), dtype=torch.int32)
    k, nk = torch.zeros((2, 5), dtype=torch.int32), torch.zeros((2,), dtype=torch.int32)
    for args in ((b.double(), p, n), (b, p.half(), n), (b, p[:, :4], n), (b, p, n.long()),
                 (b[:, :, :3], p, n), (b, p, n[:1])):
        with pytest.raises(ValueError):
            P.soft_nms_sorted_batched(*args, method='linear')
    for args in ((b, p.double(), n, k, nk), (b, p, n, k.long(), nk), (b, p, n, k, nk.long()),
                 (b, p, n, k[:, :4], nk), (b, p, n.long(), k, nk)):
        with pytest.raises(ValueError):
            P.box_vote(*args)
    with pytest.raises(ValueError):
        P.soft_nms(torch.zeros((5, 4)), torch.zeros((4,)))
