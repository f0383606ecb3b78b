"""EvalRecords, Readback and the one scoring path without a device: the read-back's bytes on CPU
tensors, score_voc / score_coco against direct calls of the matching entry points, merge, and the
utility layer's independence of the extensions."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import boundary_ref as BR
import detection_eval_ref as DR
from chainer_mask_rcnn_amd.utils.evaluations import matching
from chainer_mask_rcnn_amd.utils.evaluations.records import EvalRecords, Readback
from chainer_mask_rcnn_amd.utils.evaluations.scoring import (coco_report, score_coco, score_voc,
                                                             voc_report)
from records_util import ATTRS, check_readback, readback_parts, same_lists, take

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['c%d' % i for i in range(BR.N_CLASS)]
PREFIX = {'segm': '', 'bbox': 'bbox/', 'boundary': 'boundary/'}


# ------------------------------------------------------------------------------------ Readback
def test_readback_returns_every_part_with_its_shape_and_bits():
    parts = readback_parts()
    assert [tuple(t.shape) for t in parts] == [(0, 3), (3, 0), (2, 3), (3,), (5,), (4,), (1,)]
    readback = Readback()
    slots = [readback.add(t) for t in parts]
    assert slots == [slice(i, i + 1) for i in range(len(parts))]
    host = readback.fetch()
    check_readback(parts, host)
    assert host[6][0] == 2 ** 40 and np.signbit(host[4][1]) and np.isnan(host[4][0])
    # several tensors in one call, a non-contiguous one, and a flat tensor cut into tables
    readback = Readback()
    a = torch.arange(12, dtype=torch.int32).reshape(3, 4)
    triple = readback.add(a.t(), parts[3], parts[4])
    flat = torch.arange(7, dtype=torch.float64)
    tables = readback.add_split(flat, [(0, 3), (2, 3), (1, 1), (5, 0)])
    assert (triple, tables) == (slice(0, 3), slice(3, 7))
    host = readback.fetch()
    check_readback([a.t().contiguous(), parts[3], parts[4]], host[triple])
    assert [t.shape for t in host[tables]] == [(0, 3), (2, 3), (1, 1), (5, 0)]
    assert host[4].tolist() == [[0., 1., 2.], [3., 4., 5.]] and host[5].tolist() == [[6.]]
    with pytest.raises(ValueError):
        Readback().add_split(flat, [(2, 3)])
    with pytest.raises(TypeError):
        Readback().add(torch.zeros(2, dtype=torch.float16))


def test_an_empty_readback_returns_an_empty_list(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError('an empty read-back touched torch')
    monkeypatch.setattr(torch, 'cat', refuse)
    monkeypatch.setattr(torch.Tensor, 'cpu', refuse)
    assert Readback().fetch() == []


# ------------------------------------------------------------------------------------- scoring
def _tight_boxes(masks):
    """(N, 4) float32 (y1, x1, y2, x2): each mask's tight box, zeros for an empty mask."""
    out = np.zeros((len(masks), 4), np.float32)
    for n, m in enumerate(masks):
        ys, xs = np.nonzero(m)
        if len(ys):
            out[n] = (ys.min(), xs.min(), ys.max() + 1, xs.max() + 1)
    return out


@pytest.fixture(scope='module')
def records():
    """The crafted set of test_boundary_cpu.py with all three tables, COCO and VOC."""
    data = BR.crafted_set()
    masks, bounds = BR.all_counts(data['pred_masks'], data['gt_masks'])
    boxes = [[_tight_boxes(m) for m in data[k]] for k in ('pred_masks', 'gt_masks')]
    xywh = [[DR.xywh64(b) for b in bs] for bs in boxes]
    coco_boxes = [(DR.bb_iou(d, g, c), d[:, 2] * d[:, 3], g[:, 2] * g[:, 3])
                  for d, g, c in zip(xywh[0], xywh[1], data['gt_crowdeds'])]
    voc_boxes = [DR.voc_iou(p, g) for p, g in zip(*boxes)]
    common = (data['pred_labels'], data['pred_scores'], data['gt_labels'])
    coco = EvalRecords(*common, gt_crowdeds=data['gt_crowdeds'], gt_areas=data['gt_areas'],
                       tables={'segm': masks, 'bbox': coco_boxes, 'boundary': bounds})
    voc = EvalRecords(*common, gt_difficults=data['gt_difficults'],
                      tables={'segm': masks, 'bbox': voc_boxes, 'boundary': bounds})
    return data, coco, voc


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


@pytest.mark.parametrize('iou_types', [('segm', 'bbox', 'boundary'), ('boundary',),
                                       ('bbox', 'segm')])
def test_score_coco_is_the_matching_entry_point_behind_its_prefix(records, iou_types):
    data, rec, _ = records
    t = rec.tables
    tail = (rec.pred_labels, rec.pred_scores, data['gt_labels'], data['gt_crowdeds'],
            data['gt_areas'])
    direct = {'segm': matching.coco_evaluate_from_counts(t['segm'], *tail),
              'bbox': matching.coco_evaluate_from_ious(t['bbox'], *tail),
              'boundary': matching.coco_evaluate_from_boundary_counts(
                  t['segm'], t['boundary'], *tail)}
    want = {}
    for k in iou_types:
        report = coco_report(matching.coco_results(direct[k]), NAMES)
        assert sorted(report) == sorted(['map', 'map@0.5', 'map@0.75'] + ['ap/' + n for n in NAMES])
        want.update({PREFIX[k] + key: v for key, v in report.items()})
    got = score_coco(rec, iou_types, NAMES)
    _same(got, want)
    assert len(got) == len(iou_types) * (3 + len(NAMES))
    assert all(0 < got[PREFIX[k] + 'map'] <= 1 for k in iou_types)
    assert sorted(score_coco(rec, iou_types)) == sorted(
        PREFIX[k] + key for k in iou_types for key in ('map', 'map@0.5', 'map@0.75'))


@pytest.mark.parametrize('use_07_metric', [False, True])
@pytest.mark.parametrize('iou_types', [('segm', 'bbox', 'boundary'), ('boundary',),
                                       ('bbox', 'segm')])
def test_score_voc_is_the_matching_entry_point_behind_its_prefix(records, iou_types,
                                                                 use_07_metric):
    data, _, rec = records
    t = rec.tables
    tail = (rec.pred_labels, rec.pred_scores, data['gt_labels'], data['gt_difficults'])
    direct = {'segm': matching.voc_prec_rec_from_counts(t['segm'], *tail),
              'bbox': matching.voc_prec_rec_from_ious(t['bbox'], *tail),
              'boundary': matching.voc_prec_rec_from_boundary_counts(
                  t['segm'], t['boundary'], *tail)}
    want = {}
    for k in iou_types:
        ap = matching.calc_detection_voc_ap(*direct[k], use_07_metric=use_07_metric)
        report = voc_report(ap, NAMES)
        assert sorted(report) == sorted(['map'] + ['ap/' + n for n in NAMES])
        want.update({PREFIX[k] + key: v for key, v in report.items()})
    got = score_voc(rec, iou_types, use_07_metric, NAMES)
    _same(got, want)
    assert len(got) == len(iou_types) * (1 + len(NAMES))
    assert all(0 < got[PREFIX[k] + 'map'] <= 1 for k in iou_types)


def test_a_requested_type_without_its_table_is_refused(records):
    _, rec, _ = records
    rec.require(('segm', 'bbox', 'boundary'))
    boundary_only = EvalRecords(rec.pred_labels, rec.pred_scores, rec.gt_labels,
                                tables={'boundary': rec.tables['boundary']})
    for tables, iou_types, match in (
            ({'segm': rec.tables['segm']}, ('segm', 'bbox'), 'box IoU'),
            ({'segm': rec.tables['segm']}, ('boundary',), 'boundary'),
            ({'bbox': rec.tables['bbox']}, ('segm',), 'mask counts'),
            (boundary_only.tables, ('boundary',), 'mask counts')):
        with pytest.raises(ValueError, match=match):
            EvalRecords(rec.pred_labels, rec.pred_scores, rec.gt_labels,
                        tables=tables).require(iou_types)


# --------------------------------------------------------------------------------------- merge
def test_merge_keeps_the_order_and_refuses_records_that_differ(records):
    _, rec, voc = records
    n = len(rec)
    assert n >= 4 and set(vars(rec)) == ATTRS
    parts = [take(rec, 0, 1), take(rec, 1, 1), take(rec, 1, 3), take(rec, 3, None)]
    assert [len(p) for p in parts] == [1, 0, 2, n - 3]
    m = EvalRecords.merge(parts)
    for k in ATTRS - {'tables', 'gt_difficults'}:
        assert same_lists(getattr(m, k), getattr(rec, k)), k
    assert m.gt_difficults is None and set(m.tables) == set(rec.tables)
    for k in rec.tables:
        assert same_lists(m.tables[k], rec.tables[k]), k
    swapped = EvalRecords.merge([parts[3], parts[0]])
    assert same_lists(swapped.gt_labels, rec.gt_labels[3:] + rec.gt_labels[:1])
    assert same_lists(swapped.tables['bbox'], rec.tables['bbox'][3:] + rec.tables['bbox'][:1])
    empty = EvalRecords.merge([])
    assert len(empty) == 0 and empty.tables == {}
    assert (empty.pred_labels, empty.pred_scores, empty.gt_labels) == ([], [], [])
    assert empty.gt_difficults is empty.gt_crowdeds is empty.gt_areas is None
    fewer = take(rec, 0, 2)
    del fewer.tables['bbox']
    flagless = EvalRecords(rec.pred_labels, rec.pred_scores, rec.gt_labels, tables=rec.tables)
    for other in (fewer, flagless, voc):                # tables, crowds and areas, difficults
        for pair in ([rec, other], [other, rec]):
            with pytest.raises(ValueError):
                EvalRecords.merge(pair)
    with pytest.raises(ValueError):                     # a list of another length
        EvalRecords(rec.pred_labels, rec.pred_scores, rec.gt_labels[:-1])
    back = pickle.loads(pickle.dumps(rec))
    assert set(vars(back)) == ATTRS and set(back.tables) == set(rec.tables) and len(back) == n
    _same(score_coco(back, ('segm', 'bbox', 'boundary'), NAMES),
          score_coco(rec, ('segm', 'bbox', 'boundary'), NAMES))


# -------------------------------------------------------------------------------------- layers
def test_the_utility_layer_does_not_import_the_extensions():
    """In a fresh interpreter, importing coco_results leaves the evaluators' module out of
    sys.modules.  The package's own __init__ imports every subpackage, extensions included, so
    the child stands a bare package module in its place: what is imported then is what the
    utility layer itself asks for."""
    code = ('import os, sys, types\n'
            'pkg = types.ModuleType("chainer_mask_rcnn_amd")\n'
            'pkg.__path__ = [os.path.join(%r, "chainer_mask_rcnn_amd")]\n'
            'sys.modules["chainer_mask_rcnn_amd"] = pkg\n'
            'import chainer_mask_rcnn_amd.utils.evaluations.coco_results as CR\n'
            'assert callable(CR.eval_coco_results)\n'
            'bad = [m for m in sys.modules if m.startswith("chainer_mask_rcnn_amd.extensions")]\n'
            'assert not bad, bad\n'
            'assert "chainer_mask_rcnn_amd.utils.evaluations.scoring" in sys.modules\n' % ROOT)
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
