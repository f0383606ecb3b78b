"""Host matching and accumulation of the instance-segmentation evaluations (no GPU: counts are
computed with NumPy) against the reference's own VOC code (tests/golden/instseg_voc.npz, made by
tools/gen_instseg_golden.py), the NumPy restatement tests/instseg_eval_ref.py, and hand-worked
answers; ABI argument rejection and register use of the new kernels."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import instseg_eval_ref as R
from chainer_mask_rcnn_amd.utils.evaluations import matching
from chainer_mask_rcnn_amd.extensions import instance_segmentation_evaluators as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'chainer_mask_rcnn_amd', 'csrc')


def load_voc_cases(golden_dir):
    d = np.load(os.path.join(golden_dir, 'instseg_voc.npz'))
    out = []
    for c in range(int(d['n_case'])):
        imgs = [tuple(d['c%d/i%d/%s' % (c, i, k)] for k in ('pm', 'pl', 'ps', 'gm', 'gl', 'gd'))
                for i in range(int(d['c%d/n_img' % c]))]
        exp = {}
        for dif in (0, 1):
            key = 'c%d/d%d' % (c, dif)
            n = int(d[key + '/n_class'])
            prec = [d[key + '/prec%d' % l] if key + '/prec%d' % l in d else None for l in range(n)]
            rec = [d[key + '/rec%d' % l] if key + '/rec%d' % l in d else None for l in range(n)]
            exp[dif] = (prec, rec, d[key + '/ap0'], d[key + '/ap1'])
        ious = [d['c%d/i%d/iou' % (c, i)] for i in range(len(imgs))]
        out.append((imgs, exp, ious))
    return out


def counts_of(pms, gms):
    return R.coco_counts(pms, gms)


def _same_list(got, exp):
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        if e is None:
            assert g is None
        else:
            assert g is not None and g.shape == e.shape
            assert np.array_equal(g, e, equal_nan=True)


# ------------------------------------------------------------------------- VOC vs fixture
@pytest.mark.parametrize('use_difficult', [0, 1])
def test_voc_matching_equals_reference_fixture(golden_dir, use_difficult):
    for imgs, exp, ious in load_voc_cases(golden_dir):
        pm, pl, ps, gm, gl, gd = zip(*imgs)
        counts = counts_of(pm, gm)
        for (inter, a, b), iou in zip(counts, ious):
            # the float64 IoU of the counts is the reference's 1.0 * intersect / union
            assert np.array_equal(matching.iou_from_counts(inter, a, b), iou)
        prec, rec = matching.voc_prec_rec_from_counts(counts, pl, ps, gl,
                                                      gd if use_difficult else None)
        e_prec, e_rec, ap0, ap1 = exp[use_difficult]
        _same_list(prec, e_prec)
        _same_list(rec, e_rec)
        for m07, e_ap in ((False, ap0), (True, ap1)):
            ap = matching.calc_detection_voc_ap(prec, rec, use_07_metric=m07)
            assert np.array_equal(ap, e_ap, equal_nan=True)
            assert np.array_equal(np.nanmean(ap), np.nanmean(e_ap), equal_nan=True)


def test_voc_matching_equals_restatement(golden_dir):
    for imgs, exp, _ in load_voc_cases(golden_dir):
        pm, pl, ps, gm, gl, gd = zip(*imgs)
        prec, rec = matching.voc_prec_rec_from_counts(counts_of(pm, gm), pl, ps, gl, gd)
        r_prec, r_rec = R.voc_prec_rec(pm, pl, ps, gm, gl, gd)
        _same_list(prec, r_prec)
        _same_list(rec, r_rec)


# ------------------------------------------------------------------------ COCO vs restatement
def _coco_case(seed, n_img=5, H=48, W=64, crowd=True, areas=True):
    rng = np.random.RandomState(seed)
    pms, pls, pss, gms, gls, gcs, gas = [], [], [], [], [], [], []
    for i in range(n_img):
        G = 0 if i == 1 else rng.randint(1, 6)
        P = rng.randint(0, 12)
        gm = np.zeros((G, H, W), bool)
        for k in range(G):
            s = rng.choice([4, 8, 20, 40])
            y0, x0 = rng.randint(0, H - 2), rng.randint(0, W - 2)
            gm[k, y0:y0 + s, x0:x0 + s + rng.randint(0, 5)] = True
        pm = np.zeros((P, H, W), bool)
        for k in range(P):
            if G and rng.uniform() < 0.7:
                pm[k] = gm[rng.randint(G)] & (rng.uniform(size=(H, W)) > rng.uniform(0, 0.5))
            else:
                s = rng.choice([3, 10, 30])
                y0, x0 = rng.randint(0, H - 2), rng.randint(0, W - 2)
                pm[k, y0:y0 + s, x0:x0 + s] = True
        gl = rng.randint(0, 4, G).astype(np.int32)
        pl = rng.randint(0, 5, P).astype(np.int32)
        ps = rng.uniform(0, 1, P).astype(np.float32)
        if P > 3:
            ps[:2] = ps[2]                                       # ties
        pms.append(pm); pls.append(pl); pss.append(ps); gms.append(gm); gls.append(gl)
        gcs.append((rng.uniform(size=G) < 0.25).astype(np.int32))
        gas.append((gm.sum((1, 2)) * rng.uniform(0.8, 1.2, G)).astype(np.float32))
    return pms, pls, pss, gms, gls, (gcs if crowd else None), (gas if areas else None)


def _coco_check(case):
    pms, pls, pss, gms, gls, gcs, gas = case
    ev = matching.coco_evaluate_from_counts(counts_of(pms, gms), pls, pss, gls, gcs, gas)
    precision, recall, cat_ids = R.coco_eval(pms, pls, pss, gms, gls, gcs, gas)
    assert ev['params']['catIds'] == cat_ids
    assert np.array_equal(ev['precision'], precision)
    assert np.array_equal(ev['recall'], recall)
    got = matching.coco_results(ev)
    exp = R.coco_summary(precision, recall)
    assert set(got) == set(exp) | {'coco_eval'}
    for k, v in exp.items():
        assert np.array_equal(np.asarray(got[k]), np.asarray(v), equal_nan=True), k
        assert np.asarray(got[k]).dtype == np.asarray(v).dtype, k
    return got


@pytest.mark.parametrize('seed', [0, 1, 2, 3])
def test_coco_equals_restatement(seed):
    _coco_check(_coco_case(seed, crowd=seed != 1, areas=seed != 2))


def test_coco_equals_restatement_many_detections():
    # more than 100 detections of one class in an image: maxDets truncation
    rng = np.random.RandomState(7)
    H = W = 20
    gm = np.zeros((3, H, W), bool)
    gm[0, :5, :5] = gm[1, 5:15, 5:15] = gm[2, 12:, 12:] = True
    pm = rng.uniform(size=(130, H, W)) < 0.05
    pm[:20] |= gm[rng.randint(0, 3, 20)]
    ps = rng.uniform(size=130).astype(np.float32)
    _coco_check(([pm], [np.zeros(130, np.int32)], [ps], [gm], [np.zeros(3, np.int32)], None, None))


# --------------------------------------------------------------------------- hand answers
def _voc(pred_masks, pred_labels, pred_scores, gt_masks, gt_labels, use_07_metric=False):
    prec, rec = matching.voc_prec_rec_from_counts(counts_of(pred_masks, gt_masks), pred_labels,
                                                  pred_scores, gt_labels)
    return matching.calc_detection_voc_ap(prec, rec, use_07_metric=use_07_metric)


def _coco(pred_masks, pred_labels, pred_scores, gt_masks, gt_labels, gt_crowdeds=None,
          gt_areas=None):
    return matching.coco_results(matching.coco_evaluate_from_counts(
        counts_of(pred_masks, gt_masks), pred_labels, pred_scores, gt_labels, gt_crowdeds,
        gt_areas))


def _square(H, W, y, x, s):
    m = np.zeros((H, W), bool)
    m[y:y + s, x:x + s] = True
    return m


def test_perfect_detection_gives_ap_one():
    g = np.stack([_square(40, 40, 2, 2, 10), _square(40, 40, 20, 20, 12)])
    l = np.array([0, 1], np.int32)
    s = np.array([0.9, 0.8], np.float32)
    for m07 in (False, True):
        assert np.allclose(_voc([g], [l], [s], [g], [l], m07), [1., 1.])
    r = _coco([g], [l], [s], [g], [l])
    assert r['map/iou=0.50:0.95/area=all/maxDets=100'] == 1.
    assert r['mar/iou=0.50:0.95/area=all/maxDets=100'] == 1.


def test_false_positive_ranked_first_voc():
    g = _square(30, 30, 0, 0, 10)[None]
    fp = _square(30, 30, 20, 20, 5)
    p = np.stack([fp, g[0]])
    s = np.array([0.9, 0.5], np.float32)
    l0, l1 = np.zeros(2, np.int32), np.zeros(1, np.int32)
    # prec = [0, 1/2], rec = [0, 1]
    # area under the envelope: recall 0 -> 1 at precision 1/2
    assert _voc([p], [l0], [s], [g], [l1])[0] == 0.5
    # 11-point: every threshold t in 0..1 sees max precision 1/2 -> 11 * (0.5 / 11)
    exp07 = 0.
    for _ in range(11):
        exp07 += 0.5 / 11
    assert _voc([p], [l0], [s], [g], [l1], True)[0] == exp07


def _iou_exact(H, W, inter, union_extra):
    """gt of `inter + union_extra` pixels in row 0..; prediction = first `inter` of them."""
    g = np.zeros((H, W), bool)
    g.flat[:inter + union_extra] = True
    p = np.zeros((H, W), bool)
    p.flat[:inter] = True
    return p, g


@pytest.mark.parametrize('inter,extra,thr_index', [(75, 25, 5), (90, 10, 8)])
def test_iou_exactly_at_threshold_counts(inter, extra, thr_index):
    # IoU 0.75 == iouThrs[5]; IoU 0.9 >= iouThrs[8] = 0.8999999999999999
    p, g = _iou_exact(20, 20, inter, extra)
    assert inter / (inter + extra) >= matching.coco_params()['iouThrs'][thr_index]
    ev = matching.coco_evaluate_from_counts(counts_of([p[None]], [g[None]]), [np.zeros(1, np.int32)],
                                            [np.ones(1, np.float32)], [np.zeros(1, np.int32)])
    rec = ev['recall'][:, 0, 0, 2]
    assert np.all(rec[:thr_index + 1] == 1) and np.all(rec[thr_index + 1:] == 0)
    if thr_index == 5:
        r = matching.coco_results(ev)
        assert r['map/iou=0.75/area=all/maxDets=100'] == 1.


def test_detection_on_crowd_is_ignored_not_false_positive():
    H = W = 40
    g = np.stack([_square(H, W, 0, 0, 10), _square(H, W, 20, 20, 15)])
    p = np.stack([_square(H, W, 0, 0, 10), _square(H, W, 22, 22, 6)])   # 2nd inside the crowd
    s = np.array([0.5, 0.9], np.float32)                                  # crowd match ranked first
    l = np.zeros(2, np.int32)
    crowd = [np.array([0, 1], np.int32)]
    r = _coco([p], [l], [s], [g], [l], crowd)
    assert r['map/iou=0.50/area=all/maxDets=100'] == 1.
    r_no = _coco([p], [l], [s], [g], [l], [np.zeros(2, np.int32)])
    assert r_no['map/iou=0.50/area=all/maxDets=100'] < 1.


def test_area_boundary_32_squared_is_small_and_medium():
    g = _square(64, 64, 0, 0, 32)[None]                  # exactly 1024 pixels
    l = np.zeros(1, np.int32)
    r = _coco([g], [l], [np.ones(1, np.float32)], [g], [l])
    assert r['map/iou=0.50:0.95/area=small/maxDets=100'] == 1.
    assert r['map/iou=0.50:0.95/area=medium/maxDets=100'] == 1.
    assert np.isnan(r['map/iou=0.50:0.95/area=large/maxDets=100'])


def test_max_dets_one_counts_only_the_top_detection():
    H = W = 40
    g = np.stack([_square(H, W, 0, 0, 10), _square(H, W, 20, 20, 10)])
    l = np.zeros(2, np.int32)
    s = np.array([0.3, 0.9], np.float32)
    r = _coco([g], [l], [s], [g], [l])
    assert r['mar/iou=0.50:0.95/area=all/maxDets=1'] == 0.5
    assert r['mar/iou=0.50:0.95/area=all/maxDets=10'] == 1.


def test_absent_class_keys_land_on_the_right_names():
    H = W = 30
    g = np.stack([_square(H, W, 0, 0, 10), _square(H, W, 15, 15, 10)])
    gl = np.array([0, 2], np.int32)                      # class 1 never occurs
    p = g.copy()
    pl = gl.copy()
    s = np.array([0.9, 0.8], np.float32)
    # class 2 detected perfectly, class 0 missed
    p[0] = _square(H, W, 20, 0, 5)
    r = _coco([p], [pl], [s], [g], [gl])
    rep = E.coco_report(r, ['a', 'b', 'c'])
    assert rep['ap/c'] == 1. and rep['ap/a'] == 0. and np.isnan(rep['ap/b'])
    ap = _voc([p], [pl], [s], [g], [gl])
    rep = E.voc_report(ap, ['a', 'b', 'c', 'd'])
    assert rep['ap/c'] == 1. and rep['ap/a'] == 0. and np.isnan(rep['ap/b']) and np.isnan(rep['ap/d'])


def test_calc_detection_voc_ap_hand_cases():
    prec = [np.array([1., 1., 2 / 3.]), None, np.array([0., 0.5, 2 / 3., 0.5]),
            np.array([np.nan, 1.])]
    rec = [np.array([0.5, 1., 1.]), np.array([0.]), np.array([0., 0.5, 1., 1.]),
           np.array([0., 1.])]
    ap = matching.calc_detection_voc_ap(prec, rec)
    assert ap[0] == 1. and np.isnan(ap[1]) and ap[3] == 1.
    # envelope: precision 2/3 over recall (0, 1]
    assert ap[2] == 0.5 * (2 / 3.) + 0.5 * (2 / 3.)
    ap07 = matching.calc_detection_voc_ap(prec, rec, use_07_metric=True)
    assert np.isclose(ap07[0], 1.) and np.isnan(ap07[1]) and np.isclose(ap07[2], 2 / 3.)
    # recall never reaches 0.6: thresholds 0.6..1.0 contribute 0
    ap07b = matching.calc_detection_voc_ap([np.array([1.])], [np.array([0.5])], use_07_metric=True)
    assert np.isclose(ap07b[0], 6 / 11.)


# -------------------------------------------------------------------- ABI and kernel resources
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from chainer_mask_rcnn_amd import _lib
    return _lib.load()


def test_abi_rejects_bad_arguments(lib):
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lambda: lib.mrcnn_last_error()
    assert lib.mrcnn_mask_pack(p, 2, 1, 4, 4, p, p, p, None) != 0 and b'elem_bytes' in err()
    assert lib.mrcnn_mask_pack(p, 1, 1, 0, 4, p, p, p, None) != 0 and b'bad shape' in err()
    assert lib.mrcnn_mask_pack(p, 1, -1, 4, 4, p, p, p, None) != 0 and b'bad shape' in err()
    assert lib.mrcnn_mask_pack(p, 1, 1, 65536, 32768, p, p, p, None) != 0 and b'2^31' in err()
    assert lib.mrcnn_mask_pack(None, 1, 1, 4, 4, p, p, p, None) != 0 and b'null' in err()
    assert lib.mrcnn_mask_pack(p, 1, 1 << 20, 4096, 4, p, p, p, None) != 0 and b'grid' in err()
    assert lib.mrcnn_mask_pack(None, 1, 0, 4, 4, None, None, None, None) == 0   # nothing to do
    assert lib.mrcnn_paste_masks_packed(p, p, p, 1, 0, 81, 4, 4, p, p, p, None) != 0
    assert b'bad shape' in err()
    assert lib.mrcnn_paste_masks_packed(p, p, p, 1, 14, 81, 65536, 32768, p, p, p, None) != 0
    assert b'2^31' in err()
    assert lib.mrcnn_paste_masks_packed(p, None, p, 1, 14, 81, 4, 4, p, p, p, None) != 0
    assert b'null' in err()
    assert lib.mrcnn_paste_masks_packed(p, p, p, 1 << 20, 14, 81, 4096, 4, p, p, p, None) != 0
    assert b'grid' in err()
    assert lib.mrcnn_mask_intersect(p, p, 1, p, p, 1, 0, 4, p, None) != 0 and b'bad shape' in err()
    assert lib.mrcnn_mask_intersect(p, p, 1, p, p, -1, 4, 4, p, None) != 0 and b'bad shape' in err()
    assert lib.mrcnn_mask_intersect(p, p, 1, p, p, 1, 65536, 32768, p, None) != 0 and b'2^31' in err()
    assert lib.mrcnn_mask_intersect(p, None, 1, p, p, 1, 4, 4, p, None) != 0 and b'null' in err()
    assert lib.mrcnn_mask_intersect(p, p, 1 << 20, p, p, 1 << 14, 4, 4, p, None) != 0
    assert b'grid' in err()
    assert lib.mrcnn_abi_version() == 1


def _resources(src):
    cmd = ['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC',
           '-I' + os.path.join(ROOT, 'include'), '-I' + CSRC, '-ffp-contract=off',
           '-Rpass-analysis=kernel-resource-usage', '-c', os.path.join(CSRC, src), '-o', os.devnull]
    err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    res, name = {}, None
    for line in err.splitlines():
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            name = m.group(1)
            res[name] = {}
            continue
        m = re.search(r'remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)', line)
        if m and name:
            res[name][m.group(1).strip()] = int(m.group(2))
    return res


def test_mask_kernels_use_no_scratch():
    """Every kernel of mask_eval.hip and the packed paste keep their registers."""
    res = _resources('mask_eval.hip')
    for k in ('pack_init_kernel', 'pack_kernel', 'intersect_kernel'):
        assert any(k in n for n in res), k
    img = _resources('image.hip')
    res.update({n: v for n, v in img.items() if 'paste' in n})
    assert any('paste_packed_kernel' in n for n in res)
    for n, v in res.items():
        assert v.get('ScratchSize', 0) == 0 and v.get('VGPRs Spill', 0) == 0, (n, v)
