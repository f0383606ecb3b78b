"""Generate tests/golden/instseg_voc.npz by running the reference's own VOC evaluation code.

The bodies of ``get_mask_overlap`` (chainer_mask_rcnn/utils/geometry.py), ``mask_iou`` and
``calc_instseg_voc_prec_rec`` (chainer_mask_rcnn/utils/evaluations/
eval_instance_segmentation_voc.py) are extracted with ``ast`` and executed in a namespace that
supplies NumPy, ``six``, ``itertools`` and ``defaultdict`` (chainer / chainercv are not needed
by these three functions).  Only inputs and outputs are stored.  ``ap`` / ``ap07`` come from the
NumPy restatement tests/instseg_eval_ref.py (chainercv's calc_detection_voc_ap is not
installable here; its hand cases are pinned in tests/test_instseg_eval_cpu.py).

    python tools/gen_instseg_golden.py /path/to/chainer-mask-rcnn
"""
import ast
import itertools
import os
import sys
from collections import defaultdict

import numpy as np
import six

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'instseg_voc.npz')


def ref_functions(ref_root):
    ns = {'np': np, 'six': six, 'defaultdict': defaultdict, 'itertools': itertools}
    for rel, names in [('chainer_mask_rcnn/utils/geometry.py', ['get_mask_overlap']),
                       ('chainer_mask_rcnn/utils/evaluations/eval_instance_segmentation_voc.py',
                        ['mask_iou', 'calc_instseg_voc_prec_rec'])]:
        path = os.path.join(ref_root, rel)
        tree = ast.parse(open(path).read())
        body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
        assert sorted(n.name for n in body) == sorted(names), (path, names)
        exec(compile(ast.Module(body=body, type_ignores=[]), path, 'exec'), ns)
    return ns['mask_iou'], ns['calc_instseg_voc_prec_rec']


def _blobs(rng, n, H, W):
    m = np.zeros((n, H, W), bool)
    for k in range(n):
        y0, x0 = rng.randint(0, H - 2), rng.randint(0, W - 2)
        y1, x1 = rng.randint(y0 + 1, H + 1), rng.randint(x0 + 1, W + 1)
        m[k, y0:y1, x0:x1] = True
        m[k] &= rng.uniform(size=(H, W)) > 0.15        # ragged interiors
    return m


def _image(rng, H, W, n_gt, n_pred, labels_gt, labels_pred, tie):
    gm = _blobs(rng, n_gt, H, W)
    gl = rng.choice(labels_gt, n_gt).astype(np.int32)
    gd = rng.uniform(size=n_gt) < 0.2
    pm = _blobs(rng, n_pred, H, W)
    pl = rng.choice(labels_pred, n_pred).astype(np.int32)
    for k in range(min(n_gt, n_pred)):                 # near-duplicates of the ground truth
        if rng.uniform() < 0.7:
            pm[k] = gm[k] ^ (rng.uniform(size=(H, W)) < rng.uniform(0, 0.4)) & gm[k]
            pl[k] = gl[k]
    ps = rng.uniform(0.05, 1, n_pred).astype(np.float32)
    if tie and n_pred > 2:
        ps[rng.randint(0, n_pred, n_pred // 2)] = np.float32(0.5)     # tied scores
    return pm, pl, ps, gm, gl, gd


def cases():
    rng = np.random.RandomState(2024)
    out = []
    # (n_img, H, W, gt labels, pred labels)
    specs = [(4, 20, 30, [0, 1, 2], [0, 1, 2]),
             (5, 24, 17, [1, 3], [1, 3, 4]),                     # class 4 only in predictions
             (3, 16, 40, [0, 2, 5], [0, 2]),                     # class 5 only in ground truth
             (6, 12, 12, [0], [0]),
             (4, 30, 25, [0, 1, 2, 3], [0, 1, 2, 3])]
    for c, (n_img, H, W, lg, lp) in enumerate(specs):
        imgs = []
        for i in range(n_img):
            if i == 1:                                           # an empty image
                n_gt, n_pred = 0, 0
            elif i == 2 and c % 2:                               # predictions only
                n_gt, n_pred = 0, rng.randint(1, 5)
            else:
                n_gt, n_pred = rng.randint(1, 7), rng.randint(0, 9)
            imgs.append(_image(rng, H, W, n_gt, n_pred, lg, lp, tie=c % 2 == 0))
        out.append(imgs)
    return out


def main():
    ref_mask_iou, ref_prec_rec = ref_functions(sys.argv[1])
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import instseg_eval_ref as R
    data = {'n_case': np.int32(len(cases()))}
    for c, imgs in enumerate(cases()):
        data['c%d/n_img' % c] = np.int32(len(imgs))
        for i, (pm, pl, ps, gm, gl, gd) in enumerate(imgs):
            for k, v in dict(pm=pm, pl=pl, ps=ps, gm=gm, gl=gl, gd=gd).items():
                data['c%d/i%d/%s' % (c, i, k)] = v
            data['c%d/i%d/iou' % (c, i)] = ref_mask_iou(pm, gm)
        cols = list(zip(*imgs))
        for use_difficult in (0, 1):
            prec, rec = ref_prec_rec(cols[0], cols[1], cols[2], cols[3], cols[4],
                                     cols[5] if use_difficult else None)
            key = 'c%d/d%d' % (c, use_difficult)
            data[key + '/n_class'] = np.int32(len(prec))
            for l in range(len(prec)):
                if prec[l] is not None:
                    data[key + '/prec%d' % l] = prec[l]
                if rec[l] is not None:
                    data[key + '/rec%d' % l] = rec[l]
            for m07 in (0, 1):
                ap = R.voc_ap(prec, rec, use_07_metric=bool(m07))
                data[key + '/ap%d' % m07] = ap
    np.savez_compressed(OUT, **data)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
