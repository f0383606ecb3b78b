"""Generate tests/golden/label_instances.npz by running the reference's own label conversions.

``label2instance_boxes`` and ``instance_boxes2label`` (chainer_mask_rcnn/utils/geometry.py) are
extracted with ``ast`` and executed in a namespace that supplies NumPy and ``collections``.
Only inputs and outputs are stored (masks bit-packed along the last axis).

    python tools/gen_label_instances_golden.py /path/to/chainer-mask-rcnn
"""
import ast
import collections
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'label_instances.npz')


def ref_functions(ref_root):
    ns = {'np': np, 'collections': collections}
    path = os.path.join(ref_root, 'chainer_mask_rcnn/utils/geometry.py')
    names = ['label2instance_boxes', 'instance_boxes2label']
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(n.name for n in body) == sorted(names), path
    exec(compile(ast.Module(body=body, type_ignores=[]), path, 'exec'), ns)
    return ns['label2instance_boxes'], ns['instance_boxes2label']


def _blobs_image(rng, H, W, ids, classes, p_noise=0.0):
    """An instance image painted with random rectangles of the given ids (later ones on top),
    and a class image that is each instance's class with some pixels of another class."""
    ins = -np.ones((H, W), np.int32)
    cls = np.zeros((H, W), np.int32)
    for i, c in zip(ids, classes):
        y0, x0 = rng.randint(0, H), rng.randint(0, W)
        y1, x1 = rng.randint(y0 + 1, H + 1), rng.randint(x0 + 1, W + 1)
        ins[y0:y1, x0:x1] = i
        cls[y0:y1, x0:x1] = c
    if p_noise:
        noise = rng.uniform(size=(H, W)) < p_noise
        cls[noise] = rng.choice(classes, noise.sum())
    return ins, cls


def cases():
    """(name, ins, cls, raw) — raw = the uint8 PNG-like pair before the datasets' preprocessing,
    or None."""
    rng = np.random.RandomState(0)
    out = []
    # majority ties: the first-seen class (row-major) wins, whatever its value
    ins = -np.ones((6, 8), np.int32)
    cls = np.zeros((6, 8), np.int32)
    ins[1:5, 1:7] = 3
    cls[1:5, 1:7] = 2
    cls[1, 1:4] = 9            # 9 is seen first ...
    cls[2:5, 1:7] = np.array([9, 2] * 9).reshape(3, 6)
    cls[1, 4:7] = 2
    ins[0, :] = 4              # a second instance: class 5 then 1, two pixels each
    cls[0, :] = [5, 5, 1, 1, 6, 6, 0, 0]
    ins[0, 7] = -1
    out.append(('tie_first_seen', ins, cls, None))
    # ties where the first-seen class has fewer pixels in the whole image
    ins = -np.ones((7, 9), np.int32)
    cls = np.zeros((7, 9), np.int32)
    ins[0, 0:4] = 1
    cls[0, 0:4] = [7, 7, 3, 3]             # 7 first, tie 2:2
    ins[2:7, :] = 2
    cls[2:7, :] = 3                        # class 3 dominates the image
    out.append(('tie_fewer_overall', ins, cls, None))
    # ids -5, 0, 7, 254 with gaps; other negatives are instances
    ins, cls = _blobs_image(rng, 40, 50, [-5, 0, 7, 254], [4, 11, 4, 200], p_noise=0.05)
    out.append(('ids_gaps', ins, cls, None))
    ins, cls = _blobs_image(rng, 30, 20, [254, 7, 0], [1, 2, 254], p_noise=0.1)
    out.append(('ids_u8', ins, cls, None))
    # single pixels and instances touching every border
    H, W = 17, 23
    ins = -np.ones((H, W), np.int32)
    cls = np.zeros((H, W), np.int32)
    ins[0, :] = 1
    ins[:, 0] = 1
    ins[H - 1, :] = 2
    ins[:, W - 1] = 2
    ins[5, 5], ins[9, 13], ins[0, W - 1], ins[H - 1, 0] = 3, 4, 5, 6
    cls[ins >= 0] = (ins[ins >= 0] * 3) % 7 + 1
    out.append(('borders_singletons', ins, cls, None))
    # no instance at all
    out.append(('empty', -np.ones((5, 7), np.int32), rng.randint(-1, 4, (5, 7)).astype(np.int32),
                None))
    # H = 1 and W = 1
    ins = np.array([[2, 2, -1, 0, 0, 0, 2, 9]], np.int32)
    cls = np.array([[1, 3, 3, 4, 4, 1, 3, 2]], np.int32)
    out.append(('h1', ins, cls, None))
    out.append(('w1', ins.T.copy(), cls.T.copy(), None))
    out.append(('1x1', np.array([[0]], np.int32), np.array([[3]], np.int32), None))
    # a 375x500 VOC-like pair: palette indices with 255 (void) borders around each object
    H, W = 375, 500
    raw_ins = np.zeros((H, W), np.uint8)
    raw_cls = np.zeros((H, W), np.uint8)
    for k in range(1, 7):
        c = rng.randint(1, 21)
        y0, x0 = rng.randint(0, H - 60), rng.randint(0, W - 60)
        y1, x1 = y0 + rng.randint(20, 60), x0 + rng.randint(20, 60)
        raw_ins[y0 - 2 if y0 >= 2 else 0:y1 + 2, x0 - 2 if x0 >= 2 else 0:x1 + 2] = 255
        raw_cls[y0 - 2 if y0 >= 2 else 0:y1 + 2, x0 - 2 if x0 >= 2 else 0:x1 + 2] = 255
        raw_ins[y0:y1, x0:x1] = k
        raw_cls[y0:y1, x0:x1] = c
    raw_cls[(raw_ins > 0) & (rng.uniform(size=(H, W)) < 0.02)] = 255   # void specks inside
    ins = raw_ins.astype(np.int32)
    cls = raw_cls.astype(np.int32)
    cls[cls == 255] = -1
    ins[ins == 255] = -1
    ins[np.isin(cls, [-1, 0])] = -1
    out.append(('voc_like', ins, cls, (raw_ins, raw_cls)))
    # the custom-dataset convention: instance 0 is background
    ins, cls = _blobs_image(rng, 48, 64, [1, 2, 3, 5], [2, 2, 7, 1], p_noise=0.08)
    ins[ins == -1] = 0
    ins[ins == 0] = -1
    out.append(('custom_ins0', ins, cls, None))
    # random multi-class instances with many near-ties
    ins, cls = _blobs_image(rng, 64, 96, list(range(12)), list(rng.randint(1, 6, 12)),
                            p_noise=0.45)
    out.append(('random_ties', ins, cls, None))
    return out


def paint_cases():
    rng = np.random.RandomState(1)
    out = []
    H, W = 24, 31
    n = 7
    masks = np.zeros((n, H, W), bool)
    for k in range(n):
        y0, x0 = rng.randint(0, H - 3), rng.randint(0, W - 3)
        masks[k, y0:y0 + rng.randint(3, 15), x0:x0 + rng.randint(3, 20)] = True
    labels = rng.randint(1, 21, n).astype(np.int32)
    bboxes = np.zeros((n, 4), np.float32)
    out.append(('overlap', labels, bboxes, masks, None))
    out.append(('scores', labels, bboxes, masks, rng.uniform(size=n).astype(np.float32)))
    out.append(('tied_scores', labels, bboxes, masks,
                np.array([0.5, 0.2, 0.5, 0.9, 0.2, 0.5, 0.1], np.float32)))
    out.append(('none', np.zeros(0, np.int32), np.zeros((0, 4), np.float32),
                np.zeros((0, 5, 6), bool), None))
    return out


def main(ref_root):
    l2i, i2l = ref_functions(ref_root)
    arrays = {}
    names = []
    for name, ins, cls, raw in cases():
        names.append(name)
        classes, boxes, masks = l2i(ins, cls, return_masks=True)
        arrays[name + '_ins'] = ins
        arrays[name + '_cls'] = cls
        arrays[name + '_classes'] = classes
        arrays[name + '_boxes'] = boxes
        arrays[name + '_masks'] = np.packbits(masks, axis=-1)
        arrays[name + '_masks_shape'] = np.array(masks.shape, np.int64)
        if raw is not None:
            arrays[name + '_raw_ins'], arrays[name + '_raw_cls'] = raw
    arrays['cases'] = np.array(names)
    pnames = []
    for name, labels, bboxes, masks, scores in paint_cases():
        pnames.append(name)
        lbl_ins, lbl_cls = i2l(labels, bboxes, masks, scores)
        arrays['paint_%s_labels' % name] = labels
        arrays['paint_%s_masks' % name] = np.packbits(masks, axis=-1)
        arrays['paint_%s_masks_shape' % name] = np.array(masks.shape, np.int64)
        if scores is not None:
            arrays['paint_%s_scores' % name] = scores
        arrays['paint_%s_lbl_ins' % name] = lbl_ins
        arrays['paint_%s_lbl_cls' % name] = lbl_cls
    arrays['paint_cases'] = np.array(pnames)
    np.savez_compressed(OUT, **arrays)
    print('wrote', OUT, len(names), 'conversion cases,', len(pnames), 'painting cases')


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
