"""Generate tests/golden/draw_instances.npz by running the reference's own draw_instance_bboxes.

The function body (chainer_mask_rcnn/utils/visualizations.py) is extracted with ``ast`` and
executed in a namespace of stated stand-ins for its dependencies, none of which is importable
here:
  - fcn.utils.labelcolormap: the PASCAL bit-interleaved colormap, float32 / 255;
  - skimage.segmentation.find_boundaries(m, connectivity=2): scipy.ndimage grey dilation !=
    grey erosion over a 3x3 footprint (mode 'reflect'), skimage's mode='thick';
    skimage.__version__ = '0.14.0' and a trivial LooseVersion;
  - cv2.rectangle: the hard-edged outline of the drawing contract (pixels within Chebyshev
    distance thickness // 2 of the rectangle, colour rounded to integers), no anti-aliasing.
Captions are None in every case.  Only inputs and outputs are stored, masks bit-packed along
the last axis.

    python tools/gen_visualize_golden.py /path/to/chainer-mask-rcnn
"""
import ast
import os
import sys
import types
import warnings

import numpy as np
import scipy.ndimage as ndi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'draw_instances.npz')


def labelcolormap(N=256):
    cmap = np.zeros((N, 3))
    for i in range(N):
        c, r, g, b = i, 0, 0, 0
        for j in range(8):
            r |= ((c >> 0) & 1) << (7 - j)
            g |= ((c >> 1) & 1) << (7 - j)
            b |= ((c >> 2) & 1) << (7 - j)
            c >>= 3
        cmap[i] = (r, g, b)
    return cmap.astype(np.float32) / 255


def find_boundaries(label_img, connectivity=1):
    m = np.asarray(label_img).astype(np.uint8)
    fp = ndi.generate_binary_structure(m.ndim, connectivity)
    return ndi.grey_dilation(m, footprint=fp) != ndi.grey_erosion(m, footprint=fp)


def rectangle(img, pt1, pt2, color, thickness=1, lineType=None):
    (x1, y1), (x2, y2) = pt1, pt2
    H, W = img.shape[:2]
    by0, by1, bx0, bx1 = min(y1, y2), max(y1, y2), min(x1, x2), max(x1, x2)
    r = thickness // 2
    yy, xx = np.mgrid[:H, :W]
    outer = (yy >= by0 - r) & (yy <= by1 + r) & (xx >= bx0 - r) & (xx <= bx1 + r)
    inner = (yy > by0 + r) & (yy < by1 - r) & (xx > bx0 + r) & (xx < bx1 - r)
    img[outer & ~inner] = np.round(np.asarray(color, np.float64)).astype(np.uint8)
    return img


class LooseVersion(object):
    def __init__(self, v):
        self.v = tuple(int(p) for p in v.split('.'))

    def __ge__(self, other):
        return self.v >= other.v


def ref_function(ref_root):
    skimage = types.SimpleNamespace(__version__='0.14.0',
                                    segmentation=types.SimpleNamespace(
                                        find_boundaries=find_boundaries))
    ns = {'np': np, 'warnings': warnings, 'LooseVersion': LooseVersion, 'skimage': skimage,
          'fcn': types.SimpleNamespace(utils=types.SimpleNamespace(labelcolormap=labelcolormap)),
          'cv2': types.SimpleNamespace(rectangle=rectangle)}
    path = os.path.join(ref_root, 'chainer_mask_rcnn/utils/visualizations.py')
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef)
            and n.name == 'draw_instance_bboxes']
    assert len(body) == 1, path
    exec(compile(ast.Module(body=body, type_ignores=[]), path, 'exec'), ns)
    return ns['draw_instance_bboxes']


def _blob(rng, H, W, box):
    """A full-frame mask: an ellipse around the box's centre that reaches past the box (the
    drawing must crop it), with some holes."""
    y1, x1, y2, x2 = box
    yy, xx = np.mgrid[:H, :W]
    cy, cx = (y1 + y2) / 2., (x1 + x2) / 2.
    ry, rx = max((y2 - y1) * 0.6, 1), max((x2 - x1) * 0.6, 1)
    m = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
    m &= rng.uniform(size=(H, W)) > 0.05
    return m


def cases():
    """(name, params, img, bboxes, labels, masks) — masks: (N, H, W) bool, a list of per-instance
    masks (box-sized or full-frame), or None."""
    rng = np.random.RandomState(0)
    out = []

    def boxes_in(H, W, n, edge=False):
        b = []
        for _ in range(n):
            y1, x1 = rng.uniform(0, H - 4), rng.uniform(0, W - 4)
            y2, x2 = rng.uniform(y1 + 2, H + 0.99), rng.uniform(x1 + 2, W + 0.99)
            b.append((y1, x1, y2, x2))
        b = np.array(b, np.float32)
        if edge:
            b[0] = (0, 0, H, 10.5)
            b[1, 2:] = (H, W)
            b[2, 1] = 0
        return b

    for k, (H, W, n, alpha, th, edge) in enumerate([
            (40, 70, 5, 0.5, 1, False), (33, 65, 8, 0.3, 2, True), (64, 130, 12, 1.0, 3, True),
            (20, 20, 3, 0.5, 1, True), (50, 129, 10, 0.5, 2, False)]):
        img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
        bboxes = boxes_in(H, W, n, edge)
        labels = rng.randint(0, 6, n).astype(np.int32)
        masks = np.stack([_blob(rng, H, W, b.astype(int)) for b in bboxes])
        draw = None
        if k % 2:
            draw = list(rng.uniform(size=n) > 0.25)
        out.append(('full%d' % k, dict(n_class=6, alpha=alpha, thickness=th, bg_class=0,
                                        draw=draw), img, bboxes, labels, masks))
    # box-sized masks, and one full-frame mask among them
    H, W = 45, 80
    img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    bboxes = boxes_in(H, W, 6)
    ib = bboxes.astype(int)
    masks = [rng.uniform(size=(b[2] - b[0], b[3] - b[1])) > 0.4 for b in ib]
    masks[3] = _blob(rng, H, W, ib[3])
    out.append(('box_sized', dict(n_class=21, alpha=0.5, thickness=1, bg_class=0, draw=None),
                img, bboxes, np.array([1, 5, 20, 7, 3, 12], np.int32), masks))
    # another background class, and no masks at all
    H, W = 30, 50
    img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    bboxes = boxes_in(H, W, 5, True)
    out.append(('no_masks', dict(n_class=4, alpha=0.5, thickness=3, bg_class=2, draw=None),
                img, bboxes, np.array([1, 2, 3, 0, 2], np.int32), None))
    masks = np.stack([_blob(rng, H, W, b.astype(int)) for b in bboxes])
    out.append(('bg_class_2', dict(n_class=4, alpha=0.7, thickness=1, bg_class=2, draw=None),
                img, bboxes, np.array([1, 2, 3, 0, 2], np.int32), masks))
    # a whole-image box and a one-pixel-wide box
    H, W = 16, 24
    img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    bboxes = np.array([[0, 0, H, W], [3, 5, 12, 6], [2.9, 7.9, 9.2, 20.7]], np.float32)
    masks = np.stack([_blob(rng, H, W, b.astype(int)) for b in bboxes])
    masks[0] = True
    out.append(('whole_and_thin', dict(n_class=3, alpha=0.5, thickness=1, bg_class=0, draw=None),
                img, bboxes, np.array([1, 2, 1], np.int32), masks))
    return out


def store_masks(arrays, key, masks):
    if masks is None:
        return
    if isinstance(masks, np.ndarray):
        arrays[key] = np.packbits(masks, axis=-1)
        arrays[key + '_shape'] = np.array(masks.shape, np.int64)
        return
    for j, m in enumerate(masks):
        arrays['%s_%d' % (key, j)] = np.packbits(m, axis=-1)
        arrays['%s_%d_shape' % (key, j)] = np.array(m.shape, np.int64)
    arrays[key + '_count'] = np.array(len(masks))


def main(ref_root):
    draw = ref_function(ref_root)
    arrays, names = {}, []
    for name, p, img, bboxes, labels, masks in cases():
        names.append(name)
        out = draw(img, bboxes, labels, p['n_class'], masks=masks, captions=None,
                   bg_class=p['bg_class'], thickness=p['thickness'], alpha=p['alpha'],
                   draw=p['draw'])
        arrays[name + '_img'] = img
        arrays[name + '_bboxes'] = bboxes
        arrays[name + '_labels'] = labels
        arrays[name + '_params'] = np.array([p['n_class'], p['alpha'], p['thickness'],
                                             p['bg_class']], np.float64)
        if p['draw'] is not None:
            arrays[name + '_draw'] = np.array(p['draw'], bool)
        store_masks(arrays, name + '_masks', masks)
        arrays[name + '_out'] = out
    arrays['cases'] = np.array(names)
    np.savez_compressed(OUT, **arrays)
    print('wrote', OUT, len(names), 'cases')


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
