"""COCO instance-segmentation dataset — same class name, constructor, example layout and
annotation handling as the reference's
/root/reference/chainer_mask_rcnn/datasets/coco.py:18-183, without its
third-party readers: the annotation index that ``pycocotools.coco.COCO`` builds is built here
from the JSON directly, COCO run-length masks (``pycocotools.mask.frPyObjects`` / ``decode``)
are decoded by ``rle_decode`` below, images are read with Pillow (the reference uses
``skimage.io.imread``, which returns the same RGB uint8 array for JPEG files).  Polygons are
rasterised with ``PIL.ImageDraw`` exactly as the reference does (:136-143); ``polygon_rule='coco'``
draws them by COCO's own rule instead (``polygon_to_mask_coco``), and
``device_polygons=True`` hands the vertices on as a ``datasets.PolygonMasks`` for the device to draw.

    dataset[i] -> img (H,W,3) uint8 RGB, bboxes (G,4) f32 (y1,x1,y2,x2), labels (G,) i32,
                  masks (G,H,W) i32 {0,1} [, crowds (G,) i32] [, areas (G,) f32]

With ``packed_masks=True`` the mask field is a ``datasets.PackedMasks`` of the same rasters (bits,
1/256 of the int32 stack, which is then never built); ``unpack()`` gives the array above.

This is what ``datasets.MaskRCNNTransform`` consumes (datasets/transforms.py:10-51).
There is no network here: the data must already be under ``root_dir``.
"""
import json
import os.path as osp

import numpy as np

from .packed_masks import PackedMasks


def rle_counts_from_string(s):
    """COCO's compressed RLE string -> run lengths (pycocotools maskApi.c rleFrString): 5 data
    bits per character (offset 48), bit 5 = continuation, sign-extended, and from the third
    run on each value is a difference to the run two places back."""
    if isinstance(s, str):
        s = s.encode('ascii')
    counts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = s[p] - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def rle_decode(segmentation, height, width):
    """{'counts': list | str | bytes, 'size': [h, w]} -> (h, w) uint8 mask
    (pycocotools.mask.frPyObjects + decode: runs alternate 0 / 1 in COLUMN-major order)."""
    h, w = segmentation['size']
    counts = segmentation['counts']
    if not isinstance(counts, (list, tuple)):
        counts = rle_counts_from_string(counts)
    flat = np.zeros(h * w, dtype=np.uint8)
    pos, v = 0, 0
    for c in counts:
        if v:
            flat[pos:pos + c] = 1
        pos += c
        v ^= 1
    return flat.reshape((w, h)).T


def mask_to_bbox(mask):
    """utils/geometry.py:150-166: (y1, x1, y2, x2) of the non-zero pixels (raises on an empty
    mask, as the reference does)."""
    where = np.argwhere(mask)
    (y1, x1), (y2, x2) = where.min(0), where.max(0) + 1
    return y1, x1, y2, x2


# ---- COCO's polygon rule on the host (pycocotools maskApi.c rleFrPoly) ----
# The device draws the same rule (csrc/polygon_raster.hip); this is the CPU-only route and the
# source of the dataset's exact boxes.  NumPy's float64 multiply and adds are never fused, which
# the rule depends on.
POLYGON_SCALE = 5.0
_WALK_CHUNK = 1 << 20       # points of one edge handled at a time


def upsample_ring(ring):
    """One ring ``[x0, y0, x1, y1, ...]`` (or (k, 2)) -> (k, 2) int64 ``(int)(5.0 * c + .5)``, the
    cast truncating towards zero as C's does.  ValueError unless the coordinates are an even number
    of finite values with ``|5 c| < 2^30``."""
    a = np.asarray(ring, dtype=np.float64).reshape(-1)
    if a.size % 2:
        raise ValueError('polygon ring: the number of coordinates must be even, got %d' % a.size)
    if not np.isfinite(a).all():
        raise ValueError('polygon ring: every coordinate must be finite')
    if (np.abs(POLYGON_SCALE * a) >= 2.0 ** 30).any():
        raise ValueError('polygon ring: |5 * coordinate| must be below 2^30')
    return np.trunc(POLYGON_SCALE * a + .5).astype(np.int64).reshape(-1, 2)


def ring_crossings(xy5, h, w):
    """The crossings ``(x, y)`` (two int64 arrays) of one upsampled ring on an ``h x w`` image, in
    no particular order: ``0 <= x < w``, ``0 <= y <= h`` (``y == h`` touches no pixel).  One
    vectorised walk per edge; a ring of fewer than 3 vertices has none."""
    xs_out, ys_out = [], []
    k = len(xy5)
    for j in range(k if k >= 3 else 0):
        (xs, ys), (xe, ye) = (int(c) for c in xy5[j]), (int(c) for c in xy5[(j + 1) % k])
        dx, dy = abs(xe - xs), abs(ye - ys)
        if (dx >= dy and xs > xe) or (dx < dy and ys > ye):     # flip: the same points, met in
            xs, xe, ys, ye = xe, xs, ye, ys                     # the other order
            flip = True
        else:
            flip = False
        n = max(dx, dy)
        if n == 0:
            continue
        s = (ye - ys) / dx if dx >= dy else (xe - xs) / dy
        for a in range(0, n, _WALK_CHUNK):
            ti = np.arange(a, min(a + _WALK_CHUNK, n) + 1, dtype=np.int64)
            t = ti.astype(np.float64)
            if dx >= dy:
                u, v = ti + xs, np.trunc(ys + s * t + .5).astype(np.int64)
            else:
                v, u = ti + ys, np.trunc(xs + s * t + .5).astype(np.int64)
            if flip:
                u, v = u[::-1], v[::-1]
            ch = np.flatnonzero(u[1:] != u[:-1]) + 1
            if not ch.size:
                continue
            xd = np.where(u[ch] < u[ch - 1], u[ch], u[ch] - 1).astype(np.float64)
            xd = (xd + .5) / POLYGON_SCALE - .5
            keep = (np.floor(xd) == xd) & (xd >= 0) & (xd <= w - 1)
            yd = np.minimum(v[ch], v[ch - 1]).astype(np.float64)
            yd = np.ceil(np.clip((yd + .5) / POLYGON_SCALE - .5, 0., float(h)))
            xs_out.append(xd[keep].astype(np.int64))
            ys_out.append(yd[keep].astype(np.int64))
    if not xs_out:
        return np.zeros((0,), np.int64), np.zeros((0,), np.int64)
    return np.concatenate(xs_out), np.concatenate(ys_out)


def _fill_ring(xy5, h, w):
    """Even-odd fill of one ring: pixel (y, x) is set iff an odd number of its crossings (x, y')
    have y' <= y."""
    x, y = ring_crossings(xy5, h, w)
    inside = y < h
    toggles = np.bincount(y[inside] * w + x[inside], minlength=h * w).reshape(h, w) & 1
    return np.bitwise_xor.accumulate(toggles.astype(np.uint8), axis=0).astype(bool)


def polygon_to_mask_coco(rings, h, w):
    """COCO's own polygon rule (``pycocotools.mask.frPyObjects`` + ``merge`` + ``decode``): a list
    of rings ``[x0, y0, x1, y1, ...]`` -> (h, w) bool mask, the UNION of the rings, each ring
    filled even-odd.  Not PIL's rule: the square [1,1, 4,1, 4,4, 1,4] is pixels 1..3 here and
    1..4 under ``PIL.ImageDraw.polygon(outline=1, fill=1)``."""
    h, w = int(h), int(w)
    mask = np.zeros((h, w), bool)
    for ring in rings:
        mask |= _fill_ring(upsample_ring(ring), h, w)
    return mask


def _ring_box(xy5, h, w):
    """Tight (y1, x1, y2, x2) of one ring's fill from its crossings alone, or None when the ring
    sets nothing.  Equal crossings cancel; in a column the rest, sorted, open and close runs in
    turn (a run left open ends at h)."""
    x, y = ring_crossings(xy5, h, w)
    key, count = np.unique(x * (h + 1) + y, return_counts=True)
    key = key[(count & 1) == 1]
    if not key.size:
        return None
    cx, cy = key // (h + 1), key % (h + 1)
    cols, start, per = np.unique(cx, return_index=True, return_counts=True)
    first, last = cy[start], np.where(per & 1, h, cy[start + per - 1])
    ok = first < last
    if not ok.any():
        return None
    return (int(first[ok].min()), int(cols[ok].min()), int(last[ok].max()), int(cols[ok].max()) + 1)


def polygon_box_coco(rings, h, w):
    """Tight (y1, x1, y2, x2) of ``polygon_to_mask_coco(rings, h, w)`` without filling it — the
    hull of the non-empty rings' boxes — or (0, 0, 0, 0) when no pixel is set (the device's
    convention; ``mask_to_bbox`` raises there)."""
    boxes = [b for b in (_ring_box(upsample_ring(r), int(h), int(w)) for r in rings) if b is not None]
    if not boxes:
        return 0, 0, 0, 0
    b = np.asarray(boxes)
    return int(b[:, 0].min()), int(b[:, 1].min()), int(b[:, 2].max()), int(b[:, 3].max())


class COCOInstanceSegmentationDataset(object):

    class_names = None  # initialized by __init__
    root_dir = osp.expanduser('~/data/datasets/COCO')

    def __init__(self, split, use_crowd=False, return_crowd=False, return_area=False,
                 root_dir=None, packed_masks=False, polygon_rule='pil', device_polygons=False):
        if polygon_rule not in ('pil', 'coco'):
            raise ValueError("polygon_rule must be 'pil' or 'coco', got %r" % (polygon_rule,))
        if device_polygons and polygon_rule != 'coco':
            raise ValueError("device_polygons=True requires polygon_rule='coco' (the device draws "
                             "COCO's rule only)")
        if root_dir is not None:
            self.root_dir = root_dir
        test_dev = split == 'test-dev'
        if split == 'train':
            split = split + '2014'
            data_type = 'train2014'
        elif split in ['val', 'minival', 'valminusminival']:
            split = split + '2014'
            data_type = 'val2014'
        elif test_dev:
            data_type = 'test2015'
        else:
            raise ValueError
        if test_dev:
            # no public annotations: the image list (with categories) of the test-dev server
            ann_file = osp.join(self.root_dir, 'annotations/image_info_test-dev2015.json')
        else:
            ann_file = osp.join(self.root_dir, 'annotations/instances_%s.json' % split)
        if not osp.exists(ann_file):
            raise IOError('%s not found; the reference downloads it (coco.py:24-50), this '
                          'build has no network access: place the data there' % ann_file)
        self._use_crowd = use_crowd
        self._return_crowd = return_crowd
        self._return_area = return_area
        self._packed_masks = packed_masks
        self._polygon_rule = polygon_rule
        self._device_polygons = bool(device_polygons)

        with open(ann_file) as f:
            data = json.load(f)
        # the index pycocotools.coco.COCO.createIndex builds
        self._anns_of_img = {}
        for ann in data.get('annotations', []):
            self._anns_of_img.setdefault(ann['image_id'], []).append(ann)
        self.img_fname = osp.join(self.root_dir, data_type, 'COCO_%s_{:012}.jpg' % data_type)

        # set class_names (:83-94)
        cat_id_to_class_id = {}
        class_names = []
        for cat in sorted(data.get('categories', []), key=lambda x: x['id']):
            cat_id_to_class_id[cat['id']] = len(class_names)
            class_names.append(cat['name'])
        class_names = np.asarray(class_names)
        class_names.setflags(write=0)
        self.cat_id_to_class_id = cat_id_to_class_id
        self.class_id_to_cat_id = {c: cat for cat, c in cat_id_to_class_id.items()}
        self.class_names = class_names
        # (height, width) of every listed image, as the JSON gives it
        self.img_sizes = {img['id']: (int(img['height']), int(img['width']))
                          for img in data.get('images', [])}

        # filter images without any annotations (:96-102); test-dev keeps every listed image
        self.img_ids = [img['id'] for img in data.get('images', [])
                        if test_dev or len(self._anns_of_img.get(img['id'], [])) >= 1]

    def __len__(self):
        return len(self.img_ids)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self.get_example(j) for j in range(*i.indices(len(self)))]
        return self.get_example(i)

    def get_example(self, i):
        import PIL.Image
        img_id = self.img_ids[i]
        # Every file ends up as HxWx3 uint8 RGB whatever its JPEG colour model: grayscale is
        # replicated (the reference's cv2.COLOR_GRAY2RGB), CMYK / palette / alpha files go through
        # PIL's colour conversion (skimage.io.imread, which the reference calls, does the same);
        # slicing the first three planes of a CMYK array would be wrong pixel data.
        with PIL.Image.open(self.img_fname.format(img_id)) as f:
            img = np.asarray(f if f.mode in ('L', 'RGB') else f.convert('RGB'))
        if img.ndim == 2:
            img = np.repeat(img[:, :, None], 3, axis=2)
        example = self._annotations_to_example(self._anns_of_img.get(img_id, []), img.shape[0],
                                               img.shape[1])
        return tuple([img] + example)

    def get_annotations(self, i):
        """``get_example(i)`` without the image: (bboxes, labels, masks[, crowds][, areas]) at
        the height and width the JSON gives, without opening the JPEG (scoring a results file
        needs only the annotation file)."""
        img_id = self.img_ids[i]
        height, width = self.img_sizes[img_id]
        return tuple(self._annotations_to_example(self._anns_of_img.get(img_id, []), height, width))

    # -- annotations -> (bboxes, labels, masks[, crowds][, areas]) -------------------------------
    # Contract of the reference's datasets/coco.py:123-176 (pinned by tests/golden/coco_example.npz):
    # an instance is kept when it has a segmentation, is not a crowd region (unless use_crowd) and
    # — for run-length masks — decodes to the image size; its box is the tight box of its mask.
    @staticmethod
    def _rasterise(segmentation, height, width):
        """Polygon list or COCO RLE dict -> (height, width) bool mask, or None when a run-length
        mask does not match the image (malformed minival annotations are dropped)."""
        if isinstance(segmentation, list):
            import PIL.Image
            import PIL.ImageDraw
            canvas = PIL.Image.new('L', (width, height), 0)
            pen = PIL.ImageDraw.Draw(canvas)
            for ring in segmentation:
                pts = np.asarray(ring).reshape(-1, 2)
                pen.polygon(xy=list(map(tuple, pts)), outline=1, fill=1)
            return np.asarray(canvas) == 1
        decoded = rle_decode(segmentation, height, width)
        return decoded == 1 if decoded.shape == (height, width) else None

    def _kept_instances(self, anns, height, width):
        for ann in anns:
            if 'segmentation' not in ann or (ann['iscrowd'] == 1 and not self._use_crowd):
                continue
            seg = ann['segmentation']
            if isinstance(seg, list) and self._polygon_rule == 'coco':
                # device_polygons: the rings travel on as they are (a list), nothing is drawn here
                inst = seg if self._device_polygons else polygon_to_mask_coco(seg, height, width)
            else:
                inst = self._rasterise(seg, height, width)
            if inst is not None:
                yield ann, inst

    def _box(self, inst, height, width):
        """The tight box of one kept instance: ``mask_to_bbox`` as ever under the PIL rule; under
        COCO's rule a polygon may set no pixel at all, and its box is then zeros."""
        if self._polygon_rule == 'pil':
            return mask_to_bbox(inst)
        if isinstance(inst, list):
            return polygon_box_coco(inst, height, width)
        return mask_to_bbox(inst) if inst.any() else (0, 0, 0, 0)

    def _annotations_to_example(self, anns, height, width):
        kept = list(self._kept_instances(anns, height, width))
        col = lambda fn, dt: np.asarray([fn(a, m) for a, m in kept], dtype=dt)
        if self._device_polygons:
            from .polygon_masks import PolygonMasks
            masks = PolygonMasks.from_instances([m for _, m in kept], height, width)
        elif self._packed_masks:
            masks = PackedMasks.from_instances([m for _, m in kept], height, width)
        else:
            masks = col(lambda a, m: m, np.int32).reshape((-1, height, width))
        example = [
            col(lambda a, m: self._box(m, height, width), np.float32).reshape((-1, 4)),   # y1, x1, y2, x2
            col(lambda a, m: self.cat_id_to_class_id[a['category_id']], np.int32),
            masks,
        ]
        if self._return_crowd:
            example.append(col(lambda a, m: a['iscrowd'], np.int32))
        if self._return_area:
            example.append(col(lambda a, m: a['area'], np.float32))
        return example
