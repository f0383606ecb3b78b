"""MaskRCNNTransform — /root/reference/chainer_mask_rcnn/datasets/transforms.py:10-51.

Same call protocol and return tuple as the reference.  What moves: the image is uploaded
once as it was decoded (HWC, usually uint8) and resized / mean-subtracted / flipped by ONE
device kernel (``mrcnn_prepare_image``), so the transform returns a device tensor for the
image; boxes, labels and masks stay host NumPy arrays because the target creators that
consume them run on the host (``MaskRCNNTrainChain``).  ``device_masks=True`` moves the masks too:
they are uploaded as bits and resized / flipped by ``mrcnn_mask_resize_nearest``.  The random flip consumes one
``random.choice([True, False])`` from Python's global generator, exactly what
``chainercv.transforms.random_flip(img, x_random=True)`` draws.

``scale_jitter=(lo, hi)`` (not in the reference) turns on large-scale jitter:
the example is resized by a random factor and cropped or zero-padded to one fixed square, by
``mrcnn_prepare_image_crop`` and ``mrcnn_mask_resize_crop``.  Its draws follow the flip's, three
per attempt (``draw_scale_jitter``).
"""
import random

import numpy as np

from .packed_masks import PackedMasks


def resize_bbox(bbox, in_size, out_size):
    """chainercv.transforms.resize_bbox: scale (y_min, x_min, y_max, x_max) boxes from an
    image of ``in_size`` (H, W) to ``out_size``; float32 in, float32 out."""
    bbox = bbox.copy()
    y_scale = float(out_size[0]) / in_size[0]
    x_scale = float(out_size[1]) / in_size[1]
    bbox[:, 0] = y_scale * bbox[:, 0]
    bbox[:, 2] = y_scale * bbox[:, 2]
    bbox[:, 1] = x_scale * bbox[:, 1]
    bbox[:, 3] = x_scale * bbox[:, 3]
    return bbox


def flip_bbox(bbox, size, y_flip=False, x_flip=False):
    """chainercv.transforms.flip_bbox."""
    H, W = size
    bbox = bbox.copy()
    if y_flip:
        y_max = H - bbox[:, 0]
        y_min = H - bbox[:, 2]
        bbox[:, 0] = y_min
        bbox[:, 2] = y_max
    if x_flip:
        x_max = W - bbox[:, 1]
        x_min = W - bbox[:, 3]
        bbox[:, 1] = x_min
        bbox[:, 3] = x_max
    return bbox


def _nearest_index(n_out, n_in):
    # cv2 INTER_NEAREST: src = min(floor(dst * (n_in / n_out)), n_in - 1), ratio in double
    idx = np.floor(np.arange(n_out, dtype=np.float64) * (float(n_in) / float(n_out))).astype(np.int64)
    return np.minimum(idx, n_in - 1)


_RESIZE_POOL = None


def resize_nearest(img, size, x_flip=False):
    """chainercv.transforms.resize(img, size, interpolation=0) for a CHW array (cv2
    INTER_NEAREST index rule), optionally followed by a horizontal flip.  Separable: columns are
    gathered first (on the small source), then whole rows are copied; the planes of a mask stack
    are spread over a few threads (NumPy releases the GIL in ``take``) — 34 MB of int32 per
    800 x 1333 COCO image otherwise cost more host time than the GPU needs for the train step."""
    C, H, W = img.shape
    ys = _nearest_index(size[0], H)
    xs = _nearest_index(size[1], W)
    if x_flip:
        xs = xs[::-1]
    out = np.empty((C, size[0], size[1]), dtype=img.dtype)

    def plane(c):
        np.take(np.take(img[c], xs, axis=1), ys, axis=0, out=out[c])

    if C * size[0] * size[1] < (1 << 21) or C == 1:
        for c in range(C):
            plane(c)
    else:
        global _RESIZE_POOL
        if _RESIZE_POOL is None:
            from concurrent.futures import ThreadPoolExecutor
            _RESIZE_POOL = ThreadPoolExecutor(max_workers=4, thread_name_prefix='mrcnn-resize')
        list(_RESIZE_POOL.map(plane, range(C)))
    return out


def flip(img, y_flip=False, x_flip=False):
    """chainercv.transforms.flip for a CHW array."""
    if y_flip:
        img = img[:, ::-1, :]
    if x_flip:
        img = img[:, :, ::-1]
    return img


SCALE_JITTER_ATTEMPTS = 8


def _resized_size(in_size, scale):
    # the rounding of MaskRCNN.prepare
    return (max(1, int(np.round(in_size[0] * scale))), max(1, int(np.round(in_size[1] * scale))))


def draw_scale_jitter(in_size, crop_size, scale_range):
    """One large-scale-jitter geometry for an (H, W) example on an S x S canvas:
    ``(scale, (rH, rW), (oy, ox))``.  Exactly three draws from Python's global ``random``, in this
    order: ``r = uniform(lo, hi)`` — the longer side becomes r * S, ``scale = min(r*S/H, r*S/W)``,
    the resized size rounded as ``MaskRCNN.prepare`` rounds it — then ``random()`` for the row
    offset and ``random()`` for the column offset of the crop window, each uniform over
    ``0 .. max(resized - S, 0)``.  A resized side shorter than S is padded at the bottom / right."""
    H, W = in_size
    S = crop_size
    lo, hi = scale_range
    r = random.uniform(lo, hi)
    scale = min(r * S / H, r * S / W)
    rH, rW = _resized_size((H, W), scale)
    oy = int(np.floor(random.random() * (max(rH - S, 0) + 1)))
    ox = int(np.floor(random.random() * (max(rW - S, 0) + 1)))
    return scale, (rH, rW), (oy, ox)


class MaskRCNNTransform(object):
    """``MaskRCNNTransform(mask_rcnn, train=True)(in_data)`` with ``in_data`` =
    ``(img HWC, bbox, label, mask)`` or the 6-tuple that also carries ``crowd, area``.
    Evaluation mode only transposes the image; training mode returns
    ``(img, bbox, label, mask, scale)``.

    ``mask`` may be a ``datasets.PackedMasks``.  With ``device_masks=True`` (training mode) the
    masks cross PCIe as bits — a dense stack is packed on the host first — and the returned mask
    is the (G, o_H, o_W) uint8 device tensor that ``mrcnn_mask_resize_nearest`` builds on the
    image's stream; the draw from ``random``, boxes, labels, image and scale are the same.
    Otherwise a ``PackedMasks`` is unpacked and takes the host path.

    ``scale_jitter=(lo, hi)`` (training mode with ``device_masks=True`` only): large-scale jitter
    onto a ``crop_size`` square.  After the flip, up to ``SCALE_JITTER_ATTEMPTS`` geometries are
    drawn (``draw_scale_jitter``); the first that leaves an instance with at least one pixel on
    the canvas is taken.  Instances left with no pixel are dropped from masks, labels and boxes,
    and ``bbox`` is the tight box of each cropped mask (the dataset's ``mask_to_bbox``
    convention), float32.  When no attempt leaves anything, or there are no instances (then
    nothing is drawn), the example is resized by ``min(S/H, S/W)`` at offset 0 and every instance
    is kept with its given box resized and flipped: the plain path on an S x S canvas.  The image
    is (3, S, S), the masks (G', S, S), ``scale`` the resize scale.  With ``scale_jitter=None``
    nothing changes.

    ``crowd_ignore=True`` (training mode with ``device_masks=True`` only):
    ``in_data`` is ``(img, bbox, label, mask, crowd)`` or the 6-tuple with ``area``, as a dataset
    built with ``use_crowd=True, return_crowd=True`` gives it.  The crowd instances
    (``crowd != 0``) ride through the same device calls as the others — rows of the one packed
    upload and of the one resize launch, under the same flip and jitter geometry — and are then
    split off: ``bbox``, ``label`` and ``mask`` hold the regular instances only, and a sixth
    element ``ignore`` is returned, the union of the crowd rows as a bit plane of the output size
    (``functions.union_plane``), or ``None`` when no crowd pixel is left.  The draws are those of
    the transform without it; under ``scale_jitter`` a geometry is accepted when a REGULAR
    instance keeps a pixel, and an example whose instances are all crowds takes the path of an
    example without instances.  With ``crowd_ignore=False`` nothing changes."""

    def __init__(self, mask_rcnn, train=True, device_masks=False, scale_jitter=None,
                 crop_size=1024, crowd_ignore=False):
        self.mask_rcnn = mask_rcnn
        self.train = train
        self.device_masks = device_masks
        if crowd_ignore and not (train and device_masks):
            raise ValueError('MaskRCNNTransform: crowd_ignore requires train=True and '
                             'device_masks=True (the ignore plane is built on the device)')
        self.crowd_ignore = bool(crowd_ignore)
        if scale_jitter is not None:
            if not (train and device_masks):
                raise ValueError('MaskRCNNTransform: scale_jitter requires train=True and '
                                 'device_masks=True (the crop is built on the device)')
            lo, hi = (float(v) for v in scale_jitter)
            if not 0 < lo <= hi:
                raise ValueError('MaskRCNNTransform: scale_jitter=(lo, hi) needs 0 < lo <= hi, '
                                 'got %r' % (tuple(scale_jitter),))
            if int(crop_size) != crop_size or crop_size <= 0:
                raise ValueError('MaskRCNNTransform: crop_size must be a positive integer, got %r'
                                 % (crop_size,))
            scale_jitter, crop_size = (lo, hi), int(crop_size)
        self.scale_jitter = scale_jitter
        self.crop_size = crop_size

    def __call__(self, in_data):
        if self.crowd_ignore:
            return self._with_crowds(in_data)
        if len(in_data) not in (4, 6):
            raise ValueError
        img, bbox, label, mask = in_data[:4]
        extras = tuple(in_data[4:])
        chw = img.transpose(2, 0, 1)
        if not self.train:
            return (chw, bbox, label, mask) + extras

        # the reference resizes first and draws the flip afterwards; nothing in between
        # touches an RNG, so drawing first leaves the random stream identical
        x_flip = random.choice([True, False])
        in_size = chw.shape[1:]
        if self.scale_jitter is not None:
            return self._scale_jitter(chw, bbox, label, mask, x_flip)
        imgs, _, scales = self.mask_rcnn.prepare([chw], x_flips=[x_flip])
        x = imgs[0]                        # device tensor (3, o_H, o_W), channels-last memory
        out_size = tuple(x.shape[1:])

        if len(bbox) > 0:
            bbox = resize_bbox(bbox, in_size, out_size)
        bbox = flip_bbox(bbox, out_size, x_flip=x_flip)

        if self.device_masks:
            return x, bbox, label, self._device_mask(mask, out_size, x_flip, x.device), scales[0]
        if isinstance(mask, PackedMasks):
            mask = mask.unpack()
        stack = mask[None] if mask.ndim == 2 else mask
        if len(mask) > 0:
            stack = resize_nearest(stack, out_size, x_flip=x_flip)
        else:
            stack = flip(stack, x_flip=x_flip)
        mask = stack[0] if mask.ndim == 2 else stack
        return x, bbox, label, mask, scales[0]

    def _with_crowds(self, in_data):
        """``crowd_ignore=True`` (class docstring): the same draws and device calls as without it,
        over all the instances; the crowd rows leave as one bit plane."""
        import torch
        from ..functions import ignore_regions
        if len(in_data) not in (5, 6):
            raise ValueError('MaskRCNNTransform: crowd_ignore expects (img, bbox, label, mask, crowd[, '
                             'area]), got %d elements' % len(in_data))
        img, bbox, label, mask, crowd = in_data[:5]
        crowd = np.asarray(crowd) != 0
        if mask.ndim != 3 or crowd.shape != (len(mask),):
            raise ValueError('MaskRCNNTransform: crowd_ignore expects (G, H, W) masks and one crowd '
                             'flag per instance, got %r and %r' % (tuple(mask.shape), crowd.shape))
        if not isinstance(mask, PackedMasks):
            mask = PackedMasks.from_dense(mask)
        chw = img.transpose(2, 0, 1)
        x_flip = random.choice([True, False])
        in_size = chw.shape[1:]
        if self.scale_jitter is not None:
            x, bbox, label, masks, scale, (crowd, present) = self._scale_jitter(
                chw, bbox, label, mask, x_flip, regular=~crowd)
        else:
            imgs, _, scales = self.mask_rcnn.prepare([chw], x_flips=[x_flip])
            x, scale = imgs[0], scales[0]
            out_size = tuple(x.shape[1:])
            if len(bbox) > 0:
                bbox = resize_bbox(bbox, in_size, out_size)
            bbox = flip_bbox(bbox, out_size, x_flip=x_flip)
            masks = self._device_mask(mask, out_size, x_flip, x.device)
            present = crowd.copy()
            if crowd.any():
                # a crowd pixel survives iff one lies on a sampled row and a sampled column
                ys, xs = _nearest_index(out_size[0], in_size[0]), _nearest_index(out_size[1], in_size[1])
                dense = mask[crowd].unpack(np.uint8)
                present[crowd] = dense[:, np.unique(ys)][:, :, np.unique(xs)].any(axis=(1, 2))
        # crowd, present: over the rows of masks / bbox / label as they stand now
        rows = lambda sel: masks[torch.from_numpy(np.flatnonzero(sel)).to(masks.device)]
        ignore = ignore_regions.union_plane(rows(present)) if present.any() else None
        if crowd.any():
            masks, bbox, label = rows(~crowd), bbox[~crowd], label[~crowd]
        return x, bbox, label, masks, scale, ignore

    @staticmethod
    def _device_mask(mask, out_size, x_flip, device):
        """The network-size masks as a uint8 device tensor; only the packed words are uploaded."""
        from ..functions import gt_masks
        flat = not isinstance(mask, PackedMasks) and mask.ndim == 2
        if not isinstance(mask, PackedMasks):
            mask = PackedMasks.from_dense(mask[None] if flat else mask)
        out = gt_masks.resize_masks_nearest(gt_masks.upload_packed_masks(mask, device), out_size,
                                            x_flip=x_flip)
        return out[0] if flat else out

    def _scale_jitter(self, chw, bbox, label, mask, x_flip, regular=None):
        """The jittered example (class docstring); the flip has been drawn.  ``regular`` (G,) bool
        (``crowd_ignore``): only these instances decide whether a geometry is accepted, and the
        result — still over ALL the instances it keeps — gains a sixth element: two (G',) bool
        arrays, the crowd rows among them and the crowd rows that hold a pixel."""
        import torch
        from ..functions import gt_masks, scale_jitter as SJ
        model, S = self.mask_rcnn, self.crop_size
        dev = next(model.parameters()).device
        in_size = tuple(chw.shape[1:])
        flat = not isinstance(mask, PackedMasks) and mask.ndim == 2
        if not isinstance(mask, PackedMasks):
            mask = PackedMasks.from_dense(mask[None] if flat else mask)
        G = len(mask)
        packed = gt_masks.upload_packed_masks(mask, dev)
        masks = None
        decides = np.ones((G,), bool) if regular is None else regular
        for _ in range(SCALE_JITTER_ATTEMPTS if decides.any() else 0):
            scale, resized, offset = draw_scale_jitter(in_size, S, self.scale_jitter)
            cropped, meta = SJ.resize_crop_masks_meta(packed, resized, offset, S, x_flip)
            meta = meta.cpu().numpy()                  # boxes and areas: the one read-back
            keep = meta[4 * G:] >= 1
            if (keep & decides).any():
                masks = cropped
                break
        if masks is not None:
            if not keep.all():
                masks = masks[torch.from_numpy(np.flatnonzero(keep)).to(dev)]
                label = label[keep]
            bbox = meta[:4 * G].reshape(G, 4)[keep].astype(np.float32)
            crowd_rows = None if regular is None else (~regular[keep],) * 2
        else:
            scale = min(float(S) / in_size[0], float(S) / in_size[1])
            resized, offset = _resized_size(in_size, scale), (0, 0)
            masks, meta = SJ.resize_crop_masks_meta(packed, resized, offset, S, x_flip)
            if len(bbox) > 0:
                bbox = resize_bbox(bbox, in_size, resized)
            bbox = flip_bbox(bbox, resized, x_flip=x_flip)
            crowd_rows = None if regular is None else (~regular, ~regular)
            if regular is not None and not regular.all():
                # every instance is kept here; which crowd rows still hold a pixel is read back
                crowd_rows = (~regular, ~regular & (meta.cpu().numpy()[4 * G:] >= 1))
        x = SJ.prepare_image_crop(model.mean, chw, scale, resized, offset, S, x_flip, dev)
        if regular is not None:
            return x, bbox, label, masks, scale, crowd_rows
        return x, bbox, label, (masks[0] if flat else masks), scale
