"""NumPy references for large-scale jitter, each a composition of code that
predates the feature: ``transforms.resize_nearest`` at the full resized size, a slice and a zero
pad for the masks; ``np.argwhere`` for the tight boxes and areas; the same acceptance, drop and
fallback rules on top for the whole transform.  tests/test_scale_jitter_cpu.py checks the helpers
against a per-pixel loop; tests/test_gpu_scale_jitter.py compares the kernels and
``MaskRCNNTransform(scale_jitter=...)`` with them, exactly."""
import random

import numpy as np

from chainer_mask_rcnn_amd.datasets import PackedMasks
from chainer_mask_rcnn_amd.datasets import transforms as T

ATTEMPTS = 8


def crop_pad(resized, offset, S):
    """``resized`` (..., rH, rW) -> (..., S, S): out[y, x] = resized[y + oy, x + ox] inside, 0
    elsewhere."""
    oy, ox = offset
    window = resized[..., oy:oy + S, ox:ox + S]
    out = np.zeros(resized.shape[:-2] + (S, S), dtype=resized.dtype)
    out[..., :window.shape[-2], :window.shape[-1]] = window
    return out


def crop_masks(stack, resized, offset, S, x_flip=False):
    """(G, H, W) {0,1} -> (G, S, S) uint8: resize_nearest to ``resized`` (+ flip), slice, pad."""
    stack = np.asarray(stack)
    if len(stack) == 0:
        return np.zeros((0, S, S), np.uint8)
    return crop_pad(T.resize_nearest(stack, resized, x_flip=x_flip), offset, S).astype(np.uint8)


def boxes_areas(masks):
    """Tight half-open boxes (G, 4) int32 (y_lo, x_lo, y_hi, x_hi), (0,0,0,0) for an empty mask,
    and areas (G,) int32."""
    boxes = np.zeros((len(masks), 4), np.int32)
    areas = np.zeros((len(masks),), np.int32)
    for g, m in enumerate(masks):
        yx = np.argwhere(m)
        areas[g] = len(yx)
        if len(yx):
            boxes[g] = (yx[:, 0].min(), yx[:, 1].min(), yx[:, 0].max() + 1, yx[:, 1].max() + 1)
    return boxes, areas


def crop_masks_brute_force(stack, resized, offset, S, x_flip=False):
    """The definition, pixel by pixel: R = the cv2 INTER_NEAREST resize of the mask (mirrored for a
    flip), out[y, x] = R[y + oy, x + ox] or 0."""
    G, H, W = stack.shape
    rH, rW = resized
    out = np.zeros((G, S, S), np.uint8)
    for g in range(G):
        for y in range(S):
            for x in range(S):
                ry, rx = y + offset[0], x + offset[1]
                if ry >= rH or rx >= rW:
                    continue
                if x_flip:
                    rx = rW - 1 - rx
                sy = min(int(np.floor(ry * (float(H) / rH))), H - 1)
                sx = min(int(np.floor(rx * (float(W) / rW))), W - 1)
                out[g, y, x] = stack[g, sy, sx] != 0
    return out


def transform(example, scale_jitter, S, image):
    """What ``MaskRCNNTransform(model, device_masks=True, scale_jitter=scale_jitter, crop_size=S)``
    returns for ``example``, from the same draws of ``random``: ``(img, bbox, label, masks, scale,
    attempt)``.  ``image(chw, scale, resized, offset, x_flip)`` builds the (3, S, S) image;
    ``attempt`` is the 1-based attempt that was accepted, None for the fallback."""
    img, bbox, label, mask = example[:4]
    chw = img.transpose(2, 0, 1)
    in_size = chw.shape[1:]
    x_flip = random.choice([True, False])
    dense = mask.unpack() if isinstance(mask, PackedMasks) else np.asarray(mask)
    flat = dense.ndim == 2
    if flat:
        dense = dense[None]
    attempt = None
    for k in range(ATTEMPTS if len(dense) else 0):
        scale, resized, offset = T.draw_scale_jitter(in_size, S, scale_jitter)
        masks = crop_masks(dense, resized, offset, S, x_flip)
        boxes, areas = boxes_areas(masks)
        if (areas >= 1).any():
            attempt = k + 1
            break
    if attempt is not None:
        keep = areas >= 1
        masks, label, bbox = masks[keep], label[keep], boxes[keep].astype(np.float32)
    else:
        scale = min(float(S) / in_size[0], float(S) / in_size[1])
        resized = (max(1, int(np.round(in_size[0] * scale))), max(1, int(np.round(in_size[1] * scale))))
        offset = (0, 0)
        masks = crop_masks(dense, resized, offset, S, x_flip)
        if len(bbox) > 0:
            bbox = T.resize_bbox(bbox, in_size, resized)
        bbox = T.flip_bbox(bbox, resized, x_flip=x_flip)
    x = image(chw, scale, resized, offset, x_flip)
    return x, bbox, label, (masks[0] if flat else masks), scale, attempt
