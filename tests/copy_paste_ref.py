"""NumPy reference for copy-paste: the definition with ``any(0)``,
``np.where`` and ``argwhere``, and the acceptance rules of ``datasets.CopyPasteDataset`` on top.
tests/test_copy_paste_cpu.py checks it against a per-pixel loop; tests/test_gpu_copy_paste.py
compares ``mrcnn_copy_paste`` and the dataset wrapper with it, exactly."""
import random

import numpy as np

from scale_jitter_ref import boxes_areas


def compose(img_t, masks_t, img_s, masks_s, idx):
    """(3, S, S) images, (G, S, S) masks (a byte other than 0 is set), ``idx`` strictly increasing
    -> ``(img, masks uint8 {0, 1}, boxes, areas)``.  The image is selected, never blended: a pixel
    is a copy of one of the two inputs."""
    masks_t, masks_s = np.asarray(masks_t) != 0, np.asarray(masks_s) != 0
    pasted = masks_s[np.asarray(idx, np.intp)]
    alpha = pasted.any(0) if len(pasted) else np.zeros(masks_t.shape[1:], bool)
    img = np.where(alpha[None], img_s, img_t)
    masks = np.concatenate([masks_t & ~alpha[None], pasted]).astype(np.uint8)
    boxes, areas = boxes_areas(masks)
    return img, masks, boxes, areas


def compose_brute_force(img_t, masks_t, img_s, masks_s, idx):
    """The definition, pixel by pixel."""
    Gt, S = len(masks_t), img_t.shape[1]
    img = np.empty_like(img_t)
    masks = np.zeros((Gt + len(idx), S, S), np.uint8)
    for y in range(S):
        for x in range(S):
            alpha = any(masks_s[g][y][x] != 0 for g in idx)
            for c in range(3):
                img[c, y, x] = img_s[c, y, x] if alpha else img_t[c, y, x]
            for g in range(Gt):
                masks[g, y, x] = 1 if masks_t[g][y][x] != 0 and not alpha else 0
            for k, g in enumerate(idx):
                masks[Gt + k, y, x] = 1 if masks_s[g][y][x] != 0 else 0
    return img, masks


def paste(ex, src):
    """What ``CopyPasteDataset.__getitem__`` makes of the example ``ex`` and the source ``src``
    (host copies of ``(img, bbox, label, masks, scale)``) once the coin has passed and ``src`` is
    fetched: the two draws of the selection, the composition, the drop of every instance without a
    pixel.  Returns ``(item, idx, dropped)``; ``item`` is ``ex`` itself where nothing is pasted or
    nothing would be kept."""
    if len(src[3]) == 0:
        return ex, None, None
    k = random.randint(1, len(src[3]))
    idx = sorted(random.sample(range(len(src[3])), k))
    img, masks, boxes, areas = compose(ex[0], ex[3], src[0], src[3], idx)
    keep = areas >= 1
    if not keep.any():
        return ex, idx, ~keep
    label = np.concatenate([ex[2], src[2][idx]])[keep]
    return (img, boxes[keep].astype(np.float32), label, masks[keep], ex[4]), idx, ~keep
