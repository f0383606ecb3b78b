"""Simple Copy-Paste (Ghiasi et al., 2021; not in the reference) over the
fixed-size examples of large-scale jitter: with probability ``prob`` a random subset of another
example's instances is pasted onto the example, by ``mrcnn_copy_paste`` on the device."""
import random

import numpy as np


def draw_paste_selection(n_source):
    """The instances to paste out of ``n_source`` >= 1: exactly two draws from Python's global
    ``random``, ``k = randint(1, n_source)`` and then ``sample(range(n_source), k)``, returned
    sorted."""
    k = random.randint(1, n_source)
    return sorted(random.sample(range(n_source), k))


class CopyPasteDataset(object):
    """``dataset[i]`` = ``(img, bbox, label, mask, scale)`` as
    ``MaskRCNNTransform(device_masks=True, scale_jitter=...)`` returns it: a (3, S, S) device image
    and (G, S, S) uint8 device masks on one canvas size for every item.

    ``self[i]`` draws from Python's global ``random``, in this order: whatever ``dataset[i]``
    draws; ``random() < prob``, else the example is returned as it is; ``j = randrange(len)`` and
    whatever ``dataset[j]`` draws (j == i is allowed); ``draw_paste_selection`` unless the source
    has no instances, in which case the example is returned as it is.  The selected instances are
    pasted over the example: the image takes the source's pixels under them, the example's masks
    lose those pixels, the pasted masks are appended, labels likewise.  Instances left without a
    pixel are dropped — targets the paste covers, and pixel-less instances the jitter's fallback
    can carry on either side — and ``bbox`` becomes the tight float32 box of every kept mask.
    ``scale`` stays the example's.  If nothing would be kept the example is returned as it is.

    Examples of length 6 (``MaskRCNNTransform(crowd_ignore=True)``: an ignore plane or ``None``
    last) keep their sixth element; when a paste happens the example's plane loses the pasted
    pixels (``functions.union_plane(pasted masks, base=plane)``: what is pasted is real
    foreground).  The source's plane is not carried.  Example and source must have one length."""

    def __init__(self, dataset, prob=0.5):
        if not 0 <= prob <= 1:
            raise ValueError('CopyPasteDataset: prob must lie in [0, 1], got %r' % (prob,))
        self.dataset = dataset
        self.prob = prob
        self._pinned = None                            # read-back buffer, grown as needed

    def __len__(self):
        return len(self.dataset)

    @staticmethod
    def _check(ex, src):
        import torch
        for what, e in (('example', ex), ('source', src)):
            img, mask = e[0], e[3]
            if not (isinstance(mask, torch.Tensor) and mask.is_cuda and mask.dim() == 3
                    and mask.shape[1] == mask.shape[2]):
                raise ValueError('CopyPasteDataset: the %s masks must be a (G, S, S) device tensor: '
                                 'wrap MaskRCNNTransform(device_masks=True, scale_jitter=...)' % what)
            S = mask.shape[1]
            if not (isinstance(img, torch.Tensor) and tuple(img.shape) == (3, S, S)
                    and img.device == mask.device):
                raise ValueError('CopyPasteDataset: the %s image must be a (3, %d, %d) tensor on '
                                 'the device of its masks' % (what, S, S))
        if ex[3].shape[1:] != src[3].shape[1:] or ex[0].device != src[0].device:
            raise ValueError('CopyPasteDataset: example and source differ in canvas size or device '
                             '(%s, %s)' % (tuple(ex[3].shape), tuple(src[3].shape)))

    def __getitem__(self, i):
        ex = self.dataset[i]
        if not random.random() < self.prob:
            return ex
        src = self.dataset[random.randrange(len(self.dataset))]
        if len(ex) != len(src) or len(ex) not in (5, 6):
            raise ValueError('CopyPasteDataset: example and source must both have 5 elements, or both '
                             '6 (with an ignore plane), got %d and %d' % (len(ex), len(src)))
        self._check(ex, src)
        if len(src[3]) == 0:
            return ex
        idx = draw_paste_selection(len(src[3]))
        import torch
        from ..functions.copy_paste import copy_paste_meta
        img, masks, meta = copy_paste_meta(ex[0], ex[3], src[0], src[3], idx)
        n = masks.shape[0]
        if self._pinned is None or self._pinned.numel() < 5 * n:
            self._pinned = torch.empty((max(5 * n, 320),), dtype=torch.int32, pin_memory=True)
        host = self._pinned[:5 * n]
        host.copy_(meta, non_blocking=True)            # boxes and areas: the one read-back
        torch.cuda.current_stream(meta.device).synchronize()
        meta = host.numpy().copy()
        keep = meta[4 * n:] >= 1
        if not keep.any():
            return ex
        if not keep.all():
            masks = masks[torch.from_numpy(np.flatnonzero(keep)).to(masks.device)]
        bbox = meta[:4 * n].reshape(n, 4)[keep].astype(np.float32)
        label = np.concatenate([np.asarray(ex[2]), np.asarray(src[2])[idx]])[keep]
        if len(ex) == 5:
            return img, bbox, label, masks, ex[4]
        plane = ex[5]
        if plane is not None:
            from ..functions.ignore_regions import union_plane
            # the pasted rows are the last len(idx) of the launch's output; those the paste left
            # without a pixel add nothing to the union
            plane = union_plane(masks[int(keep[:n - len(idx)].sum()):], base=plane)
        return img, bbox, label, masks, ex[4], plane
