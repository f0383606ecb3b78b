"""Simple Copy-Paste on the device (include/mrcnn_hip.h ``mrcnn_copy_paste``,
csrc/copy_paste.hip): selected instances of a source example pasted onto a target example, both on
the S x S canvas of large-scale jitter.  Which example and which instances is drawn on the host by
``datasets.CopyPasteDataset``."""
import numpy as np
import torch

from .. import _lib


def _nhwc(img, S, what):
    """The (S, S, 3) NHWC-contiguous memory behind a (3, S, S) image, copied once if it is not."""
    if img.dtype != torch.float32 or img.dim() != 3 or tuple(img.shape) != (3, S, S):
        raise ValueError('copy_paste: %s must be a float32 (3, %d, %d) tensor, got %s %s'
                         % (what, S, S, img.dtype, tuple(img.shape)))
    return img.permute(1, 2, 0).contiguous()


def copy_paste_meta(img_t, masks_t, img_s, masks_s, idx):
    """``copy_paste`` with the boxes and areas as the one (5 * (Gt + K),) int32 buffer the kernel
    fills — boxes (Gt + K, 4) first, then areas (Gt + K) — so that a caller who needs them on the
    host reads both back with one copy (``datasets.CopyPasteDataset``).  Returns
    ``(img, masks, meta)``."""
    _lib.require_device(img_t, masks_t, img_s, masks_s)
    for what, m in (('masks_t', masks_t), ('masks_s', masks_s)):
        if m.dtype != torch.uint8 or m.dim() != 3 or m.shape[1] != m.shape[2]:
            raise ValueError('copy_paste: %s must be a uint8 (G, S, S) tensor, got %s %s'
                             % (what, m.dtype, tuple(m.shape)))
    S = int(masks_t.shape[1])
    if S <= 0 or masks_s.shape[1] != S:
        raise ValueError('copy_paste: target and source masks must share one canvas, got %s and %s'
                         % (tuple(masks_t.shape), tuple(masks_s.shape)))
    dev = masks_t.device
    if any(t.device != dev for t in (img_t, img_s, masks_s)):
        raise ValueError('copy_paste: images and masks must be on one device')
    t_nhwc, s_nhwc = _nhwc(img_t, S, 'img_t'), _nhwc(img_s, S, 'img_s')
    masks_t, masks_s = masks_t.contiguous(), masks_s.contiguous()
    Gt, Gs = int(masks_t.shape[0]), int(masks_s.shape[0])
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    K = len(idx)
    if K and (idx[0] < 0 or idx[-1] >= Gs or (np.diff(idx) <= 0).any()):
        raise ValueError('copy_paste: idx must be strictly increasing within [0, %d), got %s'
                         % (Gs, idx.tolist()))
    n = Gt + K
    out = torch.empty((S, S, 3), dtype=torch.float32, device=dev)
    masks = torch.empty((n, S, S), dtype=torch.uint8, device=dev)
    meta = torch.empty((5 * n,), dtype=torch.int32, device=dev)
    idx_d = torch.from_numpy(idx.astype(np.int32)).to(dev) if K else None
    with torch.cuda.device(dev):
        rows = _lib.workspace(n * S * 3 * 4, dev, tag='copy_paste_rows').view(torch.int32)
        _lib.call('mrcnn_copy_paste', _lib.ptr(t_nhwc), _lib.ptr(s_nhwc),
                  _lib.ptr(masks_t) if Gt else None, Gt, _lib.ptr(masks_s) if K else None, Gs,
                  _lib.ptr(idx_d), K, S, _lib.ptr(out), _lib.ptr(masks) if n else None,
                  _lib.ptr(meta) if n else None, _lib.ptr(meta[4 * n:]) if n else None,
                  _lib.ptr(rows) if n else None, _lib.stream_ptr())
    return out.permute(2, 0, 1), masks, meta


def copy_paste(img_t, masks_t, img_s, masks_s, idx):
    """The instances ``idx`` of the source pasted onto the target::

        alpha             = masks_s[idx].any(0)
        img               = where(alpha, img_s, img_t)        # a select, never a blend
        masks[g]          = masks_t[g] & ~alpha               # g < Gt: occluded by the paste
        masks[Gt + k]     = masks_s[idx[k]]                   # k < K

    ``img_t``, ``img_s``: (3, S, S) float32 device tensors, channels-last views as
    ``prepare_image_crop`` returns them (any other memory layout is copied once); ``masks_t``
    (Gt, S, S), ``masks_s`` (Gs, S, S) uint8, a byte other than 0 counts as set; ``idx``: strictly
    increasing integers within [0, Gs), possibly none.  Returns ``(img, masks, boxes, areas)``:
    (3, S, S) float32 channels-last view, (Gt + K, S, S) uint8 {0, 1}, (Gt + K, 4) int32
    ``(y_lo, x_lo, y_hi, x_hi)`` half-open ((0, 0, 0, 0) for an empty mask) and (Gt + K,) int32
    device tensors, computed on the current stream."""
    img, masks, meta = copy_paste_meta(img_t, masks_t, img_s, masks_s, idx)
    n = masks.shape[0]
    return img, masks, meta[:n * 4].view(n, 4), meta[n * 4:]
