"""Large-scale jitter on the device (include/mrcnn_hip.h
``mrcnn_prepare_image_crop`` / ``mrcnn_mask_resize_crop``, csrc/scale_jitter.hip): the S x S
training canvas cut out of, or zero-padded around, the randomly resized example.  The geometry
(scale, resized size, offset) is drawn on the host by ``datasets.transforms.draw_scale_jitter``."""
import numpy as np
import torch

from .. import _lib


def prepare_image_crop(model_mean, img_chw, scale, resized, offset, crop_size, x_flip, device):
    """Window ``offset`` = (oy, ox) of ``img_chw`` (3, H, W; uint8 or float) resized by ``scale``
    to ``resized`` = (rH, rW), mean-subtracted and mirrored when ``x_flip`` — the image
    ``MaskRCNN.prepare`` would build at that scale — on a ``crop_size`` square canvas, zero below
    and right of the resized image.  Returns the (3, S, S) float32 device tensor as a channels-last
    view, computed on the current stream; the resized image itself is never built."""
    device = torch.device(device)
    if device.type != 'cuda':
        raise _lib.MrcnnHipError('prepare_image_crop: needs a ROCm device, got %s' % (device,))
    S = int(crop_size)
    (rH, rW), (oy, ox) = (int(v) for v in resized), (int(v) for v in offset)
    _, H, W = img_chw.shape
    is_u8 = getattr(img_chw, 'dtype', None) == np.uint8
    host = np.ascontiguousarray(img_chw, dtype=np.uint8 if is_u8 else np.float32)
    # through pinned memory, asynchronously, as MaskRCNN.prepare uploads
    stage = torch.empty(host.shape, dtype=torch.uint8 if is_u8 else torch.float32, pin_memory=True)
    np.copyto(stage.numpy(), host)
    src = stage.to(device, non_blocking=True)
    return prepare_image_crop_device(model_mean, src, scale, (rH, rW), (oy, ox), S, x_flip)


def prepare_image_crop_device(model_mean, src, scale, resized, offset, crop_size, x_flip):
    """``prepare_image_crop`` for an image that is on the device already: ``src`` (3, H, W) uint8 or
    float32 device tensor, as uploaded."""
    _lib.require_device(src)
    if src.dtype not in (torch.uint8, torch.float32):
        raise TypeError('prepare_image_crop_device: src must be %s or %s, got %s'
                        % (torch.uint8, torch.float32, src.dtype))
    src = _lib.dense(src, src.dtype, 'prepare_image_crop_device', 'src')
    S = int(crop_size)
    (rH, rW), (oy, ox) = (int(v) for v in resized), (int(v) for v in offset)
    _, H, W = src.shape
    device = src.device
    canvas = torch.empty((1, S, S, 3), dtype=torch.float32, device=device)
    mean = (_lib.c_f32 * 3)(*[float(v) for v in np.asarray(model_mean).ravel()])
    with torch.cuda.device(device):
        _lib.call('mrcnn_prepare_image_crop', _lib.ptr(src), int(src.dtype == torch.uint8), 3, int(H),
                  int(W), float(scale), mean, _lib.ptr(canvas), S, S, rH, rW, oy, ox, 0,
                  int(bool(x_flip)), _lib.stream_ptr())
    return canvas.permute(0, 3, 1, 2)[0]


def crop_tables(in_size, resized, offset, crop_size, x_flip=False):
    """(ys, xs) int32 of length S for ``mrcnn_mask_resize_crop``: the source row / column of each
    canvas row / column — ``transforms._nearest_index`` over the resized size, the column table
    reversed for a flip, then the window starting at ``offset`` — and -1 beyond the resized
    mask."""
    from ..datasets.transforms import _nearest_index
    S = int(crop_size)
    tables = []
    for n_in, n_out, o, rev in ((in_size[0], resized[0], offset[0], False),
                                (in_size[1], resized[1], offset[1], x_flip)):
        idx = _nearest_index(int(n_out), int(n_in))
        if rev:
            idx = idx[::-1]
        idx = idx[int(o):int(o) + S]
        t = np.full((S,), -1, dtype=np.int32)
        t[:len(idx)] = idx
        tables.append(t)
    return tables[0], tables[1]


def resize_crop_masks_meta(packed_device, resized, offset, crop_size, x_flip=False):
    """``resize_crop_masks`` with the boxes and areas as the one (G * 5,) int32 buffer the kernel
    fills — boxes (G, 4) first, then areas (G) — so that a caller who needs them on the host reads
    both back with one copy (``datasets.MaskRCNNTransform``).  Returns ``(masks, meta)``."""
    words, W = packed_device
    W = int(W)
    _lib.require_device(words)
    if words.dtype != torch.int64 or words.dim() != 3 or not words.is_contiguous():
        raise ValueError('resize_crop_masks: words must be a contiguous int64 (G, H, Wq) tensor')
    G, H, Wq = words.shape
    if Wq != (W + 63) // 64:
        raise ValueError('resize_crop_masks: %d words per row do not hold %d pixels' % (Wq, W))
    S = int(crop_size)
    dev = words.device
    out = torch.empty((G, S, S), dtype=torch.uint8, device=dev)
    meta = torch.empty((G * 5,), dtype=torch.int32, device=dev)
    if G == 0:
        return out, meta
    ys, xs = crop_tables((H, W), resized, offset, S, x_flip)
    tables = torch.from_numpy(np.concatenate([ys, xs])).to(dev)
    with torch.cuda.device(dev):
        row_stats = _lib.workspace(G * S * 3 * 4, dev, tag='scale_jitter_rows').view(torch.int32)
        _lib.call('mrcnn_mask_resize_crop', _lib.ptr(words), G, H, W, _lib.ptr(tables[:S]),
                  _lib.ptr(tables[S:]), S, _lib.ptr(out), _lib.ptr(meta), _lib.ptr(meta[G * 4:]),
                  _lib.ptr(row_stats), _lib.stream_ptr())
    return out, meta


def resize_crop_masks(packed_device, resized, offset, crop_size, x_flip=False):
    """``resize_nearest(masks, resized, x_flip)[:, oy:oy+S, ox:ox+S]``, zero-padded to S x S, for
    packed masks on the device, with the tight boxes and the areas of the result.

    ``packed_device``: ``(words, width)`` as ``upload_packed_masks`` returns it.  Returns
    ``(masks, boxes, areas)``: (G, S, S) uint8 {0, 1}, (G, 4) int32 ``(y_lo, x_lo, y_hi, x_hi)``
    half-open ((0, 0, 0, 0) for an empty mask) and (G,) int32 device tensors, computed on the
    current stream.  The tables are ``crop_tables``, so the index rule is the host path's."""
    out, meta = resize_crop_masks_meta(packed_device, resized, offset, crop_size, x_flip)
    G = out.shape[0]
    return out, meta[:G * 4].view(G, 4), meta[G * 4:]
