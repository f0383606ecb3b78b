"""Ground-truth masks of the train step built on the device from packed bits
(include/mrcnn_hip.h ``mrcnn_mask_resize_nearest``, csrc/gt_masks.hip): the device half of
``datasets.transforms.resize_nearest`` for ``datasets.PackedMasks``."""
import numpy as np
import torch

from .. import _lib


def upload_packed_masks(packed, device):
    """``datasets.PackedMasks`` -> ``(words, width)``: the words as an int64 device tensor
    (G, H, Wq) (torch has no arithmetic on uint64; the bits are what matters) and the mask width
    in pixels, which the word count alone does not give.  Only the bits cross PCIe.

    A ``datasets.PolygonMasks`` crosses as its vertices instead: its polygons are drawn on the
    device by one ``functions.rasterize_polygons`` call, the packed rows of its run-length
    instances are copied in beside them, and the words never exist on the host."""
    from ..datasets.polygon_masks import PolygonMasks
    if isinstance(packed, PolygonMasks):
        from .polygons import rasterize_polygons
        return rasterize_polygons(packed, device)[0], packed.width
    words = torch.from_numpy(packed.words.view(np.int64)).to(device)
    return words, packed.width


def resize_masks_nearest(packed_device, out_size, x_flip=False):
    """``resize_nearest(masks, out_size, x_flip)`` for packed masks on the device.

    ``packed_device``: ``(words, width)`` as ``upload_packed_masks`` returns it — words (G, H, Wq)
    int64 device tensor in the packed format, width W in pixels.  Returns the (G, o_H, o_W) uint8
    device tensor of {0, 1} that ``mrcnn_mask_targets`` reads, computed on the current stream.  The
    row / column tables are ``transforms._nearest_index`` (the cv2 INTER_NEAREST rule), the column
    table reversed for ``x_flip``, so the result equals the host function bit for bit."""
    from ..datasets.transforms import _nearest_index
    words, W = packed_device
    W = int(W)
    _lib.require_device(words)
    if words.dtype != torch.int64 or words.dim() != 3 or not words.is_contiguous():
        raise ValueError('resize_masks_nearest: words must be a contiguous int64 (G, H, Wq) tensor')
    G, H, Wq = words.shape
    if Wq != (W + 63) // 64:
        raise ValueError('resize_masks_nearest: %d words per row do not hold %d pixels' % (Wq, W))
    o_H, o_W = int(out_size[0]), int(out_size[1])
    dev = words.device
    out = torch.empty((G, o_H, o_W), dtype=torch.uint8, device=dev)
    if G == 0:
        return out
    xs = _nearest_index(o_W, W)
    if x_flip:
        xs = xs[::-1]
    tables = torch.from_numpy(np.concatenate([_nearest_index(o_H, H), xs]).astype(np.int32)).to(dev)
    with torch.cuda.device(dev):
        _lib.call('mrcnn_mask_resize_nearest', _lib.ptr(words), G, H, W, _lib.ptr(tables[:o_H]),
                  _lib.ptr(tables[o_H:]), o_H, o_W, _lib.ptr(out), _lib.stream_ptr())
    return out
