"""PackedMasks — the instance masks of one example as bits on the host, in the packed format of
include/mrcnn_hip.h ("Packed masks"): ``words`` is uint64 ``(G, H, Wq)``, ``Wq = ceil(W / 64)``,
bit ``x & 63`` of word ``[g, y, x >> 6]`` is pixel ``(g, y, x)``, pad bits are zero — byte for byte
``np.packbits(m != 0, axis=-1, bitorder='little')`` of rows zero-padded to a multiple of 64.

A dense ``(G, H, W)`` int32 stack of an 800 x 1333 image is 34 MB for 8 instances; the same masks
as bits are 0.3 MB.  ``COCOInstanceSegmentationDataset(packed_masks=True)`` produces this class,
``MaskRCNNTransform(device_masks=True)`` uploads its words and lets ``mrcnn_mask_resize_nearest``
build the network-size uint8 masks on the device (functions/gt_masks.py)."""
import numpy as np


def _pack_into(words, rows):
    """Pack ``rows`` (..., H, W) (any nonzero value is foreground) into the zeroed uint64 array
    ``words`` (..., H, Wq): little bit order, pad bits stay zero."""
    if rows.dtype != np.bool_:
        rows = rows != 0
    bits = np.packbits(rows, axis=-1, bitorder='little')          # (..., H, ceil(W / 8)) uint8
    words.view(np.uint8)[..., :bits.shape[-1]] = bits


def packed_metadata(words, width):
    """What the device entries return beside packed words, from host words (G, H, Wq): exact
    ``area`` (G,), tight ``extent`` (G, 4) (y_lo, y_hi, wq_lo, wq_hi) and tight ``box`` (G, 4)
    (y1, x1, y2, x2), all int32; an empty mask has area 0, a box of zeros and the empty extent
    (H, 0, Wq, 0), as ``mrcnn_mask_pack`` leaves it."""
    words = np.ascontiguousarray(words, dtype=np.uint64)
    G, H, Wq = words.shape
    area, extent, box = (np.zeros(s, np.int32) for s in ((G,), (G, 4), (G, 4)))
    extent[:] = H, 0, Wq, 0
    for g in range(G):
        bits = np.unpackbits(words[g].view(np.uint8), axis=-1, bitorder='little')   # (H, 64 Wq)
        rows, cols = np.flatnonzero(bits.any(axis=1)), np.flatnonzero(bits.any(axis=0))
        if rows.size:
            area[g] = int(bits.sum())
            box[g] = rows[0], cols[0], rows[-1] + 1, cols[-1] + 1
            extent[g] = rows[0], rows[-1] + 1, cols[0] >> 6, (cols[-1] >> 6) + 1
    return area, extent, box


class PackedMasks(object):
    """``words`` uint64 (G, H, Wq) + ``height`` + ``width``; behaves like the (G, H, W) stack
    where the input pipeline looks at it (``len``, ``shape``, ``ndim``, subsetting)."""

    def __init__(self, words, height, width):
        words = np.ascontiguousarray(words, dtype=np.uint64)
        height, width = int(height), int(width)
        if words.ndim != 3 or words.shape[1:] != (height, (width + 63) // 64):
            raise ValueError('PackedMasks: words of shape %r do not hold (G, %d, %d) masks'
                             % (words.shape, height, width))
        self.words, self.height, self.width = words, height, width

    @classmethod
    def from_dense(cls, masks):
        """(G, H, W) array of any dtype: any nonzero value is foreground."""
        masks = np.asarray(masks)
        if masks.ndim != 3:
            raise ValueError('PackedMasks.from_dense: expected (G, H, W), got %r' % (masks.shape,))
        G, H, W = masks.shape
        words = np.zeros((G, H, (W + 63) // 64), dtype=np.uint64)
        _pack_into(words, masks)
        return cls(words, H, W)

    @classmethod
    def from_instances(cls, instances, height, width):
        """A sequence of (height, width) masks, packed one at a time: the dense stack is never
        built.  An empty sequence gives G = 0."""
        height, width = int(height), int(width)
        words = np.zeros((len(instances), height, (width + 63) // 64), dtype=np.uint64)
        for g, inst in enumerate(instances):
            inst = np.asarray(inst)
            if inst.shape != (height, width):
                raise ValueError('PackedMasks.from_instances: instance %d has shape %r, not %r'
                                 % (g, inst.shape, (height, width)))
            _pack_into(words[g], inst)
        return cls(words, height, width)

    def unpack(self, dtype=np.int32):
        """The dense (G, H, W) stack of {0, 1}."""
        G, H, W = self.shape
        bits = np.unpackbits(self.words.view(np.uint8), axis=-1, bitorder='little')
        return bits[..., :W].astype(dtype).reshape(G, H, W)

    def __len__(self):
        return self.words.shape[0]

    @property
    def shape(self):
        return (self.words.shape[0], self.height, self.width)

    ndim = 3

    def __getitem__(self, key):
        """A slice, an index array or a boolean array over the instances -> PackedMasks."""
        if not isinstance(key, slice):
            key = np.asarray(key)
            if key.ndim != 1:
                raise IndexError('PackedMasks: index the instances with a slice, an index array '
                                 'or a boolean array')
        return PackedMasks(self.words[key], self.height, self.width)
