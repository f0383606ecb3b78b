"""The NumPy statement of the ignore-region kernels (include/mrcnn_hip.h ``mrcnn_mask_union_pack``,
``mrcnn_box_coverage``): dense union, np.round, clip, slice sum."""
import numpy as np


def pack_plane(dense):
    """(H, W) bool -> (H, ceil(W / 64)) uint64 in the packed-mask format (pad bits zero)."""
    H, W = dense.shape
    Wq = (W + 63) // 64
    rows = np.zeros((H, Wq * 64), np.uint8)
    rows[:, :W] = dense != 0
    return np.packbits(rows, axis=1, bitorder='little').view(np.uint64).reshape(H, Wq)


def unpack_plane(words, W):
    """(H, Wq) uint64 / int64 -> (H, W) bool."""
    words = np.ascontiguousarray(words).view(np.uint8)
    return np.unpackbits(words, axis=1, bitorder='little')[:, :W].astype(bool)


def union_dense(masks, base=None):
    """(G, H, W) -> (H, W) bool: any mask nonzero; with ``base`` (H, W) bool: base & ~union."""
    u = (np.asarray(masks) != 0).any(axis=0) if len(masks) else np.zeros(np.shape(masks)[1:], bool)
    return u if base is None else (np.asarray(base, bool) & ~u)


def box_coverage(dense, boxes):
    """(H, W) bool, (n, 4) float32 (y1, x1, y2, x2) -> (n, 2) int64 (covered, area)."""
    H, W = dense.shape
    out = np.zeros((len(boxes), 2), np.int64)
    for i, b in enumerate(np.asarray(boxes, np.float32)):
        if not np.isfinite(b).all():
            continue
        y0, x0, y1, x1 = (int(v) for v in np.clip(np.round(b.astype(np.float64)), 0, [H, W, H, W]))
        out[i] = dense[y0:y1, x0:x1].sum(), max(y1 - y0, 0) * max(x1 - x0, 0)
    return out
