"""COCO polygons drawn on the device by COCO's own rule (include/mrcnn_hip.h
``mrcnn_polygon_rasterize``, csrc/polygon_raster.hip): a ``datasets.PolygonMasks`` crosses PCIe as
its vertices — a few hundred bytes per instance — and comes out as packed masks with their exact
areas, extents and tight boxes.  The device half of ``datasets.coco.polygon_to_mask_coco``."""
import numpy as np
import torch

from .. import _lib


def upsample_vertices(polys):
    """A sequence of polygon instances, each a sequence of rings ``[x0, y0, x1, y1, ...]`` ->
    ``(xy5 (V, 2), ring_off (R+1,), inst_off (G+1,))`` int32 host arrays: the vertices upsampled
    as maskApi.c does, ``(int)(5.0 * c + .5)`` in float64, one ring after another; ring r owns
    vertices ``ring_off[r] .. ring_off[r+1]`` and instance g rings ``inst_off[g] .. inst_off[g+1]``.
    ValueError for a ring with an odd number of coordinates, a non-finite one or ``|5 c| >= 2^30``."""
    from ..datasets.coco import upsample_ring
    rings, ring_off, inst_off = [], [0], [0]
    for inst in polys:
        for ring in inst:
            up = upsample_ring(ring)
            rings.append(up)
            ring_off.append(ring_off[-1] + len(up))
        inst_off.append(len(ring_off) - 1)
    if ring_off[-1] >= 2 ** 31:
        raise ValueError('upsample_vertices: the number of vertices must be below 2^31')
    xy5 = np.concatenate(rings) if rings else np.zeros((0, 2), np.int64)
    return xy5.astype(np.int32), np.asarray(ring_off, np.int32), np.asarray(inst_off, np.int32)


def _rasterize(xy5, ring_off, inst_off, H, W, dev):
    """One upload of the three tables, one ``mrcnn_polygon_rasterize``."""
    G, Wq = len(inst_off) - 1, (W + 63) // 64
    packed = torch.empty((G, H, Wq), dtype=torch.int64, device=dev)
    area = torch.empty((G,), dtype=torch.int32, device=dev)
    extent = torch.empty((G, 4), dtype=torch.int32, device=dev)
    box = torch.empty((G, 4), dtype=torch.int32, device=dev)
    if G == 0:
        return packed, area, extent, box
    n_xy, n_ring = xy5.size, ring_off.size
    tables = torch.from_numpy(np.concatenate([xy5.reshape(-1), ring_off, inst_off])).to(dev)
    _lib.require_device(tables)
    tables = _lib.dense(tables, torch.int32, 'rasterize_polygons', 'tables')
    nbytes = _lib.load().mrcnn_polygon_rasterize_workspace_bytes(G, H, W)
    with torch.cuda.device(dev):
        ws = _lib.workspace(nbytes, dev, tag='polygon_rasterize')
        _lib.call('mrcnn_polygon_rasterize', _lib.ptr(tables[:n_xy]) if n_xy else None,
                  _lib.ptr(tables[n_xy:n_xy + n_ring]), _lib.ptr(tables[n_xy + n_ring:]), G, H, W,
                  _lib.ptr(packed), _lib.ptr(area), _lib.ptr(extent), _lib.ptr(box), _lib.ptr(ws),
                  _lib.stream_ptr())
    return packed, area, extent, box


def rasterize_polygons(polys, device=None):
    """``datasets.PolygonMasks`` -> ``(packed (G, H, Wq) int64 bit pattern, area (G,), extent
    (G, 4), box (G, 4))`` int32 device tensors in the packed-mask format, on the current stream:
    ``extent`` is (y_lo, y_hi, wq_lo, wq_hi), ``box`` the tight (y1, x1, y2, x2); an empty mask has
    a box of zeros and the empty extent (H, 0, Wq, 0) of ``pack_masks``.  The polygon instances
    are drawn by one ``mrcnn_polygon_rasterize`` call from their vertices; the packed rows of
    run-length instances are uploaded as they are and copied in beside them, with their area,
    extent and box counted on the host.  There is no host fallback: a device is required."""
    from ..datasets.packed_masks import packed_metadata
    from ..datasets.polygon_masks import PolygonMasks
    if not isinstance(polys, PolygonMasks):
        raise TypeError('rasterize_polygons expects a datasets.PolygonMasks, got %s'
                        % type(polys).__name__)
    if device is None:
        from ..utils.evaluations import masks as M
        device = M._device()
    dev = torch.device(device)
    G, H, W = polys.shape
    if H <= 0 or W <= 0 or H * W >= 2 ** 31:
        raise ValueError('rasterize_polygons: H and W must be positive with H * W < 2^31, got %d x %d'
                         % (H, W))
    is_poly = polys.is_polygon()
    tables = upsample_vertices([polys.instances[g] for g in np.flatnonzero(is_poly)])
    out = _rasterize(*tables, H, W, dev)
    if is_poly.all():
        return out
    rows = np.stack([polys.instances[g] for g in np.flatnonzero(~is_poly)])
    meta = np.concatenate([m.reshape(len(rows), -1) for m in packed_metadata(rows, W)], axis=1)
    rows_d = torch.from_numpy(rows.view(np.int64)).to(dev)
    meta_d = torch.from_numpy(meta).to(dev)                   # (n, 1 + 4 + 4) int32
    at_poly = torch.from_numpy(np.flatnonzero(is_poly)).to(dev)
    at_rows = torch.from_numpy(np.flatnonzero(~is_poly)).to(dev)
    full = []
    for t, r in zip(out, (rows_d, meta_d[:, 0], meta_d[:, 1:5], meta_d[:, 5:9])):
        f = torch.empty((G,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev)
        f[at_poly] = t
        f[at_rows] = r
        full.append(f)
    return tuple(full)
