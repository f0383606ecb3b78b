"""PolygonMasks — the instance masks of one example as what the annotation file holds: the rings
of a polygon annotation (float64, as the JSON gives them) or, for a run-length annotation, its
packed row.  ``COCOInstanceSegmentationDataset(polygon_rule='coco', device_polygons=True)``
produces it; ``functions.rasterize_polygons`` draws the polygons on the device by COCO's own rule
(csrc/polygon_raster.hip), so a ground-truth mask never exists on the host.

It is a ``PackedMasks`` whose words are made on demand by the host rule
(``datasets.coco.polygon_to_mask_coco``): wherever the pipeline has no device route it takes the
existing host path unchanged."""
import numpy as np

from .packed_masks import PackedMasks, _pack_into


class PolygonMasks(PackedMasks):
    """``instances``: one entry per instance — a list of rings ``[x0, y0, x1, y1, ...]`` (a polygon
    annotation) or a uint64 ``(H, Wq)`` packed row (a decoded run-length annotation).  Behaves
    like ``PackedMasks`` where the input pipeline looks at it (``len``, ``shape``, ``ndim``,
    subsetting); the coordinates are checked here (``datasets.coco.upsample_ring``)."""

    def __init__(self, height, width, instances=()):
        from .coco import upsample_ring
        self.height, self.width = int(height), int(width)
        row_shape = (self.height, (self.width + 63) // 64)
        self.instances = []
        for g, inst in enumerate(instances):
            if isinstance(inst, np.ndarray) and inst.dtype == np.uint64:
                if inst.shape != row_shape:
                    raise ValueError('PolygonMasks: instance %d is a packed row of shape %r, must be %r'
                                     % (g, inst.shape, row_shape))
                self.instances.append(np.ascontiguousarray(inst))
            else:
                rings = tuple(np.array(r, dtype=np.float64).reshape(-1) for r in inst)
                for r in rings:
                    upsample_ring(r)                   # ValueError: odd count, non-finite, huge
                self.instances.append(rings)
        self._words = None

    @classmethod
    def from_instances(cls, instances, height, width):
        """As ``PackedMasks.from_instances``, where an instance may also be a list of rings: a
        (height, width) mask is packed, rings are kept."""
        height, width = int(height), int(width)
        out = []
        for g, inst in enumerate(instances):
            if isinstance(inst, np.ndarray) and inst.dtype != np.uint64:
                if inst.shape != (height, width):
                    raise ValueError('PolygonMasks.from_instances: instance %d has shape %r, not %r'
                                     % (g, inst.shape, (height, width)))
                row = np.zeros((height, (width + 63) // 64), dtype=np.uint64)
                _pack_into(row, inst)
                inst = row
            out.append(inst)
        return cls(height, width, out)

    def is_polygon(self):
        """(G,) bool: which instances are polygons (the others are packed rows)."""
        return np.array([isinstance(i, tuple) for i in self.instances], dtype=bool)

    def to_packed(self):
        """A host ``PackedMasks`` of all the instances, polygons drawn by the host rule."""
        from .coco import polygon_to_mask_coco
        G, H, W = self.shape
        words = np.zeros((G, H, (W + 63) // 64), dtype=np.uint64)
        for g, inst in enumerate(self.instances):
            if isinstance(inst, tuple):
                _pack_into(words[g], polygon_to_mask_coco(inst, H, W))
            else:
                words[g] = inst
        return PackedMasks(words, H, W)

    @property
    def words(self):
        if self._words is None:
            self._words = self.to_packed().words
        return self._words

    def unpack(self, dtype=np.int32):
        """The dense (G, H, W) stack of {0, 1} (host rule)."""
        return self.to_packed().unpack(dtype)

    def __len__(self):
        return len(self.instances)

    @property
    def shape(self):
        return (len(self.instances), self.height, self.width)

    def __getitem__(self, key):
        """A slice, an index array or a boolean array over the instances -> PolygonMasks."""
        if isinstance(key, slice):
            picked = self.instances[key]
        else:
            key = np.asarray(key)
            if key.ndim != 1:
                raise IndexError('PolygonMasks: index the instances with a slice, an index array '
                                 'or a boolean array')
            if key.size == 0:
                key = key.astype(np.int64)
            picked = [self.instances[i] for i in np.arange(len(self.instances))[key]]
        return PolygonMasks(self.height, self.width, picked)
