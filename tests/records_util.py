"""Helpers of the evaluation tests for ``EvalRecords``."""
from chainer_mask_rcnn_amd.utils.evaluations.records import EvalRecords

# everything a record holds: no boxes, masks or images
ATTRS = {'pred_labels', 'pred_scores', 'gt_labels', 'gt_difficults', 'gt_crowdeds', 'gt_areas',
         'tables'}


def take(rec, lo, hi):
    """Images [lo, hi) of a record: a shard."""
    cut = {k: None if getattr(rec, k) is None else getattr(rec, k)[lo:hi]
           for k in ATTRS - {'tables'}}
    return EvalRecords(tables={k: v[lo:hi] for k, v in rec.tables.items()}, **cut)


def same_lists(a, b):
    """Two per-image lists hold the same objects (or both are None)."""
    return (a is None and b is None) or (len(a) == len(b) and all(x is y for x, y in zip(a, b)))


def readback_parts():
    """CPU tensors of every type ``Readback`` carries: zero-size parts, a uint8 part of odd
    length (so that what follows it in a byte buffer is misaligned) and floats whose bits a
    conversion would lose."""
    import numpy as np
    import torch
    f32 = np.array([np.nan, -0.0, np.inf, 1e-42, 1. / 3.], np.float32)
    f32[:1].view(np.uint32)[0] = 0x7fc12345                       # a NaN with a payload
    f64 = np.array([np.nan, -0.0, 5e-324, 1. / 3.], np.float64)
    return [torch.zeros((0, 3), dtype=torch.int32), torch.zeros((3, 0), dtype=torch.int32),
            torch.arange(-3, 3, dtype=torch.int32).reshape(2, 3),
            torch.tensor([1, 255, 7], dtype=torch.uint8), torch.from_numpy(f32),
            torch.from_numpy(f64), torch.tensor([2 ** 40], dtype=torch.int64)]


def check_readback(parts, host):
    """``host`` (a ``Readback.fetch()``) is ``parts`` (CPU tensors): shapes, int64 integers with
    equal values, floats bit for bit."""
    import numpy as np
    assert len(host) == len(parts)
    for t, h in zip(parts, host):
        want = t.numpy()
        assert h.shape == want.shape, (h.shape, want.shape)
        if want.dtype.kind in 'iu':
            assert h.dtype == np.int64 and np.array_equal(h, want.astype(np.int64))
        else:
            bits = {4: np.uint32, 8: np.uint64}[want.dtype.itemsize]
            assert h.dtype == want.dtype and h.flags.aligned
            assert np.array_equal(np.ascontiguousarray(h).view(bits), want.view(bits))
