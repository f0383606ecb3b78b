"""datasets.PackedMasks (the packed format of include/mrcnn_hip.h on the host), the COCO dataset's
``packed_masks=True``, the host side of ``MaskRCNNTransform`` for packed input, and the NumPy
restatement of mrcnn_mask_resize_nearest (tests/gt_masks_ref.py) against
``datasets.transforms.resize_nearest``.  Integer data: every comparison is exact."""
import random

import numpy as np
import pytest

import chainer_mask_rcnn_amd.datasets as D
from chainer_mask_rcnn_amd.datasets import COCOInstanceSegmentationDataset, PackedMasks

import gt_masks_ref as R
from test_coco_dataset_cpu import coco_root  # noqa: F401  (fixture: the golden example's directory)
from test_datasets_cpu import _StubModel, _example


def _packbits_reference(m):
    """The header's definition: np.packbits(little) of rows zero-padded to a multiple of 64."""
    G, H, W = m.shape
    padded = np.zeros((G, H, (W + 63) // 64 * 64), bool)
    padded[..., :W] = m != 0
    return np.packbits(padded, axis=-1, bitorder='little')


@pytest.mark.parametrize('W', [1, 63, 64, 65, 130])
def test_from_dense_is_the_header_format(W):
    rng = np.random.RandomState(W)
    m = (rng.uniform(size=(3, 5, W)) > 0.5).astype(np.int32)
    m[1, :, -1] = 1                                   # the last pixel of a row, next to the pad bits
    p = PackedMasks.from_dense(m)
    assert p.words.dtype == np.uint64 and p.words.shape == (3, 5, (W + 63) // 64)
    assert p.words.flags['C_CONTIGUOUS']
    assert p.words.tobytes() == _packbits_reference(m).tobytes()
    assert (p.height, p.width) == (5, W) and p.shape == (3, 5, W) and p.ndim == 3 and len(p) == 3
    # bit x & 63 of word x >> 6 is the pixel
    for x in {0, W // 2, W - 1}:
        assert np.array_equal((p.words[:, :, x >> 6] >> np.uint64(x & 63)) & np.uint64(1), m[:, :, x])


def test_unpack_round_trips():
    rng = np.random.RandomState(0)
    for W in (1, 63, 64, 65, 130):
        m = (rng.uniform(size=(4, 7, W)) > 0.5).astype(np.int32)
        u = PackedMasks.from_dense(m).unpack()
        assert u.dtype == np.int32 and np.array_equal(u, m)
        assert PackedMasks.from_dense(m).unpack(np.uint8).dtype == np.uint8
    # any nonzero value is foreground
    v = rng.randint(-3, 4, (2, 6, 70)).astype(np.int32) * 85
    assert np.array_equal(PackedMasks.from_dense(v).unpack(), (v != 0).astype(np.int32))
    assert np.array_equal(PackedMasks.from_dense(v.astype(np.float32)).unpack(bool), v != 0)
    # no instances
    e = PackedMasks.from_dense(np.zeros((0, 6, 70), np.int32))
    assert len(e) == 0 and e.shape == (0, 6, 70) and e.words.shape == (0, 6, 2)
    assert e.unpack().shape == (0, 6, 70) and e.unpack().dtype == np.int32
    with pytest.raises(ValueError):
        PackedMasks.from_dense(np.zeros((6, 70), np.int32))
    with pytest.raises(ValueError):
        PackedMasks(np.zeros((1, 6, 1), np.uint64), 6, 70)


def test_from_instances_equals_from_dense():
    rng = np.random.RandomState(1)
    for W in (1, 64, 65, 130):
        m = rng.uniform(size=(3, 9, W)) > 0.5
        a, b = PackedMasks.from_instances(list(m), 9, W), PackedMasks.from_dense(m)
        assert a.shape == b.shape and a.words.tobytes() == b.words.tobytes()
    e = PackedMasks.from_instances([], 9, 70)
    assert e.shape == (0, 9, 70) and e.words.shape == (0, 9, 2) and e.words.dtype == np.uint64
    with pytest.raises(ValueError):
        PackedMasks.from_instances([np.zeros((9, 69), bool)], 9, 70)


def test_subsetting_equals_dense_subsetting():
    rng = np.random.RandomState(2)
    m = (rng.uniform(size=(5, 8, 67)) > 0.5).astype(np.int32)
    p = PackedMasks.from_dense(m)
    for key in (slice(1, 4), slice(None, None, 2), slice(0, 0), np.array([3, 0, 3]),
                np.zeros(0, np.int64), np.array([True, False, True, True, False]), [4, 1]):
        q = p[key]
        assert isinstance(q, PackedMasks) and q.shape == m[key].shape
        assert np.array_equal(q.unpack(), m[key])
        assert q.words.tobytes() == PackedMasks.from_dense(m[key]).words.tobytes()


@pytest.mark.parametrize('use_crowd', [False, True])
def test_coco_example_packed(coco_root, use_crowd):  # noqa: F811
    root, d = coco_root
    kw = dict(use_crowd=use_crowd, return_crowd=True, return_area=True, root_dir=root)
    dense = COCOInstanceSegmentationDataset('minival', **kw)
    packed = COCOInstanceSegmentationDataset('minival', packed_masks=True, **kw)
    tag = 'crowd' if use_crowd else 'nocrowd'
    ref_masks = np.unpackbits(d[tag + '_masks'], axis=-1)[..., :int(d['width'])].reshape(
        tuple(d[tag + '_masks_shape'])).astype(np.int32)
    for i in range(len(dense)):
        for a, b in ((dense[i], packed[i]), (dense.get_annotations(i), packed.get_annotations(i))):
            assert len(a) == len(b)
            pm = [f for f in b if isinstance(f, PackedMasks)]
            assert len(pm) == 1 and isinstance(b[-3], PackedMasks)
            for fa, fb in zip(a, b):
                if isinstance(fb, PackedMasks):
                    assert fb.shape == fa.shape and fb.unpack().dtype == fa.dtype == np.int32
                    assert np.array_equal(fb.unpack(), fa)
                else:
                    assert fa.dtype == fb.dtype and np.array_equal(fa, fb)
    assert np.array_equal(packed[0][3].unpack(), ref_masks)       # the committed masks
    assert isinstance(dense[0][3], np.ndarray)                    # the default is unchanged


@pytest.mark.parametrize('G', [1, 3])
@pytest.mark.parametrize('x_flip', [False, True])
def test_numpy_restatement_equals_resize_nearest(G, x_flip):
    rng = np.random.RandomState(3)
    for in_size, out_size in R.SHAPES:
        for fill in ((None, 0, 1) if G == 1 else (None,)):
            m = R.random_masks(rng, G, in_size[0], in_size[1], fill)
            want = D.resize_nearest(m, out_size, x_flip=x_flip)
            got = R.resize_masks_nearest(PackedMasks.from_dense(m), out_size, x_flip)
            assert got.dtype == np.uint8 and got.shape == want.shape
            assert np.array_equal(got, want)
    # tables out of range read the clamped pixel
    m = R.random_masks(rng, 3, 9, 70)
    ys, xs = np.array([-5, 0, 8, 9 + 9], np.int32), np.array([-5, 69, 70 + 9, 3], np.int32)
    got = R.resize_with_tables(PackedMasks.from_dense(m), ys, xs)
    assert np.array_equal(got, m[:, [0, 0, 8, 8]][:, :, [0, 69, 69, 3]])


@pytest.mark.parametrize('seed', [0, 1, 2, 3])
def test_transform_unpacks_packed_input_on_the_host_path(seed):
    """packed_masks=True alone never breaks a caller: without device_masks a PackedMasks takes
    today's host path and gives the same result and the same single draw from ``random``."""
    ex = _example(np.random.RandomState(seed))
    random.seed(seed)
    want = D.MaskRCNNTransform(_StubModel())(ex)
    after = random.random()
    random.seed(seed)
    got = D.MaskRCNNTransform(_StubModel())(ex[:3] + (PackedMasks.from_dense(ex[3]),))
    assert after == random.random()
    assert isinstance(got[3], np.ndarray) and got[3].dtype == np.int32
    for a, b in zip(want[1:], got[1:]):
        assert np.array_equal(a, b)
    # evaluation mode hands the mask field through untouched
    p = PackedMasks.from_dense(ex[3])
    assert D.MaskRCNNTransform(_StubModel(), train=False, device_masks=True)(ex[:3] + (p,))[3] is p
