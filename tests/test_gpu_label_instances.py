"""utils.label2instance_boxes / instance_boxes2label on the MI355X: bit-exact against the
fixture produced by the reference's own functions (int32 and uint8 images, host arrays and
device tensors), exact against the NumPy restatement on large random images, the 2^24 limits,
the reference's assertion, and the device masks feeding pack_masks."""
import os

import numpy as np
import pytest
import torch

import label_instances_ref as R
from chainer_mask_rcnn_amd import utils
from chainer_mask_rcnn_amd.utils import geometry
from chainer_mask_rcnn_amd.utils.evaluations.masks import pack_masks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'label_instances.npz'))


def unpack(d, key):
    shape = tuple(d[key + '_shape'])
    return np.unpackbits(d[key], axis=-1)[..., :shape[-1]].reshape(shape).astype(bool)


def as_u8(a):
    """int32 labels -> the uint8 encoding (255 = -1), or None when a value does not fit."""
    if a.size and (a.min() < -1 or a.max() > 254):
        return None
    return np.where(a == -1, 255, a).astype(np.uint8)


def check_host(got, d, name):
    classes, boxes, masks = got
    assert classes.dtype == np.int32 and np.array_equal(classes, d[name + '_classes']), name
    assert boxes.dtype == np.int32 and np.array_equal(boxes, d[name + '_boxes']), name
    assert masks.dtype == bool and np.array_equal(masks, unpack(d, name + '_masks')), name


def test_fixture_bit_exact_host_and_device(dev, golden):
    n_u8 = 0
    for name in golden['cases']:
        ins, cls = golden[name + '_ins'], golden[name + '_cls']
        inputs = [(ins, cls)]
        if as_u8(ins) is not None and as_u8(cls) is not None:
            inputs.append((as_u8(ins), as_u8(cls)))
            inputs.append((as_u8(ins), cls))
            n_u8 += 1
        for a, b in inputs:
            check_host(utils.label2instance_boxes(a, b, return_masks=True), golden, name)
            c2, b2 = utils.label2instance_boxes(a, b)
            assert np.array_equal(c2, golden[name + '_classes']) and b2.shape[1] == 4
            ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
            classes, boxes, masks = utils.label2instance_boxes(ta, tb, return_masks=True)
            for t in (classes, boxes, masks):
                assert isinstance(t, torch.Tensor) and t.is_cuda
            assert classes.dtype == torch.int32 and boxes.dtype == torch.int32
            assert masks.dtype == torch.bool
            check_host((classes.cpu().numpy(), boxes.cpu().numpy(), masks.cpu().numpy()), golden,
                       name)
    assert n_u8 >= 8


def test_voc_raw_labels_with_mask_by_class(dev, golden):
    raw_ins, raw_cls = golden['voc_like_raw_ins'], golden['voc_like_raw_cls']
    assert raw_ins.dtype == np.uint8
    check_host(utils.label2instance_boxes(raw_ins, raw_cls, return_masks=True, mask_by_class=True),
               golden, 'voc_like')
    # without mask_by_class the PNG background (index 0) is instance 0 of class 0: the
    # reference's assertion, as on the int32 decoding of the same pair
    with pytest.raises(AssertionError):
        utils.label2instance_boxes(raw_ins, raw_cls)
    # with the background voided by hand, the 255 specks inside instances still count as -1
    # classes (a minority): equal to the restatement on the int32 decoding
    ins = raw_ins.astype(np.int32)
    ins[(ins == 255) | (ins == 0)] = -1
    cls = raw_cls.astype(np.int32)
    cls[cls == 255] = -1
    exp = R.label2instance_boxes(ins, cls, return_masks=True)
    got = utils.label2instance_boxes(np.where(ins == -1, 255, ins).astype(np.uint8), raw_cls,
                                     return_masks=True)
    for g, e in zip(got, exp):
        assert np.array_equal(g, e)


def _random_image(rng, H, W, n, n_cls, id_lo, id_hi):
    ids = np.concatenate([[id_lo, id_hi], rng.randint(id_lo, id_hi, n - 2)]).astype(np.int64)
    ids = np.unique(ids)
    rng.shuffle(ids)
    ins = -np.ones((H, W), np.int64)
    cls = np.zeros((H, W), np.int64)
    for i in ids:
        y0, x0 = rng.randint(0, H), rng.randint(0, W)
        y1, x1 = min(H, y0 + rng.randint(1, 300)), min(W, x0 + rng.randint(1, 400))
        ins[y0:y1, x0:x1] = i
        cls[y0:y1, x0:x1] = rng.randint(1, n_cls + 1)
    noise = rng.uniform(size=(H, W)) < 0.3
    cls[noise] = rng.randint(1, n_cls + 1, noise.sum())
    ins[0, 0], ins[H - 1, W - 1] = id_lo, id_hi       # both ends of the window stay present
    cls[0, 0], cls[H - 1, W - 1] = 1, n_cls
    return ins.astype(np.int32), cls.astype(np.int32)


def test_random_large_images_exact_and_reproducible(dev):
    rng = np.random.RandomState(3)
    H, W = 800, 1333
    base = -(1 << 23) + 17
    ins, cls = _random_image(rng, H, W, 200, 81, base, base + (1 << 24) - 1)   # full window
    assert int(np.ptp(ins[ins != -1])) == (1 << 24) - 1
    exp = R.label2instance_boxes(ins, cls, return_masks=True)
    got = utils.label2instance_boxes(ins, cls, return_masks=True)
    for g, e in zip(got, exp):
        assert np.array_equal(g, e)
    t = (torch.from_numpy(ins).to(dev), torch.from_numpy(cls).to(dev))
    a = utils.label2instance_boxes(*t, return_masks=True)
    b = utils.label2instance_boxes(*t, return_masks=True)
    for x, y, e in zip(a, b, exp):
        assert torch.equal(x, y) and np.array_equal(x.cpu().numpy(), e)
    # the ids of the device entry point: the ascending unique values
    ids = geometry.label_instances(*t)[0]
    assert np.array_equal(ids.cpu().numpy(), np.unique(ins[ins != -1]))
    # per-pixel noise: every pixel its own run, the worst case of the run reduction
    ins = rng.randint(-1, 50, (257, 301)).astype(np.int32)
    cls = rng.randint(1, 9, (257, 301)).astype(np.int32)
    for g, e in zip(utils.label2instance_boxes(ins, cls, return_masks=True),
                    R.label2instance_boxes(ins, cls, return_masks=True)):
        assert np.array_equal(g, e)


def test_limits_and_reference_assertion(dev):
    ins = np.full((4, 5), -1, np.int32)
    cls = np.ones((4, 5), np.int32)
    ins[0, 0], ins[3, 4] = 0, 1 << 24                       # span 2^24 + 1
    with pytest.raises(ValueError, match='2\\^24'):
        utils.label2instance_boxes(ins, cls)
    ins[3, 4] = (1 << 24) - 1                               # span exactly 2^24: fine
    assert len(utils.label2instance_boxes(ins, cls)[0]) == 2
    cls[3, 4] = 1 + (1 << 24)                               # class span 2^24 + 1
    with pytest.raises(ValueError, match='2\\^24'):
        utils.label2instance_boxes(ins, cls)
    n = 65 * 65                                             # 4225 x 4225 > 2^24 table entries
    ins = np.arange(n, dtype=np.int32).reshape(65, 65)
    with pytest.raises(ValueError, match='table'):
        utils.label2instance_boxes(ins, ins + 1)
    ins = np.array([[1, 1, 2, 2, -1]], np.int32)
    for bad in (0, -1):
        cls = np.array([[3, 3, bad, bad, 5]], np.int32)
        with pytest.raises(AssertionError):
            utils.label2instance_boxes(ins, cls)
        with pytest.raises(AssertionError):
            utils.label2instance_boxes(torch.from_numpy(ins).to(dev), torch.from_numpy(cls).to(dev))
    # a -1 class that loses the majority is fine
    cls = np.array([[3, 3, -1, 4, 4]], np.int32)
    ins = np.array([[1, 1, 1, 1, 1]], np.int32)
    assert utils.label2instance_boxes(ins, cls)[0].tolist() == [3]


def test_device_masks_feed_pack_masks(dev, golden):
    for name in ('voc_like', 'ids_gaps', 'borders_singletons'):
        t = [torch.from_numpy(golden[name + k]).to(dev) for k in ('_ins', '_cls')]
        _, _, masks = utils.label2instance_boxes(*t, return_masks=True)
        a = pack_masks(masks)
        b = pack_masks(unpack(golden, name + '_masks'))
        for x, y in zip(a, b):
            assert torch.equal(x, y), name


def test_instance_boxes2label_fixture(dev, golden):
    for name in golden['paint_cases']:
        p = 'paint_%s_' % name
        labels, masks = golden[p + 'labels'], unpack(golden, p + 'masks')
        scores = golden[p + 'scores'] if p + 'scores' in golden else None
        bboxes = np.zeros((len(labels), 4), np.float32)
        lbl_ins, lbl_cls = utils.instance_boxes2label(labels, bboxes, masks, scores)
        assert lbl_ins.dtype == np.int32 and np.array_equal(lbl_ins, golden[p + 'lbl_ins']), name
        assert lbl_cls.dtype == np.int32 and np.array_equal(lbl_cls, golden[p + 'lbl_cls']), name
        ti, tc = utils.instance_boxes2label(torch.from_numpy(labels).to(dev), bboxes,
                                            torch.from_numpy(masks).to(dev),
                                            None if scores is None else torch.from_numpy(scores))
        assert ti.is_cuda and np.array_equal(ti.cpu().numpy(), golden[p + 'lbl_ins']), name
        assert np.array_equal(tc.cpu().numpy(), golden[p + 'lbl_cls']), name
    with pytest.raises(AssertionError):
        utils.instance_boxes2label(np.array([0]), None, np.ones((1, 2, 2), bool))
    with pytest.raises(AssertionError):
        utils.instance_boxes2label(np.array([1]), None, np.ones((1, 2, 2), np.int32))


def test_mask_to_bbox_and_mask_overlap(dev):
    m = np.zeros((9, 11), bool)
    m[2:5, 3:8] = True
    m[7, 1] = True
    assert utils.mask_to_bbox(m) == (2, 1, 8, 8)
    assert utils.mask_to_bbox(torch.from_numpy(m).to(dev)) == (2, 1, 8, 8)
    with pytest.raises(ValueError):
        utils.mask_to_bbox(np.zeros((3, 3), bool))
    m2 = np.zeros_like(m)
    m2[3:6, 3:8] = True
    inter, union = (m & m2).sum(), (m | m2).sum()
    assert utils.get_mask_overlap(m, m2) == 1.0 * inter / union
    z = np.zeros_like(m)
    assert utils.get_mask_overlap(z, z) == 0. and utils.get_mask_overlap(z, z, True) == 0.5
