"""Large-scale jitter on the device: mrcnn_prepare_image_crop and
mrcnn_mask_resize_crop through the C ABI, ``MaskRCNNTransform(scale_jitter=...)``, one train-chain
step on jittered examples and the train-loop tool.  Every reference is a composition of code that
predates the feature (tests/scale_jitter_ref.py; mrcnn_prepare_image at the full resized size and
a slice), so every comparison is exact."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import chainer_mask_rcnn_amd as cmr
import chainer_mask_rcnn_amd.datasets as D
from chainer_mask_rcnn_amd import _lib
from chainer_mask_rcnn_amd import functions as F
from chainer_mask_rcnn_amd.datasets import PackedMasks
from chainer_mask_rcnn_amd.datasets import transforms as T
from chainer_mask_rcnn_amd.functions import scale_jitter as SJ

import gt_masks_ref as GR
import scale_jitter_ref as R
import test_gpu_gt_masks as GM
import test_gpu_train_loop as TLT
from test_gpu_train_loop import TL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 37, 53
MEAN = np.array([122.7717, 115.9465, 102.9801], np.float32)
FRONT, REAR, FILL = 3, 64, 0xAB     # guard bytes around the mask output; FRONT misaligns it


def geometries(in_size, S):
    """name -> (scale, (rH, rW), (oy, ox)) for an ``in_size`` source on an S x S canvas: every
    combination of cropping and padding, the offsets at 0, inside and at their maximum."""
    h, w = in_size
    out = {}

    def add(name, scale, where):
        rH, rW = T._resized_size(in_size, scale)
        my, mx = max(rH - S, 0), max(rW - S, 0)
        oy, ox = {'zero': (0, 0), 'inside': (my // 2, mx // 2), 'max': (my, mx)}[where]
        out[name] = (scale, (rH, rW), (oy, ox))

    add('padded', (S - 5.) / max(h, w), 'zero')                       # rH, rW < S
    add('half', 0.5, 'zero')
    for where in ('zero', 'inside', 'max'):
        add('cropped-' + where, (S + 20.) / min(h, w), where)        # rH, rW > S
        add('mixed-' + where, (S + 10.) / max(h, w), where)          # longer side cropped only
    add('exact', float(S) / max(h, w), 'zero')                        # longer side == S
    assert max(out['exact'][1]) == S and max(out['padded'][1]) < S
    assert min(out['cropped-max'][1]) > S and min(out['cropped-max'][2]) > 0
    assert max(out['mixed-max'][1]) > S > min(out['mixed-max'][1]) and 0 in out['mixed-max'][2]
    return out


# ---- image ---------------------------------------------------------------------------------------
def _prepare_full(dev, src, scale, resized, x_flip, dst_size=None):
    """mrcnn_prepare_image (the kernel of the parent) into a zeroed buffer -> (dH, dW, 3) host."""
    dH, dW = dst_size or resized
    dst = torch.zeros((1, dH, dW, 3), dtype=torch.float32, device=dev)
    mean = (_lib.c_f32 * 3)(*MEAN)
    _lib.call('mrcnn_prepare_image', _lib.ptr(src), int(src.dtype == torch.uint8), 3, H, W,
              float(scale), mean, _lib.ptr(dst), dH, dW, resized[0], resized[1], 0, int(x_flip),
              _lib.stream_ptr())
    return dst[0].cpu().numpy()


def _prepare_crop(dev, src, scale, resized, offset, S, x_flip, n=0, N=1):
    dst = torch.full((N, S, S, 3), float('nan'), dtype=torch.float32, device=dev)
    mean = (_lib.c_f32 * 3)(*MEAN)
    rc = _lib.load().mrcnn_prepare_image_crop(
        _lib.ptr(src), int(src.dtype == torch.uint8), 3, H, W, float(scale), mean, _lib.ptr(dst), S, S,
        resized[0], resized[1], offset[0], offset[1], n, int(x_flip), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, dst.cpu().numpy()


def _sources(dev):
    rng = np.random.RandomState(2)
    u8 = rng.randint(0, 256, (3, H, W)).astype(np.uint8)
    f32 = rng.uniform(0, 255, (3, H, W)).astype(np.float32)
    return {'uint8': (u8, torch.from_numpy(u8).to(dev)), 'float32': (f32, torch.from_numpy(f32).to(dev))}


@pytest.mark.parametrize('x_flip', [False, True])
@pytest.mark.parametrize('dtype', ['uint8', 'float32'])
def test_image_kernel_equals_prepare_and_slice(dev, dtype, x_flip):
    host, src = _sources(dev)[dtype]
    for S in (47, 48, 64):                              # an odd S: rows start off dword alignment
        for name, (scale, resized, offset) in geometries((H, W), S).items():
            what = (S, name, resized, offset)
            full = _prepare_full(dev, src, scale, resized, x_flip)        # (rH, rW, 3)
            want = R.crop_pad(full.transpose(2, 0, 1), offset, S).transpose(1, 2, 0)
            rc, got = _prepare_crop(dev, src, scale, resized, offset, S, x_flip)
            assert rc == 0 and not np.isnan(got).any(), what             # the whole slot is written
            assert np.array_equal(got[0], want), what
            assert (want[min(resized[0] - offset[0], S):] == 0).all()
            if offset == (0, 0) and max(resized) <= S:
                # the plain path on an S x S canvas: mrcnn_prepare_image into a zeroed buffer
                assert np.array_equal(got[0], _prepare_full(dev, src, scale, resized, x_flip, (S, S))), what
        # the wrapper: same kernel from a host image, a channels-last (3, S, S) view
        scale, resized, offset = geometries((H, W), S)['cropped-inside']
        x = F.prepare_image_crop(MEAN, host, scale, resized, offset, S, x_flip, dev)
        assert tuple(x.shape) == (3, S, S) and x.stride() == (1, 3 * S, 3) and x.is_cuda
        _, want = _prepare_crop(dev, src, scale, resized, offset, S, x_flip)
        assert np.array_equal(x.permute(1, 2, 0).cpu().numpy(), want[0])


def test_image_kernel_slot_and_arguments(dev):
    _, src = _sources(dev)['uint8']
    S = 48
    scale, resized, offset = geometries((H, W), S)['mixed-inside']
    # image 1 of a batch of two: slot 0 stays as it was
    rc, got = _prepare_crop(dev, src, scale, resized, offset, S, True, n=1, N=2)
    assert rc == 0 and np.isnan(got[0]).all()
    assert np.array_equal(got[1], _prepare_crop(dev, src, scale, resized, offset, S, True)[1][0])
    lib, mean = _lib.load(), (_lib.c_f32 * 3)(*MEAN)
    dst = torch.zeros((1, S, S, 3), dtype=torch.float32, device=dev)

    def call(src_p=_lib.ptr(src), dst_p=_lib.ptr(dst), C=3, scale=1.0, S=S, rH=H, rW=W, oy=0, ox=0):
        return lib.mrcnn_prepare_image_crop(src_p, 1, C, H, W, scale, mean, dst_p, S, S, rH, rW, oy,
                                            ox, 0, 0, None)
    assert call() == 0
    for kw, msg in ((dict(src_p=None), b'null pointer'), (dict(dst_p=None), b'null pointer'),
                    (dict(C=4), b'3-channel'), (dict(scale=0.), b'3-channel'),
                    (dict(S=0), b'bad sizes'), (dict(rH=0), b'bad sizes'),
                    (dict(oy=-1), b'outside the resized image'), (dict(oy=H), b'outside the resized image'),
                    (dict(ox=W), b'outside the resized image')):
        assert call(**kw) != 0 and msg in lib.mrcnn_last_error(), kw
    torch.cuda.synchronize()
    with pytest.raises(_lib.MrcnnHipError):
        F.prepare_image_crop(MEAN, np.zeros((3, 4, 4), np.uint8), 1.0, (4, 4), (0, 0), 4, False, 'cpu')


# ---- masks ---------------------------------------------------------------------------------------
def _launch_masks(dev, packed, ys, xs, S):
    """mrcnn_mask_resize_crop on guarded buffers -> (rc, masks, boxes, areas, guards intact)."""
    G, h, w = packed.shape
    n = G * S * S
    buf = torch.full((FRONT + n + REAR,), FILL, dtype=torch.uint8, device=dev)
    meta = torch.full((4 + 5 * G + 4,), -77, dtype=torch.int32, device=dev)   # guard | box | area | guard
    stats = torch.full((3 * G * S + 4,), -77, dtype=torch.int32, device=dev)
    words = torch.from_numpy(packed.words.view(np.int64)).to(dev)
    ys_d = torch.from_numpy(np.asarray(ys, np.int32)).to(dev)
    xs_d = torch.from_numpy(np.asarray(xs, np.int32)).to(dev)
    rc = _lib.load().mrcnn_mask_resize_crop(
        _lib.ptr(words) if words.numel() else None, G, h, w, _lib.ptr(ys_d), _lib.ptr(xs_d), S,
        _lib.c_vp(buf.data_ptr() + FRONT), _lib.ptr(meta[4:]), _lib.ptr(meta[4 + 4 * G:]),
        _lib.ptr(stats), _lib.stream_ptr())
    torch.cuda.synchronize()
    host, meta, stats = buf.cpu().numpy(), meta.cpu().numpy(), stats.cpu().numpy()
    intact = bool((host[:FRONT] == FILL).all() and (host[FRONT + n:] == FILL).all()
                  and (meta[:4] == -77).all() and (meta[4 + 5 * G:] == -77).all()
                  and (stats[3 * G * S:] == -77).all())
    return (rc, host[FRONT:FRONT + n].reshape(G, S, S), meta[4:4 + 4 * G].reshape(G, 4),
            meta[4 + 4 * G:4 + 5 * G], intact)


def _special_instances(h, w):
    """(8, h, w): a corner block (outside an interior crop), a bar across the width and one across
    the height (cut by the left / right and the top / bottom crop edges), one pixel, the full
    image, a 1-pixel column, a block in the middle, nothing."""
    m = np.zeros((8, h, w), np.int32)
    m[0, :2, :2] = 1
    m[1, h // 2 - 1:h // 2 + 1, :] = 1
    m[2, :, w // 2 - 1:w // 2 + 1] = 1
    m[3, h // 2, w // 2] = 1
    m[4] = 1
    m[5, 10:14, 23] = 1
    m[6, h // 3:2 * h // 3, w // 3:2 * w // 3] = 1
    return m


def _masks(rng, G, h, w):
    if G < 8:
        return GR.random_masks(rng, G, h, w)
    m = GR.random_masks(rng, G, h, w)
    m[:8] = _special_instances(h, w)
    return m


@pytest.mark.parametrize('x_flip', [False, True])
@pytest.mark.parametrize('G', [0, 1, 3, 65])
def test_mask_kernel_equals_resize_and_slice(dev, G, x_flip):
    rng = np.random.RandomState(10 * G + x_flip)
    for w in (53, 64, 65, 130):
        m = _masks(rng, G, H, w)
        p = PackedMasks.from_dense(m)
        for S in (47, 48, 64):
            for name, (scale, resized, offset) in geometries((H, w), S).items():
                what = (w, S, name, resized, offset)
                ys, xs = SJ.crop_tables((H, w), resized, offset, S, x_flip)
                rc, got, boxes, areas, intact = _launch_masks(dev, p, ys, xs, S)
                assert rc == 0 and intact, what
                want = R.crop_masks(m, resized, offset, S, x_flip)
                want_boxes, want_areas = R.boxes_areas(want)
                assert np.array_equal(got, want), what
                assert np.array_equal(boxes, want_boxes) and np.array_equal(areas, want_areas), what
                if G == 65 and name == 'cropped-inside':
                    # the corner block is wholly outside; the bars are cut by the canvas edges
                    assert m[0].any() and areas[0] == 0 and tuple(boxes[0]) == (0, 0, 0, 0), what
                    assert boxes[1][1] == 0 and boxes[1][3] == S and boxes[1][0] > 0, what
                    assert boxes[2][0] == 0 and boxes[2][2] == S and boxes[2][1] > 0, what
                    assert tuple(boxes[4]) == (0, 0, S, S) and areas[4] == S * S, what
                    assert areas[7] == 0 and areas[3] >= 1
                if G == 65 and name == 'half' and w == 53:
                    assert m[5].sum() == 4 and areas[5] == 0, what     # the thin column vanishes
                if name in ('cropped-inside', 'padded'):
                    out, b, a = F.resize_crop_masks(F.upload_packed_masks(p, dev), resized, offset, S,
                                                    x_flip)
                    assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous()
                    assert b.dtype == a.dtype == torch.int32 and tuple(b.shape) == (G, 4)
                    assert tuple(out.shape) == (G, S, S) and tuple(a.shape) == (G,)
                    assert np.array_equal(out.cpu().numpy(), want), what
                    assert np.array_equal(b.cpu().numpy(), want_boxes), what
                    assert np.array_equal(a.cpu().numpy(), want_areas), what


def test_mask_kernel_edges(dev):
    rng = np.random.RandomState(5)
    h, w, S = 9, 70, 7
    m = GR.random_masks(rng, 3, h, w)
    p = PackedMasks.from_dense(m)
    # table entries past the end are clamped, every negative entry is "outside"; nothing is
    # written outside the outputs
    ys = np.array([-5, 0, h - 1, h + 9, 4, -1, 2], np.int32)
    xs = np.array([-5, w - 1, w + 9, 3, 64, 63, -(1 << 31)], np.int64).astype(np.int32)
    rc, got, boxes, areas, intact = _launch_masks(dev, p, ys, xs, S)
    assert rc == 0 and intact
    want = m[:, np.clip(ys, 0, h - 1)][:, :, np.clip(xs, 0, w - 1)].astype(np.uint8)
    want[:, ys < 0, :] = 0
    want[:, :, xs < 0] = 0
    assert np.array_equal(got, want) and want[1, 1:5, 1:6].all()
    want_boxes, want_areas = R.boxes_areas(want)
    assert np.array_equal(boxes, want_boxes) and np.array_equal(areas, want_areas)
    assert tuple(boxes[0]) == (0, 0, 0, 0) and tuple(boxes[1]) == (1, 1, 7, 6) and areas[1] == 25
    # no instances: success, nothing written
    rc, got, boxes, areas, intact = _launch_masks(dev, p[0:0], ys, xs, S)
    assert rc == 0 and intact and got.shape == (0, S, S)
    out, b, a = F.resize_crop_masks(F.upload_packed_masks(p[0:0], dev), (12, 90), (0, 5), 16)
    assert tuple(out.shape) == (0, 16, 16) and tuple(b.shape) == (0, 4) and tuple(a.shape) == (0,)
    # argument errors carry a message
    lib = _lib.load()
    buf = torch.zeros(256, dtype=torch.int64, device=dev)
    q = _lib.ptr(buf)
    ok = [q, 1, 4, 4, q, q, 2, q, q, q, q, None]
    assert lib.mrcnn_mask_resize_crop(*ok) == 0
    for i in (0, 4, 5, 7, 8, 9, 10):
        args = list(ok)
        args[i] = None
        assert lib.mrcnn_mask_resize_crop(*args) != 0
        assert b'mask_resize_crop: null pointer' in lib.mrcnn_last_error()
    for i, bad in ((1, -1), (2, 0), (3, 0), (6, 0)):
        args = list(ok)
        args[i] = bad
        assert lib.mrcnn_mask_resize_crop(*args) != 0
        assert b'mask_resize_crop: bad shape' in lib.mrcnn_last_error()
    args = list(ok)
    args[1], args[6] = 4, 1 << 15
    assert lib.mrcnn_mask_resize_crop(*args) != 0 and b'>= 2^31' in lib.mrcnn_last_error()
    torch.cuda.synchronize()
    with pytest.raises(_lib.MrcnnHipError):
        F.resize_crop_masks((torch.zeros((1, 4, 1), dtype=torch.int64), 4), (2, 2), (0, 0), 2)


# ---- transform -----------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def small(dev, tmp_path_factory):
    """The small model of tests/test_gpu_train_loop.py over its 5-image COCO directory."""
    root = os.path.join(str(tmp_path_factory.mktemp('scale_jitter')), 'COCO')
    TLT._write_coco(root)
    data = cmr.datasets.COCOInstanceSegmentationDataset('minival', root_dir=root)
    packed = cmr.datasets.COCOInstanceSegmentationDataset('minival', root_dir=root, packed_masks=True)
    loop, model, chain, opt, train = TLT._build(dev, data, prefetch=False)
    loop.close()
    return dict(data=data, packed=packed, model=model, chain=chain)


def _image_ref(model, dev):
    """The image of the reference composition: MaskRCNN.prepare's kernel at the full resized size
    with the same flip, sliced and zero-padded on the host -> (3, S, S)."""
    mean = (_lib.c_f32 * 3)(*[float(v) for v in np.asarray(model.mean).ravel()])

    def image(chw, scale, resized, offset, x_flip, S):
        src = torch.from_numpy(np.ascontiguousarray(chw)).to(dev)
        dst = torch.zeros((1, resized[0], resized[1], 3), dtype=torch.float32, device=dev)
        _lib.call('mrcnn_prepare_image', _lib.ptr(src), int(chw.dtype == np.uint8), 3, chw.shape[1],
                  chw.shape[2], float(scale), mean, _lib.ptr(dst), resized[0], resized[1], resized[0],
                  resized[1], 0, int(x_flip), _lib.stream_ptr())
        return R.crop_pad(dst[0].cpu().numpy().transpose(2, 0, 1), offset, S)
    return image


def _check_example(got, want, S, after):
    x, bbox, label, mask, scale = got
    assert random.random() == after
    assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (3, S, S)
    assert x.stride() == (1, 3 * S, 3)                                   # channels-last view
    assert np.array_equal(x.cpu().numpy(), want[0])
    assert bbox.dtype == np.float32 and np.array_equal(bbox, want[1])
    assert np.array_equal(label, want[2]) and label.dtype == want[2].dtype and scale == want[4]
    assert mask.is_cuda and mask.dtype == torch.uint8 and mask.is_contiguous()
    assert tuple(mask.shape) == want[3].shape and np.array_equal(mask.cpu().numpy(), want[3])


def test_transform_equals_reference_composition(dev, small):
    model, data, packed = small['model'], small['data'], small['packed']
    S, jitter = 64, (0.5, 2.0)
    image = _image_ref(model, dev)
    ex, ex_packed = data[2], packed[2]
    assert isinstance(ex_packed[3], PackedMasks) and len(ex[3]) == 3
    crowd, area = np.array([0, 1, 0], np.int32), np.array([5., 6., 7.], np.float32)
    flips, dropped = set(), 0
    for seed in range(12):
        random.seed(seed)
        want = R.transform(ex, jitter, S, lambda *a: image(*a, S))
        after = random.random()
        assert want[5] is not None                       # an attempt was accepted
        random.seed(seed)
        flips.add(random.choice([True, False]))
        dropped += len(want[2]) < 3
        t = D.MaskRCNNTransform(model, device_masks=True, scale_jitter=jitter, crop_size=S)
        for example in (ex, ex_packed, ex + (crowd, area)):             # dense, packed, with extras
            random.seed(seed)
            got = t(example)
            assert len(got) == 5
            _check_example(got, want, S, after)
        # every returned box is the tight box of its returned mask; nothing empty is returned
        boxes, areas = R.boxes_areas(got[3].cpu().numpy())
        assert np.array_equal(got[1], boxes.astype(np.float32)) and (areas >= 1).all()
        assert len(got[1]) == len(got[2]) == len(got[3]) >= 1
    assert flips == {False, True} and dropped >= 1
    # a 2-D mask keeps its 2-D form
    random.seed(3)
    flat = (ex[0], ex[1][1:2], ex[2][1:2], ex[3][1])
    want = R.transform(flat, jitter, S, lambda *a: image(*a, S))
    after = random.random()
    random.seed(3)
    got = D.MaskRCNNTransform(model, device_masks=True, scale_jitter=jitter, crop_size=S)(flat)
    assert got[3].dim() == 2 and want[3].ndim == 2
    _check_example(got, want, S, after)
    # no instances: nothing but the flip is drawn, the plain path on the canvas
    empty = (ex[0], np.zeros((0, 4), np.float32), np.zeros((0,), np.int32), ex_packed[3][0:0])
    random.seed(3)
    want = R.transform(empty, jitter, S, lambda *a: image(*a, S))
    after = random.random()
    random.seed(3)
    random.choice([True, False])
    assert random.random() == after and want[5] is None
    random.seed(3)
    got = D.MaskRCNNTransform(model, device_masks=True, scale_jitter=jitter, crop_size=S)(empty)
    _check_example(got, want, S, after)
    assert tuple(got[3].shape) == (0, S, S) and got[1].shape == (0, 4)
    assert got[4] == min(S / 96., S / 128.)


def test_transform_redraws_and_falls_back(dev, small):
    model = small['model']
    S, jitter = 16, (2.0, 2.0)
    image = _image_ref(model, dev)
    rng = np.random.RandomState(1)
    mask = np.zeros((1, 40, 40), np.int32)
    mask[0, :3, :3] = 1
    ex = (rng.randint(0, 256, (40, 40, 3)).astype(np.uint8), np.array([[0, 0, 3, 3]], np.float32),
          np.array([5], np.int32), mask)
    t = D.MaskRCNNTransform(model, device_masks=True, scale_jitter=jitter, crop_size=S)
    # find, from the host geometry and the NumPy reference alone, a seed whose attempt k > 1 is the
    # first to keep the blob and one where all eight attempts lose it
    found = {}
    for seed in range(512):
        random.seed(seed)
        x_flip = random.choice([True, False])
        first = None
        for k in range(1, R.ATTEMPTS + 1):
            scale, resized, offset = T.draw_scale_jitter((40, 40), S, jitter)
            if first is None and R.crop_masks(mask, resized, offset, S, x_flip).any():
                first = k
        assert (scale, resized) == (0.8, (32, 32))
        kind = 'fallback' if first is None else ('redraw' if first > 1 else 'first')
        found.setdefault(kind, (seed, first))
    assert 'redraw' in found and 'fallback' in found

    seed, k = found['redraw']
    random.seed(seed)
    want = R.transform(ex, jitter, S, lambda *a: image(*a, S))
    after = random.random()
    assert want[5] == k
    random.seed(seed)
    random.choice([True, False])
    for _ in range(k):
        random.uniform(*jitter), random.random(), random.random()
    assert random.random() == after                      # 1 + 3 k draws
    random.seed(seed)
    got = t(ex)
    _check_example(got, want, S, after)
    assert len(got[3]) == 1 and got[3].any()

    seed, _ = found['fallback']
    random.seed(seed)
    x_flip = random.choice([True, False])
    for _ in range(R.ATTEMPTS):
        random.uniform(*jitter), random.random(), random.random()
    after = random.random()                              # exactly 1 + 3 * 8 draws
    random.seed(seed)
    want = R.transform(ex, jitter, S, lambda *a: image(*a, S))
    assert want[5] is None and random.random() == after
    random.seed(seed)
    got = t(ex)
    _check_example(got, want, S, after)
    # the instance is kept, with the plain path's box: the given box resized and flipped
    box = T.flip_bbox(T.resize_bbox(ex[1], (40, 40), (16, 16)), (16, 16), x_flip=x_flip)
    assert got[4] == 0.4 and len(got[3]) == 1 and np.array_equal(got[1], box)
    assert np.array_equal(got[2], ex[2])
    assert np.array_equal(got[3].cpu().numpy(), T.resize_nearest(mask, (16, 16), x_flip=x_flip))


def test_transform_without_jitter_is_unchanged(dev, small):
    model, ex = small['model'], small['packed'][2]
    for seed in (0, 1, 2, 3):
        random.seed(seed)
        want = D.MaskRCNNTransform(model, device_masks=True)(ex)
        after = random.random()
        random.seed(seed)
        got = D.MaskRCNNTransform(model, True, True, scale_jitter=None, crop_size=64)(ex)
        assert random.random() == after
        random.seed(seed)
        random.choice([True, False])
        assert random.random() == after                  # the flip is the only draw
        assert torch.equal(got[0], want[0]) and got[0].stride() == want[0].stride()
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        assert torch.equal(got[3], want[3]) and got[4] == want[4]
        assert tuple(got[0].shape[1:]) != (64, 64)


# ---- train step ----------------------------------------------------------------------------------
def test_chain_step_on_jittered_examples(dev, small, monkeypatch):
    model, chain, packed = small['model'], small['chain'], small['packed']
    S = 96
    t = D.MaskRCNNTransform(model, device_masks=True, scale_jitter=(0.5, 2.0), crop_size=S)
    runs = []
    for _ in range(2):
        random.seed(7)
        batch = TL.make_converter(dev)([t(packed[j]) for j in (2, 4)])
        imgs, bboxes, labels, masks, scales = batch
        assert tuple(imgs.shape) == (2, 3, S, S) and imgs.is_cuda
        assert imgs.is_contiguous(memory_format=torch.channels_last)
        assert isinstance(masks, torch.Tensor) and masks.is_cuda and masks.dtype == torch.uint8
        assert masks.is_contiguous() and masks.dim() == 4 and tuple(masks.shape[2:]) == (S, S)
        with monkeypatch.context() as mp:
            mp.setattr(torch.Tensor, 'cpu', GM._no_mask_download(masks, torch.Tensor.cpu))
            np.random.seed(11)
            loss = chain(*batch)
            torch.cuda.synchronize()
        report = {k: float(v) for k, v in chain.report.items()}
        assert np.isfinite(float(loss.detach())) and all(np.isfinite(v) for v in report.values())
        runs.append((float(loss.detach()), report, imgs.cpu().numpy(), masks.cpu().numpy(),
                     [np.asarray(b) for b in bboxes], random.random()))
    a, b = runs
    assert a[0] == b[0] and a[1] == b[1] and a[5] == b[5]
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    assert all(np.array_equal(p, q) for p, q in zip(a[4], b[4]))


# ---- tool ----------------------------------------------------------------------------------------
def test_train_loop_tool_with_scale_jitter(dev):
    env = dict(os.environ, WARMUP='1')
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'train_loop.py'), '--synthetic', '4',
                          '--iterations', '2', '--device-masks', '--scale-jitter', '0.5,2.0',
                          '--crop-size', '256'], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert '2 iterations' in out.stdout and 'loss' in out.stdout
    assert 'nan' not in out.stdout.lower()
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'train_loop.py'), '--synthetic', '4',
                          '--scale-jitter', '0.5,2.0'], capture_output=True, text=True, timeout=600)
    assert out.returncode == 2 and '--scale-jitter needs --device-masks' in out.stderr
