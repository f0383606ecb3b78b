"""csrc/image.hip against the oracle (oracle/np_infer.py) past x = 256: prepare_kernel and
paste_masks_kernel take x from blockIdx.x * 256 + threadIdx.x, and every earlier comparison with
something independent stayed inside the first block of x.  Cases and checks are those of
tests/elementwise_cases.py (tests/test_elementwise_cases_cpu.py holds the conditions that make the
cases worth running); the tolerances are those of tests/test_gpu_inference.py."""
import ctypes

import numpy as np
import pytest
import torch

import chainer_mask_rcnn_amd as cmr
import elementwise_cases as EC
from chainer_mask_rcnn_amd import _lib
from oracle import np_infer

pytestmark = pytest.mark.gpu
f32 = np.float32


def _mean():
    return (_lib.c_f32 * 3)(*EC.MEAN)


@pytest.mark.parametrize('name', [c[0] for c in EC.PREPARE_CASES])
@pytest.mark.parametrize('flip', [0, 1])
def test_prepare_image_into_slot_one(dev, name, flip):
    """mrcnn_prepare_image directly: batch slot n = 1 of a two-image destination larger than the
    output; slot 0 and the padding of slot 1 keep the fill."""
    case = EC.prepare_case(name)
    img = case['img']
    _, H, W = img.shape
    outH, outW = case['ref'].shape[1:]
    dstH, dstW = outH + 3, outW + 5
    dst = torch.full((2, dstH, dstW, 3), EC.POISON, dtype=torch.int32, device=dev)
    src = torch.tensor(img, device=dev)
    _lib.call('mrcnn_prepare_image', _lib.ptr(src), int(img.dtype == np.uint8), 3, H, W,
              float(case['scale']), _mean(), _lib.ptr(dst), dstH, dstW, outH, outW, 1, flip,
              _lib.stream_ptr())
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    got = host[1, :outH, :outW].view(f32).transpose(2, 0, 1)
    EC.check_prepare(name, np.ascontiguousarray(got), bool(flip), '%s flip %d' % (name, flip))
    rest = host.copy()
    rest[1, :outH, :outW] = EC.POISON
    assert (rest == EC.POISON).all()


def test_model_prepare_at_these_widths(dev):
    """MaskRCNN.prepare: the scale rule (max_size takes over for the wide image), the batch
    assembly and the zero padding, with outputs 600 and 200 wide."""
    case = EC.prepare_case('maxsize-u8-3blocks')
    min_size, max_size = case['min_size'], case['max_size']
    small = np.random.RandomState(11).uniform(0, 255, (3, 60, 100)).astype(f32)
    model = cmr.models.MaskRCNN(torch.nn.Linear(1, 1).to(dev), None, None,
                                mean=np.asarray(EC.MEAN, f32).reshape(3, 1, 1),
                                min_size=min_size, max_size=max_size)
    x, sizes, scales = model.prepare([case['img'], small], x_flips=[False, True])
    x = x.cpu().numpy()
    ref1, scale1 = np_infer.prepare(small, EC.MEAN, min_size, max_size)
    assert sizes == [(90, 700), (60, 100)] and scales == [case['scale'], scale1]
    assert scales[0] == max_size / 700 and scale1 == 2.
    assert x.shape == (2, 3, 120, 600) and ref1.shape == (3, 120, 200)
    h, w = case['ref'].shape[1:]
    EC.check_prepare('maxsize-u8-3blocks', np.ascontiguousarray(x[0, :, :h, :w]))
    np.testing.assert_allclose(x[1, :, :, :200], ref1[:, :, ::-1], rtol=0, atol=2e-4)
    assert (x[0, :, h:, :] == 0).all() and (x[1, :, :, 200:] == 0).all()


def _guarded_bytes(dev, n, fill=0xAB, guard=64):
    buf = torch.full((n + 2 * guard,), fill, dtype=torch.uint8, device=dev)
    return buf, guard


@pytest.mark.parametrize('im_w', EC.PASTE_WIDTHS)
def test_paste_dense_and_packed(dev, im_w):
    case = EC.paste_case(im_w)
    D, im_h = len(case['bbox']), case['im_h']
    M, Kc = EC.PASTE_M, EC.PASTE_NFG
    logits = torch.tensor(np.ascontiguousarray(case['logits'].transpose(0, 2, 3, 1)), device=dev)
    label, bbox = torch.tensor(case['label'], device=dev), torch.tensor(case['bbox'], device=dev)
    n = D * im_h * im_w
    buf, g = _guarded_bytes(dev, n)
    _lib.call('mrcnn_paste_masks', _lib.ptr(logits), _lib.ptr(label), _lib.ptr(bbox), D, M, Kc, im_h,
              im_w, ctypes.c_void_p(buf.data_ptr() + g), _lib.stream_ptr())
    Wq = (im_w + 63) // 64
    packed = torch.full((D * im_h * Wq + 16,), -1, dtype=torch.int64, device=dev)
    area = torch.full((D + 8,), -7, dtype=torch.int32, device=dev)
    extent = torch.full((4 * D + 8,), -7, dtype=torch.int32, device=dev)
    _lib.call('mrcnn_paste_masks_packed', _lib.ptr(logits), _lib.ptr(label), _lib.ptr(bbox), D, M, Kc,
              im_h, im_w, ctypes.c_void_p(packed.data_ptr() + 64), ctypes.c_void_p(area.data_ptr() + 16),
              ctypes.c_void_p(extent.data_ptr() + 16), _lib.stream_ptr())
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:g] == 0xAB).all() and (host[g + n:] == 0xAB).all()
    EC.check_paste(case, host[g:g + n].reshape(D, im_h, im_w))
    p, a, e = packed.cpu().numpy(), area.cpu().numpy(), extent.cpu().numpy()
    assert (p[:8] == -1).all() and (p[8 + D * im_h * Wq:] == -1).all()
    assert (a[:4] == -7).all() and (a[4 + D:] == -7).all()
    assert (e[:4] == -7).all() and (e[4 + 4 * D:] == -7).all()
    EC.check_paste_packed(case, p[8:8 + D * im_h * Wq].reshape(D, im_h, Wq), a[4:4 + D],
                          e[4:4 + 4 * D].reshape(D, 4))


def test_paste_of_no_detections_writes_nothing(dev):
    im_h, im_w = EC.PASTE_H, 300
    one = torch.zeros((1, EC.PASTE_M, EC.PASTE_M, EC.PASTE_NFG), device=dev)
    label, bbox = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros((1, 4), device=dev)
    out = torch.full((im_h * im_w,), 0xAB, dtype=torch.uint8, device=dev)
    packed = torch.full((im_h * 5,), -1, dtype=torch.int64, device=dev)
    area = torch.full((4,), -7, dtype=torch.int32, device=dev)
    extent = torch.full((4,), -7, dtype=torch.int32, device=dev)
    _lib.call('mrcnn_paste_masks', _lib.ptr(one), _lib.ptr(label), _lib.ptr(bbox), 0, EC.PASTE_M,
              EC.PASTE_NFG, im_h, im_w, _lib.ptr(out), _lib.stream_ptr())
    _lib.call('mrcnn_paste_masks_packed', _lib.ptr(one), _lib.ptr(label), _lib.ptr(bbox), 0,
              EC.PASTE_M, EC.PASTE_NFG, im_h, im_w, _lib.ptr(packed), _lib.ptr(area),
              _lib.ptr(extent), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all()) and bool((packed == -1).all())
    assert bool((area == -7).all()) and bool((extent == -7).all())
    assert np_infer.segm_results(np.zeros((0, 4), f32), np.zeros(0, np.int32),
                                 np.zeros((0, EC.PASTE_NFG, EC.PASTE_M, EC.PASTE_M), f32),
                                 im_h, im_w).shape == (0, im_h, im_w)
