"""Ground-truth masks carried as bits to the device: mrcnn_mask_resize_nearest through the C ABI,
``MaskRCNNTransform(device_masks=True)``, the train chain on device masks and the train loop with
``packed_masks=True`` — each against the dense host path.  Integer data and identical random
streams: every comparison is exact."""
import os
import random

import numpy as np
import pytest
import torch

import chainer_mask_rcnn_amd as cmr
import chainer_mask_rcnn_amd.datasets as D
from chainer_mask_rcnn_amd import _lib
from chainer_mask_rcnn_amd import functions as F
from chainer_mask_rcnn_amd.datasets import PackedMasks
from chainer_mask_rcnn_amd.models.utils import ProposalTargetCreator

import gt_masks_ref as R
import test_gpu_train_loop as TLT
from test_gpu_train_loop import TL

pytestmark = pytest.mark.gpu

FRONT, REAR, FILL = 3, 64, 0xAB     # guard bytes around `out`; FRONT also misaligns its address


def _launch(dev, packed, ys, xs, out_size, rc_only=False):
    """mrcnn_mask_resize_nearest on a guarded buffer -> (rc, out (G,oH,oW) host, guards intact)."""
    G, H, W = packed.shape
    oH, oW = out_size
    n = G * oH * oW
    buf = torch.full((FRONT + n + REAR,), FILL, dtype=torch.uint8, device=dev)
    words = torch.from_numpy(packed.words.view(np.int64)).to(dev)
    ys_d, xs_d = torch.from_numpy(np.asarray(ys, np.int32)).to(dev), torch.from_numpy(np.asarray(xs, np.int32)).to(dev)
    rc = _lib.load().mrcnn_mask_resize_nearest(
        _lib.ptr(words) if words.numel() else None, G, H, W, _lib.ptr(ys_d), _lib.ptr(xs_d), oH, oW,
        _lib.c_vp(buf.data_ptr() + FRONT), _lib.stream_ptr())
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    intact = bool((host[:FRONT] == FILL).all() and (host[FRONT + n:] == FILL).all())
    return rc, host[FRONT:FRONT + n].reshape(G, oH, oW), intact


@pytest.mark.parametrize('x_flip', [False, True])
@pytest.mark.parametrize('G', [1, 3])
def test_kernel_equals_resize_nearest(dev, G, x_flip):
    rng = np.random.RandomState(10 * G + x_flip)
    for in_size, out_size in R.SHAPES:
        for fill in ((None, 0, 1) if G == 1 else (None,)):
            m = R.random_masks(rng, G, in_size[0], in_size[1], fill)
            p = PackedMasks.from_dense(m)
            ys, xs = R.tables(in_size, out_size, x_flip)
            rc, got, intact = _launch(dev, p, ys, xs, out_size)
            what = (in_size, out_size, fill)
            assert rc == 0 and intact, what
            assert np.array_equal(got, D.resize_nearest(m, out_size, x_flip=x_flip)), what
            assert np.array_equal(got, R.resize_masks_nearest(p, out_size, x_flip)), what
            # the wrapper: same tables, current stream
            out = F.resize_masks_nearest(F.upload_packed_masks(p, dev), out_size, x_flip=x_flip)
            assert out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous()
            assert np.array_equal(out.cpu().numpy(), got), what


def test_kernel_edges(dev):
    rng = np.random.RandomState(5)
    H, W = 9, 70
    m = R.random_masks(rng, 3, H, W)
    p = PackedMasks.from_dense(m)
    # no instances: success, nothing written
    rc, got, intact = _launch(dev, p[0:0], *R.tables((H, W), (13, 65)), (13, 65))
    assert rc == 0 and intact and got.shape == (0, 13, 65)
    out = F.resize_masks_nearest(F.upload_packed_masks(p[0:0], dev), (13, 65))
    assert out.shape == (0, 13, 65) and out.dtype == torch.uint8 and out.is_cuda
    # table entries out of range give the clamped pixels' values, and the launch succeeds
    ys = np.array([-5, 0, H - 1, H + 9, 4], np.int32)
    xs = np.array([-5, W - 1, W + 9, 3, 64, 63, 0], np.int32)
    rc, got, intact = _launch(dev, p, ys, xs, (5, 7))
    assert rc == 0 and intact
    want = m[:, [0, 0, H - 1, H - 1, 4]][:, :, [0, W - 1, W - 1, 3, 64, 63, 0]]
    assert np.array_equal(got, want) and np.array_equal(got, R.resize_with_tables(p, ys, xs))
    # a null pointer with G > 0 is an error with a message; so are bad sizes
    lib = _lib.load()
    buf = torch.zeros(64, dtype=torch.int64, device=dev)
    for args in ((None, 1, 4, 4, _lib.ptr(buf), _lib.ptr(buf), 2, 2, _lib.ptr(buf), None),
                 (_lib.ptr(buf), 1, 4, 4, None, _lib.ptr(buf), 2, 2, _lib.ptr(buf), None),
                 (_lib.ptr(buf), 1, 4, 4, _lib.ptr(buf), _lib.ptr(buf), 2, 2, None, None)):
        assert lib.mrcnn_mask_resize_nearest(*args) != 0
        assert b'mask_resize_nearest: null pointer' in lib.mrcnn_last_error()
    for args in ((_lib.ptr(buf), -1, 4, 4, _lib.ptr(buf), _lib.ptr(buf), 2, 2, _lib.ptr(buf), None),
                 (_lib.ptr(buf), 1, 0, 4, _lib.ptr(buf), _lib.ptr(buf), 2, 2, _lib.ptr(buf), None),
                 (_lib.ptr(buf), 1, 4, 4, _lib.ptr(buf), _lib.ptr(buf), 2, 0, _lib.ptr(buf), None)):
        assert lib.mrcnn_mask_resize_nearest(*args) != 0
        assert b'mask_resize_nearest: bad shape' in lib.mrcnn_last_error()
    assert lib.mrcnn_mask_resize_nearest(_lib.ptr(buf), 4, 4, 4, _lib.ptr(buf), _lib.ptr(buf),
                                         1 << 15, 1 << 15, _lib.ptr(buf), None) != 0
    assert b'>= 2^31' in lib.mrcnn_last_error()
    with pytest.raises(_lib.MrcnnHipError):
        F.resize_masks_nearest((torch.zeros((1, 4, 1), dtype=torch.int64), 4), (2, 2))


@pytest.fixture(scope='module')
def small(dev, tmp_path_factory):
    """The small model of tests/test_gpu_train_loop.py over its 5-image COCO directory."""
    root = os.path.join(str(tmp_path_factory.mktemp('gt_masks')), 'COCO')
    TLT._write_coco(root)
    data = cmr.datasets.COCOInstanceSegmentationDataset('minival', root_dir=root)
    packed = cmr.datasets.COCOInstanceSegmentationDataset('minival', root_dir=root, packed_masks=True)
    loop, model, chain, opt, train = TLT._build(dev, data, prefetch=False)
    loop.close()
    return dict(root=root, data=data, packed=packed, model=model, chain=chain)


def test_transform_device_masks(dev, small):
    model, data, packed = small['model'], small['data'], small['packed']
    flips = {}
    for seed in range(16):                              # one seed for each value of the flip
        random.seed(seed)
        flips.setdefault(random.choice([True, False]), seed)
    assert sorted(flips) == [False, True]
    ex, ex_packed = data[2], packed[2]
    assert isinstance(ex_packed[3], PackedMasks) and len(ex[3]) == 3
    for x_flip, seed in sorted(flips.items()):
        random.seed(seed)
        want = D.MaskRCNNTransform(model)(ex)
        after = random.random()
        assert isinstance(want[3], np.ndarray) and want[3].dtype == np.int32
        for example in (ex, ex_packed):
            random.seed(seed)
            got = D.MaskRCNNTransform(model, device_masks=True)(example)
            assert random.random() == after
            assert got[0].is_cuda and torch.equal(got[0], want[0])
            assert got[0].stride() == want[0].stride()
            assert np.array_equal(got[1], want[1]) and got[1].dtype == want[1].dtype
            assert np.array_equal(got[2], want[2]) and got[4] == want[4]
            mask = got[3]
            assert mask.is_cuda and mask.dtype == torch.uint8 and mask.is_contiguous()
            assert tuple(mask.shape) == want[3].shape == (3,) + tuple(got[0].shape[1:])
            assert np.array_equal(mask.cpu().numpy(), want[3])
        # a 2-D mask keeps its 2-D form
        random.seed(seed)
        want2 = D.MaskRCNNTransform(model)(ex[:3] + (ex[3][1],))
        random.seed(seed)
        got2 = D.MaskRCNNTransform(model, device_masks=True)(ex[:3] + (ex[3][1],))
        assert got2[3].dim() == 2 and np.array_equal(got2[3].cpu().numpy(), want2[3])
        # no instances: an empty stack at the network size
        random.seed(seed)
        got0 = D.MaskRCNNTransform(model, device_masks=True)(
            (ex[0], np.zeros((0, 4), np.float32), np.zeros((0,), np.int32), ex_packed[3][0:0]))
        assert got0[3].is_cuda and got0[3].dtype == torch.uint8
        assert tuple(got0[3].shape) == (0,) + tuple(got0[0].shape[1:])
    # evaluation mode is unchanged
    out = D.MaskRCNNTransform(model, train=False, device_masks=True)(ex_packed)
    assert out[3] is ex_packed[3] and isinstance(out[0], np.ndarray)


def _batches(dev, small):
    """The same two examples through the default and the device-mask transform + converter."""
    out = []
    for data, device_masks in ((small['data'], False), (small['packed'], True)):
        random.seed(7)
        t = D.MaskRCNNTransform(small['model'], device_masks=device_masks)
        out.append(TL.make_converter(dev)([t(data[j]) for j in (2, 4)]))
    return out


def test_converter_stacks_device_masks(dev, small):
    host, device = _batches(dev, small)
    masks = device[3]
    assert isinstance(host[3], np.ndarray) and host[3].dtype == np.int32
    assert isinstance(masks, torch.Tensor) and masks.is_cuda and masks.dtype == torch.uint8
    assert masks.is_contiguous() and tuple(masks.shape) == host[3].shape     # row-major, zero-padded
    assert host[3].shape[1] == 3 and len(small['data'][4][3]) == 2          # image 4 is padded
    assert np.array_equal(masks.cpu().numpy(), host[3])
    assert torch.equal(device[0], host[0]) and device[0].is_contiguous(memory_format=torch.channels_last)


class _NoForegroundInSecondImage(ProposalTargetCreator):
    """Every second call samples with a threshold no IoU reaches: that image has n_fg == 0."""
    calls = 0

    def _threshold(self):
        self.calls += 1
        self.pos_iou_thresh = 2.0 if self.calls % 2 == 0 else 0.5

    def sample(self, *args, **kwargs):
        self._threshold()
        return super(_NoForegroundInSecondImage, self).sample(*args, **kwargs)

    def sample_device(self, *args, **kwargs):
        self._threshold()
        return super(_NoForegroundInSecondImage, self).sample_device(*args, **kwargs)


@pytest.mark.parametrize('no_fg', [False, True])
@pytest.mark.parametrize('device_targets', [False, True])
def test_chain_on_device_masks(dev, small, monkeypatch, device_targets, no_fg):
    chain = small['chain']
    host, device = _batches(dev, small)
    monkeypatch.setattr(chain, 'device_targets', device_targets)
    make_ptc = _NoForegroundInSecondImage if no_fg else ProposalTargetCreator
    results = []
    for batch, on_device in ((host, False), (device, True)):
        monkeypatch.setattr(chain, 'proposal_target_creator', make_ptc(n_sample=32))
        with monkeypatch.context() as mp:
            if on_device:
                def never(self, job, mask):
                    raise AssertionError('the host crop ran on a device mask')
                mp.setattr(ProposalTargetCreator, 'mask_targets', never)
                mp.setattr(torch.Tensor, 'cpu', _no_mask_download(batch[3], torch.Tensor.cpu))
            np.random.seed(11)
            loss = chain(*batch)
            torch.cuda.synchronize()
        t = chain.last_targets
        results.append((float(loss.detach()), {k: float(v) for k, v in chain.report.items()},
                        t['gt_roi_masks'].cpu().numpy(), t['gt_roi_labels'].cpu().numpy(),
                        t['sample_rois'].cpu().numpy(), t['n_fg'], np.random.randint(0, 1 << 30),
                        t['sample_roi_indices'].cpu().numpy()))
    a, b = results
    assert np.isfinite(a[0]) and a[0] == b[0] and a[1] == b[1]
    assert a[2].dtype == np.int32 and np.array_equal(a[2], b[2])
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])
    assert a[5] == b[5] and a[5] > 0 and a[6] == b[6]                        # np.random stream
    assert (a[2] >= 0).any() and (a[2][a[3] == 0] == -1).all()
    if no_fg:                                            # the second image's rows are all -1
        second = a[7] == 1
        assert np.array_equal(a[7], b[7]) and second.any() and not second.all()
        assert (a[3][second] == 0).all() and (a[2][second] == -1).all() and (a[3][~second] > 0).any()


def _no_mask_download(masks, cpu):
    """``Tensor.cpu`` that refuses the ground-truth mask batch and its per-image views."""
    lo, hi = masks.data_ptr(), masks.data_ptr() + masks.numel()

    def guarded(self, *args, **kwargs):
        if self.is_cuda and self.dtype == torch.uint8 and lo <= self.data_ptr() < hi:
            raise AssertionError('a device mask was copied back to the host')
        return cpu(self, *args, **kwargs)
    return guarded


def test_loop_with_packed_device_masks(dev, small):
    runs = []
    for data, device_masks, prefetch in ((small['data'], False, True), (small['packed'], True, True),
                                         (small['packed'], True, False)):
        loop, model, chain, opt, train = TLT._build(dev, data, prefetch=prefetch)
        train._transform = D.MaskRCNNTransform(model, device_masks=device_masks)
        seen, convert = [], loop.converter

        def converter(examples, seen=seen, convert=convert):
            batch = convert(examples)
            seen.append(batch[3])
            return batch
        loop.converter = converter
        losses = [float(l.detach()) for l in loop.run(4)]
        opt.flush()
        torch.cuda.synchronize()
        loop.close()
        assert len(seen) >= 4
        for masks in seen:
            if device_masks:
                assert isinstance(masks, torch.Tensor) and masks.is_cuda
                assert masks.dtype == torch.uint8 and masks.is_contiguous() and masks.dim() == 4
            else:
                assert isinstance(masks, np.ndarray) and masks.dtype == np.int32
        w = model.head.res5.a.conv1.W.detach().cpu().numpy().copy()
        runs.append((losses, loop.iterator.epoch, random.random(), np.random.randint(0, 1 << 30), w))
    dense = runs[0]
    assert all(np.isfinite(dense[0])) and dense[1] == 1
    for run in runs[1:]:
        assert run[0] == dense[0] and run[1] == dense[1]
        assert run[2] == dense[2] and run[3] == dense[3]                     # both random streams
        assert np.array_equal(run[4], dense[4])
