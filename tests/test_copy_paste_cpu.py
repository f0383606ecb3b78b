"""Copy-paste, the host side: the NumPy reference of tests/copy_paste_ref.py
against a per-pixel loop, the draws of the selection, every host-side guard of mrcnn_copy_paste,
the wrappers' argument checks, the tools' options and the kernels' build-time resources.  The
kernels and the dataset wrapper on the device are in tests/test_gpu_copy_paste.py."""
import os
import random
import sys

import numpy as np
import pytest
import torch

import chainer_mask_rcnn_amd.datasets as D
from chainer_mask_rcnn_amd import _lib
from chainer_mask_rcnn_amd import functions as F

import copy_paste_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [(0, 1, [0]), (1, 1, []), (3, 4, [1, 3]), (2, 5, [0, 1, 2, 3, 4])])
def test_reference_equals_the_definition(case):
    Gt, Gs, idx = case
    rng = np.random.RandomState(Gt * 10 + Gs)
    S = 11
    for trial in range(2):
        img_t = rng.standard_normal((3, S, S)).astype(np.float32)
        img_s = rng.standard_normal((3, S, S)).astype(np.float32)
        masks_t = (rng.uniform(size=(Gt, S, S)) < 0.4).astype(np.uint8)
        masks_s = (rng.uniform(size=(Gs, S, S)) < 0.2).astype(np.uint8) * (1 if trial == 0 else 255)
        masks_t[:, 9:], masks_s[:, :, 9:] = 0, 0          # a 9 x 11 and an 11 x 9 extent
        img, masks, boxes, areas = R.compose(img_t, masks_t, img_s, masks_s, idx)
        want_img, want_masks = R.compose_brute_force(img_t, masks_t, img_s, masks_s, idx)
        assert masks.dtype == np.uint8 and masks.shape == (Gt + len(idx), S, S)
        assert np.array_equal(img.view(np.int32), want_img.view(np.int32))
        assert np.array_equal(masks, want_masks) and masks.max(initial=0) <= 1
        for g in range(len(masks)):
            ys, xs = np.nonzero(want_masks[g])
            box = (ys.min(), xs.min(), ys.max() + 1, xs.max() + 1) if len(ys) else (0, 0, 0, 0)
            assert tuple(boxes[g]) == box and areas[g] == len(ys)
        if idx:
            alpha = masks_s[idx].any(0)
            assert alpha.any() and not (masks[:Gt] & alpha).any()


# ---- draws ---------------------------------------------------------------------------------------
def test_selection_takes_randint_then_sample():
    sizes = set()
    for seed in range(200):
        Gs = 1 + seed % 7
        random.seed(seed)
        idx = D.draw_paste_selection(Gs)
        after = random.random()
        random.seed(seed)
        k = random.randint(1, Gs)
        want = sorted(random.sample(range(Gs), k))
        assert random.random() == after                  # exactly these two were consumed
        assert idx == want and len(idx) == k and len(set(idx)) == k
        assert idx == sorted(idx) and 0 <= idx[0] and idx[-1] < Gs
        sizes.add((Gs, k))
    assert sizes == {(Gs, k) for Gs in range(1, 8) for k in range(1, Gs + 1)}


class _Stub(object):
    def __init__(self, items):
        self.items = items

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def test_dataset_returns_the_item_when_the_coin_fails():
    stub = _Stub([object(), object(), object()])
    data = D.CopyPasteDataset(stub, prob=0.)
    assert len(data) == 3
    for seed in range(5):
        random.seed(seed)
        got = data[seed % 3]
        after = random.random()
        random.seed(seed)
        random.random()
        assert got is stub.items[seed % 3] and random.random() == after   # one draw, nothing else
    seed = next(s for s in range(100) if random.Random(s).random() >= 0.5)
    random.seed(seed)
    assert D.CopyPasteDataset(stub)[1] is stub.items[1]                    # prob = 0.5 by default
    random.seed(seed)
    random.random()
    after = random.random()
    random.seed(seed)
    D.CopyPasteDataset(stub, 0.5)[1]
    assert random.random() == after
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match='prob'):
            D.CopyPasteDataset(stub, bad)


def test_dataset_refuses_examples_that_are_not_on_the_canvas():
    host = (np.zeros((3, 8, 8), np.float32), np.zeros((1, 4), np.float32), np.zeros((1,), np.int32),
            np.zeros((1, 8, 8), np.uint8), 1.0)
    random.seed(0)
    with pytest.raises(ValueError, match='device_masks=True, scale_jitter'):
        D.CopyPasteDataset(_Stub([host, host]), prob=1.)[0]


# ---- the C ABI's guards and the wrappers (no device) ---------------------------------------------
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    return _lib.load()


def _fake_args():
    """Distinct, far-apart addresses that are never dereferenced: every call below ends in a guard."""
    p = [_lib.c_vp((1 << 40) + i * (1 << 33)) for i in range(10)]
    #       img_t img_s masks_t Gt masks_s Gs idx  K  S  img_out masks_out box  area  rows stream
    return [p[0], p[1], p[2], 2, p[3], 3, p[4], 2, 16, p[5], p[6], p[7], p[8], p[9], None]


def test_every_guard_returns_its_message_without_a_device(lib):
    assert hasattr(lib, 'mrcnn_copy_paste')

    def refused(msg, **changes):
        args = _fake_args()
        for i, v in changes.items():
            args[int(i[1:])] = v
        assert lib.mrcnn_copy_paste(*args) != 0, changes
        assert msg in lib.mrcnn_last_error(), (changes, lib.mrcnn_last_error())

    for i in (0, 1, 2, 4, 6, 9, 10, 11, 12, 13):
        refused(b'copy_paste: null pointer', **{'a%d' % i: None})
    refused(b'copy_paste: S <= 0', a8=0)
    refused(b'copy_paste: S <= 0', a8=-4)
    for i in (3, 5, 7):
        refused(b'copy_paste: negative count', **{'a%d' % i: -1})
    refused(b'copy_paste: K > Gs', a7=4)
    refused(b'copy_paste: (Gt+K)*S*S >= 2^31', a8=1 << 15)
    refused(b'copy_paste: (Gt+K)*S*S >= 2^31', a3=(1 << 23) - 2)         # (Gt + K) * 256 == 2^31
    a = _fake_args()
    overlaps = b'overlaps an input or another output'
    refused(overlaps, a9=a[0])                                            # img_out is img_t
    refused(overlaps, a9=a[1])
    refused(overlaps, a9=_lib.c_vp(a[0].value + 16 * 16 * 12 - 4))        # the last float of img_t
    refused(overlaps, a10=_lib.c_vp(a[2].value + 2 * 256 - 1))            # the last byte of masks_t
    refused(overlaps, a10=_lib.c_vp(a[4].value - 4 * 256 + 1))            # ends in masks_s
    refused(overlaps, a11=a[6])                                           # box on idx
    refused(overlaps, a13=a[2])                                           # row records on masks_t
    refused(overlaps, a13=a[1])                                           # row records on img_s
    refused(overlaps, a12=_lib.c_vp(a[11].value + 4 * 16 - 4))            # area inside box


def test_wrappers_refuse_host_tensors():
    img, masks = torch.zeros((3, 8, 8)), torch.zeros((2, 8, 8), dtype=torch.uint8)
    for fn in (F.copy_paste, F.copy_paste_meta):
        with pytest.raises(_lib.MrcnnHipError, match='no CPU path'):
            fn(img, masks, img, masks, [0])


# ---- tools ---------------------------------------------------------------------------------------
def _tools():
    path = os.path.join(ROOT, 'tools')
    if path not in sys.path:
        sys.path.insert(0, path)
    import train
    import train_loop
    return train, train_loop


@pytest.mark.parametrize('tool', ['train.py', 'train_loop.py'])
def test_tools_refuse_copy_paste_without_jitter(tool, monkeypatch, capsys):
    train, train_loop = _tools()

    def run(argv):
        with pytest.raises(SystemExit) as e:
            if tool == 'train.py':
                train.parse_args(argv)
            else:
                monkeypatch.setattr(sys, 'argv', ['train_loop.py'] + argv)
                train_loop.main()
        return e.value.code, capsys.readouterr().err

    code, err = run(['--copy-paste', '0.5'])
    assert code == 2 and '--copy-paste needs --scale-jitter' in err
    code, err = run(['--device-masks', '--copy-paste', '0.5'])
    assert code == 2 and '--copy-paste needs --scale-jitter' in err
    for bad in ('0', '-0.5', '1.01', 'often'):
        code, err = run(['--device-masks', '--scale-jitter', '0.1,2.0', '--copy-paste', bad])
        assert code == 2 and '--copy-paste' in err, bad


def test_train_records_the_probability_only_when_set():
    train, train_loop = _tools()
    rec = train.recorded_params(train.parse_args([]))
    assert 'copy_paste' not in rec                       # a default run's file is unchanged
    rec = train.recorded_params(train.parse_args(['--device-masks', '--scale-jitter', '0.1,2.0']))
    assert 'copy_paste' not in rec
    rec = train.recorded_params(train.parse_args(['--device-masks', '--scale-jitter', '0.1,2.0',
                                                  '--copy-paste', '1']))
    assert rec['copy_paste'] == 1.0 and rec['scale_jitter'] == [0.1, 2.0]
    import inspect
    assert inspect.signature(train_loop.build).parameters['copy_paste'].default is None


# ---- build-time facts ----------------------------------------------------------------------------
def test_kernels_use_no_scratch_and_the_shared_box_kernel_is_unchanged():
    from test_build_cpu import _resources
    res = _resources('copy_paste.hip', [])
    names = ' '.join(res)
    for kernel in ('paste_kernel', 'mask_box_kernel'):
        assert kernel in names, names
    for k, v in res.items():
        assert v.get('ScratchSize', 0) == 0 and v.get('VGPRs Spill', 0) == 0, (k, v)
    # mask_box_kernel moved into mask_box.h: both files compile the kernel the parent had
    jitter = _resources('scale_jitter.hip', ['-ffp-contract=off'])
    vgprs = {name: v['VGPRs'] for k, v in jitter.items()
             for name in ('mask_resize_crop_kernel', 'mask_box_kernel') if name in k}
    assert vgprs['mask_resize_crop_kernel'] == 32 and vgprs['mask_box_kernel'] == 17, vgprs
    box = [v for k, v in res.items() if 'mask_box_kernel' in k][0]
    assert box['VGPRs'] == 17 and box.get('ScratchSize', 0) == 0
