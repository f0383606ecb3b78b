"""Large-scale jitter, the host side: the geometry ``draw_scale_jitter``
draws, the table builder, the NumPy references of tests/scale_jitter_ref.py and the constructor's
argument checks.  The kernels and the transform are in tests/test_gpu_scale_jitter.py."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import chainer_mask_rcnn_amd.datasets as D
from chainer_mask_rcnn_amd.datasets import transforms as T
from chainer_mask_rcnn_amd.functions import scale_jitter as SJ

import scale_jitter_ref as R

# (H, W, S, lo, hi): padded only, cropped only, both, a tall image, the COCO recipe
CASES = [(37, 53, 64, 0.1, 0.9), (37, 53, 16, 1.5, 2.0), (480, 640, 1024, 0.1, 2.0),
         (640, 427, 96, 0.5, 2.0), (96, 128, 64, 0.5, 2.0)]


def test_draw_is_reproducible_and_takes_three_draws():
    random.seed(3)
    a = T.draw_scale_jitter((480, 640), 1024, (0.1, 2.0))
    after = random.random()
    random.seed(3)
    assert D.draw_scale_jitter((480, 640), 1024, (0.1, 2.0)) == a
    random.seed(3)
    r, u, v = random.uniform(0.1, 2.0), random.random(), random.random()
    assert random.random() == after                      # exactly these three were consumed
    scale, (rH, rW), (oy, ox) = a
    assert scale == min(r * 1024 / 480, r * 1024 / 640)
    assert (rH, rW) == (max(1, int(np.round(480 * scale))), max(1, int(np.round(640 * scale))))
    assert oy == int(np.floor(u * (max(rH - 1024, 0) + 1)))
    assert ox == int(np.floor(v * (max(rW - 1024, 0) + 1)))


@pytest.mark.parametrize('case', CASES)
def test_draw_stays_in_range(case):
    H, W, S, lo, hi = case
    for seed in range(1000):
        random.seed(seed)
        scale, (rH, rW), (oy, ox) = T.draw_scale_jitter((H, W), S, (lo, hi))
        random.seed(seed)
        r = random.uniform(lo, hi)
        assert lo <= r <= hi and scale > 0 and rH >= 1 and rW >= 1
        assert 0 <= oy <= max(rH - S, 0) and 0 <= ox <= max(rW - S, 0), (seed, rH, rW, oy, ox)
        assert abs(max(rH, rW) - r * S) <= 1, (seed, r, rH, rW)


@pytest.mark.parametrize('case', CASES)
def test_unit_range_fits_the_longer_side(case):
    H, W, S = case[:3]
    for seed in range(20):
        random.seed(seed)
        scale, (rH, rW), offset = T.draw_scale_jitter((H, W), S, (1, 1))
        assert max(rH, rW) == S and offset == (0, 0)
        assert scale == min(float(S) / H, float(S) / W)


def _instances(H, W):
    """(5, H, W) int32: a full-image instance, a single pixel, a 1-pixel column, a block in the
    middle and one in the bottom-right corner."""
    m = np.zeros((5, H, W), np.int32)
    m[0] = 1
    m[1, H // 3, W // 2] = 1
    m[2, 10:14, 23] = 1
    m[3, H // 4:H // 2, W // 4:W // 2] = 1
    m[4, H - 5:, W - 7:] = 1
    return m


@pytest.mark.parametrize('x_flip', [False, True])
def test_reference_equals_the_definition(x_flip):
    m = _instances(17, 29)
    # cropped on both axes, padded on both, one of each
    for resized, offset, S in (((31, 53), (9, 20), 12), ((9, 15), (0, 0), 12), ((31, 10), (19, 0), 12)):
        want = R.crop_masks_brute_force(m, resized, offset, S, x_flip)
        got = R.crop_masks(m, resized, offset, S, x_flip)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (resized, offset)
        boxes, areas = R.boxes_areas(got)
        for g in range(len(m)):
            assert areas[g] == want[g].sum()
            ys, xs = np.nonzero(want[g])
            box = (ys.min(), xs.min(), ys.max() + 1, xs.max() + 1) if len(ys) else (0, 0, 0, 0)
            assert tuple(boxes[g]) == box
        assert areas[0] > 0


def test_thin_column_vanishes_at_half_scale():
    # the issue's example: a 4 x 1 column of a 37 x 53 mask has no pixel left at 18 x 26
    m = _instances(37, 53)[2:3]
    assert m.sum() == 4
    out = R.crop_masks(m, (18, 26), (0, 0), 32)
    assert np.array_equal(out[:, :18, :26], T.resize_nearest(m, (18, 26)))
    assert out.sum() == 0 and tuple(R.boxes_areas(out)[0][0]) == (0, 0, 0, 0)


@pytest.mark.parametrize('x_flip', [False, True])
def test_tables_are_the_host_index_rule(x_flip):
    m = _instances(37, 53)
    for resized, offset, S in (((18, 26), (0, 0), 32), ((74, 106), (10, 42), 64), ((74, 30), (3, 0), 47)):
        ys, xs = SJ.crop_tables((37, 53), resized, offset, S, x_flip)
        assert ys.dtype == xs.dtype == np.int32 and len(ys) == len(xs) == S
        assert ((ys == -1) == (np.arange(S) + offset[0] >= resized[0])).all()
        assert ((xs == -1) == (np.arange(S) + offset[1] >= resized[1])).all()
        got = np.where((ys[:, None] >= 0) & (xs[None, :] >= 0), m[:, ys.clip(0)][:, :, xs.clip(0)], 0)
        assert np.array_equal(got, R.crop_masks(m, resized, offset, S, x_flip))


def test_constructor_checks():
    with pytest.raises(ValueError, match='requires train=True and device_masks=True'):
        D.MaskRCNNTransform(None, scale_jitter=(0.5, 2.0))
    with pytest.raises(ValueError, match='requires train=True and device_masks=True'):
        D.MaskRCNNTransform(None, train=False, device_masks=True, scale_jitter=(0.5, 2.0))
    for bad in ((0, 1), (-1, 1), (2.0, 0.5)):
        with pytest.raises(ValueError, match='0 < lo <= hi'):
            D.MaskRCNNTransform(None, device_masks=True, scale_jitter=bad)
    for bad in (0, -4, 12.5):
        with pytest.raises(ValueError, match='crop_size'):
            D.MaskRCNNTransform(None, device_masks=True, scale_jitter=(0.5, 2.0), crop_size=bad)
    t = D.MaskRCNNTransform(None, device_masks=True, scale_jitter=(1, 1), crop_size=64)
    assert t.scale_jitter == (1.0, 1.0) and t.crop_size == 64
    t = D.MaskRCNNTransform(None)                        # off by default
    assert t.scale_jitter is None and t.device_masks is False and t.train is True


# ---- build-time facts and the tools (no device) ---------------------------------------------------
def test_kernels_use_no_scratch_and_share_the_pixel_function():
    from test_build_cpu import CSRC, _resources
    res = _resources('scale_jitter.hip', ['-ffp-contract=off'])
    names = ' '.join(res)
    for kernel in ('prepare_crop_kernel<unsigned char>', 'prepare_crop_kernel<float>',
                   'mask_resize_crop_kernel', 'mask_box_kernel'):
        assert kernel in names, names
    for k, v in res.items():
        assert v.get('ScratchSize', 0) == 0 and v.get('VGPRs Spill', 0) == 0, (k, v)
    # one definition of the prepare pixel, called by both kernels
    src = {f: open(os.path.join(CSRC, f)).read() for f in ('image.hip', 'scale_jitter.hip', 'prepare_pixel.h')}
    assert 'void prepare_pixel(' in src['prepare_pixel.h']
    for f in ('image.hip', 'scale_jitter.hip'):
        assert '#include "prepare_pixel.h"' in src[f] and 'mrcnn::prepare_pixel(' in src[f]
        assert '2048.f' not in src[f]                    # the 8-bit path's coefficients live in the header


def _tool(name, argv):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return subprocess.run([sys.executable, os.path.join(root, 'tools', name)] + argv,
                          capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize('tool', ['train.py', 'train_loop.py'])
def test_tools_refuse_jitter_without_device_masks(tool):
    out = _tool(tool, ['--scale-jitter', '0.1,2.0'])
    assert out.returncode == 2 and '--scale-jitter needs --device-masks' in out.stderr
    for bad in ('2.0', '2,1'):
        out = _tool(tool, ['--device-masks', '--scale-jitter', bad])
        assert out.returncode == 2 and '--scale-jitter' in out.stderr, bad
    out = _tool(tool, ['--device-masks', '--scale-jitter', '0.1,2.0', '--crop-size', '0'])
    assert out.returncode == 2 and '--crop-size must be positive' in out.stderr


def test_train_records_both_values_only_when_set():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import train
    rec = train.recorded_params(train.parse_args([]))
    assert 'scale_jitter' not in rec and 'crop_size' not in rec        # a default run's file is unchanged
    rec = train.recorded_params(train.parse_args(['--device-masks', '--scale-jitter', '0.1,2.0']))
    assert rec['scale_jitter'] == [0.1, 2.0] and rec['crop_size'] == 1024
    rec = train.recorded_params(train.parse_args(['--device-masks', '--scale-jitter', '0.5,1.5',
                                                  '--crop-size', '512']))
    assert rec['scale_jitter'] == [0.5, 1.5] and rec['crop_size'] == 512
