"""roi_pooling_2d / crop_and_resize without a device: hand-computed answers of the NumPy
restatements (tests/pool_variants_ref.py), crop-and-resize against torch's bilinear resize in
float64, argument errors, CPU-tensor refusal, host-side validation of the new C entry points and
the kernels' resource usage."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import pool_variants_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'chainer_mask_rcnn_amd', 'csrc')


# ---- known answers of the restatements ---------------------------------------------------------

def test_tie_rounds_half_away_for_pooling_and_half_even_for_crop():
    # 40 / 16 = 2.5 and 72 / 16 = 4.5: roundf gives 3 and 5, Python's round 2 and 4
    hw, ww = ref.pool_windows([0, 40, 40, 72, 72], 1, 1, 1 / 16., 10, 10)
    assert hw == [(3, 6)] and ww == [(3, 6)]
    assert ref.crop_box([0, 40, 40, 72, 72], 1 / 16., 10, 10) == (2, 2, 2, 2)
    # negative tie: -2.5 -> -3 (half away), and the window clamps at 0
    hw, ww = ref.pool_windows([0, -40, 0, 8, 8], 1, 1, 1 / 16., 10, 10)
    assert ww == [(0, 2)]          # start -3, end round(0.5) = 1: size 5, [-3, 2) clamped


def test_malformed_roi_is_one_by_one():
    # x2 < x1: start 5, end 1 -> size max(1 - 5 + 1, 1) = 1; two bins of 0.5 both read pixel 5
    hw, ww = ref.pool_windows([0, 80, 80, 16, 16], 2, 2, 1 / 16., 10, 10)
    assert hw == [(5, 6), (5, 6)] and ww == [(5, 6), (5, 6)]
    x = np.arange(100, dtype=np.float32).reshape(1, 1, 10, 10)
    y, am = ref.roi_pooling_2d_fwd(x, [[0, 80, 80, 16, 16]], 2, 2, 1 / 16.)
    assert (y == 55).all() and (am == 55).all()


def test_empty_bins_give_zero_and_minus_one():
    x = np.ones((1, 2, 4, 4), np.float32)
    y, am = ref.roi_pooling_2d_fwd(x, [[0, 100, 100, 120, 120]], 2, 3, 1.0)
    assert (y == 0).all() and (am == -1).all()


def test_first_maximum_wins_and_nan_never_wins():
    x = np.array([[[[1, 5], [5, 1]]]], np.float32)
    y, am = ref.roi_pooling_2d_fwd(x, [[0, 0, 0, 1, 1]], 1, 1, 1.0)
    assert y[0, 0, 0, 0] == 5 and am[0, 0, 0, 0] == 1
    x = np.array([[[[np.nan, 2], [3, np.nan]]]], np.float32)
    y, am = ref.roi_pooling_2d_fwd(x, [[0, 0, 0, 1, 1]], 1, 1, 1.0)
    assert y[0, 0, 0, 0] == 3 and am[0, 0, 0, 0] == 2
    # every value at most -1e37: the initial value stays, argmax -1 (chainer's kernel)
    x = np.full((1, 1, 2, 2), -np.inf, np.float32)
    y, am = ref.roi_pooling_2d_fwd(x, [[0, 0, 0, 1, 1]], 1, 1, 1.0)
    assert y[0, 0, 0, 0] == np.float32(-1e37) and am[0, 0, 0, 0] == -1


def test_pooling_backward_sums_into_argmax():
    x = np.array([[[[1, 5], [5, 1]]]], np.float32)
    rois = [[0, 0, 0, 1, 1], [0, 0, 0, 0, 0]]
    y, am = ref.roi_pooling_2d_fwd(x, rois, 1, 1, 1.0)
    assert am[:, 0, 0, 0].tolist() == [1, 0]
    gx = ref.roi_pooling_2d_bwd(np.array([2, 3], np.float32).reshape(2, 1, 1, 1), am, rois, x.shape)
    assert gx.ravel().tolist() == [3, 2, 0, 0]


def test_crop_one_pixel_wide_reads_that_column():
    x = np.arange(40, dtype=np.float32).reshape(1, 1, 5, 8)
    # x1 = x2 = 3: crop columns [3, 4), rows [1, 5)
    assert ref.crop_box([0, 3, 1, 3, 5], 1.0, 5, 8) == (1, 3, 4, 1)
    y = ref.crop_and_resize_fwd(x, [[0, 3, 1, 3, 5]], 3, 2, 1.0)
    # rows 1, 2.5, 4 of column 3: 11, 23, 35 in both output columns
    np.testing.assert_array_equal(y[0, 0], [[11, 11], [23, 23], [35, 35]])


def test_crop_out_one_samples_the_crop_start():
    x = np.arange(40, dtype=np.float32).reshape(1, 1, 5, 8)
    y = ref.crop_and_resize_fwd(x, [[0, 2, 1, 6, 4]], 1, 1, 1.0)
    assert y[0, 0, 0, 0] == x[0, 0, 1, 2]
    y = ref.crop_and_resize_fwd(x, [[0, 2, 1, 7, 4]], 1, 3, 1.0)
    np.testing.assert_array_equal(y[0, 0, 0], [10, 12, 14])     # columns 2, 4, 6 of row 1


def test_crop_truncated_at_the_map_edge_and_clamped_start():
    assert ref.crop_box([0, 5, 2, 100, 3], 1.0, 5, 8) == (2, 5, 1, 3)      # wc = 8 - 5
    assert ref.crop_box([0, -4, -7, 2, 1], 1.0, 5, 8) == (0, 0, 1, 2)      # starts clamped to 0
    assert ref.crop_box([0, 20, 9, 30, 12], 1.0, 5, 8) == (4, 7, 1, 1)     # start past the map
    x = np.arange(40, dtype=np.float32).reshape(1, 1, 5, 8)
    y = ref.crop_and_resize_fwd(x, [[0, 5, 2, 100, 3]], 1, 2, 1.0)
    np.testing.assert_array_equal(y[0, 0, 0], [21, 23])


def test_crop_output_rows_follow_batch_order():
    rois = [[1, 0, 0, 1, 1], [0, 0, 0, 1, 1], [1, 1, 1, 2, 2], [0, 2, 2, 3, 3]]
    assert ref.output_rows(rois).tolist() == [2, 0, 3, 1]
    x = np.arange(2 * 16, dtype=np.float32).reshape(2, 1, 4, 4)
    y = ref.crop_and_resize_fwd(x, rois, 1, 1, 1.0)
    # row k = the k-th RoI of image 0, then of image 1; each samples its crop start
    assert y[:, 0, 0, 0].tolist() == [0, 10, 16, 21]


def test_crop_and_resize_matches_torch_bilinear_align_corners():
    rng = np.random.RandomState(3)
    x = rng.standard_normal((2, 3, 13, 17)).astype(np.float32)
    rois = np.array([[0, 8, 16, 120, 150], [1, 0, 0, 271, 207], [1, 40, 40, 40, 200],
                     [0, 100, 30, 300, 33]], np.float32)
    for outh, outw in ((7, 5), (1, 4), (14, 14)):
        got = ref.crop_and_resize_fwd(x, rois, outh, outw, 1 / 16.)
        for r, row in enumerate(ref.output_rows(rois)):
            y1, x1, hc, wc = ref.crop_box(rois[r], 1 / 16., 13, 17)
            crop = torch.tensor(x[int(rois[r][0]):int(rois[r][0]) + 1, :, y1:y1 + hc, x1:x1 + wc],
                                dtype=torch.float64)
            want = torch.nn.functional.interpolate(crop, (outh, outw), mode='bilinear',
                                                   align_corners=True)[0].numpy()
            np.testing.assert_allclose(got[row], want, rtol=1e-6, atol=1e-6)


def test_crop_backward_is_the_adjoint():
    rng = np.random.RandomState(4)
    x = rng.standard_normal((2, 2, 9, 11)).astype(np.float64)
    rois = np.array([[1, 8, 16, 120, 150], [0, 3, 5, 60, 90], [1, 20, 20, 20, 20]], np.float32)
    gy = rng.standard_normal((3, 2, 4, 3))
    y = ref.crop_and_resize_fwd(x.astype(np.float32), rois, 4, 3, 1 / 8.)
    gx = ref.crop_and_resize_bwd(gy, rois, x.shape, 1 / 8.)
    # <f(x), gy> == <x, f^T(gy)> (f is linear in x)
    np.testing.assert_allclose((y.astype(np.float64) * gy).sum(), (x * gx).sum(), rtol=1e-5)


# ---- the Python functions ---------------------------------------------------------------------

def test_argument_errors():
    from chainer_mask_rcnn_amd import functions
    for cls in (functions.ROIPooling2D, functions.CropAndResize):
        with pytest.raises(TypeError):
            cls(2.0, 2, 1.0)
        with pytest.raises(TypeError):
            cls(2, 0, 1.0)
        with pytest.raises(TypeError):
            cls(2, 2, 1.0, bin_stride=0)
        with pytest.raises(TypeError):
            cls(2, 2, 'a')
        assert cls(2, 2, 1).spatial_scale == 1.0
        with pytest.raises(TypeError):
            cls(2, 2, 1.0)(torch.zeros(1, 1, 2, 2), torch.zeros(1, 4))
        with pytest.raises(TypeError):
            cls(2, 2, 1.0)(torch.zeros(1, 1, 2, 2, dtype=torch.float64), torch.zeros(1, 5))
    for fn in (functions.roi_pooling_2d, functions.crop_and_resize):
        with pytest.raises(ValueError, match='Unsupported axes'):
            fn(torch.zeros(1, 1, 2, 2), torch.zeros(1, 5), 2, 2, 1.0, axes='zz')


def test_cpu_tensors_are_refused():
    from chainer_mask_rcnn_amd import functions, _lib
    for fn in (functions.roi_pooling_2d, functions.crop_and_resize):
        with pytest.raises(_lib.MrcnnHipError, match='ROCm device'):
            fn(torch.zeros(1, 4, 6, 6), torch.zeros(2, 5), 2, 2, 1.0)


# ---- the C entry points without a device ----------------------------------------------------

@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from chainer_mask_rcnn_amd import _lib
    return _lib.load()


def _err(lib):
    return lib.mrcnn_last_error()


def test_abi_rejects_bad_arguments(lib):
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    f, d = ctypes.c_float(1 / 16.), ctypes.c_double(1 / 16.)
    pool = lambda *a: lib.mrcnn_roi_pool_fwd(a[0], a[1], a[2], a[3], *a[4:], f, None, None)
    crop = lambda *a: lib.mrcnn_crop_resize_fwd(a[0], a[1], None, a[2], *a[4:], d, None, None)
    for call in (pool, crop):
        # outh / outw < 1, C < 1, bin_stride < 1
        assert call(p, p, p, p, 1, 8, 8, 4, 2, 0, 7, 1) != 0 and b'bad shape' in _err(lib)
        assert call(p, p, p, p, 1, 8, 8, 4, 2, 7, 0, 1) != 0 and b'bad shape' in _err(lib)
        assert call(p, p, p, p, 1, 8, 8, 0, 2, 7, 7, 1) != 0 and b'bad shape' in _err(lib)
        assert call(p, p, p, p, 1, 8, 8, 4, 2, 7, 7, 0) != 0 and b'bin_stride' in _err(lib)
        # a missing pointer with R > 0
        assert call(None, p, p, p, 1, 8, 8, 4, 2, 7, 7, 1) != 0 and b'null' in _err(lib)
        assert call(p, None, p, p, 1, 8, 8, 4, 2, 7, 7, 1) != 0 and b'null' in _err(lib)
        assert call(p, p, None, p, 1, 8, 8, 4, 2, 7, 7, 1) != 0 and b'null' in _err(lib)
        # R == 0: nothing to do, nothing touched
        assert call(None, None, None, None, 1, 8, 8, 4, 0, 7, 7, 1) == 0
    assert pool(p, p, p, None, 1, 8, 8, 4, 2, 7, 7, 1) != 0 and b'null argmax' in _err(lib)
    # the backwards: a missing or undersized workspace, a missing argmax
    for q, name in ((lib.mrcnn_roi_pool_bwd_workspace_bytes, 'pool'),
                    (lib.mrcnn_crop_resize_bwd_workspace_bytes, 'crop')):
        need = q(1, 8, 8, 4, 7, 7, 1)
        assert need > 0 and q(1, 8, 8, 4, 14, 14, 2) == need and q(1, 8, 8, 0, 7, 7, 1) == 0
        assert q(1, 8, 8, 4, 7, 7, 0) == 0
        if name == 'pool':
            bwd = lambda ws, n, am=p: lib.mrcnn_roi_pool_bwd_ws(p, am, p, p, 1, 8, 8, 4, 4, 7, 7, 1, f, ws, n, None)
        else:
            bwd = lambda ws, n, am=p: lib.mrcnn_crop_resize_bwd_ws(p, p, None, p, 1, 8, 8, 4, 4, 7, 7, 1, d, ws, n, None)
        assert bwd(p, need - 1) != 0 and b'workspace smaller' in _err(lib)
        assert bwd(None, need) != 0 and b'workspace is required' in _err(lib)
    assert lib.mrcnn_roi_pool_bwd_ws(p, None, p, p, 1, 8, 8, 4, 4, 7, 7, 1, f, p, 1 << 20, None) != 0
    assert b'null' in _err(lib)
    assert lib.mrcnn_abi_version() == 1


def test_new_kernels_use_no_scratch():
    """Every kernel of roi_pool_variants.hip keeps its registers: no scratch, no VGPR spills."""
    cmd = ['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC',
           '-I' + os.path.join(ROOT, 'include'), '-I' + CSRC, '-ffp-contract=off',
           '-Rpass-analysis=kernel-resource-usage', '-c',
           os.path.join(CSRC, 'roi_pool_variants.hip'), '-o', os.devnull]
    err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    res, name = {}, None
    for line in err.splitlines():
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            name = m.group(1)
            res[name] = {}
            continue
        m = re.search(r'remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)', line)
        if m and name:
            res[name][m.group(1).strip()] = int(m.group(2))
    for k in ('roi_pool_fwd_kernel', 'crop_resize_fwd_kernel', 'pv_tables_kernel', 'pv_bwd_owner_kernel'):
        assert any(k in n for n in res), k
    for n, v in res.items():
        assert v.get('ScratchSize', 0) == 0 and v.get('VGPRs Spill', 0) == 0, (n, v)
