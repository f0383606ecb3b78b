"""Instance drawing without a device: the NumPy restatement against the fixture produced by the
reference's own draw_instance_bboxes, the fixture against its generator, the boundary rule
against scipy, the colormap's known values, the C ABI's argument checks and the kernels'
register budget."""
import ctypes
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'chainer_mask_rcnn_amd', 'csrc')
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import visualize_ref as R  # noqa: E402


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'draw_instances.npz'))


def unpack(d, key):
    shape = tuple(d[key + '_shape'])
    return np.unpackbits(d[key], axis=-1)[..., :shape[-1]].reshape(shape).astype(bool)


def case(d, name):
    """(img, bboxes, labels, params, draw, masks as stored, full-frame masks)."""
    img, bboxes, labels = d[name + '_img'], d[name + '_bboxes'], d[name + '_labels']
    n_class, alpha, thickness, bg = d[name + '_params']
    p = dict(n_class=int(n_class), alpha=float(alpha), thickness=int(thickness), bg_class=int(bg),
             draw=list(d[name + '_draw']) if name + '_draw' in d else None)
    H, W = img.shape[:2]
    key = name + '_masks'
    if key + '_shape' in d:
        masks = full = unpack(d, key)
    elif key + '_count' in d:
        masks = [unpack(d, '%s_%d' % (key, j)) for j in range(int(d[key + '_count']))]
        full = np.zeros((len(masks), H, W), bool)
        for i, (m, b) in enumerate(zip(masks, bboxes.astype(int))):
            if m.shape == (H, W):
                full[i] = m
            else:
                full[i, b[0]:b[2], b[1]:b[3]] = m
    else:
        masks = full = None
    return img, bboxes, labels, p, masks, full


def test_restatement_matches_reference_fixture(golden):
    names = list(golden['cases'])
    assert len(names) == 9
    for name in names:
        img, bboxes, labels, p, _, full = case(golden, name)
        got = R.draw(img, bboxes, labels, p['n_class'], full, None, p['bg_class'],
                     p['thickness'], p['alpha'], p['draw'])
        assert got.dtype == np.uint8 and np.array_equal(got, golden[name + '_out']), name


def test_fixture_cases_cover_the_contract(golden):
    alphas, thick = set(), set()
    for name in golden['cases']:
        img, bboxes, labels, p, masks, full = case(golden, name)
        alphas.add(p['alpha'])
        thick.add(p['thickness'])
        assert not np.array_equal(golden[name + '_out'], img), name     # something was drawn
    assert {0.3, 0.5, 1.0} <= alphas and thick == {1, 2, 3}
    assert isinstance(case(golden, 'box_sized')[4], list)
    assert case(golden, 'no_masks')[4] is None
    assert '_draw' in ''.join(k for k in golden.files if k.startswith('full1'))
    # fractional boxes (truncated) and boxes on the image edge
    b = golden['full2_bboxes']
    assert (b != np.floor(b)).any() and (b[:, 2] == golden['full2_img'].shape[0]).any()


def test_fixture_inputs_regenerate_identically(golden):
    import gen_visualize_golden as gen
    for name, p, img, bboxes, labels, masks in gen.cases():
        assert np.array_equal(img, golden[name + '_img']), name
        assert np.array_equal(bboxes, golden[name + '_bboxes']), name
        assert np.array_equal(labels, golden[name + '_labels']), name
        _, _, _, q, stored, _ = case(golden, name)
        assert q['draw'] == (None if p['draw'] is None else list(p['draw'])), name
        if masks is None:
            assert stored is None
        elif isinstance(masks, np.ndarray):
            assert np.array_equal(masks, stored), name
        else:
            assert all(np.array_equal(a, b) for a, b in zip(masks, stored)), name


def test_fixture_outputs_regenerate_from_reference(golden):
    """Runs the reference's own function body (set CHAINER_MASK_RCNN_REFERENCE to its
    checkout)."""
    ref = os.environ.get('CHAINER_MASK_RCNN_REFERENCE')
    if not ref or not os.path.exists(os.path.join(ref, 'chainer_mask_rcnn/utils/visualizations.py')):
        pytest.skip('the reference checkout is not available')
    import gen_visualize_golden as gen
    draw = gen.ref_function(ref)
    for name, p, img, bboxes, labels, masks in gen.cases():
        out = draw(img, bboxes, labels, p['n_class'], masks=masks, captions=None,
                   bg_class=p['bg_class'], thickness=p['thickness'], alpha=p['alpha'],
                   draw=p['draw'])
        assert np.array_equal(out, golden[name + '_out']), name


def test_boundary_rule_matches_scipy():
    import scipy.ndimage as ndi
    rng = np.random.RandomState(0)
    fp = np.ones((3, 3), bool)
    for _ in range(200):
        h, w = rng.randint(1, 12, 2)
        m = rng.uniform(size=(h, w)) < rng.uniform(0.1, 0.9)
        u = m.astype(np.uint8)
        want = ndi.grey_dilation(u, footprint=fp) != ndi.grey_erosion(u, footprint=fp)
        assert np.array_equal(R.boundary(m), want)


def test_colormap_known_values():
    from chainer_mask_rcnn_amd import utils
    cmap = utils.label_colormap(21)
    assert cmap.dtype == np.float32 and cmap.shape == (21, 3)
    want = np.array([[0, 0, 0], [128, 0, 0], [0, 128, 0], [128, 128, 0], [0, 0, 128],
                     [128, 0, 128], [0, 128, 128], [128, 128, 128], [64, 0, 0]], np.float32)
    assert np.array_equal(cmap[:9], want / 255)
    assert np.array_equal(cmap[20] * 255, np.float32([0, 64, 128]) / 255 * 255)
    assert np.array_equal(utils.label_colormap(256), R.label_colormap(256))
    assert np.array_equal(utils.label_colormap(256)[255] * 255, np.float32([224, 224, 192]) / 255 * 255)


def test_tile_layout_is_fcns_rule():
    from chainer_mask_rcnn_amd.utils import visualizations as V
    cell_h, cell_w, cells = V.tile_layout([(100, 200, 3), (50, 60, 3), (80, 40, 3)], (2, 2))
    assert (cell_h, cell_w) == (50, 40)
    # scale min(50/100, 40/200) = 0.2 -> (20, 40); min(1, 40/60) -> (33, 40); (50, 25)
    assert cells == [(20, 40, 15, 0), (33, 40, 8, 0), (50, 25, 0, 7)]
    assert V._tile_shape(9) == (3, 3) and V._tile_shape(5) == (2, 3)


def test_captions_render_with_pillow():
    from chainer_mask_rcnn_amd.utils import visualizations as V
    a, dy, dx = V.caption_coverage('person 98.7%')
    assert a.dtype == np.uint8 and a.ndim == 2 and a.max() > 200 and dy < 0
    lay = V.caption_layout(['x', 'car 1.0%'], np.array([[5, 6, 30, 40], [0, 0, 9, 9]]),
                           [False, True])
    assert lay[0] is None and lay[1][2].shape[0] > 0
    assert lay[1][1] == 0 + V.caption_coverage('car 1.0%')[2]


def test_deprecated_alias_warns_and_forwards(monkeypatch):
    from chainer_mask_rcnn_amd.utils import visualizations as V
    seen = {}
    monkeypatch.setattr(V, 'draw_instance_bboxes', lambda *a, **k: seen.update(a=a, k=k) or 'ok')
    with pytest.warns(UserWarning, match='deprecated'):
        assert V.draw_instance_boxes('img', 'b', 'l', 3, thickness=2) == 'ok'
    assert seen['k']['thickness'] == 2 and seen['a'][3] == 3


def test_report_extension_is_exported():
    from chainer_mask_rcnn_amd import extensions
    r = extensions.InstanceSegmentationVisReport(None, None, ['a', 'b'])
    assert r.file_name == 'visualizations/iteration=%08d.jpg' and r._shape == (3, 3)
    assert list(r.label_names) == ['a', 'b'] and r._copy_latest


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from chainer_mask_rcnn_amd import _lib
    return _lib.load()


def test_abi_rejects_bad_arguments(lib):
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lambda: lib.mrcnn_last_error()
    d = lib.mrcnn_draw_instances
    ok = dict(img=p, H=4, W=4, packed=p, extent=p, N=2, inst=p, atlas=p, ab=16, alpha=0.5, th=1,
              stream=None)

    def call(**kw):
        a = dict(ok)
        a.update(kw)
        return d(*a.values())
    assert call(H=0) != 0 and b'bad shape' in err()
    assert call(W=-1) != 0 and b'bad shape' in err()
    assert call(N=-1) != 0 and b'bad shape' in err()
    assert call(H=65536, W=32768) != 0 and b'2^31' in err()
    assert call(H=300000, W=2) != 0 and b'H >' in err()
    assert call(N=4097) != 0 and b'4096' in err()
    assert call(alpha=1.5) != 0 and b'alpha' in err()
    assert call(alpha=float('nan')) != 0 and b'alpha' in err()
    assert call(th=0) != 0 and b'thickness' in err()
    assert call(ab=-1) != 0 and b'atlas' in err()
    assert call(img=None) != 0 and b'null' in err()
    assert call(inst=None) != 0 and b'null' in err()
    assert call(atlas=None) != 0 and b'null' in err()
    assert call(N=0, inst=None, packed=None, extent=None) == 0          # nothing to draw
    from chainer_mask_rcnn_amd.utils.visualizations import _TileCell
    assert ctypes.sizeof(_TileCell) == 32
    t = lib.mrcnn_tile_images
    cells = (_TileCell * 2)(_TileCell(p.value, 4, 4, 4, 4, 0, 0), _TileCell(p.value, 4, 4, 4, 4, 0, 0))
    assert t(cells, 2, 0, 2, 4, 4, p, None) != 0 and b'bad shape' in err()
    assert t(cells, 3, 1, 2, 4, 4, p, None) != 0 and b'cells' in err()
    assert t(cells, 2, 8, 9, 4, 4, p, None) != 0 and b'64' in err()
    assert t(cells, 2, 1, 2, 70000, 4, p, None) != 0 and b'65535' in err()
    assert t(cells, 2, 1, 2, 50000, 50000, p, None) != 0 and b'2^31' in err()
    assert t(None, 2, 1, 2, 4, 4, p, None) != 0 and b'null' in err()
    assert t(cells, 2, 1, 2, 4, 4, None, None) != 0 and b'null' in err()
    bad = (_TileCell * 1)(_TileCell(p.value, 4, 4, 5, 4, 0, 0))
    assert t(bad, 1, 1, 1, 4, 4, p, None) != 0 and b'outside its cell' in err()
    bad = (_TileCell * 1)(_TileCell(p.value, 4, 4, 3, 4, 2, 0))
    assert t(bad, 1, 1, 1, 4, 4, p, None) != 0 and b'outside its cell' in err()
    bad = (_TileCell * 1)(_TileCell(None, 4, 4, 4, 4, 0, 0))
    assert t(bad, 1, 1, 1, 4, 4, p, None) != 0 and b'bad source' in err()
    bad = (_TileCell * 1)(_TileCell(p.value, 0, 4, 4, 4, 0, 0))
    assert t(bad, 1, 1, 1, 4, 4, p, None) != 0 and b'bad source' in err()
    assert lib.mrcnn_abi_version() == 1


def test_python_side_rejects_bad_arguments():
    from chainer_mask_rcnn_amd import utils
    img = np.zeros((4, 5, 3), np.uint8)
    with pytest.raises(AssertionError):
        utils.draw_instance_bboxes(img.astype(np.float32), np.zeros((0, 4)), np.zeros(0), 2)
    with pytest.raises(AssertionError):
        utils.draw_instance_bboxes(img, np.zeros((2, 3)), np.zeros(2), 2)
    with pytest.raises(AssertionError):
        utils.draw_instance_bboxes(img, np.zeros((2, 4)), np.zeros((2, 1)), 2)
    with pytest.raises(AssertionError):
        utils.draw_instance_bboxes(img, np.zeros((2, 4)), np.zeros(2), 2, draw=[True])
    with pytest.raises(AssertionError):
        utils.draw_instance_bboxes(img, np.zeros((2, 4)), np.zeros(2), 2,
                                   masks=np.zeros((1, 4, 5), bool))
    with pytest.raises(AssertionError):
        utils.draw_instance_bboxes(img, np.zeros((2, 4)), np.zeros(2), 2, captions=['a'])


def _resources(src):
    cmd = ['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC',
           '-ffp-contract=off', '-I' + os.path.join(ROOT, 'include'), '-I' + CSRC,
           '-Rpass-analysis=kernel-resource-usage', '-c', os.path.join(CSRC, src), '-o', os.devnull]
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
    return res


def test_visualize_kernels_use_no_scratch():
    res = _resources('visualize.hip')
    for k in ('draw_instances_kernel', 'tile_images_kernel'):
        assert any(k in n for n in res), k
    assert len(res) == 2
    for n, v in res.items():
        assert v.get('ScratchSize', 0) == 0 and v.get('VGPRs Spill', 0) == 0, (n, v)
        assert v.get('SGPRs Spill', 0) == 0, (n, v)


def test_lin_coord_lives_in_one_header():
    src = {f: open(os.path.join(CSRC, f)).read() for f in ('image.hip', 'visualize.hip',
                                                             'bilinear.h')}
    assert 'Lin lin_coord(' in src['bilinear.h']
    assert 'Lin lin_coord(' not in src['image.hip'] and 'Lin lin_coord(' not in src['visualize.hip']
    assert '#include "bilinear.h"' in src['image.hip'] and '#include "bilinear.h"' in src['visualize.hip']
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert R.lin_coord(3, 7)[0].tolist() == [0, 3, 5]
