"""COCO's polygon rule without a device: the package's host rule and its
box helper against the literal restatement (tests/polygon_ref.py), the known answers, the dataset
options and the PolygonMasks container on a synthetic annotation file, and the kernel's per-point
and per-crossing arithmetic (csrc/polygon_walk.h) run by a host program under the sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import polygon_ref as PR
from chainer_mask_rcnn_amd.datasets import COCOInstanceSegmentationDataset, PackedMasks, PolygonMasks
from chainer_mask_rcnn_amd.datasets import coco as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def rings():
    """(ring, h, w, reference mask) of the seeded random set, computed once."""
    return [(r, h, w, PR.mask([r], h, w)) for r, h, w in PR.random_rings()]


def host(rings_, h, w):
    return C.polygon_to_mask_coco(rings_, h, w).astype(np.uint8)


def pil(rings_, h, w):
    import PIL.Image
    import PIL.ImageDraw
    canvas = PIL.Image.new('L', (w, h), 0)
    for ring in rings_:
        PIL.ImageDraw.Draw(canvas).polygon(list(map(tuple, np.asarray(ring).reshape(-1, 2))),
                                           outline=1, fill=1)
    return (np.asarray(canvas) == 1).astype(np.uint8)


# ------------------------------------------------------------------------------------ the rule
def test_host_rule_equals_the_reference_on_random_rings(rings):
    assert len(rings) >= 300
    filled = 0
    for ring, h, w, want in rings:
        assert np.array_equal(host([ring], h, w), want), (ring, h, w)
        filled += bool(want.any())
    assert filled > 100                                  # the set is not mostly empty masks


def test_the_square_is_three_by_three_and_not_what_pil_draws():
    m = PR.mask([PR.SQUARE], 6, 6)
    want = np.zeros((6, 6), np.uint8)
    want[1:4, 1:4] = 1
    assert m.sum() == 9 and np.array_equal(m, want) and np.array_equal(host([PR.SQUARE], 6, 6), want)
    p = pil([PR.SQUARE], 6, 6)
    assert p.sum() == 16 and np.array_equal(np.argwhere(p).min(0), [1, 1])
    assert np.array_equal(np.argwhere(p).max(0), [4, 4]) and not np.array_equal(p, m)


def test_known_answers():
    for fn in (lambda r, h, w: PR.mask(r, h, w), host):
        m = fn([PR.TRIANGLE], 5, 5)
        assert {tuple(p) for p in np.argwhere(m).tolist()} == {(0, 1), (0, 2), (1, 2)}
        m = fn([PR.COVER], 7, 70)
        assert m.sum() == 490 and m.all()
        m = fn([PR.STRADDLE], 5, 130)
        want = np.zeros((5, 130), np.uint8)
        want[:, 63:65] = 1
        assert np.array_equal(m, want)
        assert fn([[2, 2]], 5, 5).sum() == 0 and fn([[1, 1, 3, 3]], 5, 5).sum() == 0
        m = fn([PR.FMA_TRIANGLE], 40, 40)
        assert m.sum() == 106 and m[5, 17] == 0


def test_the_bow_tie_is_filled_even_odd_within_the_ring():
    m = PR.mask([PR.BOWTIE], 10, 10)
    assert m.sum() == 24 and np.array_equal(host([PR.BOWTIE], 10, 10), m)
    # the vertical edges x = 1 and x = 8 each span a triangle with the centre (4.5, 4.5): the left
    # and right quarters of the square are filled, the top and bottom quarters stay clear
    assert m[4, 1] == 1 and m[4, 7] == 1 and m[1, 4] == 0 and m[7, 4] == 0
    cols = np.flatnonzero(m.any(0))
    assert cols.min() == 1 and cols.max() == 7
    assert m[1:8, 1:8].sum() == 24


def test_rings_of_an_instance_are_united_not_xored():
    a, b = [2, 2, 12, 2, 12, 9, 2, 9], [8, 5, 20, 5, 20, 14, 8, 14]
    ma, mb = PR.mask([a], 16, 24), PR.mask([b], 16, 24)
    assert (ma & mb).sum() > 0
    both = PR.mask([a, b], 16, 24)
    assert np.array_equal(both, ma | mb) and np.array_equal(host([a, b], 16, 24), ma | mb)
    assert not np.array_equal(both, ma ^ mb)


def test_repeated_vertices_change_nothing(rings):
    for ring, h, w, want in rings[:60]:
        if len(ring) < 6:
            continue
        closed = ring + ring[:2]                         # the first vertex again at the end
        doubled = ring[:4] + ring[2:4] + ring[4:]        # the second vertex twice in a row
        for variant in (closed, doubled):
            assert np.array_equal(PR.mask([variant], h, w), want)
            assert np.array_equal(host([variant], h, w), want)


def test_box_helper_equals_the_tight_box_of_the_filled_mask(rings):
    for ring, h, w, want in rings:
        assert C.polygon_box_coco([ring], h, w) == PR.tight_box(want), (ring, h, w)
    for seed, (h, w) in enumerate(((40, 90), (7, 130), (80, 150))):
        for inst in PR.random_instances(25, h, w, seed):
            assert C.polygon_box_coco(inst, h, w) == PR.tight_box(PR.mask(inst, h, w))
    assert C.polygon_box_coco([], 5, 5) == (0, 0, 0, 0)
    assert C.polygon_box_coco([[2, 2], [200, 200, 210, 200, 210, 210]], 5, 5) == (0, 0, 0, 0)


def test_bad_coordinates_raise():
    for bad in ([1, 1, 2, 2, 3], [1, 1, float('nan'), 2, 3, 3], [1, 1, float('inf'), 2, 3, 3],
                [1, 1, 2 ** 28, 2, 3, 3], [1, 1, 2, -2.0 ** 28, 3, 3]):
        with pytest.raises(ValueError):
            C.polygon_to_mask_coco([bad], 8, 8)
        with pytest.raises(ValueError):
            C.polygon_box_coco([bad], 8, 8)
        with pytest.raises(ValueError):
            PolygonMasks(8, 8, [[bad]])
    ok = [1, 1, 2.0 ** 27, 2, 3, 3]                      # |5 x| < 2^30: legal
    assert C.upsample_ring(ok)[1, 0] == 5 * 2 ** 27
    assert C.upsample_ring([-0.3, -0.1, 1.5, 2.5]).tolist() == [[-1, 0], [8, 13]]   # truncation


# ---------------------------------------------------------------------------------- the dataset
@pytest.fixture
def root(tmp_path):
    PR.write_coco(str(tmp_path))
    return str(tmp_path)


def dataset(root, **kw):
    return COCOInstanceSegmentationDataset('minival', root_dir=root, use_crowd=True, return_crowd=True,
                                           return_area=True, **kw)


def test_defaults_are_todays(root):
    d = dataset(root)
    bbox, label, masks, crowd, area = d.get_annotations(0)
    assert np.array_equal(masks[0], pil([PR.SQUARE], 6, 6)) and masks.dtype == np.int32
    assert bbox.tolist() == [[1., 1., 5., 5.]] and bbox.dtype == np.float32
    bbox, label, masks, crowd, area = d.get_annotations(1)
    assert np.array_equal(masks[0], pil(PR.TWO_RINGS, 12, 70))
    assert np.array_equal(masks[1], PR.RLE_BLOB) and np.array_equal(masks[2], PR.RLE_CROWD)
    assert label.tolist() == [1, 2, 0] and crowd.tolist() == [0, 0, 1]
    assert np.array_equal(dataset(root, polygon_rule='pil', packed_masks=True).get_annotations(1)[2].unpack(),
                          masks)


def test_coco_rule_changes_polygons_and_nothing_else(root):
    d, c = dataset(root), dataset(root, polygon_rule='coco')
    for i in range(3):
        old, new = d.get_annotations(i), c.get_annotations(i)
        assert len(old[2]) == len(new[2])                        # the kept set
        for k in (1, 3, 4):                                      # labels, crowds, areas
            assert np.array_equal(old[k], new[k]) and old[k].dtype == new[k].dtype
        assert new[2].dtype == np.int32 and new[0].dtype == np.float32
    new = c.get_annotations(0)
    assert np.array_equal(new[2][0], PR.mask([PR.SQUARE], 6, 6)) and new[0].tolist() == [[1., 1., 4., 4.]]
    new = c.get_annotations(1)
    assert np.array_equal(new[2][0], PR.mask(PR.TWO_RINGS, 12, 70))
    assert np.array_equal(new[2][1], PR.RLE_BLOB) and np.array_equal(new[2][2], PR.RLE_CROWD)
    assert new[0].tolist() == [list(map(float, PR.tight_box(m))) for m in new[2]]
    new = c.get_annotations(2)                                   # the malformed run-length one is dropped
    assert len(new[2]) == 1 and np.array_equal(new[2][0], PR.mask([PR.TRIANGLE], 9, 8))
    packed = dataset(root, polygon_rule='coco', packed_masks=True).get_annotations(1)[2]
    assert type(packed) is PackedMasks and np.array_equal(packed.unpack(), c.get_annotations(1)[2])


def test_option_errors(root):
    with pytest.raises(ValueError):
        dataset(root, device_polygons=True)
    with pytest.raises(ValueError):
        dataset(root, polygon_rule='pil', device_polygons=True)
    with pytest.raises(ValueError):
        dataset(root, polygon_rule='pycocotools')


def test_device_polygons_hands_on_a_polygon_masks(root):
    c, p = dataset(root, polygon_rule='coco'), dataset(root, polygon_rule='coco', device_polygons=True)
    for i in range(3):
        dense, poly = c.get_annotations(i), p.get_annotations(i)
        masks = poly[2]
        assert isinstance(masks, PolygonMasks) and isinstance(masks, PackedMasks)
        G = len(dense[2])
        assert len(masks) == G and masks.shape == dense[2].shape and masks.ndim == 3
        assert np.array_equal(masks.to_packed().unpack(), dense[2])
        assert np.array_equal(masks.unpack(np.uint8), dense[2]) and masks.unpack(np.uint8).dtype == np.uint8
        assert np.array_equal(poly[0], dense[0]) and poly[0].dtype == np.float32      # exact boxes
        for k in (1, 3, 4):
            assert np.array_equal(poly[k], dense[k])
    masks, dense = p.get_annotations(1)[2], c.get_annotations(1)[2]
    assert masks.is_polygon().tolist() == [True, False, False]
    for key in (slice(1, 3), slice(0, 0), np.array([2, 0]), np.array([True, False, True]),
                np.array([], np.int64), np.zeros(3, bool)):
        sub = masks[key]
        assert isinstance(sub, PolygonMasks) and np.array_equal(sub.unpack(), dense[key])
        assert sub.shape == dense[key].shape
    with pytest.raises(IndexError):
        masks[np.zeros((1, 1), np.int64)]
    assert np.array_equal(masks.words, PackedMasks.from_dense(dense).words)


def test_bad_polygon_in_the_file_raises(root, tmp_path):
    import json
    path = os.path.join(root, 'annotations', 'instances_minival2014.json')
    data = json.load(open(path))
    data['annotations'][0]['segmentation'] = [[1, 1, 4, 1, 4]]
    json.dump(data, open(path, 'w'))
    for kw in (dict(polygon_rule='coco'), dict(polygon_rule='coco', device_polygons=True)):
        with pytest.raises(ValueError):
            dataset(root, **kw).get_annotations(0)


def test_tools_take_the_polygon_switches(capsys):
    import sys
    for tool, devpoly in (('evaluate.py', False), ('train.py', True), ('train_loop.py', True)):
        src = open(os.path.join(ROOT, 'tools', tool)).read()
        assert '--polygon-rule' in src and ('--device-polygons' in src) == devpoly
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import train
    finally:
        sys.path.pop(0)
    base = ['--dataset', 'coco', '--device-masks']
    plain = train.parse_args(base)
    assert not hasattr(plain, 'polygon_rule') and not hasattr(plain, 'device_polygons')
    assert 'polygon_rule' not in train.recorded_params(plain)
    args = train.parse_args(base + ['--polygon-rule', 'coco', '--device-polygons'])
    assert args.polygon_rule == 'coco' and args.device_polygons is True
    assert train.recorded_params(args)['polygon_rule'] == 'coco'
    for argv in (base + ['--device-polygons'], base + ['--polygon-rule', 'pil', '--device-polygons'],
                 ['--dataset', 'coco', '--polygon-rule', 'coco', '--device-polygons']):
        with pytest.raises(SystemExit) as e:
            train.parse_args(argv)
        assert e.value.code == 2 and '--device-masks --polygon-rule coco' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        train.parse_args(base + ['--polygon-rule', 'pycocotools'])


# ----------------------------------------------------------- the kernel's arithmetic, on the host
@pytest.fixture(scope='module')
def host_program(tmp_path_factory):
    """tests/polygon_walk_host.cpp: csrc/polygon_walk.h as the kernel calls it, built without
    contraction and with the address and undefined-behaviour sanitizers."""
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path_factory.mktemp('polygon_walk') / 'polygon_walk_host')
    subprocess.run([cxx, '-O1', '-g', '-std=c++17', '-ffp-contract=off',
                    '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I' + os.path.join(ROOT, 'chainer_mask_rcnn_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'polygon_walk_host.cpp'), '-o', exe],
                   check=True, capture_output=True, text=True)
    return exe


def test_walk_arithmetic_gives_the_rules_crossings(host_program, tmp_path, rings):
    cases = [(r, h, w) for _, rs, h, w in PR.KNOWN for r in rs]
    cases += [(r, h, w) for r, h, w, _ in rings]
    cases += [([3.0, -2.0, 1300.4, 3.0, 700.0, 790.0], 800, 1333),      # ~5 x 1300 upsampled steps
              ([-8.0, -8.0, -3.0, -9.0, -1.0, 30.0, 2.0, -4.0], 20, 20),  # negative: the casts truncate
              ([2.0, 2.0, 2.0, 2.0, 9.0, 2.0, 9.0, 9.0, 9.0, 9.0, 2.0, 9.0], 12, 12)]   # zero-length edges
    src, dst = str(tmp_path / 'rings.txt'), str(tmp_path / 'crossings.txt')
    with open(src, 'w') as f:
        for ring, h, w in cases:
            up = C.upsample_ring(ring).reshape(-1)
            f.write('%d %d %d %s\n' % (h, w, len(up) // 2, ' '.join(str(int(c)) for c in up)))
    r = subprocess.run([host_program, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = open(dst).read().splitlines()
    assert len(lines) == len(cases)
    total = 0
    for (ring, h, w), line in zip(cases, lines):
        got = [int(v) for v in line.split()]
        got = sorted(zip(got[1::2], got[2::2]))
        want = sorted(PR.crossings(ring, h, w))
        assert got == want, (ring, h, w)
        total += len(want)
    assert total > 5000
