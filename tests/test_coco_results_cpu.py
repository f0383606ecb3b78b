"""COCO results files without a GPU: the vectorised NumPy RLE reference against the oracle's
per-pixel codec, results entries, the streaming writer and the loader's checks, the 'test-dev'
split and the annotations-only accessor, ABI argument rejection and register use of the RLE
kernels (csrc/mask_rle.hip)."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import np_data
from chainer_mask_rcnn_amd.datasets.coco import COCOInstanceSegmentationDataset
from chainer_mask_rcnn_amd.utils.evaluations import coco_results as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'chainer_mask_rcnn_amd', 'csrc')


# ------------------------------------------------------------- vectorised NumPy reference
def np_rle_counts(mask):
    """(H, W) mask -> COCO's uncompressed counts (column-major runs, zeros first)."""
    flat = (np.asarray(mask) != 0).astype(np.int8).T.reshape(-1)
    change = np.flatnonzero(np.diff(np.concatenate([[0], flat])))
    return np.diff(np.concatenate([[0], change, [flat.size]])).astype(np.int64)


def np_rle_string(counts):
    """Counts -> compressed string (maskApi.c rleToString), all values at once."""
    c = np.asarray(counts, np.int64)
    v = c.copy()
    v[3:] = c[3:] - c[1:-2]
    chars = np.zeros((len(v), 7), np.uint8)
    n = np.zeros(len(v), np.int64)
    active = np.ones(len(v), bool)
    x = v.copy()
    for k in range(7):
        d = x & 0x1f
        x = x >> 5
        more = np.where(d & 0x10, x != -1, x != 0)
        chars[:, k] = (d | np.where(more, 0x20, 0)) + 48
        n += active
        active &= more
    return chars[np.arange(7)[None, :] < n[:, None]].tobytes().decode('ascii')


def small_masks(rng):
    out = [np.zeros((3, 4), np.uint8), np.ones((3, 4), np.uint8), np.ones((1, 1), np.uint8),
           np.zeros((1, 1), np.uint8), np.ones((1, 5), np.uint8), np.ones((5, 1), np.uint8)]
    for H, W in ((2, 2), (3, 5), (7, 6), (1, 9), (9, 1)):
        for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
            m = np.zeros((H, W), np.uint8)
            m[y, x] = 1
            out.append(m)
    cb = (np.indices((6, 7)).sum(0) % 2).astype(np.uint8)
    out += [cb, 1 - cb, np.tile([[1], [0]], (3, 5)).astype(np.uint8)]
    for _ in range(20):
        H, W = rng.randint(1, 12, 2)
        out.append((rng.uniform(size=(H, W)) < rng.uniform()).astype(np.uint8))
    big = np.zeros((40, 70), np.uint8)           # long runs: multi-character and negative deltas
    big[3:37, 5:60] = 1
    big[10:12, :] = 0
    out.append(big)
    return out


def test_numpy_reference_equals_oracle():
    rng = np.random.RandomState(0)
    for m in small_masks(rng):
        counts = np_rle_counts(m)
        assert counts.tolist() == np_data.mask_to_rle_counts(m)
        s = np_rle_string(counts)
        assert s == np_data.rle_to_string(counts.tolist())
        assert np_data.rle_from_string(s) == counts.tolist()
        assert np.array_equal(np_data.rle_decode({'size': list(m.shape), 'counts': s}), m)
        assert all(48 <= ord(ch) <= 111 for ch in s)


# ------------------------------------------------------------------------- COCO layout
CATS = (1, 3, 18)


def write_coco(root, test_dev=False):
    """Three annotated images (RLE and polygon masks, a crowd region) and one without
    annotations; sparse category ids 1, 3, 18.  test_dev: the image list only."""
    os.makedirs(os.path.join(root, 'annotations'), exist_ok=True)
    images = [dict(id=11, height=6, width=7), dict(id=12, height=5, width=4),
              dict(id=13, height=8, width=9), dict(id=14, height=3, width=3)]
    cats = [dict(id=c, name='cat%d' % c) for c in CATS]
    if test_dev:
        with open(os.path.join(root, 'annotations', 'image_info_test-dev2015.json'), 'w') as f:
            json.dump(dict(images=images, categories=cats), f)
        return images
    m = np.zeros((6, 7), np.uint8)
    m[1:4, 2:6] = 1
    m2 = np.zeros((5, 4), np.uint8)
    m2[0, :] = 1
    anns = [
        dict(id=1, image_id=11, category_id=18, iscrowd=0, area=12.,
             segmentation={'size': [6, 7], 'counts': np_data.rle_to_string(np_data.mask_to_rle_counts(m))}),
        dict(id=2, image_id=12, category_id=3, iscrowd=0, area=4.,
             segmentation={'size': [5, 4], 'counts': np_data.mask_to_rle_counts(m2)}),
        dict(id=3, image_id=13, category_id=1, iscrowd=0, area=9.,
             segmentation=[[1., 1., 5., 1., 5., 5., 1., 5.]]),
        dict(id=4, image_id=13, category_id=3, iscrowd=1, area=4.,
             segmentation={'size': [8, 9], 'counts': [0, 2, 6, 2, 62]}),
    ]
    with open(os.path.join(root, 'annotations', 'instances_minival2014.json'), 'w') as f:
        json.dump(dict(images=images, annotations=anns, categories=cats), f)
    return images


@pytest.fixture
def coco(tmp_path):
    write_coco(str(tmp_path))
    return COCOInstanceSegmentationDataset('minival', root_dir=str(tmp_path), use_crowd=True,
                                           return_crowd=True, return_area=True)


def test_class_id_to_cat_id_inverts_the_sparse_ids(coco):
    assert coco.cat_id_to_class_id == {1: 0, 3: 1, 18: 2}
    assert coco.class_id_to_cat_id == {0: 1, 1: 3, 2: 18}
    assert coco.img_ids == [11, 12, 13]                    # 14 has no annotation
    assert coco.img_sizes[14] == (3, 3)


def test_annotations_accessor_needs_no_image(coco):
    bboxes, labels, masks, crowds, areas = coco.get_annotations(0)
    assert masks.shape == (1, 6, 7) and masks.dtype == np.int32
    assert labels.tolist() == [2] and bboxes.tolist() == [[1., 2., 4., 6.]]
    bboxes, labels, masks, crowds, areas = coco.get_annotations(2)
    assert labels.tolist() == [0, 1] and crowds.tolist() == [0, 1]
    assert masks.shape == (2, 8, 9) and areas.tolist() == [9., 4.]


def test_results_entries_xywh_and_category_ids():
    bb = np.array([[1.5, 2.25, 10., 20.5], [0., 0., 3., 4.]], np.float32)   # y1 x1 y2 x2
    segs = [{'size': [30, 40], 'counts': 'PT1'}, {'size': [30, 40], 'counts': '0`0'}]
    scores = np.array([0.9, 1 / 3.], np.float32)
    ents = CR.results_entries(12, bb, np.array([2, 0], np.int32), scores, segs,
                              {0: 1, 1: 3, 2: 18})
    assert ents[0]['bbox'] == [2.25, 1.5, 18.25, 8.5]
    assert ents[1]['bbox'] == [0., 0., 4., 3.]
    assert [e['category_id'] for e in ents] == [18, 1]
    assert [e['image_id'] for e in ents] == [12, 12]
    assert ents[1]['score'] == float(np.float32(1 / 3.))
    assert np.float32(json.loads(json.dumps(ents[1]['score']))) == scores[1]
    assert ents[0]['segmentation'] == segs[0]


def test_writer_loader_round_trip_with_backslashes(coco, tmp_path):
    # a first count of 44 is the characters '\' (44 | 0x20 + 48 = 92) then '1'
    counts = [44, 3, 12, 1]
    s = np_rle_string(counts)
    assert '\\' in s and s == np_data.rle_to_string(counts)
    m = np_data.rle_decode({'size': [6, 10], 'counts': s})
    assert m.sum() == 4
    path = str(tmp_path / 'res.json')
    with CR.ResultsWriter(path, coco.img_ids, coco.class_id_to_cat_id) as w:
        w(0, np.zeros((1, 4), np.float32), [2], np.array([0.5], np.float32),
          [{'size': [6, 7], 'counts': np_rle_string(np_rle_counts(np.eye(6, 7)))}])
        w(1, np.zeros((0, 4), np.float32), [], np.zeros(0, np.float32), [])
        w(2, np.ones((2, 4), np.float32), [0, 1], np.array([0.25, 0.75], np.float32),
          [{'size': [8, 9], 'counts': np_rle_string(c)} for c in ([25, 1, 44, 2], [44, 28])])
    text = open(path).read()
    assert '\\\\' in text                                   # JSON escapes the backslash
    data = json.loads(text)
    assert len(data) == 3 and w.n_entries == 3 and w.image_ids == [11, 12, 13]
    grouped = CR.load_results(path, coco)
    assert list(grouped) == [11, 13]
    assert [e['score'] for e in grouped[13]] == [0.25, 0.75]
    assert grouped[13][1]['segmentation']['counts'] == np_rle_string([44, 28])
    assert np_data.rle_from_string(grouped[13][1]['segmentation']['counts']) == [44, 28]


def test_loader_keeps_file_order_and_accepts_no_bbox_and_count_lists(coco):
    seg = lambda: {'size': [8, 9], 'counts': [72]}
    res = [dict(image_id=13, category_id=1, score=0.1, segmentation=seg()),
           dict(image_id=11, category_id=3, score=0.2,
                segmentation={'size': [6, 7], 'counts': '0e0'}),
           dict(image_id=13, category_id=18, score=0.3, segmentation=seg(), bbox=[0, 0, 1, 1])]
    g = CR.load_results(res, coco)
    assert list(g) == [13, 11]
    assert [e['score'] for e in g[13]] == [0.1, 0.3]


@pytest.mark.parametrize('bad, match', [
    (dict(image_id=99), 'unknown image_id'),
    (dict(category_id=2), 'unknown category_id'),
    (dict(segmentation={'size': [7, 6], 'counts': '0e0'}), 'size'),
    (dict(segmentation=[[0., 0., 3., 0., 3., 3.]]), 'polygon'),
    (dict(segmentation={'counts': '0e0'}), 'segmentation'),
    (dict(segmentation={'size': [6, 7], 'counts': 42}), 'counts'),
    (dict(score=None), None),
])
def test_loader_errors(coco, bad, match):
    e = dict(image_id=11, category_id=3, score=0.5, segmentation={'size': [6, 7], 'counts': '0e0'})
    e.update(bad)
    if match is None:                                       # a missing key
        del e['score']
        match = 'score'
    with pytest.raises(ValueError, match=match):
        CR.load_results([dict(image_id=12, category_id=3, score=1.,
                              segmentation={'size': [5, 4], 'counts': [20]}), e], coco)
    with pytest.raises(ValueError, match='list'):
        CR.load_results({'image_id': 11}, coco)


def test_test_dev_split_lists_every_image_with_empty_annotations(tmp_path):
    import PIL.Image
    root = str(tmp_path)
    images = write_coco(root, test_dev=True)
    d = COCOInstanceSegmentationDataset('test-dev', root_dir=root, return_crowd=True,
                                        return_area=True)
    assert d.img_ids == [im['id'] for im in images] and len(d) == 4
    assert d.class_id_to_cat_id == {0: 1, 1: 3, 2: 18}
    bboxes, labels, masks, crowds, areas = d.get_annotations(1)
    assert bboxes.shape == (0, 4) and labels.shape == (0,) and masks.shape == (0, 5, 4)
    assert crowds.shape == (0,) and areas.shape == (0,)
    os.makedirs(os.path.join(root, 'test2015'))
    img = np.zeros((5, 4, 3), np.uint8)
    PIL.Image.fromarray(img).save(os.path.join(root, 'test2015', 'COCO_test2015_%012d.jpg' % 12))
    ex = d[1]
    assert ex[0].shape == (5, 4, 3) and ex[1].shape == (0, 4) and ex[3].shape == (0, 5, 4)
    with pytest.raises(ValueError):
        COCOInstanceSegmentationDataset('test', root_dir=root)


# ------------------------------------------------------------------ ABI and kernel resources
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from chainer_mask_rcnn_amd import _lib
    return _lib.load()


def test_rle_abi_rejects_bad_arguments(lib):
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lambda: lib.mrcnn_last_error()
    enc = lambda N, H, W, cv=4, cc=4, q=p: lib.mrcnn_rle_encode(q, p, N, H, W, p, p, p, p, cv, p,
                                                                 p, cc, None)
    assert enc(1, 0, 4) != 0 and b'bad shape' in err()
    assert enc(-1, 4, 4) != 0 and b'bad shape' in err()
    assert enc(1, 4, 4, cv=-1) != 0 and b'bad shape' in err()
    assert enc(1, 65536, 32768) != 0 and b'2^31' in err()
    assert enc(1000, 1000, 1000) != 0 and b'too large' in err()
    assert enc(1, 4, 4, q=None) != 0 and b'null' in err()
    assert enc(0, 4, 4, q=None) == 0                      # nothing to do
    dec = lambda c, v, N=1, H=4, W=4: lib.mrcnn_rle_decode(c, v, p, N, H, W, p, p, p, p, p, p,
                                                           None)
    assert dec(p, None, H=0) != 0 and b'bad shape' in err()
    assert dec(p, None, H=65536, W=32768) != 0 and b'2^31' in err()
    assert dec(p, p) != 0 and b'exactly one' in err()
    assert dec(None, None) != 0 and b'exactly one' in err()
    assert dec(None, None, N=0) == 0
    assert lib.mrcnn_mask_unpack(p, 1, 0, 4, p, None) != 0 and b'bad shape' in err()
    assert lib.mrcnn_mask_unpack(None, 1, 4, 4, p, None) != 0 and b'null' in err()
    assert lib.mrcnn_abi_version() == 1


def _resources(src):
    cmd = ['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC',
           '-I' + os.path.join(ROOT, 'include'), '-I' + CSRC,
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


def test_rle_kernels_use_no_scratch():
    """Every kernel of mask_rle.hip keeps its registers: no scratch, no spills."""
    res = _resources('mask_rle.hip')
    for k in ('rle_count_kernel', 'rle_scan_kernel', 'rle_value_offsets_kernel',
              'rle_positions_kernel', 'rle_counts_kernel', 'rle_string_kernel',
              'rle_parse_kernel', 'rle_decode_init_kernel', 'rle_fill_kernel', 'unpack_kernel'):
        assert any(k in n for n in res), k
    for n, v in res.items():
        assert v.get('ScratchSize', 0) == 0, (n, v)
        assert v.get('VGPRs Spill', 0) == 0 and v.get('SGPRs Spill', 0) == 0, (n, v)
