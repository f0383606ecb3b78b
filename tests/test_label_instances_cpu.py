"""Instance label conversion without a device: the NumPy restatement against the fixture
produced by the reference's own functions, the fixture's inputs against its generator, the
C ABI's argument checks, the kernels' register budget, and the VOC / SBD dataset classes up to
the point where an example would need the device."""
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

import label_instances_ref as R  # noqa: E402


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'label_instances.npz'))


def unpack(d, key):
    shape = tuple(d[key + '_shape'])
    return np.unpackbits(d[key], axis=-1)[..., :shape[-1]].reshape(shape).astype(bool)


def test_restatement_matches_reference_fixture(golden):
    names = list(golden['cases'])
    assert len(names) == 12
    for name in names:
        classes, boxes, masks = R.label2instance_boxes(golden[name + '_ins'], golden[name + '_cls'],
                                                       return_masks=True)
        assert classes.dtype == np.int32 and np.array_equal(classes, golden[name + '_classes']), name
        assert boxes.dtype == np.int32 and np.array_equal(boxes, golden[name + '_boxes']), name
        assert masks.dtype == bool and np.array_equal(masks, unpack(golden, name + '_masks')), name
    for name in golden['paint_cases']:
        p = 'paint_%s_' % name
        scores = golden[p + 'scores'] if p + 'scores' in golden else None
        lbl_ins, lbl_cls = R.instance_boxes2label(golden[p + 'labels'], None,
                                                  unpack(golden, p + 'masks'), scores)
        assert np.array_equal(lbl_ins, golden[p + 'lbl_ins']), name
        assert np.array_equal(lbl_cls, golden[p + 'lbl_cls']), name


def test_fixture_cases_cover_the_contract(golden):
    c = lambda n, k: golden[n + '_' + k]
    # first-seen tie winners that are neither the smaller value nor the image-wide majority
    assert list(c('tie_first_seen', 'classes')) == [9, 5]
    assert list(c('tie_fewer_overall', 'classes')) == [7, 3]
    assert set(np.unique(c('ids_gaps', 'ins'))) == {-1, -5, 0, 7, 254}
    assert tuple(c('empty', 'masks_shape')) == (0, 5, 7) and c('empty', 'boxes').shape == (0, 4)
    assert c('h1', 'ins').shape[0] == 1 and c('w1', 'ins').shape[1] == 1
    assert (c('voc_like', 'raw_cls') == 255).any() and c('voc_like', 'ins').shape == (375, 500)
    ins, cls = R.voc_preprocess(c('voc_like', 'raw_ins'), c('voc_like', 'raw_cls'))
    assert np.array_equal(ins, c('voc_like', 'ins')) and np.array_equal(cls, c('voc_like', 'cls'))
    tied = golden['paint_tied_scores_scores']
    assert len(np.unique(tied)) < len(tied)


def test_fixture_inputs_regenerate_identically(golden):
    import gen_label_instances_golden as gen
    for name, ins, cls, raw in gen.cases():
        assert np.array_equal(ins, golden[name + '_ins']) and ins.dtype == golden[name + '_ins'].dtype
        assert np.array_equal(cls, golden[name + '_cls'])
        if raw is not None:
            assert np.array_equal(raw[0], golden[name + '_raw_ins'])
            assert np.array_equal(raw[1], golden[name + '_raw_cls'])
        # and the outputs through the restatement
        got = R.label2instance_boxes(ins, cls, return_masks=True)
        assert np.array_equal(got[0], golden[name + '_classes'])
        assert np.array_equal(np.packbits(got[2], axis=-1), golden[name + '_masks'])
    for name, labels, bboxes, masks, scores in gen.paint_cases():
        p = 'paint_%s_' % name
        assert np.array_equal(labels, golden[p + 'labels'])
        assert np.array_equal(np.packbits(masks, axis=-1), golden[p + 'masks'])
        if scores is not None:
            assert np.array_equal(scores, golden[p + 'scores'])


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
    scan = lib.mrcnn_label_scan
    assert scan(p, 4, p, 4, 0, 4, 0, p, p, p, None) != 0 and b'bad shape' in err()
    assert scan(p, 4, p, 4, 4, -1, 0, p, p, p, None) != 0 and b'bad shape' in err()
    assert scan(p, 2, p, 4, 4, 4, 0, p, p, p, None) != 0 and b'elem_bytes' in err()
    assert scan(p, 4, p, 8, 4, 4, 0, p, p, p, None) != 0 and b'elem_bytes' in err()
    assert scan(p, 4, p, 4, 65536, 32768, 0, p, p, p, None) != 0 and b'2^31' in err()
    assert scan(p, 4, None, 4, 4, 4, 0, p, p, p, None) != 0 and b'null' in err()
    assert scan(p, 4, p, 4, 4, 4, 0, p, None, p, None) != 0 and b'null' in err()
    inst = lib.mrcnn_label_instances
    ok = (p, 4, p, 4, 4, 4, 0, p, p, p, 8, 3, 2, 3, p, p, p, p, p, None)

    def call(**kw):
        names = ['ins', 'ib', 'cls', 'cb', 'H', 'W', 'mbc', 'meta', 'bm', 'pre', 'span_i', 'span_c',
                 'n', 'ncls', 'table', 'ids', 'classes', 'boxes', 'masks', 'stream']
        args = dict(zip(names, ok))
        args.update(kw)
        return inst(*[args[k] for k in names])
    assert call(H=0) != 0 and b'bad shape' in err()
    assert call(n=-1) != 0 and b'bad shape' in err()
    assert call(ncls=0) != 0 and b'bad shape' in err()
    assert call(ib=3) != 0 and b'elem_bytes' in err()
    assert call(H=65536, W=32768) != 0 and b'2^31' in err()
    assert call(span_i=(1 << 24) + 1) != 0 and b'span' in err()
    assert call(span_c=1) != 0 and b'span' in err()                      # fewer values than ncls
    assert call(n=4096, ncls=4097, span_i=4096, span_c=4097) != 0 and b'2^24' in err()
    assert call(table=None) != 0 and b'null' in err()
    assert call(boxes=None) != 0 and b'null' in err()
    assert call(n=0, ins=None, table=None) == 0                          # nothing to do
    paint = lib.mrcnn_instances_to_label
    assert paint(p, None, p, 1, 0, 4, p, p, None) != 0 and b'bad shape' in err()
    assert paint(p, None, p, -1, 4, 4, p, p, None) != 0 and b'bad shape' in err()
    assert paint(p, None, p, 1, 65536, 32768, p, p, None) != 0 and b'2^31' in err()
    assert paint(None, None, p, 1, 4, 4, p, p, None) != 0 and b'null' in err()
    assert paint(p, None, p, 1, 4, 4, None, p, None) != 0 and b'null' in err()
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


def test_label_kernels_use_no_scratch():
    res = _resources('instance_labels.hip')
    for k in ('meta_init_kernel', 'range_kernel', 'bitmap_clear_kernel', 'bitmap_set_kernel',
              'bitmap_scan_kernel', 'table_init_kernel', 'values_kernel', 'histogram_kernel',
              'argmax_kernel', 'masks_kernel', 'paint_kernel'):
        assert any(k in n for n in res), k
    assert len(res) >= 11 + 3 * 4         # 4 label dtype pairs of the templated kernels
    for n, v in res.items():
        assert v.get('ScratchSize', 0) == 0 and v.get('VGPRs Spill', 0) == 0, (n, v)


# ---- datasets: construction needs no device ----------------------------------------------------

def _voc_tree(root, ids):
    for d in ('ImageSets/Segmentation', 'JPEGImages', 'SegmentationClass', 'SegmentationObject'):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    for split, sel in (('train', ids[:2]), ('val', ids[2:])):
        with open(os.path.join(root, 'ImageSets/Segmentation/%s.txt' % split), 'w') as f:
            f.write(''.join(i + '\n' for i in sel))


def test_voc_dataset_construction(tmp_path):
    from chainer_mask_rcnn_amd import datasets
    root = str(tmp_path / 'VOC2012')
    with pytest.raises(IOError, match='VOC2012'):
        datasets.VOC2012InstanceSegmentationDataset('train', root_dir=root)
    _voc_tree(root, ['2007_000032', '2007_000039', '2007_000063'])
    with pytest.raises(ValueError):
        datasets.VOC2012InstanceSegmentationDataset('test', root_dir=root)
    tr = datasets.VOC2012InstanceSegmentationDataset('train', root_dir=root)
    va = datasets.VOC2012InstanceSegmentationDataset('val', root_dir=root)
    assert len(tr) == 2 and len(va) == 1
    assert va.files[0]['seg_object'].endswith('SegmentationObject/2007_000063.png')
    assert tr.files[1]['img'].endswith('JPEGImages/2007_000039.jpg')
    names = tr.class_names
    assert len(names) == 20 and names[0] == 'aeroplane' and names[-1] == 'tvmonitor'
    with pytest.raises(ValueError):
        names[0] = 'x'                                   # read-only
    with pytest.warns(UserWarning, match='renamed'):
        alias = datasets.VOC2012InstanceSeg('val', root_dir=root)
    assert len(alias) == 1


def test_sbd_dataset_construction(tmp_path):
    from chainer_mask_rcnn_amd import datasets
    root = tmp_path / 'dataset'
    with pytest.raises(IOError, match='benchmark_RELEASE|dataset'):
        datasets.SBDInstanceSegmentationDataset('train', root_dir=str(root))
    root.mkdir()
    (root / 'train.txt').write_text('2008_000002\n2008_000003\n2008_000007\n')
    (root / 'val.txt').write_text('2008_000009\n')
    (root / 'mine.txt').write_text('2008_000033\n\n')
    ds = datasets.SBDInstanceSegmentationDataset(root_dir=str(root))          # train by default
    assert len(ds) == 3 and ds.files[2]['ins'].endswith('inst/2008_000007.mat')
    assert ds.files[0]['cls'].endswith('cls/2008_000002.mat')
    assert len(datasets.SBDInstanceSegmentationDataset('val', root_dir=str(root))) == 1
    mine = datasets.SBDInstanceSegmentationDataset('val', root_dir=str(root),
                                                   imgsets_file=str(root / 'mine.txt'))
    assert [f['img'][-15:] for f in mine.files] == ['2008_000033.jpg']
    with pytest.raises(IOError, match='test.txt'):
        datasets.SBDInstanceSegmentationDataset('test', root_dir=str(root))
    assert list(ds.class_names) == list(datasets.VOC2012InstanceSegmentationDataset.class_names)
    with pytest.warns(UserWarning, match='renamed'):
        datasets.SBDInstanceSeg('train', root_dir=str(root))


def test_mask_rcnn_dataset_wrapper_warns():
    from chainer_mask_rcnn_amd import datasets

    class Inst(object):
        class_names = np.array(['__background__', 'a', 'b'])

        def __len__(self):
            return 5
    with pytest.warns(UserWarning, match='deprecated'):
        ds = datasets.MaskRcnnDataset(Inst())
    assert len(ds) == 5 and ds.n_fg_class == 2 and list(ds.fg_class_names) == ['a', 'b']


def test_geometry_host_helpers():
    from chainer_mask_rcnn_amd import utils
    for name in ('label2instance_boxes', 'instance_boxes2label', 'mask_to_bbox',
                 'get_bbox_overlap', 'get_mask_overlap'):
        assert callable(getattr(utils, name))
    assert utils.get_bbox_overlap((0, 0, 10, 10), (5, 5, 15, 15)) == 25. / 175.
    assert utils.get_bbox_overlap((0, 0, 2, 2), (2, 2, 4, 4)) == 0.
    from chainer_mask_rcnn_amd.utils import geometry
    assert geometry.LABEL_WINDOW == 1 << 24
    text = open(os.path.join(ROOT, 'include', 'mrcnn_hip.h')).read()
    assert '#define MRCNN_LABEL_WINDOW (1 << 24)' in text
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        with pytest.raises(TypeError):
            geometry._as_device_label(np.zeros((2, 2), np.float32), 'cpu')
