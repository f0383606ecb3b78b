"""COCO polygons drawn on the device: ``mrcnn_polygon_rasterize`` against the
literal restatement of the rule (tests/polygon_ref.py) — words, areas and boxes bit for bit, the
extent containing every set bit — and the feature through ``upload_packed_masks``, the transform
and ``eval_coco_results``."""
import random

import numpy as np
import pytest
import torch

import polygon_ref as PR
import chainer_mask_rcnn_amd as cmr
from chainer_mask_rcnn_amd import _lib
from chainer_mask_rcnn_amd import datasets as D
from chainer_mask_rcnn_amd import functions as F

pytestmark = pytest.mark.gpu

GUARD = 64
SENT64, SENT32 = -0x5A5A5A5A5A5A5A5B, -0x5A5A5A5B


def _guarded(shape, dtype, dev):
    n = int(np.prod(shape))
    sent = SENT64 if dtype == torch.int64 else SENT32
    buf = torch.full((n + 2 * GUARD,), sent, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n].view(shape), sent


def raw(insts, H, W, dev):
    """mrcnn_polygon_rasterize into guarded, sentinel-filled outputs -> host (words, area, extent,
    box); every output element must have been written and nothing beside them."""
    xy5, ring_off, inst_off = F.upsample_vertices(insts)
    G, Wq = len(insts), (W + 63) // 64
    t = [torch.from_numpy(a.reshape(-1)).to(dev) for a in (xy5, ring_off, inst_off)]
    outs = [_guarded(s, d, dev) for s, d in (((G, H, Wq), torch.int64), ((G,), torch.int32),
                                             ((G, 4), torch.int32), ((G, 4), torch.int32))]
    ws = torch.empty((max(_lib.load().mrcnn_polygon_rasterize_workspace_bytes(G, H, W), 4),),
                     dtype=torch.uint8, device=dev)
    _lib.call('mrcnn_polygon_rasterize', _lib.ptr(t[0]) if xy5.size else None, _lib.ptr(t[1]),
              _lib.ptr(t[2]), G, H, W, *[_lib.ptr(v) for _, v, _ in outs], _lib.ptr(ws), _lib.stream_ptr())
    torch.cuda.synchronize()
    host = []
    for buf, view, sent in outs:
        b = buf.cpu().numpy()
        assert (b[:GUARD] == sent).all() and (b[-GUARD:] == sent).all()
        host.append(view.cpu().numpy())
    return host


def check(insts, H, W, dev, want=None):
    """Device against reference for G instances of one image; returns the reference masks."""
    want = np.stack([PR.mask(rings, H, W) for rings in insts]) if want is None else want
    words, area, extent, box = raw(insts, H, W, dev)
    assert np.array_equal(words, PR.packbits(want)), (H, W)           # also: pad bits zero
    assert np.array_equal(area, want.reshape(len(insts), -1).sum(1))
    assert np.array_equal(box, np.array([PR.tight_box(m) for m in want], np.int32).reshape(-1, 4))
    for m, (y_lo, y_hi, q_lo, q_hi) in zip(want, extent):
        if not m.any():
            assert y_lo >= y_hi and q_lo >= q_hi
        else:
            ys, xs = np.nonzero(m)
            assert 0 <= y_lo <= ys.min() and ys.max() < y_hi <= H
            assert 0 <= q_lo <= xs.min() >> 6 and xs.max() >> 6 < q_hi <= (W + 63) // 64
    return want


def rect(x0, y0, x1, y1):
    return [x0, y0, x1, y0, x1, y1, x0, y1]


# ------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize('name, rings, H, W', PR.KNOWN, ids=[k[0] for k in PR.KNOWN])
def test_known_answers(dev, name, rings, H, W):
    want = check([rings], H, W, dev)[0]
    if name == 'square':
        assert want.sum() == 9 and want[1:4, 1:4].all()
    if name == 'fma_triangle':                            # 107 pixels if ys + s*t were fused
        assert want.sum() == 106 and want[5, 17] == 0
    if name in ('one_vertex', 'two_vertices'):
        assert want.sum() == 0


@pytest.mark.parametrize('W', [1, 63, 64, 65, 130])
@pytest.mark.parametrize('H', [1, 5])
def test_widths_around_the_word_size(dev, H, W):
    insts = PR.random_instances(12, H, W, seed=H * 1000 + W, min_vertices=3)
    insts += [[rect(-5, -5, W + 5, H + 5)], [rect(W - 1.5, -1, W + 3, H + 1)], [rect(-2, -2, 0.6, H + 2)]]
    want = check(insts, H, W, dev)
    assert want[12].all() and want[:12].any()


def test_rings_outside_the_image_are_empty(dev):
    H, W = 20, 70
    outside = [[rect(-30, 2, -4, 15)], [rect(W + 2, 2, W + 30, 15)], [rect(5, -30, 60, -3)],
               [rect(5, H + 3, 60, H + 30)], [rect(-20, -20, -3, -3)], [rect(W + 3, H + 3, W + 9, H + 9)]]
    words, area, extent, box = raw(outside, H, W, dev)
    assert not words.any() and not area.any() and not box.any()
    check(outside, H, W, dev)


def test_rings_across_every_edge_and_corner(dev):
    H, W = 20, 70
    insts = [[rect(-5, 5, 6, 12)], [rect(60, 5, 80, 12)], [rect(20, -6, 50, 4)], [rect(20, 15, 50, 28)],
             [rect(-4, -4, 5, 5)], [rect(62, -4, 75, 5)], [rect(-4, 14, 5, 25)], [rect(62, 14, 75, 25)],
             [[-9.3, 10.2, 35.1, -8.7, 80.4, 9.9, 34.6, 30.2]],                 # a diamond over all four
             [rect(5, 10, 15, H + 10)],                                         # crossings clamped to y = h
             [[10.2, H - 0.3, 30.7, H - 0.3, 20.1, H + 9.0]]]                   # ... all of them: empty or a sliver
    want = check(insts, H, W, dev)
    assert all(m.any() for m in want[:10])
    assert want[9][H - 1, 5:15].all() and want[0][:, 0].any() and want[1][:, W - 1].any()
    clamped = [c for c in PR.crossings(insts[9][0], H, W) if c[1] == H]
    assert len(clamped) == 10                             # the bottom edge: one per column, all at y = h


def test_zero_length_edges(dev):
    H, W = 12, 12
    base = [2.0, 2.0, 9.0, 2.0, 9.0, 9.0, 2.0, 9.0]
    insts = [[base], [base + base[:2]], [base[:2] + base], [base[:4] + base[2:4] + base[2:4] + base[4:]],
             [[2, 2, 2, 2, 2, 2]], [[2, 2, 2, 2, 9, 9, 9, 9]], [[3.04, 3.0, 3.0, 3.04, 3.02, 3.02]]]
    want = check(insts, H, W, dev)
    for k in (1, 2, 3):
        assert np.array_equal(want[k], want[0])
    assert not want[4].any() and not want[5].any()


def test_an_instance_is_the_union_of_its_rings(dev):
    a, b, c = rect(2, 2, 40, 9), rect(30, 5, 75, 14), [20.5, 1.0, 68.0, 3.5, 50.0, 15.5]
    H, W = 16, 80
    want = check([[a, b, c], [a], [b], [c], []], H, W, dev)
    assert np.array_equal(want[0], want[1] | want[2] | want[3])
    assert (want[1] & want[2]).any() and not np.array_equal(want[0], want[1] ^ want[2] ^ want[3])
    assert not want[4].any()


def test_no_instances_and_many(dev):
    words, area, extent, box = raw([], 5, 70, dev)
    assert words.shape == (0, 5, 2) and area.shape == (0,) and box.shape == (0, 4)
    out = F.rasterize_polygons(D.PolygonMasks(5, 70, []), dev)
    assert [tuple(t.shape) for t in out] == [(0, 5, 2), (0,), (0, 4), (0, 4)]
    insts = PR.random_instances(70, 9, 75, seed=70, min_vertices=3)
    want = check(insts, 9, 75, dev)
    assert sum(bool(m.any()) for m in want) > 40


def test_random_instances(dev):
    n = 0
    for seed, (H, W) in enumerate(((80, 150), (37, 129), (64, 64), (11, 100))):
        insts = PR.random_instances(50, H, W, seed=100 + seed)
        want = check(insts, H, W, dev)
        n += len(insts)
        assert sum(bool(m.any()) for m in want) > 25
    assert n == 200


@pytest.fixture(scope='module')
def full_size():
    """One 800 x 1333 image with 8 instances; the first has an edge of about 5 x 1333 steps."""
    H, W = 800, 1333
    rng = np.random.RandomState(5)
    insts = [[[0.4, 10.2, 1332.6, 40.7, 900.3, 420.9, 200.8, 300.1]]]
    for g in range(7):
        cy, cx, ry, rx = rng.uniform(100, 700), rng.uniform(100, 1230), rng.uniform(20, 250), rng.uniform(20, 400)
        k = int(rng.randint(5, 40))
        ang = np.sort(rng.uniform(0, 2 * np.pi, k))
        rad = rng.uniform(0.5, 1.0, k)
        ring = np.stack([cx + rx * rad * np.cos(ang), cy + ry * rad * np.sin(ang)], 1).round(2)
        insts.append([ring.reshape(-1).tolist()] + ([rect(cx - 9, cy - 300, cx + 9, cy + 300)] if g % 3 == 0 else []))
    return insts, H, W, np.stack([PR.mask(rings, H, W) for rings in insts])


def test_full_size_image_and_two_runs_identical(dev, full_size):
    insts, H, W, want = full_size
    check(insts, H, W, dev, want)
    assert want[0].sum() > 100000
    polys = D.PolygonMasks(H, W, insts)
    a = F.rasterize_polygons(polys, dev)
    b = F.rasterize_polygons(polys, dev)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert a[0].dtype == torch.int64 and np.array_equal(a[0].cpu().numpy(), PR.packbits(want))
    assert np.array_equal(a[3].cpu().numpy(), [PR.tight_box(m) for m in want])


def _mixed(H=12, W=70):
    row = lambda m: D.PackedMasks.from_dense(m[None]).words[0]
    insts = [row(PR.RLE_BLOB), PR.TWO_RINGS, row(PR.RLE_CROWD), [rect(60, 1, 69.5, 11)], row(np.zeros((H, W)))]
    dense = np.stack([PR.RLE_BLOB, PR.mask(PR.TWO_RINGS, H, W), PR.RLE_CROWD,
                      PR.mask([rect(60, 1, 69.5, 11)], H, W), np.zeros((H, W), np.uint8)])
    return D.PolygonMasks(H, W, insts), dense


def test_run_length_rows_are_copied_in_beside_the_polygons(dev):
    polys, dense = _mixed()
    words, width = F.upload_packed_masks(polys, dev)
    assert width == 70 and words.dtype == torch.int64 and words.is_contiguous()
    assert np.array_equal(words.cpu().numpy(), PR.packbits(dense))
    packed, area, extent, box = F.rasterize_polygons(polys, dev)
    assert np.array_equal(area.cpu().numpy(), dense.reshape(5, -1).sum(1))
    assert np.array_equal(box.cpu().numpy(), [PR.tight_box(m) for m in dense])
    from chainer_mask_rcnn_amd.utils.evaluations import masks as M
    for given in (polys, polys.to_packed()):
        got = M.pack_masks(given, device=dev)
        for t, w in zip(got, M.pack_masks(dense, device=dev)):
            assert t.dtype == w.dtype and torch.equal(t, w)
    # only run-length rows: no launch at all
    only = polys[np.array([0, 2])]
    assert np.array_equal(F.upload_packed_masks(only, dev)[0].cpu().numpy(), PR.packbits(dense[[0, 2]]))
    with pytest.raises(TypeError):
        F.rasterize_polygons(polys.to_packed(), dev)


# ---------------------------------------------------------------------------------- the pipeline
class _Model(torch.nn.Module):
    """What the transform reads of a model: mean, sizes, the device of its parameters, prepare()."""
    prepare = cmr.models.MaskRCNN.prepare

    def __init__(self, dev):
        super(_Model, self).__init__()
        self.mean = np.array([122.7717, 115.9465, 102.9801], np.float32).reshape(3, 1, 1)
        self.min_size, self.max_size = 160, 240
        self.p = torch.nn.Parameter(torch.zeros(1, device=dev))


def _example(H=97, W=131):
    """3 polygon instances, one of two rings, and one run-length crowd over part of them."""
    rng = np.random.RandomState(0)
    img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    crowd_mask = np.zeros((H, W), np.uint8)
    crowd_mask[30:80, 20:125] = rng.rand(50, 105) < 0.7
    row = D.PackedMasks.from_dense(crowd_mask[None]).words[0]
    insts = [[[5.5, 8.0, 60.2, 12.5, 50.0, 44.4, 9.1, 39.0]], row,
             [rect(70.5, 30.2, 128.8, 90.9), [60.0, 50.0, 100.0, 55.0, 80.0, 96.5]],
             [[3.0, 60.0, 50.5, 62.0, 45.0, 95.0, 20.0, 80.0, 4.0, 96.0]]]
    polys = D.PolygonMasks(H, W, insts)
    packed = polys.to_packed()
    assert type(packed) is D.PackedMasks
    dense = packed.unpack()
    bbox = np.array([PR.tight_box(m) for m in dense], np.float32)
    return img, bbox, np.array([3, 9, 17, 42], np.int32), polys, packed, np.array([0, 1, 0, 0], np.int32)


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if isinstance(w, torch.Tensor):
            assert g.dtype == w.dtype and g.stride() == w.stride() and torch.equal(g, w)
        elif isinstance(w, np.ndarray):
            assert g.dtype == w.dtype and np.array_equal(g, w)
        else:
            assert (g is None and w is None) or g == w


@pytest.mark.parametrize('kw', [dict(), dict(scale_jitter=(0.5, 2.0), crop_size=64), dict(crowd_ignore=True),
                                dict(crowd_ignore=True, scale_jitter=(0.5, 2.0), crop_size=64)],
                         ids=['plain', 'scale_jitter', 'crowd_ignore', 'crowd_ignore+scale_jitter'])
def test_transform_gives_what_the_host_rule_gives(dev, kw):
    img, bbox, label, polys, packed, crowd = _example()
    t = D.MaskRCNNTransform(_Model(dev), device_masks=True, **kw)
    tail = (crowd,) if kw.get('crowd_ignore') else ()
    reg = slice(None) if kw.get('crowd_ignore') else crowd == 0
    flips, planes = set(), 0
    for seed in range(6):
        random.seed(seed)
        flips.add(random.choice([True, False]))
        random.seed(seed)
        want = t((img, bbox[reg], label[reg], packed[reg]) + tail)
        after = random.random()
        random.seed(seed)
        got = t((img, bbox[reg], label[reg], polys[reg]) + tail)
        assert random.random() == after
        _same(got, want)
        assert got[3].dtype == torch.uint8 and got[3].shape[0] == len(got[2]) > 0
        planes += len(got) == 6 and got[5] is not None
    assert flips == {False, True}
    assert planes >= (3 if kw.get('crowd_ignore') else 0)


def test_host_path_of_the_transform_takes_the_host_rule(dev):
    img, bbox, label, polys, packed, _ = _example()
    t = D.MaskRCNNTransform(_Model(dev))
    random.seed(3)
    want = t((img, bbox, label, packed.unpack()))
    random.seed(3)
    _same(t((img, bbox, label, polys)), want)


# -------------------------------------------------------------------------------- the evaluation
def _dataset(root, **kw):
    return D.COCOInstanceSegmentationDataset('minival', root_dir=root, use_crowd=True, return_crowd=True,
                                             return_area=True, **kw)


def _equal(a, b):
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(_equal(a[k], b[k]) for k in a)
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def test_eval_coco_results_scores_the_same_from_vertices(dev, tmp_path):
    from chainer_mask_rcnn_amd.utils.evaluations.coco_results import eval_coco_results
    PR.write_coco(str(tmp_path))
    pil = _dataset(str(tmp_path))
    dense = _dataset(str(tmp_path), polygon_rule='coco')
    poly = _dataset(str(tmp_path), polygon_rule='coco', device_polygons=True)
    results = []                       # every regular instance predicted exactly, by COCO's rule
    for i, img_id in enumerate(dense.img_ids):
        bbox, label, masks, crowd, area = dense.get_annotations(i)
        for g in np.flatnonzero(crowd == 0):
            results.append(dict(image_id=img_id, category_id=dense.class_id_to_cat_id[int(label[g])],
                                score=0.9 - 0.1 * g,
                                segmentation={'size': list(masks[g].shape), 'counts': PR.rle_counts(masks[g])}))
    assert np.array_equal(dense.get_annotations(0)[2][0], PR.mask([PR.SQUARE], 6, 6))
    for iou_type in ('segm', 'boundary'):
        a = eval_coco_results(results, dense, iou_type=iou_type)
        b = eval_coco_results(results, poly, iou_type=iou_type)
        c = eval_coco_results(results, pil, iou_type=iou_type)
        assert _equal(a, b), iou_type
        key = 'validation/main/%smap' % ('' if iou_type == 'segm' else 'boundary/')
        assert a[key] == 1.0 and c[key] < 1.0, (iou_type, a[key], c[key])
        assert not _equal(a, c)
