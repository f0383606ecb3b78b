"""Copy-paste on the device: mrcnn_copy_paste through the C ABI and
``functions.copy_paste``, ``datasets.CopyPasteDataset`` over large-scale jitter, one train-chain
step on pasted examples and the train-loop tool.  Every comparison is exact, against the NumPy
definition of tests/copy_paste_ref.py; the image is compared as int32 bit patterns."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import chainer_mask_rcnn_amd as cmr
import chainer_mask_rcnn_amd.datasets as D
from chainer_mask_rcnn_amd import _lib
from chainer_mask_rcnn_amd import functions as F

import copy_paste_ref as R
import test_gpu_gt_masks as GM
import test_gpu_train_loop as TLT
from scale_jitter_ref import boxes_areas
from test_gpu_train_loop import TL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRONT, REAR, FILL = 3, 64, 0xAB     # guard bytes around the mask output; FRONT misaligns it
GUARD = -77
# (Gt, Gs, K): nothing to occlude, nothing to paste, a subset, the whole source
COUNTS = [(0, 1, 1), (1, 1, 0), (3, 4, 2), (2, 5, 5)]


def _offset(dev, host, lead):
    """``host`` on the device ``lead`` bytes into its allocation -> (buffer, address)."""
    flat = np.ascontiguousarray(host).view(np.uint8).reshape(-1)
    buf = torch.full((lead + flat.size + 8,), 0x5C, dtype=torch.uint8, device=dev)
    buf[lead:lead + flat.size] = torch.from_numpy(flat).to(dev)
    return buf, buf.data_ptr() + lead


def _launch(dev, img_t, masks_t, img_s, masks_s, idx, null_unused=False):
    """mrcnn_copy_paste on guarded buffers, the mask inputs at odd byte offsets of their
    allocations -> (rc, img (3, S, S), masks, boxes, areas, guards intact and inputs unchanged)."""
    S = img_t.shape[1]
    Gt, Gs, K = len(masks_t), len(masks_s), len(idx)
    n = Gt + K
    t_hwc, s_hwc = (np.ascontiguousarray(a.transpose(1, 2, 0)) for a in (img_t, img_s))
    ins = [_offset(dev, t_hwc, 16), _offset(dev, s_hwc, 32), _offset(dev, masks_t, 2),
           _offset(dev, masks_s, 1), _offset(dev, np.asarray(idx, np.int32), 4)]
    before = [b.clone() for b, _ in ins]
    img = torch.full((4 + 3 * S * S + 4,), float(GUARD), dtype=torch.float32, device=dev)
    buf = torch.full((FRONT + n * S * S + REAR,), FILL, dtype=torch.uint8, device=dev)
    meta = torch.full((4 + 5 * n + 4,), GUARD, dtype=torch.int32, device=dev)   # guard | box | area | guard
    stats = torch.full((3 * n * S + 4,), GUARD, dtype=torch.int32, device=dev)
    p = [_lib.c_vp(a) for _, a in ins]
    out = [_lib.ptr(img[4:]), _lib.c_vp(buf.data_ptr() + FRONT), _lib.ptr(meta[4:]),
           _lib.ptr(meta[4 + 4 * n:]), _lib.ptr(stats)]
    if null_unused:                                      # a pointer may be null where its count is 0
        if Gt == 0:
            p[2] = None
        if K == 0:
            p[3] = p[4] = None
        if n == 0:
            out[1] = out[2] = out[3] = out[4] = None
    rc = _lib.load().mrcnn_copy_paste(p[0], p[1], p[2], Gt, p[3], Gs, p[4], K, S, *out,
                                      _lib.stream_ptr())
    torch.cuda.current_stream().synchronize()
    img, host, meta, stats = (t.cpu().numpy() for t in (img, buf, meta, stats))
    intact = bool((img[:4] == GUARD).all() and (img[4 + 3 * S * S:] == GUARD).all()
                  and (host[:FRONT] == FILL).all() and (host[FRONT + n * S * S:] == FILL).all()
                  and (meta[:4] == GUARD).all() and (meta[4 + 5 * n:] == GUARD).all()
                  and (stats[3 * n * S:] == GUARD).all()
                  and all(torch.equal(a, b) for a, (b, _) in zip(before, ins)))
    return (rc, img[4:4 + 3 * S * S].reshape(S, S, 3).transpose(2, 0, 1),
            host[FRONT:FRONT + n * S * S].reshape(n, S, S), meta[4:4 + 4 * n].reshape(n, 4),
            meta[4 + 4 * n:4 + 5 * n], intact)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _example(rng, Gt, Gs, K, S, density=0.3):
    img_t = rng.standard_normal((3, S, S)).astype(np.float32)
    img_s = rng.standard_normal((3, S, S)).astype(np.float32)
    masks_t = (rng.uniform(size=(Gt, S, S)) < density).astype(np.uint8)
    masks_s = (rng.uniform(size=(Gs, S, S)) < density).astype(np.uint8)
    idx = sorted(rng.choice(Gs, K, replace=False).tolist()) if K else []
    return img_t, masks_t, img_s, masks_s, idx


def _check(dev, args, what=None, **kw):
    rc, img, masks, boxes, areas, intact = _launch(dev, *args, **kw)
    want = R.compose(*args)
    assert rc == 0 and intact, what
    assert np.array_equal(_bits(img), _bits(want[0])), what
    assert masks.dtype == np.uint8 and np.array_equal(masks, want[1]), what
    assert np.array_equal(boxes, want[2]) and np.array_equal(areas, want[3]), what
    return img, masks, boxes, areas


# ---- kernels -------------------------------------------------------------------------------------
# S below a dword; odd S (rows start misaligned); the 64-bit word of the packed alpha and one past
# it; more than 256 pixels per row (a wave's second step).  All but 64 are no multiple of the 8 rows
# a workgroup owns.
@pytest.mark.parametrize('S', [1, 3, 37, 64, 65, 130, 261])
def test_kernel_equals_the_definition(dev, S):
    rng = np.random.RandomState(S)
    for Gt, Gs, K in COUNTS + ([(40, 33, 30)] if S == 37 else []):    # many planes: grid indexing
        args = _example(rng, Gt, Gs, K, S)
        img, masks, boxes, areas = _check(dev, args, (S, Gt, Gs, K))
        assert len(masks) == Gt + K
        if K == 0:
            assert np.array_equal(_bits(img), _bits(args[0]))
            assert np.array_equal(masks, args[1])
        if K and Gt and S >= 37:
            assert (areas[:Gt] < args[1].reshape(Gt, -1).sum(1)).all()   # every target lost pixels
        # the wrapper: the same call from (3, S, S) channels-last views
        dv = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in args[:4]]
        dv[0], dv[2] = (t.permute(1, 2, 0).contiguous().permute(2, 0, 1) for t in (dv[0], dv[2]))
        out, m, b, a = F.copy_paste(dv[0], dv[1], dv[2], dv[3], args[4])
        assert tuple(out.shape) == (3, S, S) and out.stride() == (1, 3 * S, 3) and out.is_cuda
        assert m.dtype == torch.uint8 and m.is_contiguous() and tuple(m.shape) == (Gt + K, S, S)
        assert b.dtype == a.dtype == torch.int32 and tuple(b.shape) == (Gt + K, 4)
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(img))
        assert np.array_equal(m.cpu().numpy(), masks) and np.array_equal(b.cpu().numpy(), boxes)
        assert np.array_equal(a.cpu().numpy(), areas)
        assert all(torch.equal(t, torch.from_numpy(np.ascontiguousarray(h)).to(dev))
                   for t, h in zip(dv, args[:4]))        # inputs unchanged


def _blobs(rng, G, S):
    """(G, S, S) uint8: one filled ellipse per instance, as instances look on the training canvas."""
    yy, xx = np.mgrid[:S, :S]
    out = np.zeros((G, S, S), np.uint8)
    for g in range(G):
        (cy, cx), (ry, rx) = rng.uniform(0, S, 2), rng.uniform(20, 200, 2)
        out[g] = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
    return out


def _canvas_cases():
    """(S, Gt, K) -> arguments at the workload's sizes, blob-shaped instances, all of the source
    pasted.  One seeded stream over all five cases: (1024, 8, 8), 17 planes in three chunks per row
    group, and (768, 4, 4) are the data on which an earlier form of the kernels, with the alpha
    handed from one launch to the next through global memory, gave wrong rows in the occluded
    planes in every call while the three other cases passed."""
    rng = np.random.RandomState(0)
    out = {}
    for S, Gt, K in ((1024, 3, 2), (1024, 1, 1), (1024, 8, 8), (1024, 2, 3), (768, 4, 4)):
        img_t, img_s = (rng.standard_normal((3, S, S)).astype(np.float32) for _ in range(2))
        out[S, Gt, K] = (img_t, _blobs(rng, Gt, S), img_s, _blobs(rng, K, S), list(range(K)))
    return out


def test_kernel_at_the_training_canvas(dev):
    """Freshly uploaded inputs, three calls each: every call gives the definition's result."""
    cases = _canvas_cases()
    for key in ((1024, 8, 8), (768, 4, 4)):
        args = cases[key]
        want = R.compose(*args)
        for rep in range(3):
            rc, img, masks, boxes, areas, intact = _launch(dev, *args)
            assert rc == 0 and intact, key
            assert int((masks != want[1]).sum()) == 0, (key, rep, int((masks != want[1]).sum()))
            assert np.array_equal(_bits(img), _bits(want[0])), key
            assert np.array_equal(boxes, want[2]) and np.array_equal(areas, want[3]), key


def test_kernel_edges(dev):
    S = 37
    rng = np.random.RandomState(1)
    img_t, masks_t, img_s, masks_s, idx = _example(rng, 3, 4, 2, S)
    # alpha all zero: the target comes back, with the boxes and areas of its untouched masks
    empty = np.zeros_like(masks_s)
    img, masks, boxes, areas = _check(dev, (img_t, masks_t, img_s, empty, idx))
    assert np.array_equal(_bits(img), _bits(img_t)) and np.array_equal(masks[:3], masks_t)
    want_boxes, want_areas = boxes_areas(masks_t)
    assert np.array_equal(boxes[:3], want_boxes) and np.array_equal(areas[:3], want_areas)
    assert (areas[3:] == 0).all() and (boxes[3:] == 0).all()
    # alpha all one: every target is gone, the image is the source's
    full = np.zeros_like(masks_s)
    full[idx[1]] = 1
    img, masks, boxes, areas = _check(dev, (img_t, masks_t, img_s, full, idx))
    assert np.array_equal(_bits(img), _bits(img_s))
    assert (areas[:3] == 0).all() and (boxes[:3] == 0).all() and not masks[:3].any()
    assert areas[4] == S * S and tuple(boxes[4]) == (0, 0, S, S)
    # a target exactly covered by a pasted instance goes; its neighbour, one column wider, stays
    t = np.zeros((2, S, S), np.uint8)
    s = np.zeros((1, S, S), np.uint8)
    t[0, 5:20, 7:30] = 1
    t[1, 5:20, 7:31] = 1
    s[0, 5:20, 7:30] = 1
    img, masks, boxes, areas = _check(dev, (img_t, t, img_s, s, [0]))
    assert areas[0] == 0 and tuple(boxes[0]) == (0, 0, 0, 0)
    assert areas[1] == 15 and tuple(boxes[1]) == (5, 30, 20, 31)
    assert areas[2] == 15 * 23 and tuple(boxes[2]) == (5, 7, 20, 30)
    # one pixel in each corner, as targets and as pasted instances
    for S_ in (37, 64, 65):
        c = np.zeros((4, S_, S_), np.uint8)
        corners = [(0, 0), (0, S_ - 1), (S_ - 1, 0), (S_ - 1, S_ - 1)]
        for g, (y, x) in enumerate(corners):
            c[g, y, x] = 1
        a, b = (rng.standard_normal((3, S_, S_)).astype(np.float32) for _ in range(2))
        img, masks, boxes, areas = _check(dev, (a, c, b, c[::-1].copy(), [1, 2]), S_)
        assert areas.tolist() == [1, 0, 0, 1, 1, 1]
        assert [tuple(v) for v in boxes[[0, 3]]] == [(0, 0, 1, 1), (S_ - 1, S_ - 1, S_, S_)]
        assert tuple(boxes[4]) == (S_ - 1, 0, S_, 1) and tuple(boxes[5]) == (0, S_ - 1, 1, S_)
        changed = (_bits(img) != _bits(a)).any(0)
        assert changed.sum() == 2 and changed[S_ - 1, 0] and changed[0, S_ - 1]
    # a byte other than 0 is set, and is written as 1
    loud_t, loud_s = masks_t * np.uint8(255), masks_s * np.uint8(2)
    loud_s[idx[0]][masks_s[idx[0]] != 0] = 255
    img, masks, boxes, areas = _check(dev, (img_t, loud_t, img_s, loud_s, idx))
    quiet = _check(dev, (img_t, masks_t, img_s, masks_s, idx))
    assert masks.max() == 1 and all(np.array_equal(p, q) for p, q in zip((img, masks, boxes, areas), quiet))


def test_image_is_selected_not_blended(dev):
    S = 65
    rng = np.random.RandomState(2)
    img_t, masks_t, img_s, masks_s, idx = _example(rng, 2, 3, 2, S)
    alpha = masks_s[idx].any(0)
    # payload NaNs, both infinities and -0.0 wherever an image is NOT taken from
    poison = np.array([0x7fc00000, 0x7fc12345, 0xffc00001, 0x7f800000, 0xff800000, 0x80000000],
                      np.uint32).view(np.float32)
    fill = poison[rng.randint(0, len(poison), (3, S, S))]
    img_t = np.where(alpha[None], fill, img_t)
    img_s = np.where(alpha[None], img_s, fill)
    img, _, _, _ = _check(dev, (img_t, masks_t, img_s, masks_s, idx))
    assert np.isfinite(img).all() and not (_bits(img) == np.int32(-2 ** 31)).any()
    # and where they ARE taken from, the patterns survive bit for bit
    img, _, _, _ = _check(dev, (img_s, masks_t, img_t, masks_s, idx))
    assert np.array_equal(_bits(img), _bits(fill))


def test_calls_are_deterministic_on_any_stream(dev):
    rng = np.random.RandomState(3)
    args = _example(rng, 5, 6, 4, 130)
    first = _launch(dev, *args)
    again = _launch(dev, *args)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        other = _launch(dev, *args)
    assert side.cuda_stream != torch.cuda.current_stream().cuda_stream
    for run in (again, other):
        assert run[0] == 0 and run[5]
        assert np.array_equal(_bits(run[1]), _bits(first[1]))
        assert all(np.array_equal(p, q) for p, q in zip(run[2:5], first[2:5]))
    dv = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in args[:4]]
    a = F.copy_paste(*dv, args[4])
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        b = F.copy_paste(*dv, args[4])
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    assert np.array_equal(_bits(a[0].cpu().numpy()), _bits(first[1]))   # a CHW image is made NHWC once


def test_empty_sides_and_arguments(dev):
    rng = np.random.RandomState(4)
    S = 20
    # null pointers where the count is 0: no target, nothing pasted, neither (the image is written)
    for Gt, Gs, K in ((0, 2, 1), (2, 2, 0), (0, 3, 0), (0, 0, 0)):
        args = _example(rng, Gt, Gs, K, S)
        img, masks, _, _ = _check(dev, args, (Gt, Gs, K), null_unused=True)
        if K == 0:
            assert np.array_equal(_bits(img), _bits(args[0])) and np.array_equal(masks, args[1])
    img_t, masks_t, img_s, masks_s, idx = _example(rng, 2, 3, 2, S)
    # the index is clamped on the device: no read leaves the source whatever it holds
    rc, _, masks, _, _, intact = _launch(dev, img_t, masks_t, img_s, masks_s, [-9, 1 << 30])
    assert rc == 0 and intact and np.array_equal(masks[2:], masks_s[[0, 2]])
    dv = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (img_t, masks_t, img_s, masks_s)]
    for bad in ([1, 1], [2, 0], [-1, 1], [0, 3], [3]):
        with pytest.raises(ValueError, match='strictly increasing'):
            F.copy_paste(*dv, bad)
    with pytest.raises(ValueError, match='uint8'):
        F.copy_paste(dv[0], dv[1].int(), dv[2], dv[3], [0])
    with pytest.raises(ValueError, match='float32'):
        F.copy_paste(dv[0].double(), dv[1], dv[2], dv[3], [0])
    with pytest.raises(ValueError, match='float32'):
        F.copy_paste(dv[0][:, :-1], dv[1], dv[2], dv[3], [0])
    with pytest.raises(ValueError, match='one canvas'):
        F.copy_paste(dv[0], dv[1], dv[2], dv[3][:, :-1, :-1], [0])
    with pytest.raises(_lib.MrcnnHipError):
        F.copy_paste(dv[0], dv[1], dv[2].cpu(), dv[3], [0])
    # nothing pasted through the wrapper; one buffer holds boxes, then areas
    out, m, meta = F.copy_paste_meta(*dv, [])
    assert torch.equal(out, dv[0]) and torch.equal(m, dv[1]) and tuple(meta.shape) == (10,)
    want_boxes, want_areas = boxes_areas(masks_t)
    assert np.array_equal(meta.cpu().numpy(), np.concatenate([want_boxes.ravel(), want_areas]))


# ---- dataset -------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def small(dev, tmp_path_factory):
    """The small model of tests/test_gpu_train_loop.py over its 5-image COCO directory."""
    root = os.path.join(str(tmp_path_factory.mktemp('copy_paste')), 'COCO')
    TLT._write_coco(root)
    packed = cmr.datasets.COCOInstanceSegmentationDataset('minival', root_dir=root, packed_masks=True)
    loop, model, chain, opt, train = TLT._build(dev, packed, prefetch=False)
    loop.close()
    return dict(packed=packed, model=model, chain=chain)


def _host(ex):
    return (ex[0].cpu().numpy(), ex[1], ex[2], ex[3].cpu().numpy(), ex[4])


def _jittered(small, S):
    t = D.MaskRCNNTransform(small['model'], device_masks=True, scale_jitter=(0.5, 2.0), crop_size=S)
    return TL.TransformDataset(small['packed'], t)


# seeds found on the host with tests/copy_paste_ref.py over tests/scale_jitter_ref.py: with seed 21
# the paste covers target instance 1 of example 2 entirely; with seed 12 the partner is the example
# itself, redrawn, and two targets go
@pytest.mark.parametrize('seed,i,gone', [(21, 2, [1]), (12, 2, [1, 2]), (0, 4, None), (1, 0, None),
                                         (2, 3, None)])
def test_dataset_equals_the_reference_composition(dev, small, seed, i, gone):
    S = 64
    wrapped = _jittered(small, S)
    data = D.CopyPasteDataset(wrapped, prob=1.)
    assert len(data) == len(wrapped) == 5
    random.seed(seed)
    got = data[i]
    after = random.random()
    random.seed(seed)
    ex = _host(wrapped[i])
    assert random.random() < 1.
    src = _host(wrapped[random.randrange(5)])
    want, idx, dropped = R.paste(ex, src)
    assert random.random() == after and idx
    if gone is not None:
        assert np.flatnonzero(dropped[:len(ex[3])]).tolist() == gone and want is not ex
    x, bbox, label, mask, scale = got
    assert x.is_cuda and x.dtype == torch.float32 and x.stride() == (1, 3 * S, 3)
    assert np.array_equal(_bits(x.cpu().numpy()), _bits(want[0]))
    assert bbox.dtype == np.float32 and np.array_equal(bbox, want[1])
    assert label.dtype == ex[2].dtype and np.array_equal(label, want[2]) and scale == ex[4]
    assert mask.is_cuda and mask.dtype == torch.uint8 and mask.is_contiguous()
    assert np.array_equal(mask.cpu().numpy(), want[3])
    boxes, areas = boxes_areas(want[3])
    assert (areas >= 1).all() and np.array_equal(bbox, boxes.astype(np.float32))
    assert len(bbox) == len(label) == len(mask) == len(ex[3]) + len(idx) - dropped.sum()


def test_dataset_leaves_alone_what_it_cannot_paste(dev, small):
    S = 64
    wrapped = _jittered(small, S)
    random.seed(5)
    items = [wrapped[i] for i in range(2)]
    bare = (items[1][0], np.zeros((0, 4), np.float32), np.zeros((0,), np.int32), items[1][3][:0],
            items[1][4])

    class Two(object):                                   # item 0 has instances, item 1 has none
        def __len__(self):
            return 2

        def __getitem__(self, i):
            return (items[0], bare)[i]

    def partner(s):
        r = random.Random(s)
        r.random()
        return r.randrange(2)

    seed = next(s for s in range(100) if partner(s) == 1)
    random.seed(seed)
    random.random()
    j = random.randrange(2)
    after = random.random()
    random.seed(seed)
    got = D.CopyPasteDataset(Two(), prob=1.)[0]
    assert j == 1 and got is items[0] and random.random() == after      # coin, partner, nothing more
    # with the coin failing the wrapper hands on the transform's own example and adds one draw
    t = D.MaskRCNNTransform(small['model'], device_masks=True, scale_jitter=(0.5, 2.0), crop_size=S)
    random.seed(9)
    a = t(small['packed'][2])
    after = random.random()
    random.seed(9)
    b = wrapped[2]
    assert random.random() == after
    random.seed(9)
    c = D.CopyPasteDataset(wrapped, prob=0.)[2]
    after_coin = random.random()
    random.seed(9)
    t(small['packed'][2]), random.random()
    assert random.random() == after_coin
    for other in (b, c):
        assert torch.equal(a[0], other[0]) and torch.equal(a[3], other[3]) and a[4] == other[4]
        assert np.array_equal(a[1], other[1]) and np.array_equal(a[2], other[2])

    class Pair(object):                                  # the example, then its partner
        def __init__(self, *items):
            self.items = list(items)

        def __len__(self):
            return 1

        def __getitem__(self, i):
            return self.items.pop(0)

    # a 2-D mask, a host example or another canvas is refused
    flat = (items[0][0], items[0][1][:1], items[0][2][:1], items[0][3][0], items[0][4])
    host = _host(items[0])
    smaller = _jittered(small, 48)[0]
    for pair, msg in (((flat, items[0]), 'device_masks=True, scale_jitter'),
                      ((items[0], flat), 'device_masks=True, scale_jitter'),
                      ((host, items[0]), 'device_masks=True, scale_jitter'),
                      ((items[0], smaller), 'canvas size'), ((smaller, items[0]), 'canvas size')):
        with pytest.raises(ValueError, match=msg):
            D.CopyPasteDataset(Pair(*pair), prob=1.)[0]


# ---- train step ----------------------------------------------------------------------------------
def test_chain_step_on_pasted_examples(dev, small, monkeypatch):
    chain, S = small['chain'], 96
    data = D.CopyPasteDataset(_jittered(small, S), prob=1.)
    runs = []
    for _ in range(2):
        random.seed(7)
        examples = [data[j] for j in (2, 4)]
        batch = TL.make_converter(dev)(examples)
        imgs, bboxes, labels, masks, scales = batch
        assert tuple(imgs.shape) == (2, 3, S, S) and imgs.is_cuda
        assert imgs.is_contiguous(memory_format=torch.channels_last)
        assert isinstance(masks, torch.Tensor) and masks.is_cuda and masks.dtype == torch.uint8
        assert masks.is_contiguous() and masks.dim() == 4 and tuple(masks.shape[2:]) == (S, S)
        with monkeypatch.context() as mp:
            mp.setattr(torch.Tensor, 'cpu', GM._no_mask_download(masks, torch.Tensor.cpu))
            np.random.seed(11)
            loss = chain(*batch)
            torch.cuda.synchronize()
        report = {k: float(v) for k, v in chain.report.items()}
        assert np.isfinite(float(loss.detach())) and all(np.isfinite(v) for v in report.values())
        runs.append((float(loss.detach()), report, imgs.cpu().numpy(), masks.cpu().numpy(),
                     [np.asarray(b) for b in bboxes], random.random()))
    a, b = runs
    assert a[0] == b[0] and a[1] == b[1] and a[5] == b[5]
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    assert all(np.array_equal(p, q) for p, q in zip(a[4], b[4]))


# ---- tool ----------------------------------------------------------------------------------------
def test_train_loop_tool_with_copy_paste(dev):
    env = dict(os.environ, WARMUP='1')
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'train_loop.py'), '--synthetic', '4',
                          '--iterations', '2', '--device-masks', '--scale-jitter', '0.5,1.5',
                          '--crop-size', '64', '--copy-paste', '1.0'],
                         capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert '2 iterations' in out.stdout and 'loss' in out.stdout
    assert 'nan' not in out.stdout.lower()
