"""Ignore regions on the device: the two kernels against the NumPy statement
of tests/ignore_regions_ref.py, bit for bit, and the feature through the transform, large-scale
jitter, copy-paste and one train step of the small test model."""
import numpy as np
import pytest
import torch

import ignore_regions_ref as R
from chainer_mask_rcnn_amd import _lib
from chainer_mask_rcnn_amd import functions as F

pytestmark = pytest.mark.gpu

GUARD = 64              # elements of guard band on either side of every output
SENTINEL = -0x5A5A5A5A5A5A5A5B


def _guarded(shape, dtype, dev):
    """An output of ``shape`` inside a larger buffer prefilled with a sentinel -> (buffer, view)."""
    n = int(np.prod(shape))
    sent = SENTINEL if dtype == torch.int64 else -0x5A5A5A5B
    buf = torch.full((n + 2 * GUARD,), sent, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n].view(shape), sent


def _guards_intact(buf, sent):
    b = buf.cpu().numpy()
    return (b[:GUARD] == sent).all() and (b[-GUARD:] == sent).all()


def _raw_union(masks, base, dev):
    """mrcnn_mask_union_pack into a guarded, sentinel-filled plane -> (H, Wq) uint64 host array."""
    G, H, W = masks.shape
    Wq = (W + 63) // 64
    m_d = torch.from_numpy(masks).to(dev) if G else None
    b_d = None if base is None else torch.from_numpy(base.view(np.int64)).to(dev)
    buf, plane, sent = _guarded((H, Wq), torch.int64, dev)
    _lib.call('mrcnn_mask_union_pack', _lib.ptr(m_d), G, H, W, _lib.ptr(b_d), _lib.ptr(plane),
              _lib.stream_ptr())
    torch.cuda.synchronize()
    assert _guards_intact(buf, sent)
    return plane.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize('G, H, W', [(1, 1, 1), (3, 2, 63), (2, 3, 64), (3, 3, 65), (4, 5, 130), (0, 3, 70)])
def test_union_pack_is_packbits_of_the_dense_union(dev, G, H, W):
    rng = np.random.RandomState(G * 1000 + W)
    masks = rng.choice(np.array([0, 0, 0, 1, 255], np.uint8), size=(G, H, W))
    want = R.pack_plane(R.union_dense(masks))
    got = _raw_union(masks, None, dev)
    assert got.dtype == want.dtype and np.array_equal(got, want)
    # pad bits zero: nothing beyond column W
    pad = np.unpackbits(got.view(np.uint8), axis=1, bitorder='little')[:, W:]
    assert not pad.any()
    # base & ~U with a random base (its pad bits zero, as the format has them)
    base_dense = rng.randint(0, 2, (H, W)).astype(bool)
    base = R.pack_plane(base_dense)
    got = _raw_union(masks, base, dev)
    assert np.array_equal(got, R.pack_plane(R.union_dense(masks, base_dense)))
    assert np.array_equal(got, base & ~want)
    # the Python wrapper: the same words as int64
    if G:
        m_d = torch.from_numpy(masks).to(dev)
        assert np.array_equal(F.union_plane(m_d).cpu().numpy().view(np.uint64), want)
        b_d = torch.from_numpy(base.view(np.int64)).to(dev)
        assert np.array_equal(F.union_plane(m_d, b_d).cpu().numpy().view(np.uint64), base & ~want)


def test_union_pack_clears_pad_bits_of_a_base_that_has_some(dev):
    masks = np.zeros((1, 2, 70), np.uint8)
    base = np.full((2, 2), ~np.uint64(0), np.uint64)
    got = _raw_union(masks, base, dev)
    assert np.array_equal(R.unpack_plane(got, 128), np.arange(128)[None, :].repeat(2, 0) < 70)


def test_union_pack_refuses_aliasing_and_bad_shapes(dev):
    lib = _lib.load()
    p = torch.zeros((2, 2), dtype=torch.int64, device=dev)
    m = torch.zeros((1, 2, 70), dtype=torch.uint8, device=dev)
    assert lib.mrcnn_mask_union_pack(_lib.ptr(m), 1, 2, 70, _lib.ptr(p), _lib.ptr(p), None) != 0
    assert b'alias' in lib.mrcnn_last_error()
    assert lib.mrcnn_mask_union_pack(_lib.ptr(m), 1, 0, 70, None, _lib.ptr(p), None) != 0
    assert lib.mrcnn_mask_union_pack(None, 1, 2, 70, None, _lib.ptr(p), None) != 0
    assert lib.mrcnn_box_coverage(_lib.ptr(p), 2, 70, None, 3, None, None) != 0
    assert lib.mrcnn_box_coverage(None, 2, 70, None, 0, None, None) == 0      # n == 0: no launch


# ---- box coverage ----------------------------------------------------------------------------
PH, PW = 37, 130        # three words per row, the last partial


def _edge_boxes(H, W):
    """The boxes of the issue's list, for an H x W plane."""
    cols = [0, 1, 63, 64, 65, 127, 128, 129, 130]
    b = []
    for i, c0 in enumerate(cols):                       # every pair of column edges
        for c1 in cols[i:]:
            b.append([3, c0, 20, c1])
    b += [[0.5, 0.5, 10, 10], [1.5, 1.5, 10, 10], [2.5, 2.5, 10.5, 11.5], [0.5, 63.5, 1.5, 64.5],
          [2.5, 64.5, 3.5, 65.5], [0.49999997, 0.50000006, 2.4999998, 2.5000002]]      # half to even
    b += [[-20, 10, -5, 50], [H + 3, 10, H + 30, 50], [5, -40, 20, -1], [5, W + 1, 20, W + 90],   # wholly outside
          [-7.3, 10, 12, 50], [20, 10, H + 9, 50], [5, -8, 20, 40.2], [5, 100, 20, W + 33]]      # partly outside
    b += [[-1e9, -2e9, 1e9, 3e9], [-3e10, 5, 1e30, 70], [2e9, 2e9, 4e9, 4e9], [-1e38, -1e38, 3e38, 3e38],
          [5, 5, 2147483648.0, 2147483648.0], [-2147483648.0, -2147483904.0, 5, 5]]
    b += [[20, 50, 5, 10], [5, 50, 20, 10], [20, 10, 5, 50],                           # inverted
          [5, 10, 5, 50], [5, 10, 20, 10], [7, 7, 7, 7], [7.2, 7.1, 7.4, 7.3]]         # zero area
    b += [[0, 0, H, W], [-0.4, -0.4, H + 0.4, W + 0.4]]                                # the whole image
    for bad in (np.nan, np.inf, -np.inf):
        for pos in range(4):
            box = [2, 3, 30, 100]
            box[pos] = bad
            b.append(box)
    b.append([np.nan] * 4)
    return np.array(b, np.float32)


def _raw_coverage(plane_words, H, W, boxes, dev):
    n = len(boxes)
    p_d = torch.from_numpy(plane_words.view(np.int64)).to(dev)
    b_d = torch.from_numpy(np.ascontiguousarray(boxes, np.float32)).to(dev)
    buf, out, sent = _guarded((n, 2), torch.int32, dev)
    _lib.call('mrcnn_box_coverage', _lib.ptr(p_d), H, W, _lib.ptr(b_d) if n else None, n,
              _lib.ptr(out) if n else None, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert _guards_intact(buf, sent)
    return out.cpu().numpy()


def _planes(H, W):
    rng = np.random.RandomState(7)
    return {'random': rng.randint(0, 2, (H, W)).astype(bool), 'ones': np.ones((H, W), bool),
            'zeros': np.zeros((H, W), bool)}


@pytest.mark.parametrize('kind', ['random', 'ones', 'zeros'])
def test_box_coverage_matches_the_slice_sum(dev, kind):
    dense = _planes(PH, PW)[kind]
    words = R.pack_plane(dense)
    rng = np.random.RandomState(11)
    y = rng.uniform(-10, PH + 10, (1000, 2))
    x = rng.uniform(-20, PW + 20, (1000, 2))
    rand = np.stack([y[:, 0], x[:, 0], y[:, 1], x[:, 1]], 1).astype(np.float32)   # a quarter inverted per axis
    rand[::7] = np.round(rand[::7]) + 0.5                                          # exact halves
    for boxes in (_edge_boxes(PH, PW), rand, rand[:1]):
        want = R.box_coverage(dense, boxes)
        got = _raw_coverage(words, PH, PW, boxes, dev)
        assert got.dtype == np.int32 and np.array_equal(got, want), \
            (boxes[np.where((got != want).any(1))[0][:5]], got[(got != want).any(1)][:5], want[(got != want).any(1)][:5])
        if kind == 'ones':
            assert np.array_equal(got[:, 0], got[:, 1])
        if kind == 'zeros':
            assert not got[:, 0].any()
    assert (R.box_coverage(dense, _edge_boxes(PH, PW))[:, 1] > 0).sum() > 40      # the list is not all empty
    # the wrapper, and n == 0
    p_d = torch.from_numpy(words.view(np.int64)).to(dev)
    got = F.box_coverage(p_d, PW, torch.from_numpy(rand).to(dev))
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), R.box_coverage(dense, rand))
    empty = F.box_coverage(p_d, PW, torch.zeros((0, 4), device=dev))
    assert tuple(empty.shape) == (0, 2)
    assert _raw_coverage(words, PH, PW, np.zeros((0, 4), np.float32), dev).shape == (0, 2)


@pytest.mark.parametrize('bit', [0, 1])
def test_box_coverage_on_a_one_pixel_plane(dev, bit):
    dense = np.full((1, 1), bool(bit))
    boxes = np.concatenate([_edge_boxes(1, 1), [[0, 0, 1, 1], [0.5, 0.5, 1.5, 1.5], [0.4, 0.4, 0.6, 0.6],
                                                [-5, -5, 5, 5]]]).astype(np.float32)
    got = _raw_coverage(R.pack_plane(dense), 1, 1, boxes, dev)
    assert np.array_equal(got, R.box_coverage(dense, boxes))
    assert got[:, 1].max() == 1 and got[:, 0].max() == bit


# ---- pipeline --------------------------------------------------------------------------------
import random                                                     # noqa: E402

import chainer_mask_rcnn_amd as cmr                               # noqa: E402
from chainer_mask_rcnn_amd import datasets as D                   # noqa: E402
from chainer_mask_rcnn_amd.datasets import transforms as T        # noqa: E402
import scale_jitter_ref as SJR                                    # noqa: E402


@pytest.fixture(scope='module')
def small(dev):
    torch.manual_seed(4)
    model = cmr.models.MaskRCNNResNet(
        50, n_fg_class=80, anchor_scales=(2, 4, 8, 16, 32), roi_size=14, min_size=160, max_size=240,
        proposal_creator_params=dict(min_size=0, n_train_pre_nms=600, n_train_post_nms=100))
    chain = cmr.models.MaskRCNNTrainChain(
        model, proposal_target_creator=cmr.models.utils.ProposalTargetCreator(n_sample=32)).to(dev)
    chain.train()
    with torch.no_grad():                   # keep the activations of the random network O(1)
        model.extractor.bn1.W.fill_(1. / 64.)
        for m in model.modules():
            if isinstance(m, cmr.models.resnet_extractor.Bottleneck):
                m.bn3.W.fill_(0.25)
    return model, chain


def _example(H=97, W=131):
    """3 regular and 2 crowd instances, interleaved; the crowds overlap the others."""
    rng = np.random.RandomState(0)
    img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    boxes = np.array([[5, 8, 40, 60], [0, 0, 50, 131], [30, 70, 90, 125], [60, 3, 96, 50], [45, 40, 97, 100]])
    crowd = np.array([0, 1, 0, 0, 1], np.int32)
    mask = np.zeros((5, H, W), np.int32)
    for g, (y0, x0, y1, x1) in enumerate(boxes):
        mask[g, y0:y1, x0:x1] = rng.rand(y1 - y0, x1 - x0) < 0.8
        mask[g, y0, x0] = mask[g, y1 - 1, x1 - 1] = 1
    label = np.array([3, 9, 17, 0, 42], np.int32)
    return img, boxes.astype(np.float32), label, mask, crowd


def _plane_of(ignore):
    assert ignore.is_cuda and ignore.dtype == torch.int64 and ignore.is_contiguous()
    return ignore.cpu().numpy().view(np.uint64)


def test_transform_splits_the_crowds_off(dev, small):
    model, _ = small
    img, bbox, label, mask, crowd = _example()
    reg = crowd == 0
    area = np.arange(5, dtype=np.float32)
    today = D.MaskRCNNTransform(model, device_masks=True)
    t = D.MaskRCNNTransform(model, device_masks=True, crowd_ignore=True)
    flips = set()
    for seed in range(6):
        random.seed(seed)
        want = today((img, bbox[reg], label[reg], mask[reg]))
        after = random.random()
        random.seed(seed)
        x_flip = random.choice([True, False])
        flips.add(x_flip)
        out_size = tuple(want[0].shape[1:])
        plane = R.pack_plane(T.resize_nearest(mask[crowd != 0], out_size, x_flip=x_flip).any(0))
        for example in ((img, bbox, label, mask, crowd), (img, bbox, label, mask, crowd, area),
                        (img, bbox, label, D.PackedMasks.from_dense(mask), crowd)):
            random.seed(seed)
            got = t(example)
            assert random.random() == after and len(got) == 6
            assert torch.equal(got[0], want[0]) and got[0].stride() == want[0].stride()
            assert np.array_equal(got[1], want[1]) and got[1].dtype == want[1].dtype
            assert np.array_equal(got[2], want[2]) and got[4] == want[4]
            assert got[3].dtype == torch.uint8 and torch.equal(got[3], want[3])
            assert np.array_equal(_plane_of(got[5]), plane)
    assert flips == {False, True} and out_size[0] == 160
    # no crowd instance, and a crowd instance without a pixel: None, the rest as today
    random.seed(1)
    want = today((img, bbox[reg], label[reg], mask[reg]))
    for example in ((img, bbox[reg], label[reg], mask[reg], crowd[reg]),
                    (img, np.concatenate([bbox[reg], bbox[:1]]), np.concatenate([label[reg], label[:1]]),
                     np.concatenate([mask[reg], mask[:1] * 0]), np.array([0, 0, 0, 1]))):
        random.seed(1)
        got = t(example)
        assert got[5] is None and torch.equal(got[3], want[3]) and np.array_equal(got[1], want[1][:3])
    # crowds only: an example without instances, plus its plane
    random.seed(1)
    want = today((img, bbox[:0], label[:0], mask[:0]))
    random.seed(1)
    got = t((img, bbox[~reg], label[~reg], mask[~reg], crowd[~reg]))
    assert got[1].shape == (0, 4) and got[2].shape == (0,) and tuple(got[3].shape) == tuple(want[3].shape)
    assert torch.equal(got[0], want[0]) and got[3].shape[0] == 0
    assert np.array_equal(_plane_of(got[5]), R.pack_plane(
        T.resize_nearest(mask[~reg], tuple(want[0].shape[1:]), x_flip=random.Random(1).choice([True, False])).any(0)))


def _replay(seed, in_size, S, jitter, regular_masks):
    """The flip and the accepted geometry of ``seed`` (None: the fallback), from the regular
    instances alone, as tests/scale_jitter_ref.py accepts one."""
    random.seed(seed)
    x_flip = random.choice([True, False])
    for k in range(SJR.ATTEMPTS if len(regular_masks) else 0):
        scale, resized, offset = T.draw_scale_jitter(in_size, S, jitter)
        if SJR.crop_masks(regular_masks, resized, offset, S, x_flip).any():
            return x_flip, (resized, offset), k + 1
    scale = min(float(S) / in_size[0], float(S) / in_size[1])
    return x_flip, (T._resized_size(in_size, scale), (0, 0)), None


def test_transform_with_scale_jitter_crops_the_plane(dev, small):
    model, _ = small
    img, bbox, label, mask, crowd = _example()
    reg = crowd == 0
    S, jitter = 64, (0.5, 2.0)
    today = D.MaskRCNNTransform(model, device_masks=True, scale_jitter=jitter, crop_size=S)
    t = D.MaskRCNNTransform(model, device_masks=True, scale_jitter=jitter, crop_size=S, crowd_ignore=True)
    planes = 0
    for seed in range(10):
        random.seed(seed)
        want = today((img, bbox[reg], label[reg], mask[reg]))
        after = random.random()
        x_flip, (resized, offset), k = _replay(seed, (97, 131), S, jitter, mask[reg])
        assert k is not None and random.random() == after
        random.seed(seed)
        got = t((img, bbox, label, mask, crowd))
        assert random.random() == after
        assert torch.equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert np.array_equal(got[2], want[2]) and torch.equal(got[3], want[3]) and got[4] == want[4]
        union = SJR.crop_masks(mask[~reg], resized, offset, S, x_flip).any(0)
        if union.any():
            planes += 1
            assert np.array_equal(_plane_of(got[5]), R.pack_plane(union))
        else:
            assert got[5] is None
    assert planes >= 5


def test_scale_jitter_never_accepts_a_geometry_for_its_crowd_pixels(dev, small):
    model, _ = small
    S, jitter = 16, (2.0, 2.0)
    rng = np.random.RandomState(1)
    mask = np.zeros((2, 40, 40), np.int32)
    mask[0, :3, :3] = 1                                 # the regular blob: lost by most windows
    mask[1] = 1                                         # the crowd: in every window
    ex = (rng.randint(0, 256, (40, 40, 3)).astype(np.uint8), np.array([[0, 0, 3, 3], [0, 0, 40, 40]], np.float32),
          np.array([5, 7], np.int32), mask, np.array([0, 1], np.int32))
    found = {}
    for seed in range(512):
        _, _, k = _replay(seed, (40, 40), S, jitter, mask[:1])
        found.setdefault('fallback' if k is None else ('redraw' if k > 1 else 'first'), seed)
    assert 'redraw' in found and 'fallback' in found
    today = D.MaskRCNNTransform(model, device_masks=True, scale_jitter=jitter, crop_size=S)
    t = D.MaskRCNNTransform(model, device_masks=True, scale_jitter=jitter, crop_size=S, crowd_ignore=True)
    for kind in ('redraw', 'fallback'):
        seed = found[kind]
        random.seed(seed)
        want = today(tuple(e[:1] if i else e for i, e in enumerate(ex[:4])))
        after = random.random()
        x_flip, (resized, offset), k = _replay(seed, (40, 40), S, jitter, mask[:1])
        random.seed(seed)
        got = t(ex)
        assert random.random() == after                 # the draws of the regular instance alone
        assert torch.equal(got[0], want[0]) and torch.equal(got[3], want[3]) and len(got[3]) == 1
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and got[4] == want[4]
        union = SJR.crop_masks(mask[1:], resized, offset, S, x_flip).any(0)
        assert union.all() and np.array_equal(_plane_of(got[5]), R.pack_plane(union))


class _Listed(object):
    def __init__(self, examples):
        self.examples = examples

    def __len__(self):
        return len(self.examples)

    def __getitem__(self, i):
        return self.examples[i]


def test_copy_paste_cuts_the_pasted_pixels_out_of_the_plane(dev):
    S = 70

    def example(G, seed, with_plane):
        r = np.random.RandomState(seed)
        m = np.zeros((G, S, S), np.uint8)
        for g in range(G):
            y, x = r.randint(0, S - 20, 2)
            m[g, y:y + r.randint(5, 20), x:x + r.randint(5, 20)] = 1
        img = torch.from_numpy(r.standard_normal((S, S, 3)).astype(np.float32)).to(dev).permute(2, 0, 1)
        dense = r.rand(S, S) < 0.5
        plane = F.union_plane(torch.from_numpy(dense[None].astype(np.uint8)).to(dev)) if with_plane else None
        ex = (img, SJR.boxes_areas(m)[0].astype(np.float32), r.randint(0, 80, G).astype(np.int32),
              torch.from_numpy(m).to(dev), 1.0, plane)
        return ex, dense
    (e0, dense0), (e1, _), (e2, _) = example(3, 0, True), example(4, 1, True), example(2, 2, False)
    six, five = _Listed([e0, e1, e2]), _Listed([e[:5] for e in (e0, e1, e2)])
    for seed in range(4):
        random.seed(seed)
        want = D.CopyPasteDataset(five, prob=1.0)[0]
        after = random.random()
        random.seed(seed)
        random.random()
        j = random.randrange(3)
        idx = D.copy_paste.draw_paste_selection(len(six[j][3]))
        random.seed(seed)
        got = D.CopyPasteDataset(six, prob=1.0)[0]
        assert random.random() == after and len(got) == 6 and len(want) == 5
        assert torch.equal(got[0], want[0]) and torch.equal(got[3], want[3])
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and got[4] == want[4]
        pasted = six[j][3].cpu().numpy()[idx].any(0)
        assert pasted.any() and (dense0 & pasted).any()
        assert np.array_equal(R.unpack_plane(_plane_of(got[5]), S), dense0 & ~pasted)
        assert got[5] is not e0[5] and np.array_equal(R.unpack_plane(_plane_of(e0[5]), S), dense0)
    # a target without a plane stays without one
    random.seed(0)
    assert D.CopyPasteDataset(six, prob=1.0)[2][5] is None
    # not pasted: the example as it is
    assert D.CopyPasteDataset(six, prob=0.0)[0] is e0


# ---- train step ------------------------------------------------------------------------------
SH, SW = 160, 240


def _batch(dev):
    rng = np.random.RandomState(0)
    imgs = torch.from_numpy(rng.uniform(-120, 130, (2, 3, SH, SW)).astype(np.float32)).to(dev)
    imgs = imgs.contiguous(memory_format=torch.channels_last)
    bboxes = [np.array([[20, 30, 120, 160], [60, 100, 150, 210]], np.float32),
              np.array([[10, 10, 90, 80], [70, 120, 150, 230]], np.float32)]
    labels = [np.array([3, 17], np.int32), np.array([42, 5], np.int32)]
    masks = []
    for b in bboxes:
        m = np.zeros((len(b), SH, SW), np.int32)
        for g, (y0, x0, y1, x1) in enumerate(b.astype(int)):
            m[g, y0 + 5:y1 - 5, x0 + 5:x1 - 5] = 1
        masks.append(m)
    dense = np.zeros((SH, SW), bool)
    dense[:, SW // 2:] = True                                   # a crowd over the right half
    plane = F.union_plane(torch.from_numpy(dense[None].astype(np.uint8)).to(dev))
    return imgs, bboxes, labels, masks, dense, plane


class _Reseed(object):
    """Every call of a target creator's drawing half starts from a seed of its own (1000 + the
    call's number within the step), so that one image's draws do not depend on how much of the
    stream another image's pools consumed."""

    def __init__(self, chain, monkeypatch):
        self.k = 0
        ptc, atc = chain.proposal_target_creator, chain.anchor_target_creator
        for obj, names in ((ptc, ('sample', 'sample_device')), (atc, ('finish', 'finish_device'))):
            for name in names:
                monkeypatch.setattr(obj, name, self._wrap(getattr(obj, name)), raising=True)

    def _wrap(self, fn):
        def call(*a, **kw):
            np.random.seed(1000 + self.k)
            self.k += 1
            return fn(*a, **kw)
        return call


def _step(chain, batch, ignores, device_targets, seen):
    imgs, bboxes, labels, masks = batch[:4]
    chain.device_targets = device_targets
    del seen[:]
    loss = chain(imgs, bboxes, labels, masks, [1., 1.], **({} if ignores is None else dict(ignores=ignores)))
    torch.cuda.synchronize()
    lt = chain.last_targets
    idx = lt['sample_roi_indices'].cpu().numpy()
    rois = lt['sample_rois'].cpu().numpy()
    rpn = lt['gt_rpn_labels'].cpu().numpy().reshape(2, -1)
    prop = seen[-1]
    rois0 = prop.rois[:int(prop.counts[0])].detach().cpu().numpy()
    return dict(loss=float(loss.detach()), rois=[rois[idx == i] for i in (0, 1)], rpn=rpn, proposals0=rois0,
                labels=[lt['gt_roi_labels'].cpu().numpy()[idx == i] for i in (0, 1)],
                n=(lt['n_ignored_rois'], lt['n_ignored_anchors']), shape=lt['feature_shape'])


def test_train_step_leaves_the_crowd_out(dev, small, monkeypatch):
    model, chain = small
    batch = _batch(dev)
    bboxes, dense, plane = batch[1], batch[4], batch[5]
    seen = []
    orig = model.rpn.propose
    monkeypatch.setattr(model.rpn, 'propose', lambda *a, **kw: (seen.append(orig(*a, **kw)), seen[-1])[1])
    rs = _Reseed(chain, monkeypatch)
    runs = {}
    for device_targets in (False, True):
        for key, ignores in (('off', None), ('on', [plane, None])):
            rs.k = 0
            runs[device_targets, key] = _step(chain, batch, ignores, device_targets, seen)
            chain.zero_grad()
    chain.device_targets = False
    for device_targets in (False, True):
        on, off = runs[device_targets, 'on'], runs[device_targets, 'off']
        assert np.isfinite(on['loss']) and off['n'] == (0, 0)
        anchor = model.rpn.host_anchor(on['shape'][2], on['shape'][3], dev)
        assert on['rpn'].shape[1] == len(anchor)
        # sampled RoIs of image 0: only a ground-truth box may lie on the crowd
        ign = F.ignored_from_counts(R.box_coverage(dense, on['rois'][0]), chain.crowd_ignore_thresh)
        is_gt = (on['rois'][0][:, None, :] == bboxes[0][None]).all(2).any(1)
        assert not (ign & ~is_gt).any()
        # (the check bites: without the plane, proposals on the crowd are sampled)
        ign_off = F.ignored_from_counts(R.box_coverage(dense, off['rois'][0]), chain.crowd_ignore_thresh)
        is_gt_off = (off['rois'][0][:, None, :] == bboxes[0][None]).all(2).any(1)
        assert (ign_off & ~is_gt_off).any()
        # anchors of image 0: no negative lies on the crowd; the count of ignored anchors
        ign_a = F.ignored_from_counts(R.box_coverage(dense, anchor), chain.crowd_ignore_thresh)
        assert ign_a.sum() > 50 and not (ign_a & (on['rpn'][0] == 0)).any()
        assert (ign_a & (off['rpn'][0] == 0)).any()
        assert (on['rpn'][0] >= 0).sum() <= chain.anchor_target_creator.n_sample
        ign_p = F.ignored_from_counts(R.box_coverage(dense, on['proposals0']), chain.crowd_ignore_thresh)
        assert on['n'] == (int(ign_p.sum()), int(ign_a.sum())) and on['n'][0] > 0
        assert isinstance(on['n'][0], int) and isinstance(on['n'][1], int)
        # image 1 has no plane: its targets are those of the run without planes
        assert np.array_equal(on['rois'][1], off['rois'][1]) and np.array_equal(on['labels'][1], off['labels'][1])
        assert np.array_equal(on['rpn'][1], off['rpn'][1])
        assert np.array_equal(on['proposals0'], off['proposals0'])
    # the host path and the device path sample identical sets from the same seeds
    h, d = runs[False, 'on'], runs[True, 'on']
    assert all(np.array_equal(a, b) for a, b in zip(h['rois'], d['rois']))
    assert all(np.array_equal(a, b) for a, b in zip(h['labels'], d['labels']))
    assert np.array_equal(h['rpn'], d['rpn']) and h['n'] == d['n']


@pytest.mark.parametrize('device_targets', [False, True])
def test_off_state_is_bit_identical(dev, small, device_targets):
    model, chain = small
    imgs, bboxes, labels, masks = _batch(dev)[:4]
    chain.device_targets = device_targets
    params = [p for p in chain.parameters() if p.requires_grad]
    results = []
    try:
        for kw in ({}, dict(ignores=None), dict(ignores=[None, None])):
            chain.zero_grad()
            np.random.seed(9)
            loss = chain(imgs, bboxes, labels, masks, [1., 1.], **kw)
            loss.backward()
            torch.cuda.synchronize()
            state = np.random.get_state()
            results.append((loss.detach().clone(), [None if p.grad is None else p.grad.clone() for p in params],
                            state, chain.last_targets['n_ignored_rois'], chain.last_targets['n_ignored_anchors']))
    finally:
        chain.device_targets = False
        chain.zero_grad()
    first = results[0]
    assert sum(g is not None for g in first[1]) > 50 and np.isfinite(float(first[0]))
    for other in results[1:]:
        assert torch.equal(other[0], first[0])
        assert all((a is None) == (b is None) and (a is None or torch.equal(a, b)) for a, b in zip(other[1], first[1]))
        assert other[2][0] == first[2][0] and np.array_equal(other[2][1], first[2][1]) and other[2][2:] == first[2][2:]
        assert other[3:] == (0, 0)
    with pytest.raises(ValueError, match='one entry'):
        chain(imgs, bboxes, labels, masks, [1., 1.], ignores=[None])


# ---- tools/train.py --crowd-ignore -----------------------------------------------------------
def _write_coco_with_crowds(root, H=96, W=128):
    """A COCO-layout directory: train (3 images), valminusminival (1) and minival (2), every image
    with two polygon instances and one crowd region (uncompressed RLE) over its right half."""
    import json
    import os
    import PIL.Image
    rng = np.random.RandomState(0)
    os.makedirs(os.path.join(root, 'annotations'))
    img_id = 10
    for split, folder, n in (('train', 'train2014', 3), ('valminusminival', 'val2014', 1), ('minival', 'val2014', 2)):
        os.makedirs(os.path.join(root, folder), exist_ok=True)
        images, anns = [], []
        for _ in range(n):
            img_id += 1
            PIL.Image.fromarray(rng.randint(0, 256, (H, W, 3)).astype(np.uint8)).save(
                os.path.join(root, folder, 'COCO_%s_%012d.jpg' % (folder, img_id)), quality=95)
            images.append(dict(id=img_id, height=H, width=W))
            for g in range(2):
                y0, x0 = int(rng.randint(4, H // 2)), int(rng.randint(4, W // 2))
                h, w = int(rng.randint(24, H // 2 - 4)), int(rng.randint(24, W // 2 - 4))
                poly = [x0, y0, x0 + w, y0, x0 + w, y0 + h, x0, y0 + h]
                anns.append(dict(id=len(anns) + 1 + 100 * img_id, image_id=img_id, category_id=[1, 3][g],
                                 segmentation=[[float(v) for v in poly]], iscrowd=0, area=float(h * w),
                                 bbox=[x0, y0, w, h]))
            anns.append(dict(id=99 + 100 * img_id, image_id=img_id, category_id=1, iscrowd=1,
                             segmentation=dict(size=[H, W], counts=[H * (W // 2), H * (W - W // 2)]),
                             area=float(H * (W - W // 2)), bbox=[W // 2, 0, W - W // 2, H]))
        with open(os.path.join(root, 'annotations', 'instances_%s2014.json' % split), 'w') as f:
            json.dump(dict(images=images, annotations=anns,
                           # (four classes: the mask head's output channels come in fours)
                           categories=[dict(id=c, name='cat%d' % c) for c in (1, 3, 18, 25)]), f)


def test_train_tool_with_crowd_ignore(dev, tmp_path):
    import io
    import json
    import os
    import sys
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools')
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import train
    root, logs = str(tmp_path / 'COCO'), str(tmp_path / 'logs')
    _write_coco_with_crowds(root)
    args = train.parse_args(['--dataset', 'coco', '--coco-root', root, '--device-masks', '--crowd-ignore',
                             '--allow-random-init', '--max-epoch', '1', '--batch-size-per-gpu', '2',
                             '--logs-dir', logs, '--no-plot'])
    assert args.crowd_ignore == 0.7
    comm = train.setup_comm(args)
    train_data, test_data, class_names, _, evaluator_type = train.datasets(args)
    assert len(train_data) == 4 and len(train_data[0]) == 5 and train_data[0][4].tolist() == [0, 0, 1]
    train.configure(args, comm, class_names, dict(min_size=160, max_size=240, anchor_scales=(2, 4, 8, 16, 32)))
    model = train.build_model(args, None, proposal_creator_params=dict(
        min_size=0, n_train_pre_nms=600, n_train_post_nms=100, n_test_pre_nms=300, n_test_post_nms=50))
    run = train.assemble(args, comm, model, train_data, test_data, evaluator_type, synthetic_weights=True,
                         print_out=io.StringIO(), eval_interval=(1, 'epoch'), log_interval=(1, 'iteration'),
                         plot_interval=(1, 'epoch'), print_interval=(1, 'iteration'))
    assert run.chain.crowd_ignore_thresh == 0.7
    try:
        run.trainer.run()
    finally:
        run.loop.close()
    torch.cuda.synchronize()
    with open(os.path.join(args.out, 'log')) as f:
        log = json.load(f)
    assert len(log) == 2
    assert all(np.isfinite(e['main/loss']) for e in log)
    assert all(e['main/n_ignored_rois'] > 0 and e['main/n_ignored_anchors'] > 0 for e in log)
    with open(os.path.join(args.out, 'params.yaml')) as f:
        assert 'crowd_ignore: 0.7' in f.read()
