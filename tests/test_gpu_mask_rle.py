"""The device COCO RLE codec (csrc/mask_rle.hip, utils/evaluations/rle.py) against the
vectorised NumPy reference of tests/test_coco_results_cpu.py (itself pinned to the oracle's
per-pixel codec): encode bit-exact in counts and strings, decode bit-exact in bits, areas and
extents, round trips, both packed inputs, malformed input."""
import numpy as np
import pytest
import torch

import chainer_mask_rcnn_amd as cmr
from chainer_mask_rcnn_amd.datasets.coco import rle_decode
from chainer_mask_rcnn_amd.utils.evaluations import masks as M
from chainer_mask_rcnn_amd.utils.evaluations import rle as R
from oracle import np_data
from test_coco_results_cpu import np_rle_counts, np_rle_string

pytestmark = pytest.mark.gpu

WS = (1, 63, 64, 65, 640, 1333)
HS = (1, 2, 480, 800)


def pattern_masks(H, W, rng):
    ms = [np.zeros((H, W), np.uint8), np.ones((H, W), np.uint8)]
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        m = np.zeros((H, W), np.uint8)
        m[y, x] = 1
        ms.append(m)
    m = np.zeros((H, W), np.uint8)                       # runs across column boundaries
    m[H // 2:, :W // 2 + 1] = 1
    m[:max(H // 3, 1), W // 2:] = 1
    ms.append(m)
    ms.append(np.tile((np.arange(W) % 3 == 0)[None, :], (H, 1)).astype(np.uint8))   # stripes
    ms.append(np.tile((np.arange(H) % 2 == 0)[:, None], (1, W)).astype(np.uint8))
    ms.append((np.indices((H, W)).sum(0) % 2).astype(np.uint8))                     # checkerboard
    ms.append((rng.uniform(size=(H, W)) < 0.5).astype(np.uint8))
    m = np.zeros((H, W), np.uint8)                       # a blob
    y0, x0 = rng.randint(0, H), rng.randint(0, W)
    m[y0:y0 + rng.randint(1, H + 1), x0:x0 + rng.randint(1, W + 1)] = 1
    ms.append(m)
    return np.stack(ms)


def ref(masks):
    counts = [np_rle_counts(m) for m in masks]
    return counts, [np_rle_string(c) for c in counts]


def check_decoded(packed, masks):
    """Decoded packed triple == pack_masks(masks) bit for bit, exact area, extent containing
    every set bit."""
    p, area, extent = (t.cpu().numpy() for t in packed)
    want = M.pack_masks(masks)
    assert np.array_equal(p, want[0].cpu().numpy())
    assert np.array_equal(area, want[1].cpu().numpy())
    for e, m in zip(extent, masks):
        ys, xs = np.nonzero(m)
        if len(ys):
            assert e[0] <= ys.min() and ys.max() < e[1]
            assert e[2] <= xs.min() // 64 and xs.max() // 64 < e[3]


@pytest.mark.parametrize('H', HS)
@pytest.mark.parametrize('W', WS)
def test_encode_decode_patterns(dev, H, W):
    rng = np.random.RandomState(H * 7 + W)
    masks = pattern_masks(H, W, rng)
    counts, strings = ref(masks)
    got = R.encode_masks(masks)
    assert [g['counts'] for g in got] == strings
    assert all(g['size'] == [H, W] for g in got)
    got_c = R.encode_masks(torch.tensor(masks, device=dev).bool(), uncompressed=True)
    assert [g['counts'] for g in got_c] == [c.tolist() for c in counts]
    # decode: strings and count lists, against pack_masks of the host decode
    host = np.stack([rle_decode({'size': [H, W], 'counts': s}, H, W) for s in strings])
    assert np.array_equal(host, masks)
    check_decoded(R.decode_masks(got, packed=True), host)
    check_decoded(R.decode_masks(got_c, packed=True), host)
    assert np.array_equal(R.decode_masks(got).cpu().numpy(), masks)


def test_small_masks_against_the_oracle_decoder(dev):
    rng = np.random.RandomState(1)
    for H, W in ((1, 1), (3, 5), (7, 66), (9, 2)):
        masks = (rng.uniform(size=(4, H, W)) < 0.4).astype(np.uint8)
        for g, m in zip(R.encode_masks(masks), masks):
            assert g['counts'] == np_data.rle_to_string(np_data.mask_to_rle_counts(m))
            assert np.array_equal(np_data.rle_decode(g), m)
        dec = R.decode_masks([{'size': [H, W], 'counts': np_data.mask_to_rle_counts(m)}
                              for m in masks])
        assert np.array_equal(dec.cpu().numpy(), masks)


def test_hundred_masks_full_size_and_repeatable(dev):
    rng = np.random.RandomState(2)
    H, W = 800, 1333
    masks = np.zeros((100, H, W), np.uint8)
    for m in masks:
        for _ in range(rng.randint(1, 4)):
            y0, x0 = rng.randint(0, H), rng.randint(0, W)
            m[y0:y0 + rng.randint(1, 500), x0:x0 + rng.randint(1, 700)] ^= 1
    masks[7, :, 100:300] = 1                             # full-height columns
    counts, strings = ref(masks)
    md = torch.tensor(masks, device=dev)
    a = R.encode_masks(md)
    b = R.encode_masks(M.pack_masks(md), size=(H, W))
    assert [g['counts'] for g in a] == strings
    assert a == b
    check_decoded(R.decode_masks(a, packed=True), masks)


def test_paste_packed_input_equals_byte_paste(dev):
    """encode(paste_packed(...)) == encode of MaskRCNN._to_masks' byte masks: the widened,
    non-tight extents of the packed paste."""
    rng = np.random.RandomState(3)
    for H, W, D in ((480, 640, 100), (800, 1333, 30), (37, 70, 12)):
        bbox = np.zeros((D, 4), np.float32)
        bbox[:, :2] = rng.uniform(-20, [H, W], (D, 2))
        bbox[:, 2:] = bbox[:, :2] + rng.uniform(1, [H / 2, W / 2], (D, 2))
        bbox[0] = [-5, -5, H + 5, W + 5]                  # spans every row and column
        label = rng.randint(0, 80, D).astype(np.int32)
        logits = torch.tensor(rng.standard_normal((D, 80, 14, 14)).astype(np.float32) * 3,
                              device=dev)
        logits[0] = 5.                                   # a full-image mask
        byte = cmr.models.mask_rcnn.MaskRCNN._to_masks(None, [bbox], [label], None, [logits],
                                                       [(H, W)])[0]
        pk = M.paste_packed(logits, label, bbox, (H, W))
        got = R.encode_masks(pk, size=(H, W))
        assert [g['counts'] for g in got] == ref(byte)[1]
        check_decoded(R.decode_masks(got, packed=True), byte)


def test_mixed_strings_and_count_lists(dev):
    masks = pattern_masks(5, 70, np.random.RandomState(4))
    counts, strings = ref(masks)
    rles = [{'size': [5, 70], 'counts': (strings[i] if i % 2 else counts[i].tolist())}
            for i in range(len(masks))]
    assert np.array_equal(R.decode_masks(rles).cpu().numpy(), masks)
    empty = R.decode_masks([], packed=True, size=(5, 70))
    assert empty[0].shape == (0, 5, 2) and empty[1].shape == (0,)


@pytest.mark.parametrize('counts, why', [
    ('S1\x7f', 'outside 48..111'),                      # a character above 111
    ('/S1', 'outside 48..111'),                          # a character below 48
    ('S', 'unterminated'),                               # 'S' has the continuation bit
    ('oooooooo', 'unterminated'),                        # more than 7 groups
    ('1', 'sum'),
    ('S1S1', 'sum'),
    ('', 'sum'),
    ([5, 31], 'sum'),
    ([-5, 40], 'negative'),
])
def test_malformed_input_raises(dev, counts, why):
    good = {'size': [5, 7], 'counts': np_rle_string([35])}
    assert good['counts'] == 'S1'
    bad = {'size': [5, 7], 'counts': counts}
    with pytest.raises(ValueError, match='RLE entry 1: malformed RLE: .*%s' % why):
        R.decode_masks([good, bad, good])
    # nothing faulted: a valid decode right after
    assert R.decode_masks([good]).sum().item() == 0


def test_malformed_shapes_raise(dev):
    with pytest.raises(ValueError, match='different sizes'):
        R.decode_masks([{'size': [5, 7], 'counts': [35]}, {'size': [7, 5], 'counts': [35]}])
    with pytest.raises(ValueError, match='32-bit'):
        R.decode_masks([{'size': [5, 7], 'counts': [1 << 40]}])
    with pytest.raises(ValueError, match='RLE entry 0'):
        R.decode_masks([{'counts': [35]}])
