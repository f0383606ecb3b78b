"""utils.draw_instance_bboxes, utils.get_tile_image and InstanceSegmentationVisReport on the
MI355X: bit-exact against the fixture produced by the reference's own draw_instance_bboxes,
exact against the NumPy restatement on full-size images with 100 overlapping instances and
captions, every mask form giving the same image, the packed paste of predicted logits against
the host masks of predict, the mosaic kernel against its restatement, and the report written
for a fake trainer."""
import os

import numpy as np
import pytest
import torch

import chainer_mask_rcnn_amd as cmr
import visualize_ref as R
from chainer_mask_rcnn_amd import utils
from chainer_mask_rcnn_amd.utils import visualizations as V
from chainer_mask_rcnn_amd.utils.evaluations import masks as M

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'draw_instances.npz'))


def unpack(d, key):
    shape = tuple(d[key + '_shape'])
    return np.unpackbits(d[key], axis=-1)[..., :shape[-1]].reshape(shape).astype(bool)


def test_fixture_bit_exact_host_and_device(dev, golden):
    for name in golden['cases']:
        img, bboxes, labels = golden[name + '_img'], golden[name + '_bboxes'], golden[name + '_labels']
        n_class, alpha, thickness, bg = golden[name + '_params']
        draw = list(golden[name + '_draw']) if name + '_draw' in golden else None
        key = name + '_masks'
        if key + '_shape' in golden:
            masks = unpack(golden, key)
        elif key + '_count' in golden:
            masks = [unpack(golden, '%s_%d' % (key, j)) for j in range(int(golden[key + '_count']))]
        else:
            masks = None
        kw = dict(masks=masks, bg_class=int(bg), thickness=int(thickness), alpha=float(alpha),
                  draw=draw)
        before = img.copy()
        out = utils.draw_instance_bboxes(img, bboxes, labels, int(n_class), **kw)
        assert isinstance(out, np.ndarray) and out.dtype == np.uint8
        assert np.array_equal(out, golden[name + '_out']), name
        assert np.array_equal(img, before), name                 # the input is not modified
        img_d = torch.from_numpy(img).to(dev)
        out_d = utils.draw_instance_bboxes(img_d, bboxes, labels, int(n_class), **kw)
        assert isinstance(out_d, torch.Tensor) and out_d.is_cuda and out_d.dtype == torch.uint8
        assert np.array_equal(out_d.cpu().numpy(), out), name
        assert np.array_equal(img_d.cpu().numpy(), before), name


def _scene(rng, H, W, N):
    """Random image, N overlapping boxes (some touching or crossing the edges, some with
    negative corners), labels with background entries, full-frame masks that reach past their
    boxes, skip flags."""
    img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    y1 = rng.uniform(-40, H - 20, N)
    x1 = rng.uniform(-40, W - 20, N)
    bboxes = np.stack([y1, x1, y1 + rng.uniform(5, 400, N), x1 + rng.uniform(5, 500, N)],
                      1).astype(np.float32)
    bboxes[0] = (0, 0, H, W)
    bboxes[1] = (H - 30, W - 50, H, W)
    bboxes[2] = (-10, 100, 60, W + 20)
    labels = rng.randint(0, 21, N).astype(np.int32)
    yy, xx = np.mgrid[:H, :W]
    masks = np.zeros((N, H, W), bool)
    for i, b in enumerate(bboxes):
        cy, cx = (b[0] + b[2]) / 2, (b[1] + b[3]) / 2
        ry, rx = (b[2] - b[0]) * 0.6 + 1, (b[3] - b[1]) * 0.6 + 1
        masks[i] = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
    masks &= rng.uniform(size=(1, H, W)) > 0.02
    draw = rng.uniform(size=N) > 0.15
    return img, bboxes, labels, masks, draw


def _full_frame(masks, bboxes, H, W):
    full = np.zeros((len(masks), H, W), bool)
    for i, (m, b) in enumerate(zip(masks, np.asarray(bboxes).astype(int))):
        if m.shape == (H, W):
            full[i] = m
        else:
            y1, x1, y2, x2 = b
            sy0, sy1, sx0, sx1 = max(y1, 0), min(y2, H), max(x1, 0), min(x2, W)
            full[i, sy0:sy1, sx0:sx1] = m[sy0 - y1:sy1 - y1, sx0 - x1:sx1 - x1]
    return full


@pytest.mark.parametrize('alpha,thickness', [(0.3, 1), (0.5, 2), (1.0, 3)])
def test_full_size_exact_against_restatement(dev, alpha, thickness):
    rng = np.random.RandomState(int(alpha * 10) + thickness)
    H, W, N = 800, 1333, 100
    img, bboxes, labels, masks, draw = _scene(rng, H, W, N)
    # a few box-sized masks (the crop of the full-frame one) in a list input
    ib = bboxes.astype(int)
    inner = [i for i in range(3, N) if ib[i, 0] >= 0 and ib[i, 1] >= 0 and ib[i, 2] <= H and
             ib[i, 3] <= W][:10]
    listed = list(masks)
    for i in inner:
        listed[i] = masks[i, ib[i, 0]:ib[i, 2], ib[i, 1]:ib[i, 3]]
    captions = ['c%d %.1f%%' % (l, 100 * s) for l, s in zip(labels, rng.uniform(size=N))]
    on = [bool(draw[i]) and labels[i] != 0 for i in range(N)]
    layout = V.caption_layout(np.asarray(captions), ib, on)
    assert sum(c is not None for c in layout) > 50
    want = R.draw(img, bboxes, labels, 21, _full_frame(listed, bboxes, H, W), layout, 0,
                  thickness, alpha, draw)
    got = utils.draw_instance_bboxes(img, bboxes, labels, 21, masks=listed, captions=captions,
                                     thickness=thickness, alpha=alpha, draw=draw)
    assert np.array_equal(got, want)
    # without captions, and with every mask full-frame on the device
    want = R.draw(img, bboxes, labels, 21, masks, None, 0, thickness, alpha, draw)
    got = utils.draw_instance_bboxes(torch.from_numpy(img).to(dev), bboxes, labels, 21,
                                     masks=torch.from_numpy(masks).to(dev), thickness=thickness,
                                     alpha=alpha, draw=draw)
    assert np.array_equal(got.cpu().numpy(), want)


def test_background_class_and_skips(dev):
    rng = np.random.RandomState(3)
    H, W, N = 120, 200, 30
    img, bboxes, labels, masks, draw = _scene(rng, H, W, N)
    for bg in (0, 5, -1):
        want = R.draw(img, bboxes, labels, 21, masks, None, bg, 1, 0.5, draw)
        got = utils.draw_instance_bboxes(img, bboxes, labels, 21, masks=masks, bg_class=bg,
                                         draw=draw)
        assert np.array_equal(got, want), bg
    # nothing drawn: every instance skipped
    got = utils.draw_instance_bboxes(img, bboxes, labels, 21, masks=masks, draw=[False] * N)
    assert np.array_equal(got, img)
    got = utils.draw_instance_bboxes(img, np.zeros((0, 4)), np.zeros(0, np.int32), 21,
                                     masks=np.zeros((0, H, W), bool))
    assert np.array_equal(got, img)


def test_mask_forms_give_identical_images(dev):
    rng = np.random.RandomState(5)
    H, W, N = 150, 257, 40
    img, bboxes, labels, masks, draw = _scene(rng, H, W, N)
    kw = dict(draw=draw, thickness=2, alpha=0.4)
    ref = utils.draw_instance_bboxes(img, bboxes, labels, 21, masks=masks, **kw)
    assert np.array_equal(ref, R.draw(img, bboxes, labels, 21, masks, None, 0, 2, 0.4, draw))
    for m in (masks.astype(np.uint8), masks.astype(np.int32) * 7,
              torch.from_numpy(masks).to(dev), torch.from_numpy(masks.astype(np.uint8)).to(dev),
              M.pack_masks(masks, device=dev)):
        got = utils.draw_instance_bboxes(img, bboxes, labels, 21, masks=m, **kw)
        assert np.array_equal(got, ref)


def _small_model(dev):
    torch.manual_seed(0)
    model = cmr.models.MaskRCNNResNet(50, n_fg_class=80, min_size=160, max_size=240,
                                      anchor_scales=(2, 4, 8, 16, 32), roi_size=14,
                                      proposal_creator_params=dict(min_size=0, n_test_pre_nms=300,
                                                                   n_test_post_nms=50)).to(dev)
    with torch.no_grad():
        model.extractor.bn1.W.fill_(1. / 64.)
        model.head.cls_loc_score.W[4 * 81:5 * 81] *= 300.
    return model


def _synthetic(rng, n):
    out = []
    for i in range(n):
        H, W = [(100, 140), (120, 90), (96, 128)][i % 3]
        img = rng.randint(0, 256, (3, H, W)).astype(np.uint8)
        G = rng.randint(1, 5)
        mask = np.zeros((G, H, W), np.int32)
        bbox = np.zeros((G, 4), np.float32)
        for g in range(G):
            y0, x0 = rng.randint(0, H - 20), rng.randint(0, W - 20)
            h, w = rng.randint(8, 60), rng.randint(8, 60)
            mask[g, y0:y0 + h, x0:x0 + w] = 1
            bbox[g] = (y0, x0, min(y0 + h, H), min(x0 + w, W))
        label = rng.randint(0, 80, G).astype(np.int32)
        out.append((img, bbox, label, mask))
    return out


def test_packed_paste_of_predictions_equals_host_masks(dev):
    rng = np.random.RandomState(7)
    model = _small_model(dev)
    data = _synthetic(rng, 3)
    imgs = [ex[0] for ex in data]
    bboxes, masks, labels, scores = model.predict(imgs)
    x, sizes, scales = model.prepare(imgs)
    b2, roi_masks, l2, s2 = model.predict_prepared(x, scales, sizes, masks_to_host=False)
    n = 0
    for j in range(len(imgs)):
        assert np.array_equal(b2[j], bboxes[j]) and np.array_equal(l2[j], labels[j])
        img = np.ascontiguousarray(imgs[j].transpose(1, 2, 0))
        packed = M.paste_packed(roi_masks[j], l2[j], b2[j], sizes[j])
        a = utils.draw_instance_bboxes(img, b2[j], l2[j] + 1, 81, masks=packed)
        b = utils.draw_instance_bboxes(img, bboxes[j], labels[j] + 1, 81, masks=masks[j])
        assert np.array_equal(a, b)
        n += len(bboxes[j])
    assert n > 0


def test_tile_kernel_exact(dev):
    rng = np.random.RandomState(9)
    sizes = [(100, 140), (120, 90), (96, 128), (37, 250), (300, 41), (64, 64), (1, 5)]
    imgs = [rng.randint(0, 256, s + (3,)).astype(np.uint8) for s in sizes]
    for subset, shape in ((imgs[:6], (3, 3)), (imgs[:4], (2, 2)), (imgs[:5], (2, 3)),
                          (imgs[:3], (1, 3)), (imgs, (3, 3))):
        want = R.tile(subset, shape)
        got = utils.get_tile_image(subset, tile_shape=shape)
        assert got.dtype == np.uint8 and np.array_equal(got, want), shape
        got_d = utils.get_tile_image([torch.from_numpy(a).to(dev) for a in subset], shape)
        assert got_d.is_cuda and np.array_equal(got_d.cpu().numpy(), want), shape
    # default grid
    assert utils.get_tile_image(imgs[:5]).shape[:2] == R.tile(imgs[:5], (2, 3)).shape[:2]


class _FakeTrainer(object):
    def __init__(self, out, iteration):
        self.out = out
        self.updater = type('U', (), {'iteration': iteration})()


def test_report_writes_files_and_renders_the_host_composition(dev, tmp_path):
    from PIL import Image
    rng = np.random.RandomState(13)
    model = _small_model(dev)
    data = _synthetic(rng, 6)
    batches = [data[0:2], data[2:4], data[4:6]]
    names = ['c%d' % l for l in range(80)]
    rep = cmr.extensions.InstanceSegmentationVisReport(batches, model, names, shape=(2, 2))
    rep(_FakeTrainer(str(tmp_path), 5))
    f = tmp_path / 'visualizations' / 'iteration=00000005.jpg'
    assert f.exists() and (tmp_path / 'visualizations' / 'latest.jpg').exists()
    mosaic = rep.render()
    assert Image.open(str(f)).size == (mosaic.shape[1], mosaic.shape[0])
    # the host composition: predict on the same batches, draw each panel, stack, tile
    label_names = np.hstack((['__background__'], names))
    vizs = []
    n_kept = 0
    for b in batches:
        bb, mm, ll, ss = model.predict([ex[0] for ex in b])
        for ex, pb, pm, pl, ps in zip(b, bb, mm, ll, ss):
            img = np.ascontiguousarray(ex[0].transpose(1, 2, 0))
            gt = utils.draw_instance_bboxes(img, ex[1], ex[2] + 1, 81, masks=ex[3].astype(bool),
                                            captions=label_names[ex[2] + 1])
            k = ps >= 0.7
            n_kept += int(k.sum())
            caps = ['{:s} {:.1%}'.format(n, s) for s, n in zip(ps[k], label_names[pl[k] + 1])]
            pr = utils.draw_instance_bboxes(img, pb[k], pl[k] + 1, 81, masks=pm[k], captions=caps)
            vizs.append(np.vstack([gt, pr]))
    assert n_kept > 0
    assert np.array_equal(mosaic, R.tile(vizs[:4], (2, 2)))
    # the evaluation tool's form: a fixed name, no copy
    rep2 = cmr.extensions.InstanceSegmentationVisReport(batches, model, names,
                                                        file_name='iteration=%s.jpg',
                                                        copy_latest=False)
    rep2(_FakeTrainer(str(tmp_path / 'eval'), 'best'))
    assert (tmp_path / 'eval' / 'iteration=best.jpg').exists()
    assert not (tmp_path / 'eval' / 'latest.jpg').exists()
