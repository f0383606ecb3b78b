"""The RoI head with and without the tables its caller may pass beside the RoIs
(functions.RoiHints): the hints change which workgroup pools which RoI and who builds two small
tables, never a value; and the head pools with the indices it is given, whatever tensor carries
the RoIs."""
import numpy as np
import pytest
import torch

from chainer_mask_rcnn_amd.functions import RoiHints, roi_spatial_order
from chainer_mask_rcnn_amd.streams import join_wgrad_stream
from chainer_mask_rcnn_amd.models.mask_rcnn_resnet import ResNetRoIHead
from chainer_mask_rcnn_amd.models.mask_rcnn_train_chain import _upload_many
from test_gpu_projected_pooling import _rois

pytestmark = pytest.mark.gpu

N, MAP_H, MAP_W = 2, 12, 14


def _head(dev, roi_size):
    torch.manual_seed(0)
    return ResNetRoIHead(50, 5, roi_size, 1 / 16.).to(dev)


@pytest.mark.parametrize('projected', [False, True])
@pytest.mark.parametrize('roi_size', [7, 14])
def test_hints_change_nothing(dev, roi_size, projected):
    """20 RoIs, 13 on image 0 and 7 on image 1, the mask branch on 7 scattered rows (first and last
    included): outputs and every gradient with the hints MaskRCNNTrainChain builds are bit-equal
    to those without (the order is not an input of any sum; the backward does not take it; the
    host-built rows and slot table hold the values the head builds on the device)."""
    head = _head(dev, roi_size)
    head.projected_pooling = projected
    rng = np.random.RandomState(4)
    r5 = _rois(rng, 20, N, MAP_H, MAP_W)
    idx_h = np.repeat([0, 1], [13, 7]).astype(np.int32)
    rois_h = r5[:, [2, 1, 4, 3]]                                 # (y1, x1, y2, x2)
    rows_h = np.array([0, 2, 5, 9, 13, 16, 19], np.int64)
    # the chain's construction (models/mask_rcnn_train_chain.py:_forward_host_targets)
    slot_h = np.full((20,), -1, np.int32)
    slot_h[rows_h] = np.arange(len(rows_h), dtype=np.int32)
    order_h = roi_spatial_order(rois_h, idx_h, head.spatial_scale)
    rois5_h = np.concatenate([idx_h[:, None].astype(np.float32), rois_h[:, [1, 0, 3, 2]]], axis=1)
    rois, idx, rows, slot, order, rois5 = _upload_many(
        [rois_h, idx_h, rows_h, slot_h, order_h, rois5_h],
        [torch.float32, torch.int32, torch.int64, torch.int32, torch.int32, torch.float32], dev)
    assert sorted(order_h.tolist()) == list(range(20)) and order_h.tolist() != list(range(20))
    x = torch.randn((N, 1024, MAP_H, MAP_W), device=dev)
    gs = None
    results = []
    for hints in (RoiHints(rois5, order, slot), None):
        head.zero_grad(set_to_none=True)
        xt = x.clone().requires_grad_(True)
        outs = head(xt, rois, idx, mask_rows=rows, hints=hints)
        assert tuple(outs[2].shape) == (7, 4, 14, 14)
        if gs is None:
            gs = [torch.randn_like(o) for o in outs]
        torch.autograd.backward(outs, gs)
        join_wgrad_stream()
        torch.cuda.synchronize()
        grads = {k: p.grad.clone() for k, p in head.named_parameters() if p.grad is not None}
        for k in ('res5.a.conv1.W', 'res5.a.conv4.W', 'res5.b2.conv3.W', 'cls_loc_score.W', 'deconv6.W', 'mask.W'):
            assert float(grads[k].abs().max()) > 0, k
        results.append(([o.detach() for o in outs], xt.grad, grads))
    (outs_a, gx_a, g_a), (outs_b, gx_b, g_b) = results
    for a, b in zip(outs_a, outs_b):
        assert torch.equal(a, b)
    assert torch.equal(gx_a, gx_b) and float(gx_a.abs().max()) > 0
    assert set(g_a) == set(g_b)
    for k in g_a:
        assert torch.equal(g_a[k], g_b[k]), k


def test_head_uses_the_indices_it_is_given(dev):
    """The sampled RoIs of a train step, pooled with all-zero indices: the tensor the chain stored
    and a clone of it give the same outputs (nothing travels on the tensor itself)."""
    from test_gpu_model import _build
    model, chain, imgs, bboxes, labels, masks = _build(dev)
    np.random.seed(5)
    chain(torch.tensor(imgs, device=dev), bboxes, labels, masks, [1., 1.])
    t = chain.last_targets
    rois = t['sample_rois']
    assert int(t['sample_roi_indices'].max()) == 1          # the sample holds RoIs of image 1
    head = _head(dev, 14)
    x = torch.randn((N, 1024, MAP_H, MAP_W), device=dev)
    zero = torch.zeros(len(rois), dtype=torch.int32, device=dev)
    with torch.no_grad():
        stored = head(x, rois, zero)
        cloned = head(x, rois.clone(), zero)
    for a, b in zip(stored, cloned):
        assert torch.equal(a, b)
