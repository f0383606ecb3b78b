"""Every launch of the full-size step against a float64 reference (tests/launch_ref.py).

tests/test_gpu_fullsize.py checks the bench.py step at full size only for properties that hold at
any size (finite, repeatable, work reductions on == off); a deterministic but wrong kernel passes
them.  Here every call of a checked entry point during two consecutive full-size train steps and
the final flush, and during a full-size batch-8 inference, is compared with its float64
restatement on the device — at the shapes where the GEMM host code takes the routes the small
tests never reach (W8 256x128 tiles, the one-round big_split_k rule, fused-tail K-split pieces,
tiny_split, strided 1x1 data gradients on the transposed filter, split-K weight gradients, the
PW / K3 instantiations, the Winograd route at the shipped threshold).  The five losses and the
inference softmax are among them: in place, with the step's label distributions and the strides of
the fused cls_loc / score layer's output, under the bounds derived in tests/launch_ref.py.  Then the non-default
settings of those routes and the ROIAlign lane caps on a RoI-head and a backbone block.
"""
import ctypes
import gc

import numpy as np
import pytest
import torch

import bench
import launch_ref
from chainer_mask_rcnn_amd import _lib, streams
from chainer_mask_rcnn_amd.functions import conv

pytestmark = pytest.mark.gpu

H, W, BATCH = 800, 1333, 2

# entry points of the train step (two updates + flush)
TRAIN_CHECKED = {
    'mrcnn_conv_stem_fwd', 'mrcnn_maxpool3x3s2p1_fwd', 'mrcnn_conv2d_fwd', 'mrcnn_conv2d_dgrad_wt',
    'mrcnn_conv2d_wgrad', 'mrcnn_conv2d_wgrad_ex', 'mrcnn_epilogue_bwd', 'mrcnn_filter_flip_transpose',
    'mrcnn_filter_flip_transpose_batched', 'mrcnn_conv3x3_wino_fwd', 'mrcnn_conv3x3_wino_dgrad',
    'mrcnn_conv3x3_wino_wgrad', 'mrcnn_sparse3x3_gather', 'mrcnn_sparse3x3_scatter',
    'mrcnn_roi_align_fwd_affine', 'mrcnn_roi_align_bwd_ws', 'mrcnn_avgpool_fwd',
    'mrcnn_head_tail_bwd', 'mrcnn_deconv2x2s2_fwd_wt', 'mrcnn_deconv2x2s2_dgrad',
    'mrcnn_deconv2x2s2_wgrad', 'mrcnn_colsum', 'mrcnn_sgd_momentum_wd_ex',
    # the five losses, in place: 256 sampled anchors of 128 520, 1024 RoIs on the fused
    # cls_loc / score layer's 408-wide rows, the foreground-only mask rows
    'mrcnn_sigmoid_ce', 'mrcnn_smooth_l1', 'mrcnn_softmax_ce', 'mrcnn_mask_sigmoid_ce',
}


def _profile_kinds():
    lib = _lib.load()
    seen = {}
    for k in range(lib.mrcnn_profile_num_kinds()):
        ms, fl, by, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
        _lib.check(lib.mrcnn_profile_summary(k, ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by),
                                             ctypes.byref(n)), 'profile_summary')
        if n.value:
            seen[lib.mrcnn_profile_kind_name(k).decode()] = n.value
    return seen


def _report(title, chk, kinds=None):
    print('\n== %s ==\n%s' % (title, chk.table()))
    if kinds is not None:
        print('profiler kinds: %s' % kinds)


@pytest.fixture
def shipped(dev):
    """The `dev` fixture lowers the Winograd work threshold for the small test models; here the
    shipped value must decide the routes."""
    saved = conv.WINOGRAD_MIN_WORK
    conv.WINOGRAD_MIN_WORK = 1 << 27
    yield dev
    conv.WINOGRAD_MIN_WORK = saved
    gc.collect()
    torch.cuda.empty_cache()


def test_train_step_launches_match_float64(shipped, monkeypatch):
    """bench.py's headline step (ResNet50-C4, 2 x 800 x 1333, 512 RoIs / image, projected pooling,
    sparse RPN backward, foreground-only mask branch): every launch of two updates (the second runs
    the first's deferred weight gradients) and the flush."""
    import random
    dev = shipped
    random.seed(0)
    np.random.seed(0)
    torch.manual_seed(0)
    imgs, bboxes, labels, masks, scales = bench.synthetic_batch(np.random.RandomState(0), BATCH, H, W)
    model, chain, opt, _ = bench.build_trainer(50, dev, 1, BATCH, defer=5)
    chain.mask_branch_fg_only = True
    x = torch.tensor(imgs, device=dev).contiguous(memory_format=torch.channels_last)
    chain.next_imgs = x
    monkeypatch.setattr(conv, 'SPARSE_CONV_BACKWARD', True)
    chk = launch_ref.LaunchChecker()
    lib = _lib.load()
    _lib.check(lib.mrcnn_profile_enable(3), 'profile_enable')
    try:
        chk.install(monkeypatch)
        for _ in range(2):
            loss = opt.update(chain, x, bboxes, labels, masks, scales)
            assert torch.isfinite(loss).all()
        opt.flush()
        torch.cuda.synchronize()
        kinds = _profile_kinds()
    finally:
        lib.mrcnn_profile_enable(0)
    _report('train step', chk, kinds)
    chk.assert_clean()
    assert set(chk.stats) == TRAIN_CHECKED
    # the kinds of the GEMM routes: forward on both tile sizes and W8, weight gradients on both
    for k in ('conv_gemm_kernel<2,2,FWD>', 'conv_gemm_kernel<1,1,FWD>', 'conv_gemm_kernel<2,2,FWD,W8>',
              'conv_gemm_kernel<2,2,WGRAD>', 'conv_gemm_kernel<1,1,WGRAD>', 'wino_transform_kernels'):
        assert k in kinds, (k, kinds)


def test_inference_launches_match_float64(dev, monkeypatch):
    """predict_prepared at 8 x 1024 x 1024 with test_c5_full_size_predict's weight recipe: batch-8
    map shapes, 1000 RoIs / image, Winograd forward with EXACT_SIGNS on cached filter transforms,
    the deconvolution's forward form."""
    import chainer_mask_rcnn_amd as cmr
    from chainer_mask_rcnn_amd.models.resnet_extractor import Bottleneck
    torch.manual_seed(0)
    rng = np.random.RandomState(0)
    N, H_, W_ = 8, 1024, 1024
    saved = conv.WINOGRAD_MIN_WORK
    conv.WINOGRAD_MIN_WORK = 1 << 27
    try:
        model = cmr.models.MaskRCNNResNet(50, n_fg_class=80, min_size=800, max_size=1333,
                                          anchor_scales=(2, 4, 8, 16, 32), roi_size=14).to(dev)
        with torch.no_grad():
            model.extractor.bn1.W.fill_(1. / 64.)
            for m in model.modules():
                if isinstance(m, Bottleneck):
                    m.bn3.W.fill_(0.25)
                    if m.projection:
                        m.bn4.W.fill_(0.5)
            model.head.cls_loc_score.W[4 * 81:5 * 81] *= 60.
        mean = np.asarray(model.mean, np.float32).reshape(3, 1, 1)
        x = torch.tensor(rng.uniform(0, 255, (N, 3, H_, W_)).astype(np.float32) - mean, device=dev)
        chk = launch_ref.LaunchChecker()
        chk.install(monkeypatch)
        bboxes, _, _, _ = model.predict_prepared(x, [1.6] * N, [(640, 640)] * N)
        torch.cuda.synchronize()
    finally:
        conv.WINOGRAD_MIN_WORK = saved
    _report('inference', chk)
    chk.assert_clean()
    assert sum(len(b) for b in bboxes) > 0
    assert {'mrcnn_conv_stem_fwd', 'mrcnn_maxpool3x3s2p1_fwd', 'mrcnn_conv2d_fwd',
            'mrcnn_conv3x3_wino_fwd', 'mrcnn_avgpool_fwd', 'mrcnn_softmax'} <= set(chk.stats), \
        sorted(chk.stats)


def _head_block(dev):
    from chainer_mask_rcnn_amd.models.resnet_extractor import BuildingBlock
    torch.manual_seed(11)
    blk = BuildingBlock(3, 1024, 512, 2048, 1).to(dev)
    with torch.no_grad():
        for name, p in blk.named_parameters():
            if '.bn' in name and name.endswith('.W'):
                p.uniform_(0.5, 1.5)
            elif '.bn' in name:
                p.normal_(0, 0.3)
    x = torch.randn((1000, 1024, 7, 7), device=dev).contiguous(memory_format=torch.channels_last)
    return blk, x


def _res4_block(dev):
    """One batch-2 res4 block (the projection block, stride 1 here) on the full-size 50 x 84 map."""
    from chainer_mask_rcnn_amd.models.resnet_extractor import BuildingBlock
    torch.manual_seed(12)
    blk = BuildingBlock(2, 512, 256, 1024, 1).to(dev)
    with torch.no_grad():
        for name, p in blk.named_parameters():
            if '.bn' in name and name.endswith('.W'):
                p.uniform_(0.5, 1.5)
            elif '.bn' in name:
                p.normal_(0, 0.3)
    x = torch.randn((2, 512, 50, 84), device=dev).contiguous(memory_format=torch.channels_last)
    return blk, x


def _run_block(blk, x, seed=5):
    xt = x.clone().requires_grad_(True)
    y = blk(xt)
    g = torch.randn(y.shape, generator=torch.Generator(device=y.device).manual_seed(seed),
                    device=y.device).contiguous(memory_format=torch.channels_last)
    y.backward(g)
    streams.join_wgrad_stream(x.device)
    torch.cuda.synchronize()
    out = [y.detach().clone(), xt.grad.clone()] + [p.grad.clone() for p in blk.parameters() if p.grad is not None]
    for p in blk.parameters():
        p.grad = None
    return out


KNOBS = [('fused_tail', 0, 512), ('tiny_split', 0, 1), ('big_split_k', 0, -1),
         ('small_m_split', 256, 0), ('w8', 0, 1)]


@pytest.mark.parametrize('block', ['head_res5', 'res4'])
def test_non_default_routes_match_float64(shipped, monkeypatch, block):
    """Each non-default route setting stays within the bound; pw in {0, 1, 2} is bit-identical to
    the default 3, as the header claims."""
    dev = shipped
    blk, x = (_head_block if block == 'head_res5' else _res4_block)(dev)
    for name, value, default in KNOBS:
        chk = launch_ref.LaunchChecker()
        with monkeypatch.context() as m:
            chk.install(m)
            try:
                _lib.set_tuning(name, value)
                _run_block(blk, x)
            finally:
                _lib.set_tuning(name, default)
        _report('%s %s=%d' % (block, name, value), chk)
        chk.assert_clean()
    ref = _run_block(blk, x)
    try:
        for pw in (0, 1, 2):
            _lib.set_tuning('pw', pw)
            got = _run_block(blk, x)
            assert all(torch.equal(a, b) for a, b in zip(got, ref)), 'pw=%d differs from pw=3' % pw
    finally:
        _lib.set_tuning('pw', 3)


@pytest.mark.parametrize('C', [1024, 2048])
def test_roi_lane_caps_match_float64(dev, monkeypatch, C):
    """roi_fwd_lanes / roi_bwd_lanes in {64, 128, 192} at the head's channel widths on the full-size
    map (1024 RoIs over 2 images): forward and pixel-owner backward within the bound of float64;
    whether they are bit-identical to the default 256 lanes is reported."""
    from chainer_mask_rcnn_amd import functions as Fn
    rng = np.random.RandomState(3)
    N, Hm, Wm, R = 2, 50, 84, 1024
    x = torch.randn((N, C, Hm, Wm), device=dev).contiguous(memory_format=torch.channels_last)
    y1 = rng.uniform(0, 700, R)
    x1 = rng.uniform(0, 1200, R)
    rois = np.stack([np.repeat(np.arange(N), R // N), x1, y1, x1 + rng.uniform(8, 400, R),
                     y1 + rng.uniform(8, 300, R)], 1).astype(np.float32)
    rois_t = torch.tensor(rois, device=dev)
    gy = torch.randn((R, C, 14, 14), device=dev).contiguous(memory_format=torch.channels_last)

    def run():
        xt = x.clone().requires_grad_(True)
        y = Fn.roi_align_2d(xt, rois_t, 14, 14, 1 / 16.)
        y.backward(gy)
        torch.cuda.synchronize()
        return y.detach().clone(), xt.grad.clone()

    base = run()
    same = {}
    for lanes in (64, 128, 192):
        chk = launch_ref.LaunchChecker()
        with monkeypatch.context() as m:
            chk.install(m)
            try:
                _lib.set_tuning('roi_fwd_lanes', lanes)
                _lib.set_tuning('roi_bwd_lanes', lanes)
                got = run()
            finally:
                _lib.set_tuning('roi_fwd_lanes', 0)
                _lib.set_tuning('roi_bwd_lanes', 0)
        _report('ROIAlign C=%d lanes=%d' % (C, lanes), chk)
        chk.assert_clean()
        assert chk.stats, 'no ROIAlign launch was checked'
        same[lanes] = (torch.equal(got[0], base[0]), torch.equal(got[1], base[1]))
    print('bit-identical to 256 lanes (forward, backward): %s' % same)


TARGET_ENTRY_POINTS = ('mrcnn_bbox_iou_argmax', 'mrcnn_anchor_labels', 'mrcnn_anchor_targets_finish',
                       'mrcnn_proposal_targets_gather', 'mrcnn_mask_targets')


@pytest.mark.parametrize('n_gt', [8, 100])
def test_device_targets_launches_at_full_size(shipped, monkeypatch, n_gt):
    """The headline step's forward with chain.device_targets: the five target entry points of
    csrc/targets.hip under their references (64 260 anchors, 2 000 + G candidates, 512 RoIs per
    image, 800 x 1333 masks), once with host masks and once with device masks (only then does
    mrcnn_mask_targets run), and the same sampled RoIs, labels, mask / RPN targets and np.random
    position as the host creators.  n_gt = 100: a crowded COCO image."""
    import random
    dev = shipped
    random.seed(0)
    np.random.seed(0)
    torch.manual_seed(0)
    imgs, bboxes, labels, masks, scales = bench.synthetic_batch(np.random.RandomState(0), BATCH, H, W,
                                                                n_gt=n_gt)
    model, chain, opt, _ = bench.build_trainer(50, dev, 1, BATCH, defer=5)
    chain.mask_branch_fg_only = True
    x = torch.tensor(imgs, device=dev).contiguous(memory_format=torch.channels_last)
    out = {}
    for mode in ('host', 'device', 'device-masks'):
        chain.device_targets = mode != 'host'
        mm = masks if mode != 'device-masks' else [torch.tensor(m, device=dev) for m in masks]
        chk = launch_ref.LaunchChecker(only=TARGET_ENTRY_POINTS)
        with monkeypatch.context() as m:
            chk.install(m)
            np.random.seed(123)
            with torch.no_grad():
                chain(x, bboxes, labels, mm, scales)
            torch.cuda.synchronize()
        t = chain.last_targets
        out[mode] = ({k: t[k].cpu().numpy() for k in ('sample_rois', 'gt_roi_labels', 'gt_roi_masks',
                                                       'gt_rpn_labels')},
                     np.random.randint(0, 2 ** 31 - 1))
        del mm
        _report('device targets, n_gt %d, %s' % (n_gt, mode), chk)
        chk.assert_clean()
        expect = {} if mode == 'host' else {
            'mrcnn_bbox_iou_argmax': 2 * BATCH, 'mrcnn_anchor_labels': BATCH,
            'mrcnn_anchor_targets_finish': BATCH, 'mrcnn_proposal_targets_gather': BATCH}
        if mode == 'device-masks':
            expect['mrcnn_mask_targets'] = BATCH
        assert dict(chk.launches) == expect, (mode, dict(chk.launches))
        assert set(chk.stats) == set(expect)
    chain.device_targets = False
    host = out['host']
    assert host[0]['sample_rois'].shape == (BATCH * 512, 4)
    assert (host[0]['gt_roi_labels'] > 0).sum() > 0 and (host[0]['gt_rpn_labels'] == 1).sum() > 0
    for mode in ('device', 'device-masks'):
        for k, v in host[0].items():
            assert np.array_equal(out[mode][0][k], v), (mode, k)
        assert out[mode][1] == host[1], mode
