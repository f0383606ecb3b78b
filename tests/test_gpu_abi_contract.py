"""The contract of tests/abi_contract.py on the device.

* Wrong dtypes and a CPU tensor among device tensors, on device tensors: under the recorder, which
  never launches a call it has found wrong — a missing guard shows as a recorded crossing, never as
  a kernel reading a buffer as another type.
* Accepted layouts (strided, transposed, the other memory format, offset views), launched for
  real: the same call on a dense copy of the same values gives bit-identical outputs and gradients
  (both runs execute the same kernel on the same values: no tolerance).
* One train step, one predict and one evaluation pass of the small test model under the live
  recorder: every tensor that crosses obeys the rule.
"""
import numpy as np
import pytest
import torch

import abi_contract as A
from chainer_mask_rcnn_amd._lib import MrcnnHipError

pytestmark = pytest.mark.gpu

IDS = [p.name for p in A.PROBES]


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.shape == b.shape and a.dtype == b.dtype \
            and torch.equal(a.detach(), b.detach())
    return np.array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize('p', A.PROBES, ids=IDS)
def test_wrong_dtypes_are_refused_before_the_launch(dev, p):
    """Dry mode on device tensors: nothing is launched for a perturbed dtype."""
    fails, entries = A.dry_sweep(p, dev, kinds=('dtype',))
    assert not fails, '\n'.join(fails)
    assert entries


@pytest.mark.parametrize('p', A.PROBES, ids=IDS)
def test_a_cpu_tensor_among_device_tensors_is_refused(dev, p):
    """Live recorder: the wrapper raises (MrcnnHipError from require_device, TypeError, ValueError,
    or torch's own device-mismatch RuntimeError), or moves the tensor to the device where it
    documents that it accepts host data; a CPU tensor never reaches a launch."""
    args, _ = p.make(dev)
    for name in p.tensors:
        with A.Recorder(dry=False) as rec:
            try:
                p.run(dev, {name: A._like(args[name], args[name].detach().cpu())})
            except A.AbiViolation as e:
                pytest.fail('%s [%s on the CPU]: %s' % (p.name, name, e))
            except (MrcnnHipError, TypeError, ValueError) + p.rejects:
                pass                # refused by the wrapper
            except RuntimeError as e:
                # torch's own refusal of an operation on tensors of two devices
                assert 'device' in str(e), '%s [%s on the CPU]: %r' % (p.name, name, e)
        torch.cuda.synchronize()
        assert not rec.violations(), A.format_crossings(rec.violations())


@pytest.mark.parametrize('p', A.PROBES, ids=IDS)
def test_accepted_layouts_give_the_dense_result(dev, p):
    """Every layout perturbation of every tensor argument that the wrapper accepts == the same
    call on a dense copy, bit for bit, gradients included; whatever crosses obeys the rule.
    An expanded view of an integer operand is left to the dry sweep: it repeats one value, which
    breaks what index operands promise (a permutation, increasing rows) before any layout does."""
    fails, base, _ = A.baseline(p, dev, dry=False)
    assert not fails, '\n'.join(fails)
    torch.cuda.synchronize()
    compared = 0
    for label, replace, _ in A.perturbed_cases(p, dev, kinds=('layout',)):
        if label.endswith('=expand') and not next(iter(replace.values())).is_floating_point():
            continue
        if next(iter(replace)) in p.reroute:
            continue
        dense, _ = p.make(dev)        # (before the call: a function may write its argument in place)
        dense.update({k: A.dense_copy(v) for k, v in replace.items()})
        args, _ = p.make(dev)
        args.update(replace)
        outcome, rec, out = A.run_recorded(p, dev, False, args)
        bad = rec.violations() + A._against_baseline(rec.crossings, base)
        assert not bad, '%s [%s]:\n%s' % (p.name, label, A.format_crossings(bad))
        if outcome.startswith('rejected'):
            continue
        assert outcome == 'ok', '%s [%s]: %s' % (p.name, label, outcome)
        ref_outcome, _, ref = A.run_recorded(p, dev, False, dense)
        assert ref_outcome == 'ok', '%s [%s] on the dense copy: %s' % (p.name, label, ref_outcome)
        got, want = A.flatten_outputs(out), A.flatten_outputs(ref)
        assert len(got) == len(want) and all(_same(g, w) for g, w in zip(got, want)), \
            '%s [%s]: the result differs from the dense copy\'s' % (p.name, label)
        for n in p.tensors:
            g, w = args[n].grad, dense[n].grad
            assert (g is None) == (w is None) and (g is None or _same(g, w)), \
                '%s [%s]: the gradient of %s differs from the dense copy\'s' % (p.name, label, n)
        compared += 1
    torch.cuda.synchronize()
    assert compared or not p.tensors, 'no layout of any argument was accepted'


def test_gradient_layouts_give_the_dense_gradient(dev):
    """The incoming gradient in a strided / expanded / offset layout (``y.sum().backward()`` hands
    an expanded one over) == the contiguous gradient, for every row with a backward."""
    for p in A.PROBES:
        if not p.backward:
            continue
        ref_args, _ = p.make(dev)
        outcome, rec, _ = A.run_recorded(p, dev, False, ref_args)
        assert outcome == 'ok' and not rec.violations(), (p.name, outcome)
        ref = [ref_args[n].grad for n in p.tensors if ref_args[n].grad is not None]
        assert ref, p.name
        for lab in ('cols2', 'transposed', 'offset_elem'):      # these hold the dense values
            args, _ = p.make(dev)
            outcome, rec, _ = A.run_recorded(p, dev, False, args, lab)
            assert outcome == 'ok', (p.name, lab, outcome)
            assert not rec.violations(), '%s [gy=%s]:\n%s' % (p.name, lab, A.format_crossings(rec.violations()))
            got = [args[n].grad for n in p.tensors if args[n].grad is not None]
            assert len(got) == len(ref) and all(_same(g, w) for g, w in zip(got, ref)), (p.name, lab)
    torch.cuda.synchronize()


def test_live_recorder_on_a_train_step_a_predict_and_an_evaluation_pass(dev):
    """The small test model of test_gpu_model.py: everything it hands to the library obeys the
    rule, and the run reaches the entry points the dry sweep leaves to it."""
    import test_gpu_model as TM
    from chainer_mask_rcnn_amd import optimizers
    from chainer_mask_rcnn_amd.utils.evaluations import boxes as B, masks as M, rle
    model, chain, imgs, bboxes, labels, masks = TM._build(dev)
    opt = optimizers.MomentumSGD(lr=0.01, momentum=0.9)
    opt.setup(chain)
    opt.add_hook(optimizers.WeightDecay(1e-4))
    opt.add_hook(optimizers.GradientClipping(10.))
    TM.freeze_like_reference(model, chain)
    np.random.seed(5)
    rng = np.random.RandomState(1)
    with A.Recorder(dry=False) as rec:
        opt.update(chain, torch.tensor(imgs, device=dev), bboxes, labels, masks, [1., 1.])
        opt.flush()
        torch.cuda.synchronize()
        step = set(rec.entries)
        model.score_thresh = 0.0        # random weights: keep some detections to evaluate
        pred_b, pred_m, pred_l, pred_s = model.predict([rng.randint(0, 255, (3, TM.H, TM.W)).astype(np.uint8),
                                                        imgs[1]])
        torch.cuda.synchronize()
        predict = set(rec.entries) - step
        gt_m = [m.astype(bool) for m in masks]
        for pm, gm, pb, gb in zip(pred_m, gt_m, pred_b, bboxes):
            M.mask_iou(pm, gm)
            B.queue_box_ious([pb], [gb], 'voc')
            rle.encode_masks(pm)
        torch.cuda.synchronize()
    assert not rec.violations(), A.format_crossings(rec.violations())
    seen = set(rec.entries)
    assert set(A.LIVE_COVERED) <= seen, sorted(set(A.LIVE_COVERED) - seen)
    for must in ('mrcnn_conv2d_fwd', 'mrcnn_conv_stem_fwd', 'mrcnn_softmax_ce', 'mrcnn_mask_sigmoid_ce',
                 'mrcnn_smooth_l1', 'mrcnn_topk_desc_batched', 'mrcnn_nms_sorted_batched',
                 'mrcnn_roi_align_bwd_ws', 'mrcnn_grad_sumsq', 'mrcnn_sgd_momentum_wd_ctl'):
        assert must in step, must
    for must in ('mrcnn_prepare_image', 'mrcnn_decode_cls_boxes', 'mrcnn_detect_sort', 'mrcnn_detect_compact',
                 'mrcnn_paste_masks'):
        assert must in predict, must
    for must in ('mrcnn_mask_pack', 'mrcnn_mask_intersect', 'mrcnn_box_iou_voc', 'mrcnn_rle_encode'):
        assert must in seen, must
    assert sum(len(b) for b in pred_b) > 0
