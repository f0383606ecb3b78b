"""Instance-segmentation evaluation of a model: the counterpart of the reference's
examples/evaluate_common.py + examples/coco/evaluate.py.

    python tools/evaluate.py --coco-root DIR --split minival --detectron model.pkl
    python tools/evaluate.py --coco-root DIR --snapshot snapshot_model.npz --evaluator voc
    python tools/evaluate.py --synthetic 16            # no dataset: random weights, synthetic images
    python tools/evaluate.py --dataset sbd --sbd-root DIR --snapshot snapshot_model.npz
    python tools/evaluate.py --synthetic 4 --vis       # also writes iteration=best.jpg
    python tools/evaluate.py --log-dir logs/20261016_120000 [--coco-root DIR]   # a tools/train.py run
    python tools/evaluate.py --coco-root DIR --detectron model.pkl --save-results res.json
    python tools/evaluate.py --coco-root DIR --split test-dev --detectron model.pkl --save-results res.json
    python tools/evaluate.py --coco-root DIR --results res.json   # score a results file (no model)
    python tools/evaluate.py --synthetic 16 --iou-types segm,bbox   # box AP beside mask AP
    python tools/evaluate.py --synthetic 16 --iou-types segm,boundary   # Boundary AP beside mask AP
    python tools/evaluate.py --coco-root DIR --detectron model.pkl --soft-nms linear --bbox-vote 0.8
    python tools/evaluate.py --coco-root DIR --detectron model.pkl --test-aug-h-flip \
        --test-aug-scales 500,1000 --test-aug-scale-h-flip --soft-nms linear --bbox-vote 0.8

Runs the evaluator (predicted masks stay on the device; extensions/), prints the report and
the seconds per image spent in prediction and in evaluation, and writes the result as YAML (or
JSON when PyYAML is missing) next to the snapshot as ``<snapshot>.eval_result.yaml``.
``--save-results`` also writes the predictions as a COCO results file (masks as compressed RLE,
encoded on the device); on test-dev, which has no public annotations, it writes the file and
does not score.  ``--results`` scores such a file against the annotations alone.
``--iou-types segm,bbox`` adds the box AP block (``validation/main/bbox/...``: the predicted boxes
against the dataset's boxes, IoU tables from the device); ``--iou-types bbox`` alone skips the mask
work, and with ``--save-results`` then writes a bbox-only file, the detection track's format.
``--iou-types segm,boundary`` adds Boundary AP (``validation/main/boundary/...``: matching on
min(mask IoU, boundary IoU), the boundaries cut from the packed masks on the device, DESIGN.md
section 22); ``--boundary-dilation-ratio R`` sets the boundary width as a fraction of the image
diagonal.
``--soft-nms {linear,gaussian}`` and ``--bbox-vote THRESH`` turn on Detectron's test-time options
(TEST.SOFT_NMS, TEST.BBOX_VOTE; both decided on the device); the values
used are written into the result file as ``postprocessing``.
``--test-aug-h-flip``, ``--test-aug-scales`` (with ``--test-aug-max-size``, ``--test-aug-scale-h-flip``)
and ``--mask-aug-heur`` turn on Detectron's test-time augmentation (TEST.BBOX_AUG / TEST.MASK_AUG;
the views merged on the device); the views run are recorded there too.
"""
import argparse
import json
import os
import pprint
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

POOLING_FUNCS = {'align': 'roi_align_2d', 'pooling': 'roi_pooling_2d', 'resize': 'crop_and_resize'}


class _TimedTarget(object):
    """The model, with the seconds spent in predict_images counted."""

    def __init__(self, model):
        self.model, self.seconds = model, 0.

    def predict_images(self, *a, **k):
        t0 = time.perf_counter()
        out = self.model.predict_images(*a, **k)
        torch.cuda.synchronize()
        self.seconds += time.perf_counter() - t0
        return out


def _iou_types(text):
    types = tuple(t.strip() for t in text.split(',') if t.strip())
    if (not types or any(t not in ('segm', 'bbox', 'boundary') for t in types)
            or len(set(types)) != len(types)):
        raise argparse.ArgumentTypeError("a comma-separated subset of 'segm,bbox,boundary', got %r"
                                         % text)
    return types


def _scale_list(text):
    try:
        scales = tuple(int(t) for t in text.split(',') if t.strip())
    except ValueError:
        scales = ()
    if not scales or any(s <= 0 for s in scales):
        raise argparse.ArgumentTypeError('a comma-separated list of positive integers, got %r' % text)
    return scales


def add_postprocessing_flags(ap):
    """Detectron's test-time options of MaskRCNN (soft_nms, bbox_vote_thresh, test-time
    augmentation): off by default."""
    ap.add_argument('--soft-nms', default=None, choices=['linear', 'gaussian'],
                    help='Soft-NMS in the place of the hard per-class NMS (Detectron TEST.SOFT_NMS): '
                         'scores of overlapping boxes decay instead of the boxes being deleted')
    ap.add_argument('--soft-nms-thresh', type=float, default=None, metavar='IOU',
                    help='linear Soft-NMS: the IoU from which a score decays (model default 0.3); '
                         'needs --soft-nms linear')
    ap.add_argument('--soft-nms-sigma', type=float, default=None, metavar='SIGMA',
                    help='gaussian Soft-NMS sigma (model default 0.5); needs --soft-nms gaussian')
    ap.add_argument('--soft-nms-min-score', type=float, default=None, metavar='SCORE',
                    help='Soft-NMS drops a box once its score has decayed below this (model '
                         'default 0.001); needs --soft-nms')
    ap.add_argument('--bbox-vote', type=float, default=None, metavar='THRESH',
                    help='bounding-box voting (Detectron TEST.BBOX_VOTE, 0.8 there): each kept box '
                         'becomes the score-weighted mean of the candidates with IoU >= THRESH')
    ap.add_argument('--test-aug-h-flip', action='store_true',
                    help='test-time augmentation (Detectron TEST.BBOX_AUG / MASK_AUG): also run the '
                         'mirrored image and pool both views\' candidates into the one suppression')
    ap.add_argument('--test-aug-scales', type=_scale_list, default=None, metavar='S[,S...]',
                    help='test-time augmentation: also run the image at these min sizes '
                         '(e.g. 500,1000)')
    ap.add_argument('--test-aug-max-size', type=int, default=None, metavar='N',
                    help='the max size of the extra scales (default: the model\'s); needs '
                         '--test-aug-scales')
    ap.add_argument('--test-aug-scale-h-flip', action='store_true',
                    help='also run every extra scale mirrored; needs --test-aug-scales')
    ap.add_argument('--mask-aug-heur', default=None, choices=['soft_avg', 'soft_max', 'logit_avg'],
                    help='how the views\' mask maps are combined (Detectron MASK_AUG.HEUR; model '
                         'default soft_avg); needs --test-aug-h-flip or --test-aug-scales')


def check_postprocessing_flags(ap, args, no_model=False):
    """A flag that would be ignored is an error, not a silent no-op."""
    given = [flag for flag, value in (('--soft-nms', args.soft_nms),
                                      ('--soft-nms-thresh', args.soft_nms_thresh),
                                      ('--soft-nms-sigma', args.soft_nms_sigma),
                                      ('--soft-nms-min-score', args.soft_nms_min_score),
                                      ('--bbox-vote', args.bbox_vote)) if value is not None]
    aug = [flag for flag, on in (('--test-aug-h-flip', args.test_aug_h_flip),
                                 ('--test-aug-scales', args.test_aug_scales is not None),
                                 ('--test-aug-max-size', args.test_aug_max_size is not None),
                                 ('--test-aug-scale-h-flip', args.test_aug_scale_h_flip),
                                 ('--mask-aug-heur', args.mask_aug_heur is not None)) if on]
    if no_model and (given or aug):
        ap.error('%s: nothing is predicted when a results file is scored' % ', '.join(given + aug))
    if args.test_aug_scales is None:
        for flag in ('--test-aug-max-size', '--test-aug-scale-h-flip'):
            if flag in aug:
                ap.error('%s given without --test-aug-scales' % flag)
    if args.test_aug_max_size is not None and args.test_aug_max_size <= 0:
        ap.error('--test-aug-max-size must be positive')
    if args.mask_aug_heur is not None and not (args.test_aug_h_flip or args.test_aug_scales):
        ap.error('--mask-aug-heur given without --test-aug-h-flip or --test-aug-scales: one view '
                 'has nothing to combine')
    n_views = (1 + bool(args.test_aug_h_flip)
               + len(args.test_aug_scales or ()) * (1 + bool(args.test_aug_scale_h_flip)))
    if n_views > 8:
        ap.error('%d test-time augmentation views asked for, at most 8 are handled' % n_views)
    if args.soft_nms is None and given and given != ['--bbox-vote']:
        ap.error('%s given without --soft-nms' % ', '.join(f for f in given if f != '--bbox-vote'))
    if args.soft_nms_thresh is not None and args.soft_nms != 'linear':
        ap.error('--soft-nms-thresh is the linear method\'s (got --soft-nms %s)' % args.soft_nms)
    if args.soft_nms_sigma is not None and args.soft_nms != 'gaussian':
        ap.error('--soft-nms-sigma is the gaussian method\'s (got --soft-nms %s)' % args.soft_nms)
    if args.soft_nms_sigma is not None and not args.soft_nms_sigma > 0:
        ap.error('--soft-nms-sigma must be positive')


def apply_postprocessing_flags(model, args):
    """Set the model's attributes from the flags; returns what is in force, for the result file."""
    if getattr(args, 'soft_nms', None):
        model.soft_nms = args.soft_nms
        for flag, attr in (('soft_nms_thresh', 'soft_nms_thresh'), ('soft_nms_sigma', 'soft_nms_sigma'),
                           ('soft_nms_min_score', 'soft_nms_min_score')):
            if getattr(args, flag, None) is not None:
                setattr(model, attr, float(getattr(args, flag)))
    if getattr(args, 'bbox_vote', None) is not None:
        model.bbox_vote_thresh = float(args.bbox_vote)
    used = {'nms_thresh': float(model.nms_thresh), 'score_thresh': float(model.score_thresh),
            'soft_nms': model.soft_nms, 'bbox_vote_thresh': model.bbox_vote_thresh}
    if model.soft_nms:
        used.update(soft_nms_thresh=float(model.soft_nms_thresh),
                    soft_nms_sigma=float(model.soft_nms_sigma),
                    soft_nms_min_score=float(model.soft_nms_min_score))
    if getattr(args, 'test_aug_h_flip', False):
        model.test_aug_h_flip = True
    if getattr(args, 'test_aug_scales', None):
        model.test_aug_scales = tuple(args.test_aug_scales)
        model.test_aug_scale_h_flip = bool(getattr(args, 'test_aug_scale_h_flip', False))
        if getattr(args, 'test_aug_max_size', None) is not None:
            model.test_aug_max_size = int(args.test_aug_max_size)
    if getattr(args, 'mask_aug_heur', None):
        model.mask_aug_heur = args.mask_aug_heur
    views = model.test_aug_views()
    if len(views) > 1:          # (without augmentation the dict is as it always was)
        used.update(test_aug_views=[[int(lo), int(hi), bool(flip)] for lo, hi, flip in views],
                    mask_aug_heur=model.mask_aug_heur)
    return used


def _print_result(result):
    """The report: one block as it always was; a segm, a bbox and a boundary block when box AP
    or Boundary AP was asked for."""
    bbox = {k: v for k, v in result.items() if '/bbox/' in k}
    boundary = {k: v for k, v in result.items() if '/boundary/' in k}
    if not bbox and not boundary:
        pprint.pprint(result)
        return
    segm = {k: v for k, v in result.items() if k not in bbox and k not in boundary}
    for name, block in (('segm', segm), ('bbox', bbox), ('boundary', boundary)):
        if block:
            print('%s:' % name)
            pprint.pprint(block)


def _evaluator_kwargs(args):
    """iou_types / boundary_dilation_ratio for the evaluators, only when they differ from the
    defaults."""
    kw = {}
    iou_types = getattr(args, 'iou_types', ('segm',))
    if iou_types != ('segm',):
        kw['iou_types'] = iou_types
    if 'boundary' in iou_types:
        kw['boundary_dilation_ratio'] = getattr(args, 'boundary_dilation_ratio', 0.02)
    return kw


def main():
    ap = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument('--dataset', default='coco', choices=['coco', 'voc', 'sbd'],
                    help='voc (VOC2012) and sbd evaluate the 20-class model of examples/voc/train.py')
    ap.add_argument('--coco-root', default=None, help='COCO-layout directory')
    ap.add_argument('--voc-root', default=None, help='VOCdevkit/VOC2012 directory')
    ap.add_argument('--sbd-root', default=None, help='benchmark_RELEASE/dataset directory of SBD')
    ap.add_argument('--split', default=None, help='default: minival (coco), val (voc, sbd)')
    ap.add_argument('--snapshot', default=None, help='snapshot_model.npz of this package / the reference')
    ap.add_argument('--detectron', default=None, help='Detectron R-50-C4 / R-101-C4 .pkl')
    ap.add_argument('--layers', type=int, default=50, choices=[50, 101])
    ap.add_argument('--pooling-func', default='align', choices=sorted(POOLING_FUNCS))
    ap.add_argument('--evaluator', default=None, choices=['voc', 'coco'],
                    help='default: voc for --dataset voc / sbd, else coco')
    ap.add_argument('--limit', type=int, default=0, help='evaluate the first N images only')
    ap.add_argument('--synthetic', type=int, default=0, help='N synthetic images, no dataset')
    ap.add_argument('--batch', type=int, default=1)
    ap.add_argument('--out', default=None, help='result file (default: next to the weights)')
    ap.add_argument('--vis', action='store_true',
                    help='also write the visual report of the first 9 images as iteration=best.jpg '
                         'next to the result file (examples/evaluate_common.py)')
    ap.add_argument('--log-dir', default=None,
                    help='a tools/train.py output directory: the model from its params.yaml, the '
                         'weights from its snapshot_model.npz (examples/evaluate_common.py); writes '
                         'snapshot_model.npz.eval_result.yaml and iteration=best.jpg there')
    ap.add_argument('--custom-root', default=None, help='VOC-like directory (--log-dir of a custom run)')
    ap.add_argument('--save-results', default=None, metavar='FILE',
                    help='also write the predictions as a COCO results file (COCO only; with '
                         '--split test-dev the file is written and nothing is scored)')
    ap.add_argument('--results', default=None, metavar='FILE',
                    help='score a COCO results file against --coco-root / --split (no model, '
                         'no images needed)')
    ap.add_argument('--iou-types', type=_iou_types, default=('segm',),
                    metavar='segm[,bbox][,boundary]',
                    help='what to score: mask AP (segm), box AP (bbox), Boundary AP (boundary) or '
                         'any of them together; with --results, each type is scored from the file')
    ap.add_argument('--boundary-dilation-ratio', type=float, default=0.02, metavar='R',
                    help='Boundary AP: the boundary width as a fraction of the image diagonal')
    ap.add_argument('--polygon-rule', choices=['pil', 'coco'], default='pil',
                    help="how COCO polygon annotations become ground-truth masks: pil (PIL.ImageDraw, "
                         "the reference's; about one pixel fatter) or coco (COCO's own rule, what "
                         "pycocotools scores against; DESIGN.md section 25).  Also with --results")
    ap.add_argument('--arithmetic', default=None, choices=['fp32', 'split_bf16x3', 'split_bf16x2', 'bf16x1'],
                    help='arithmetic of the convolution GEMMs (functions.conv.set_gemm_arithmetic; default '
                         'split_bf16x3: fp32-accurate; split_bf16x2: 16-bit-class operands; bf16x1: bf16 '
                         'operands; all with fp32 accumulation and fp32 weights)')
    add_postprocessing_flags(ap)
    args = ap.parse_args()
    check_postprocessing_flags(ap, args, no_model=bool(args.results))
    if args.results:
        if args.coco_root is None:
            ap.error('--results needs --coco-root')
        return score_results(args)
    if args.arithmetic is not None:          # (a --log-dir run's own arithmetic is not re-applied: say it here)
        from chainer_mask_rcnn_amd.functions import conv
        conv.set_gemm_arithmetic(args.arithmetic)
    if args.save_results and (args.synthetic or (args.dataset != 'coco' and not args.log_dir)):
        ap.error('--save-results needs COCO data: VOC, SBD and --synthetic have no COCO image or '
                 'category ids')
    if args.save_results and args.evaluator == 'voc':
        ap.error('--save-results needs the coco evaluator')
    if args.log_dir:
        return evaluate_log_dir(args)
    voc = args.dataset in ('voc', 'sbd') and not args.synthetic
    if args.evaluator is None:
        args.evaluator = 'voc' if voc else 'coco'
    if args.split is None:
        args.split = 'val' if voc else 'minival'

    import chainer_mask_rcnn_amd as cmr
    from chainer_mask_rcnn_amd import serializers
    dev = torch.device('cuda:0')

    if args.synthetic:
        import train_loop
        data = train_loop.SyntheticInstances(args.synthetic, seed=1)
        class_names = ['class%d' % i for i in range(80)]
    elif voc:
        if args.dataset == 'voc':
            data = cmr.datasets.VOC2012InstanceSegmentationDataset(args.split, root_dir=args.voc_root)
        else:
            data = cmr.datasets.SBDInstanceSegmentationDataset(args.split, root_dir=args.sbd_root)
        class_names = [str(n) for n in data.class_names]
    else:
        if args.coco_root is None:
            ap.error('--coco-root or --synthetic is required')
        data = cmr.datasets.COCOInstanceSegmentationDataset(
            args.split, root_dir=args.coco_root, use_crowd=True, return_crowd=True,
            return_area=True, polygon_rule=args.polygon_rule)
        class_names = [str(n) for n in data.class_names]
    if args.split == 'test-dev' and not args.save_results:
        ap.error('--split test-dev has no annotations to score: use --save-results FILE')

    torch.manual_seed(0)
    # examples/voc/train.py: 600 / 1000 and anchor scales (4, 8, 16, 32); COCO: 800 / 1333
    size = dict(min_size=600, max_size=1000, anchor_scales=(4, 8, 16, 32)) if voc else dict(
        min_size=800, max_size=1333, anchor_scales=(2, 4, 8, 16, 32))
    model = cmr.models.MaskRCNNResNet(
        n_layers=args.layers, n_fg_class=len(class_names), roi_size=14,
        pooling_func=getattr(cmr.functions, POOLING_FUNCS[args.pooling_func]), **size).to(dev)
    weights = args.snapshot or args.detectron
    if args.snapshot:
        serializers.load_npz(args.snapshot, model)
    elif args.detectron:
        serializers.load_detectron(args.detectron, model, n_layers=args.layers)
    else:
        import bench
        bench.stabilise_synthetic_weights(model)
        with torch.no_grad():                 # random weights: sharpen scores to get detections
            n_class = len(class_names) + 1
            model.head.cls_loc_score.W[4 * n_class:5 * n_class] *= 60.
    model.eval()
    postprocessing = apply_postprocessing_flags(model, args)

    transform = cmr.datasets.MaskRCNNTransform(model, train=False)
    n = len(data) if not args.limit else min(args.limit, len(data))
    batches = ([transform(data[j]) for j in range(i, min(i + args.batch, n))]
               for i in range(0, n, args.batch))

    target = _TimedTarget(model)
    cls = (cmr.extensions.InstanceSegmentationVOCEvaluator if args.evaluator == 'voc'
           else cmr.extensions.InstanceSegmentationCOCOEvaluator)
    kw = {'use_07_metric': True} if args.evaluator == 'voc' else {}
    writer = _results_writer(args, data)
    if writer is not None:
        kw['results_sink'] = writer
    kw.update(_evaluator_kwargs(args))
    evaluator = cls(batches, target, label_names=class_names, **kw)
    t0 = time.perf_counter()
    if args.split == 'test-dev':
        evaluator.collect()
        result = {}
        print('test-dev has no public annotations: results written to %s, not scored'
              % args.save_results)
    else:
        result = evaluator.evaluate()
    total = time.perf_counter() - t0
    if writer is not None:
        writer.close()
        print('Saved results: %s (%d entries, %d images)'
              % (args.save_results, writer.n_entries, len(writer.image_ids)))
    result = {k: float(v) for k, v in result.items()}
    timing = {'images': n, 'predict_s_per_image': target.seconds / n,
              'eval_s_per_image': (total - target.seconds) / n}
    _print_result(result)
    print('timing:', json.dumps(timing))

    out = args.out or ((weights + '.eval_result.yaml') if weights else
                       'synthetic.eval_result.yaml')
    payload = {'result': result, 'timing': timing, 'evaluator': args.evaluator,
               'weights': weights, 'split': None if args.synthetic else args.split,
               'postprocessing': postprocessing}
    if args.save_results:
        payload['results_file'] = os.path.abspath(args.save_results)
    try:
        import yaml
        with open(out, 'w') as f:
            yaml.safe_dump(payload, f, default_flow_style=False)
    except ImportError:
        out = os.path.splitext(out)[0] + '.json'
        with open(out, 'w') as f:
            json.dump(payload, f, indent=1)
    print('Saved evaluation:', out)

    if args.vis:
        vis_dir = os.path.dirname(os.path.abspath(out))

        class DummyTrainer(object):
            class DummyUpdater(object):
                iteration = 'best'
            updater = DummyUpdater()
            out = vis_dir

        vis = ([transform(data[j])] for j in range(min(9, n)))
        visualizer = cmr.extensions.InstanceSegmentationVisReport(
            vis, model, label_names=class_names, file_name='iteration=%s.jpg', copy_latest=False)
        visualizer(trainer=DummyTrainer())
        print('Saved visualization:', os.path.join(DummyTrainer.out, 'iteration=best.jpg'))


def _results_writer(args, data):
    """The COCO results file of --save-results: a streaming writer that maps the i-th evaluated
    image to the dataset's image id and labels to its category ids."""
    path = getattr(args, 'save_results', None)      # absent from callers' own namespaces
    if not path:
        return None
    if not (hasattr(data, 'img_ids') and hasattr(data, 'class_id_to_cat_id')):
        raise SystemExit('--save-results needs a COCO dataset (image and category ids)')
    from chainer_mask_rcnn_amd.utils.evaluations.coco_results import ResultsWriter
    return ResultsWriter(path, data.img_ids, data.class_id_to_cat_id)


def score_results(args):
    """--results: score a COCO results file against the annotations of --coco-root / --split
    (the first --limit images); writes ``<results>.eval_result.yaml`` (or --out)."""
    import chainer_mask_rcnn_amd as cmr
    from chainer_mask_rcnn_amd.utils.evaluations.coco_results import eval_coco_results
    split = args.split or 'minival'
    if split == 'test-dev':
        raise SystemExit('test-dev has no public annotations: its results are scored by the '
                         'COCO evaluation server')
    data = cmr.datasets.COCOInstanceSegmentationDataset(
        split, root_dir=args.coco_root, use_crowd=True, return_crowd=True, return_area=True,
        polygon_rule=getattr(args, 'polygon_rule', 'pil'))
    torch.cuda.set_device(0)
    t0 = time.perf_counter()
    result = {}
    for iou_type in getattr(args, 'iou_types', ('segm',)):
        result.update(eval_coco_results(args.results, data, limit=args.limit or None,
                                        label_names=[str(n) for n in data.class_names],
                                        iou_type=iou_type,
                                        **({'dilation_ratio': getattr(
                                            args, 'boundary_dilation_ratio', 0.02)}
                                           if iou_type == 'boundary' else {})))
    seconds = time.perf_counter() - t0
    result = {k: float(v) for k, v in result.items()}
    _print_result(result)
    n = len(data) if not args.limit else min(args.limit, len(data))
    timing = {'images': n, 'eval_s_per_image': seconds / max(n, 1)}
    print('timing:', json.dumps(timing))
    out = args.out or (args.results + '.eval_result.yaml')
    payload = {'result': result, 'timing': timing, 'evaluator': 'coco', 'split': split,
               'results_file': os.path.abspath(args.results)}
    try:
        import yaml
        with open(out, 'w') as f:
            yaml.safe_dump(payload, f, default_flow_style=False)
    except ImportError:
        out = os.path.splitext(out)[0] + '.json'
        with open(out, 'w') as f:
            json.dump(payload, f, indent=1)
    print('Saved evaluation:', out)
    return result


def evaluate_log_dir(args):
    """examples/evaluate_common.py: the test split of the run's dataset (dataset roots from the
    command line, else from params.yaml), the model as params.yaml describes it with the weights of
    snapshot_model.npz, the visual report of the first 9 test images as iteration=best.jpg and the
    evaluator's result as snapshot_model.npz.eval_result.yaml, both in the log directory."""
    import yaml
    import chainer_mask_rcnn_amd as cmr
    import train as train_tool
    with open(os.path.join(args.log_dir, 'params.yaml')) as f:
        params = yaml.safe_load(f)
    print('Training config:')
    pprint.pprint(params)
    run = argparse.Namespace(**params)
    for key in ('coco_root', 'sbd_root', 'custom_root'):
        if getattr(args, key, None):
            setattr(run, key, getattr(args, key))
    test_data, evaluator_type = train_tool.test_dataset(run)
    class_names = list(params['class_names'])
    pretrained_model = os.path.join(args.log_dir, 'snapshot_model.npz')
    print('Using pretrained_model:', pretrained_model)
    dev = torch.device('cuda:0')
    model = cmr.models.MaskRCNNResNet(
        n_layers=int(params['model'][len('resnet'):]), n_fg_class=len(class_names),
        pretrained_model=pretrained_model,
        pooling_func=getattr(cmr.functions, POOLING_FUNCS[params['pooling_func']]),
        anchor_scales=tuple(params['anchor_scales']),
        mean=tuple(params.get('mean', (123.152, 115.903, 103.063))),
        min_size=params['min_size'], max_size=params['max_size'],
        roi_size=params['roi_size']).to(dev)
    model.eval()
    postprocessing = apply_postprocessing_flags(model, args)
    transform = cmr.datasets.MaskRCNNTransform(model, train=False)

    class DummyTrainer(object):
        class DummyUpdater(object):
            iteration = 'best'
        updater = DummyUpdater()
        out = args.log_dir

    print('Visualizing...')
    vis = ([transform(test_data[j])] for j in range(min(9, len(test_data))))
    visualizer = cmr.extensions.InstanceSegmentationVisReport(
        vis, model, label_names=class_names, file_name='iteration=%s.jpg', copy_latest=False)
    visualizer(trainer=DummyTrainer())
    print('Saved visualization:', os.path.join(args.log_dir, 'iteration=best.jpg'))

    print('Evaluating...')
    n = len(test_data) if not args.limit else min(args.limit, len(test_data))
    batches = ([transform(test_data[j])] for j in range(n))
    writer = _results_writer(args, test_data)
    if writer is not None and evaluator_type != 'coco':
        raise SystemExit('--save-results needs the coco evaluator')
    kw = _evaluator_kwargs(args)
    if evaluator_type == 'voc':
        evaluator = cmr.extensions.InstanceSegmentationVOCEvaluator(
            batches, model, use_07_metric=True, label_names=class_names, **kw)
    else:
        evaluator = cmr.extensions.InstanceSegmentationCOCOEvaluator(
            batches, model, label_names=class_names, results_sink=writer, **kw)
    result = {k: float(v) for k, v in evaluator.evaluate().items()}
    yaml_file = pretrained_model + '.eval_result.yaml'
    # one dump: the metrics as they always were, then whatever else describes the run
    payload = dict(result)
    if (postprocessing['soft_nms'] or postprocessing['bbox_vote_thresh'] is not None
            or 'test_aug_views' in postprocessing):
        payload['postprocessing'] = postprocessing
    if writer is not None:
        writer.close()
        print('Saved results: %s (%d entries)' % (writer.path, writer.n_entries))
        payload['results_file'] = os.path.abspath(writer.path)
    with open(yaml_file, 'w') as f:
        yaml.safe_dump(payload, f, default_flow_style=False)
    print('Saved evaluation:', yaml_file)
    _print_result(result)
    return result


if __name__ == '__main__':
    main()
