"""MaskRCNNTrainChain — same interface and call sequence as the reference's
/root/reference/chainer_mask_rcnn/models/mask_rcnn_train_chain.py:25-189.

forward(imgs, bboxes, labels, masks, scales) -> scalar loss (sum of the five losses);
the six reported scalars are kept in ``self.report`` (device tensors, no sync) as the
reference reports them through chainer.reporter (:182-188).
"""
import collections
import time

import numpy as np
import torch

from .. import functions as F
from ..functions.conv import SparseRows
from ..functions.roi_align_2d import spatial_order
from ..streams import copy_stream      # (the benchmark imports it from here)
from .utils import AnchorTargetCreator
from .utils import ProposalTargetCreator


_POOL = None

_NP_OF = {torch.float32: np.float32, torch.int32: np.int32, torch.int64: np.int64,
          torch.uint8: np.uint8}


class _PinnedRing(object):
    """Pinned host staging buffers for ``_upload``: a buffer is reused once the copy that read it
    has completed (its event), so the host never waits for a copy and never for the copy stream's
    other work (the input pipeline's next-batch upload shares that stream)."""

    MAX_BYTES = 256 << 20        # pinned bytes the ring may hold (buffers in flight included)

    def __init__(self):
        import threading
        self.lock = threading.Lock()
        self.free = []           # [(buffer, event of its last copy or None)], oldest first
        self.total = 0           # bytes of every live buffer: the free list + those handed out

    def take(self, nbytes):
        with self.lock:
            for i, (buf, ev) in enumerate(self.free):
                if buf.numel() >= nbytes and (ev is None or ev.query()):
                    return self.free.pop(i)[0]
            size = max(int(nbytes), 1 << 16)
            # at the cap: wait for the OLDEST copy and recycle / release its buffer instead of
            # growing (the copy stream is backed up; pinned memory must stay bounded)
            while self.free and self.total + size > self.MAX_BYTES:
                buf, ev = self.free.pop(0)
                if ev is not None:
                    ev.synchronize()
                if buf.numel() >= nbytes:
                    return buf
                self.total -= buf.numel()
            self.total += size
        return torch.empty(size, dtype=torch.uint8).pin_memory()

    def give(self, buf, ev):
        with self.lock:
            self.free.append((buf, ev))
            if len(self.free) > 16:      # drop the smallest finished one
                done = [i for i, (b, e) in enumerate(self.free) if e is None or e.query()]
                if done:
                    self.total -= self.free.pop(min(done, key=lambda i: self.free[i][0].numel()))[0].numel()


_PINNED = _PinnedRing()


def _upload(array, dtype, dev):
    """Host array -> device tensor: staged in pinned memory and copied asynchronously on the copy
    stream; the compute stream is ordered after an EVENT recorded right behind this copy — not
    after the whole copy stream, which also carries the input pipeline's next-batch upload and
    its prepare kernels (tools/train_loop.py) — and the host does not wait at all."""
    if dev.type != 'cuda' or dtype not in _NP_OF:
        return torch.tensor(array, dtype=dtype, device=dev)     # (bool, float64, int16, ...: plain path)
    a = np.require(np.asarray(array, dtype=_NP_OF[dtype]), requirements='C')    # keeps a 0-d shape
    side = copy_stream(dev)
    main = torch.cuda.current_stream(dev)
    n = a.nbytes
    with torch.cuda.stream(side):
        t = torch.empty(a.shape, dtype=dtype, device=dev)
        if n > 0:
            stage = _PINNED.take(n)
            stage[:n].numpy()[:] = a.reshape(-1).view(np.uint8)
            t.view(-1).view(torch.uint8).copy_(stage[:n], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(side)
    if n > 0:
        _PINNED.give(stage, ev)
    main.wait_event(ev)
    t.record_stream(main)
    return t


def _pool():
    global _POOL
    if _POOL is None:
        from concurrent.futures import ThreadPoolExecutor
        _POOL = ThreadPoolExecutor(max_workers=4, thread_name_prefix='mrcnn-targets')
    return _POOL


def _upload_many(arrays, dtypes, dev):
    """Several host arrays -> device tensors with ONE copy: the arrays are packed (64-byte
    aligned) into one byte buffer, uploaded through ``_upload`` and returned as typed views."""
    parts, spans, off = [], [], 0
    for a, dt in zip(arrays, dtypes):
        a = np.ascontiguousarray(a, dtype=_NP_OF[dt])
        pad = (-off) % 64
        if pad:
            parts.append(np.zeros(pad, np.uint8))
            off += pad
        parts.append(a.reshape(-1).view(np.uint8))
        spans.append((off, a.nbytes, a.shape, dt))
        off += a.nbytes
    flat = _upload(np.concatenate(parts), torch.uint8, dev)
    return [flat[o:o + n].view(dt).reshape(shape) for o, n, shape, dt in spans]


# what either target path hands ``forward`` (n_fg: a host count; roi_hints: the head's, or None)
StepTargets = collections.namedtuple('StepTargets', (
    'rpn_locs rpn_scores sample_rois sample_roi_indices gt_roi_locs gt_roi_labels gt_roi_masks '
    'gt_rpn_locs gt_rpn_labels roi_cls_locs roi_scores roi_masks mask_rows n_fg roi_hints'))


class MaskRCNNTrainChain(torch.nn.Module):

    def __init__(self, mask_rcnn, rpn_sigma=3., roi_sigma=1.,
                 anchor_target_creator=None, proposal_target_creator=None):
        super(MaskRCNNTrainChain, self).__init__()
        self.mask_rcnn = mask_rcnn
        self.rpn_sigma = rpn_sigma
        self.roi_sigma = roi_sigma
        self.anchor_target_creator = anchor_target_creator or AnchorTargetCreator()
        self.proposal_target_creator = proposal_target_creator or ProposalTargetCreator()
        self.loc_normalize_mean = mask_rcnn.loc_normalize_mean
        self.loc_normalize_std = mask_rcnn.loc_normalize_std
        self.report = {}
        self.features_grad_hook = None     # set by parallel.DataParallelGradSync
        self.mask_branch_fg_only = True
        # run the arithmetic of both target creators as HIP kernels
        # (IoU matrices, label rules, regression targets, mask targets when the ground-truth
        # masks are device tensors); the np.random draws stay on the host, in the reference's
        # order, so the sampled sets are identical.  Off by default: at COCO sizes the host
        # creators already overlap with the GPU and the device path adds read-backs.
        self.device_targets = False
        # The RPN losses ignore all but the sampled anchors, so conv1 of the RPN receives a gradient
        # that is exactly zero outside <= 256 positions per image: its backward runs on those rows
        # only (same sums, 6 % of the dense GEMM work; functions/conv.py SparseRows).  Host-target
        # path only (the positions are known on the host there without a read-back).
        self.sparse_rpn_backward = True
        self.host_timeline = None          # developer aid: list of (label, perf_counter) marks
        # The image batch of the NEXT iteration (device tensor, or a callable returning it / None),
        # when the caller already has it — a resident batch, the input pipeline's prefetched one.
        # Its frozen prefix then runs beside this step's backbone backward.  None: off.
        self.next_imgs = None
        # Ignore regions: a proposal or an anchor is ignored when the image's
        # ignore plane covers MORE than this fraction of its pixels (Detectron's
        # TRAIN.CROWD_FILTER_THRESH).  Read only for images that come with a plane.
        self.crowd_ignore_thresh = 0.7

    def forward(self, imgs, bboxes, labels, masks, scales, ignores=None):
        """imgs (N,3,H,W) device tensor; bboxes / labels / masks: per-image sequences of
        host (or device) arrays (G,4) f32 / (G,) i32 / (G,H,W) i32; scales (N,) floats.  Masks
        that are device tensors (uint8, ``MaskRCNNTransform(device_masks=True)``) are never copied
        back: their mask targets come from ``mrcnn_mask_targets`` in both target paths.

        ``ignores``: per image ``None`` or the ignore plane of its network-size image (int64
        (H_i, Wq_i) device tensor as ``functions.union_plane`` returns it).  For such an
        image one ``mrcnn_box_coverage`` launch over its anchors and proposals and one read-back
        decide which of them the target creators leave out (``crowd_ignore_thresh``).  ``None``, or
        no image with a plane: the launches, draws and loss of a call without the argument.  With a
        list, ``report`` also carries the host counts ``n_ignored_rois`` / ``n_ignored_anchors``."""
        tl = self.host_timeline
        mark = (lambda label: tl.append((label, time.perf_counter()))) if tl is not None \
            else (lambda label: None)
        mark('begin')
        scales = np.asarray([float(s) for s in scales], dtype=np.float32)
        to_np = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        bboxes = [to_np(b).astype(np.float32) for b in bboxes]
        labels = [to_np(l).astype(np.int32) for l in labels]
        dev = imgs.device

        batch_size, _, H, W = imgs.shape
        img_size = (H, W)

        features = self.mask_rcnn.extractor(imgs)
        if self.features_grad_hook is not None and features.requires_grad:
            # fires once the head's and the RPN's backward are both done
            features.register_hook(self.features_grad_hook)
        nxt = self.next_imgs
        if nxt is not None and features.requires_grad and hasattr(self.mask_rcnn.extractor, 'prefetch_frozen'):
            # the NEXT batch's frozen prefix (conv1 .. res2) is queued on a side stream at the
            # moment the backbone's backward begins (models/resnet_extractor.py:prefetch_frozen)
            def _prefetch(g, nxt=nxt, ext=self.mask_rcnn.extractor):
                t = nxt() if callable(nxt) else nxt
                if t is not None:
                    ext.prefetch_frozen(t)
                return None
            features.register_hook(_prefetch)
        # The deterministic half of the RPN target assignment needs only the ground truth:
        # start it on worker threads now (NumPy releases the GIL) so it overlaps with the
        # GPU's extractor/RPN/head work; its np.random draws happen later, in order.
        anchor_h = self.mask_rcnn.rpn.host_anchor(features.shape[2], features.shape[3], dev)
        atc = self.anchor_target_creator
        ptc = self.proposal_target_creator
        device_path = self.device_targets and dev.type == 'cuda' and hasattr(ptc, 'sample_device') \
            and hasattr(atc, 'prepare_device')
        reports_ignored = ignores is not None
        if ignores is not None:
            ignores = list(ignores)
            if len(ignores) != batch_size:
                raise ValueError('ignores must hold one entry (a plane or None) per image, got %d for '
                                 '%d images' % (len(ignores), batch_size))
            if all(p is None for p in ignores):
                ignores = None
        t = (self._forward_device_targets if device_path else self._forward_host_targets)(
            features, img_size, scales, bboxes, labels, masks, anchor_h, mark, ignores)
        rpn_locs = t.rpn_locs.reshape(-1, 4)
        rpn_scores = t.rpn_scores.reshape(-1)
        rpn_loc_loss = F.fast_rcnn_loc_loss(rpn_locs, t.gt_rpn_locs, t.gt_rpn_labels, self.rpn_sigma)
        rpn_cls_loss = F.sigmoid_cross_entropy(rpn_scores, t.gt_rpn_labels)

        # Losses for outputs of the head: the class-specific 4-vector is selected inside
        # the kernel (roi_cls_locs[arange(n), gt_roi_labels], :168-170).
        roi_loc_loss = F.fast_rcnn_loc_loss(
            t.roi_cls_locs, t.gt_roi_locs, t.gt_roi_labels, self.roi_sigma, cls=t.gt_roi_labels)
        roi_cls_loss = F.softmax_cross_entropy(t.roi_scores, t.gt_roi_labels)

        # Losses for outputs of mask branch (:176-178)
        if t.mask_rows is not None:
            roi_mask_loss = F.mask_sigmoid_cross_entropy(
                t.roi_masks, t.gt_roi_labels.index_select(0, t.mask_rows),
                t.gt_roi_masks.index_select(0, t.mask_rows))
        else:
            roi_mask_loss = F.mask_sigmoid_cross_entropy(t.roi_masks, t.gt_roi_labels, t.gt_roi_masks)

        loss = rpn_loc_loss + rpn_cls_loss + roi_loc_loss + roi_cls_loss + roi_mask_loss
        self.report = {'rpn_loc_loss': rpn_loc_loss.detach(),
                       'rpn_cls_loss': rpn_cls_loss.detach(),
                       'roi_loc_loss': roi_loc_loss.detach(),
                       'roi_cls_loss': roi_cls_loss.detach(),
                       'roi_mask_loss': roi_mask_loss.detach(),
                       'loss': loss.detach()}
        if reports_ignored:
            # host counts, logged beside the losses (as main/n_ignored_*) where planes are passed
            self.report['n_ignored_rois'], self.report['n_ignored_anchors'] = self._n_ignored
        mark('losses queued')
        self.last_targets = {'sample_rois': t.sample_rois, 'sample_roi_indices': t.sample_roi_indices,
                             'feature_shape': tuple(features.shape), 'gt_roi_labels': t.gt_roi_labels,
                             'gt_roi_masks': t.gt_roi_masks, 'gt_rpn_labels': t.gt_rpn_labels,
                             'n_rois': int(t.sample_rois.shape[0]), 'roi_hints': t.roi_hints,
                             'n_fg': t.n_fg,                  # host count, no read-back
                             'n_ignored_rois': self._n_ignored[0],
                             'n_ignored_anchors': self._n_ignored[1]}
        if t.roi_hints is not None:
            # read by the benchmark's isolated ROIAlign measurement only, never by this package
            t.sample_rois._mrcnn_order = t.roi_hints.order
        return loss

    def _ignored_boxes(self, ignores, proposals, img_size):
        """Per image ``None`` or ``(ignored anchors (S,) bool, ignored proposals (R_i,) bool)``: one
        ``mrcnn_box_coverage`` launch over cat(anchors, the image's proposals) and one read-back
        for each image that has a plane, none for the others.  The boxes are clipped by the plane's
        own H_i x W_i (the image before batch padding).  Sets ``self._n_ignored`` (host ints)."""
        self._n_ignored = (0, 0)
        if ignores is None:
            return None
        out, n_roi, n_anchor = [], 0, 0
        bounds = np.concatenate([[0], np.cumsum(proposals.counts)]).astype(int)
        S = int(proposals.anchor.shape[0])
        for i, plane in enumerate(ignores):
            if plane is None:
                out.append(None)
                continue
            # (a plane that does not say how many pixels its rows hold: all its words' worth)
            width = getattr(plane, '_mrcnn_width', min(int(img_size[1]), 64 * int(plane.shape[1])))
            rois = proposals.rois[int(bounds[i]):int(bounds[i + 1])].detach()
            counts = F.box_coverage(plane, int(width), torch.cat((proposals.anchor, rois), 0))
            ign = F.ignored_from_counts(counts.cpu().numpy(), self.crowd_ignore_thresh)
            out.append((ign[:S], ign[S:]))
            n_anchor += int(ign[:S].sum())
            n_roi += int(ign[S:].sum())
        self._n_ignored = (n_roi, n_anchor)
        return out

    def _forward_host_targets(self, features, img_size, scales, bboxes, labels, masks, anchor_h, mark,
                              ignores=None):
        """RPN, host target creators (the reference's arrangement, :126-158) and the RoI head."""
        dev = features.device
        to_np = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        atc = self.anchor_target_creator
        atc_jobs = None
        if hasattr(atc, 'prepare') and hasattr(atc, 'finish'):
            atc_jobs = [_pool().submit(atc.prepare, bbox, anchor_h, img_size) for bbox in bboxes]
        # (proposals also as host arrays, in the synchronisation that reads their counts)
        proposals = self.mask_rcnn.rpn.propose(features, img_size, scales, host_copy=True)
        ignored = self._ignored_boxes(ignores, proposals, img_size)
        # (the keyword is passed only where an image has a plane: creators without it keep working)
        ign = lambda i, k: {} if ignored is None or ignored[i] is None else dict(ignore=ignored[i][k])
        # proposal targets: host-side sampling, exactly as the reference (:126-146)
        mark('extractor+rpn queued')
        mark('rois on host')
        ptc = self.proposal_target_creator
        split = hasattr(ptc, 'sample') and hasattr(ptc, 'mask_targets')
        sample_rois, sample_roi_indices = [], []
        gt_roi_locs, gt_roi_labels, gt_roi_masks, mask_jobs = [], [], [], []
        for batch_index, (bbox, label, mask) in enumerate(zip(bboxes, labels, masks)):
            roi = proposals.host_rois[batch_index]
            if split:
                sample_roi, gt_roi_loc, gt_roi_label, job = ptc.sample(roi, bbox, label,
                                                                       **ign(batch_index, 1))
                mask_jobs.append((job, mask, sample_roi))
            else:
                sample_roi, gt_roi_loc, gt_roi_label, gt_roi_mask = \
                    ptc(roi, bbox, label, to_np(mask), **ign(batch_index, 1))
                gt_roi_masks.append(gt_roi_mask)
            mark('ptc.sample')
            sample_rois.append(sample_roi)
            sample_roi_indices.append(np.full((len(sample_roi),), batch_index, dtype=np.int32))
            gt_roi_locs.append(gt_roi_loc)
            gt_roi_labels.append(gt_roi_label)
        up = lambda parts, dt: _upload(np.concatenate(parts, axis=0), dt, dev)
        gt_roi_labels_h = np.concatenate(gt_roi_labels, axis=0)
        n_fg = int((gt_roi_labels_h > 0).sum())
        fg_rows = np.flatnonzero(gt_roi_labels_h > 0) if self.mask_branch_fg_only else np.zeros(0)
        cat = lambda parts: np.concatenate(parts, axis=0)
        # row -> position among the foreground rows (-1: background), for the fused res5 tail
        fg_slot = np.full((len(gt_roi_labels_h),), -1, np.int32)
        fg_slot[fg_rows.astype(np.int64)] = np.arange(len(fg_rows), dtype=np.int32)
        # processing order of the RoIs for the ROIAlign forward (same values in any order)
        roi_order = spatial_order(cat(sample_rois), cat(sample_roi_indices), self.mask_rcnn.head.spatial_scale)
        # the (batch index, x1, y1, x2, y2) rows ROIAlign reads, built here instead of by three small
        # device launches (cat, cast, column permutation) in front of the head
        rois_h, idx_h = cat(sample_rois), cat(sample_roi_indices)
        rois5_h = np.concatenate([idx_h[:, None].astype(np.float32), rois_h[:, [1, 0, 3, 2]]], axis=1)
        (sample_rois, sample_roi_indices, gt_roi_locs, gt_roi_labels, fg_rows_d, fg_slot_d,
         roi_order_d, rois5_d) = _upload_many(
            [rois_h, idx_h, cat(gt_roi_locs), gt_roi_labels_h, fg_rows, fg_slot,
             roi_order, rois5_h],
            [torch.float32, torch.int32, torch.float32, torch.int32, torch.int64, torch.int32,
             torch.int32, torch.float32], dev)

        # The reference runs the mask branch on every sampled RoI (:147-148) although
        # background rows carry all-ignored (-1) mask targets and therefore contribute
        # neither to the loss nor to any gradient.  With
        # ``mask_branch_fg_only`` the branch runs on the foreground rows only: identical loss
        # (same normaliser: the count of non-ignored target pixels) and identical gradients.
        mark('rois sampled')
        mask_rows = None
        if self.mask_branch_fg_only and len(fg_rows) > 0:
            mask_rows = fg_rows_d
        hints = F.RoiHints(rois5_d, roi_order_d, fg_slot_d if mask_rows is not None else None)
        roi_cls_locs, roi_scores, roi_masks = self.mask_rcnn.head(
            features, sample_rois, sample_roi_indices, mask_rows=mask_rows, hints=hints)

        mark('head queued')
        # the head is now queued on the GPU: build the 14x14 mask targets on the host meanwhile
        on_device = lambda m: isinstance(m, torch.Tensor) and m.is_cuda
        if split and any(on_device(mask) for _, mask, _ in mask_jobs):
            # ground-truth masks that already live on the device (MaskRCNNTransform's
            # device_masks) stay there: mrcnn_mask_targets crops them at the foreground rows of
            # the host's sample (it rounds half-even, as np.round does in ptc.sample)
            parts = []
            for job, mask, sample_roi in mask_jobs:
                if on_device(mask):
                    parts.append(self._mask_targets_of_device_mask(job, mask, sample_roi, dev))
                else:
                    parts.append(_upload(ptc.mask_targets(job, to_np(mask)), torch.int32, dev))
            gt_roi_masks = torch.cat(parts, 0)
        else:
            if split:
                gt_roi_masks = [ptc.mask_targets(job, to_np(mask)) for job, mask, _ in mask_jobs]
            gt_roi_masks = up(gt_roi_masks, torch.int32)
        mark('mask targets')

        # RPN targets (host) — after all ProposalTargetCreator calls, as in the reference,
        # so the global np.random stream is consumed in the same order (:150-158).
        gt_rpn_locs, gt_rpn_labels = [], []
        for i, bbox in enumerate(bboxes):
            if atc_jobs is not None:
                gt_rpn_loc, gt_rpn_label = atc.finish(atc_jobs[i].result(), **ign(i, 0))
            else:
                if ign(i, 0):
                    raise ValueError('ignores: the anchor target creator needs prepare / finish')
                gt_rpn_loc, gt_rpn_label = atc(bbox, anchor_h, img_size)
            gt_rpn_locs.append(gt_rpn_loc)
            gt_rpn_labels.append(gt_rpn_label)
        # Both RPN losses ignore every anchor with label -1 (:150-166), so the gradient of the RPN's
        # conv1 output is exactly zero outside the map positions of the sampled anchors: hand
        # those positions to its backward (functions/conv.py: SparseRows; anchor index =
        # position * A + a, utils/bbox.py enumerate_shifted_anchor)
        extra, extra_dt = [], []
        n_rows = 0
        if self.sparse_rpn_backward:
            hw = int(features.shape[2] * features.shape[3])
            pos = [np.flatnonzero(np.asarray(lab) >= 0) // self.mask_rcnn.rpn.n_anchor + i * hw
                   for i, lab in enumerate(gt_rpn_labels)]
            rows_h, lookup_h = SparseRows.host_tables(np.concatenate(pos), hw * len(gt_rpn_labels))
            n_rows = len(rows_h)
            extra, extra_dt = [rows_h, lookup_h], [torch.int32, torch.int32]
        up_all = _upload_many(
            [np.concatenate(gt_rpn_locs, axis=0), np.concatenate(gt_rpn_labels, axis=0)] + extra,
            [torch.float32, torch.int32] + extra_dt, dev)
        gt_rpn_locs, gt_rpn_labels = up_all[0], up_all[1]
        if n_rows > 0:
            proposals.grad_rows.set(up_all[2], up_all[3], n_rows)
        mark('rpn targets')
        return StepTargets(proposals.rpn_locs, proposals.rpn_scores, sample_rois, sample_roi_indices,
                           gt_roi_locs, gt_roi_labels, gt_roi_masks, gt_rpn_locs, gt_rpn_labels,
                           roi_cls_locs, roi_scores, roi_masks, mask_rows, n_fg, hints)

    def _mask_targets_of_device_mask(self, job, mask, sample_roi, dev):
        """(n, M, M) int32 mask targets of one image of the host-target path whose ground-truth
        masks (G, H, W) are a device tensor: only the image's foreground rows of the sampled RoIs
        and their ground-truth indices are uploaded; background rows are -1."""
        from ..functions import target_ops as T
        n, n_fg, _, gt_index = job
        M = self.proposal_target_creator.mask_size
        if n_fg == 0:
            return torch.full((n, M, M), -1, dtype=torch.int32, device=dev)
        roi_d, gt_index_d = _upload_many([sample_roi[:n_fg], gt_index], [torch.float32, torch.int32],
                                         dev)
        m = mask.to(device=dev)
        m = m if m.dtype == torch.uint8 else (m != 0).to(torch.uint8)
        return T.mask_targets(m.contiguous(), roi_d, gt_index_d, n_fg, M, n=n)

    def _forward_device_targets(self, features, img_size, scales, bboxes, labels, masks, anchor_h,
                                mark, ignores=None):
        """Same step with the target arithmetic on the device.  The
        np.random call order is the reference's: every ProposalTargetCreator draw (foreground,
        background, image by image), then every AnchorTargetCreator draw."""
        dev = features.device
        atc, ptc = self.anchor_target_creator, self.proposal_target_creator
        anchor_d = self.mask_rcnn.rpn._anchor(features.shape[2], features.shape[3], dev)[1]
        # RPN label rule: needs only the ground truth -> queued ahead of the RPN itself; the
        # labels travel to pinned host memory asynchronously
        atc_states = [atc.prepare_device(bbox, anchor_d, anchor_h, img_size, upload=_upload)
                      for bbox in bboxes]
        proposals = self.mask_rcnn.rpn.propose(features, img_size, scales)
        ignored = self._ignored_boxes(ignores, proposals, img_size)
        ign = lambda i, k: {} if ignored is None or ignored[i] is None else dict(ignore=ignored[i][k])
        mark('extractor+rpn queued')
        bounds = np.concatenate([[0], np.cumsum(proposals.counts)]).astype(int)
        mark('rois on host')
        s_rois, s_idx, g_locs, g_labels, jobs = [], [], [], [], []
        for i, (bbox, label) in enumerate(zip(bboxes, labels)):
            roi_i = proposals.rois[int(bounds[i]):int(bounds[i + 1])]
            sample_roi, gt_roi_loc, gt_roi_label, job = ptc.sample_device(roi_i, bbox, label,
                                                                          upload=_upload, **ign(i, 1))
            mark('ptc.sample')
            s_rois.append(sample_roi)
            s_idx.append(torch.full((job['n'],), i, dtype=torch.int32, device=dev))
            g_locs.append(gt_roi_loc)
            g_labels.append(gt_roi_label)
            jobs.append(job)
        sample_rois, sample_roi_indices = torch.cat(s_rois, 0), torch.cat(s_idx, 0)
        gt_roi_locs, gt_roi_labels = torch.cat(g_locs, 0), torch.cat(g_labels, 0)
        offs = np.concatenate([[0], np.cumsum([j['n'] for j in jobs])]).astype(int)
        n_fg = int(sum(j['n_fg'] for j in jobs))
        fg_rows = np.concatenate([np.arange(offs[i], offs[i] + j['n_fg']) for i, j in enumerate(jobs)]) \
            if self.mask_branch_fg_only else np.zeros(0, np.int64)
        # ground-truth masks that live on the host: their 14x14 targets are built there (as in
        # the host path) from the foreground boxes, read back BEFORE the head is queued
        host_mask = [not (isinstance(m, torch.Tensor) and m.is_cuda) for m in masks]
        fg_boxes_h = {}
        for i, j in enumerate(jobs):
            if host_mask[i] and j['n_fg'] > 0:
                fg_boxes_h[i] = (j['sample_roi'][:j['n_fg']].cpu().numpy(),
                                 j['gt_index'][:j['n_fg']].cpu().numpy())
        mark('rois sampled')
        mask_rows = None
        if self.mask_branch_fg_only and len(fg_rows) > 0:
            mask_rows = _upload(np.asarray(fg_rows, np.int64), torch.int64, dev)
        roi_cls_locs, roi_scores, roi_masks = self.mask_rcnn.head(
            features, sample_rois, sample_roi_indices, mask_rows=mask_rows)
        mark('head queued')
        from .utils.proposal_target_creator import _mask_targets
        parts = []
        for i, (j, m) in enumerate(zip(jobs, masks)):
            if not host_mask[i]:
                parts.append(ptc.mask_targets_device(j, m))
                continue
            t = -np.ones((j['n'], ptc.mask_size, ptc.mask_size), dtype=np.int32)
            if j['n_fg'] > 0:
                boxes, gt_index = fg_boxes_h[i]
                t[:j['n_fg']] = _mask_targets(np.round(boxes).astype(np.int32), gt_index,
                                              np.asarray(m), ptc.mask_size)
            parts.append(_upload(t, torch.int32, dev))
        gt_roi_masks = torch.cat(parts, 0)
        mark('mask targets')
        g_rl, g_rlab = zip(*[atc.finish_device(st, **ign(i, 0)) for i, st in enumerate(atc_states)])
        gt_rpn_locs, gt_rpn_labels = torch.cat(g_rl, 0), torch.cat(g_rlab, 0)
        mark('rpn targets')
        return StepTargets(proposals.rpn_locs, proposals.rpn_scores, sample_rois, sample_roi_indices,
                           gt_roi_locs, gt_roi_labels, gt_roi_masks, gt_rpn_locs, gt_rpn_labels,
                           roi_cls_locs, roi_scores, roi_masks, mask_rows, n_fg, None)
