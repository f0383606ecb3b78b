"""MaskRCNN base model — same interface as the reference's
/root/reference/chainer_mask_rcnn/models/mask_rcnn.py:110-337 for the hot path
(``__call__``, ``_to_bboxes`` / ``_suppress`` / ``_to_roi_masks``, ``predict``).

Inference post-processing runs on the device: softmax, per-class decode+clip, a batched
per-class stable sort and one batched bit-mask NMS launch for all 80 classes (the
reference loops over classes in Python on CPU copies, :178-202).  ``prepare`` and
``segm_results`` (cv2 resize / paste of the final image-size masks) are host-side image
I/O and are out of the hot-path scope ("next" row f-2); ``predict``
therefore returns the 14x14 per-detection mask probabilities instead of pasted masks.
"""
import numpy as np
import torch

from .. import functions as F
from .. import _lib
from ..functions import proposal_ops as P


class MaskRCNN(torch.nn.Module):

    def __init__(self, extractor, rpn, head, mean, min_size=600, max_size=1000,
                 loc_normalize_mean=(0., 0., 0., 0.),
                 loc_normalize_std=(0.1, 0.1, 0.2, 0.2), detections_per_im=100):
        super(MaskRCNN, self).__init__()
        self.extractor = extractor
        self.rpn = rpn
        self.head = head

        self.mean = mean
        self.min_size = min_size
        self.max_size = max_size
        self.loc_normalize_mean = loc_normalize_mean
        self.loc_normalize_std = loc_normalize_std

        self.nms_thresh = 0.5
        self.score_thresh = 0.05
        # Detectron's test-time options (TEST.SOFT_NMS, TEST.BBOX_VOTE), off by default: set
        # after construction like nms_thresh and score_thresh
        self.soft_nms = None                # None, 'linear' or 'gaussian' (at most 4096 RoIs per image)
        self.soft_nms_thresh = 0.3          # linear: the IoU from which scores decay
        self.soft_nms_sigma = 0.5           # gaussian
        self.soft_nms_min_score = 0.001     # rows decayed below it are dropped
        self.bbox_vote_thresh = None        # None, or the IoU of a vote (Detectron: 0.8)
        # Detectron's test-time augmentation (TEST.BBOX_AUG / TEST.MASK_AUG), off by default: see
        # test_aug_views() and predict_images()
        self.test_aug_h_flip = False        # also run the mirrored image
        self.test_aug_scales = ()           # extra min_size values
        self.test_aug_max_size = None       # the extra scales' max_size; None: the model's
        self.test_aug_scale_h_flip = False  # also run every extra scale mirrored
        self.mask_aug_heur = 'soft_avg'     # 'soft_avg', 'soft_max' or 'logit_avg' (MASK_AUG.HEUR)

        self._detections_per_im = detections_per_im

    @property
    def n_class(self):
        # Total number of classes including the background.
        return self.head.n_class

    def forward(self, x, scales):
        img_size = x.shape[2:]
        h = self.extractor(x)
        rpn_locs, rpn_scores, rois, roi_indices, anchor = self.rpn(h, img_size, scales)
        roi_cls_locs, roi_scores, roi_masks = self.head(h, rois, roi_indices)
        return roi_cls_locs, roi_scores, rois, roi_indices, roi_masks

    # ------------------------------------------------------------------ inference
    def _suppress_queue(self, cls_bbox, prob, n_views=1):
        """Device half of the per-class score threshold + NMS (:178-202) for one image, all
        classes batched: queues the kernels and returns the device results without
        synchronising.  cls_bbox (R, n_class, 4), prob (R, n_class) device tensors.
        With ``soft_nms`` set the Soft-NMS launch stands in the place of the NMS launch, with
        ``bbox_vote_thresh`` set the vote launch follows either; with both off (the default) the
        launches are the reference's rule and nothing else.  ``n_views``: how many test-time
        augmentation views the rows are the union of (for the error message only)."""
        if self.soft_nms is not None and self.soft_nms not in ('linear', 'gaussian'):
            raise ValueError("soft_nms must be None, 'linear' or 'gaussian', got %r"
                             % (self.soft_nms,))
        R = cls_bbox.shape[0]
        if self.soft_nms is not None and R > 4096:
            raise ValueError('soft_nms handles at most 4096 RoIs per image (mrcnn_soft_nms_sorted_'
                             'batched keeps a class in one workgroup), got %d%s'
                             % (R, ' as the union of %d test-time augmentation views' % n_views
                                if n_views > 1 else ''))
        n_fg = self.n_class - 1
        dev = cls_bbox.device
        sorted_boxes = torch.empty((n_fg, max(R, 1), 4), dtype=torch.float32, device=dev)
        sorted_prob = torch.empty((n_fg, max(R, 1)), dtype=torch.float32, device=dev)
        counts = torch.empty((n_fg,), dtype=torch.int32, device=dev)
        ws = _lib.workspace(_lib.load().mrcnn_detect_sort_workspace_bytes(R, self.n_class), dev,
                            'detect')
        _lib.require_device(prob, cls_bbox)
        prob = _lib.dense(prob, torch.float32, '_suppress_queue', 'prob')
        cls_bbox = _lib.dense(cls_bbox, torch.float32, '_suppress_queue', 'cls_bbox', align=True)
        _lib.call('mrcnn_detect_sort', _lib.ptr(prob), _lib.ptr(cls_bbox),
                  R, self.n_class, float(self.score_thresh), _lib.ptr(sorted_boxes),
                  _lib.ptr(sorted_prob), _lib.ptr(counts), _lib.ptr(ws), _lib.stream_ptr())
        undecayed = sorted_prob
        if self.soft_nms is None:
            keep, n_keep = P.nms_sorted_batched(sorted_boxes, counts, self.nms_thresh)
        else:
            # scores decay instead of rows being deleted; the decayed scores go to compact
            keep, n_keep, sorted_prob = P.soft_nms_sorted_batched(
                sorted_boxes, undecayed, counts, self.soft_nms, self.soft_nms_thresh,
                self.soft_nms_sigma, self.soft_nms_min_score)
        if self.bbox_vote_thresh is not None:
            # every kept box becomes the mean of the candidates that overlap it, weighted by
            # their undecayed scores; compact reads the kept rows only
            sorted_boxes = P.box_vote(sorted_boxes, undecayed, counts, keep, n_keep,
                                      self.bbox_vote_thresh)
        # pack the kept rows of all classes on the device: the host then reads one count and
        # D rows instead of four (n_fg, R) arrays
        cap = n_fg * max(R, 1)
        bbox = torch.empty((cap, 4), dtype=torch.float32, device=dev)
        label = torch.empty((cap,), dtype=torch.int32, device=dev)
        score = torch.empty((cap,), dtype=torch.float32, device=dev)
        total = torch.empty((1,), dtype=torch.int32, device=dev)
        _lib.call('mrcnn_detect_compact', _lib.ptr(keep), _lib.ptr(n_keep), _lib.ptr(sorted_boxes),
                  _lib.ptr(sorted_prob), n_fg, max(R, 1) if R else 0, _lib.ptr(bbox), _lib.ptr(label),
                  _lib.ptr(score), _lib.ptr(total), _lib.stream_ptr())
        return bbox, label, score, total

    @staticmethod
    def _suppress_finish(bbox, label, score, total):
        """Host half: read the packed rows back.  Returns host arrays bbox (D,4) f32, label (D,)
        i32, score (D,) f32 ordered by class then by score."""
        d = int(total.item())
        return (bbox[:d].cpu().numpy().astype(np.float32, copy=False),
                label[:d].cpu().numpy().astype(np.int32, copy=False),
                score[:d].cpu().numpy().astype(np.float32, copy=False))

    def _suppress(self, cls_bbox, prob):
        return self._suppress_finish(*self._suppress_queue(cls_bbox, prob))

    def _to_bboxes(self, roi_cls_locs, roi_scores, rois, roi_indices, sizes, scales):
        queued = self._queue_detections(roi_cls_locs, roi_scores, rois, roi_indices, sizes, scales)
        bboxes, labels, scores = [], [], []
        for q in queued:
            bbox, label, score = self._finish_detections(q)
            bboxes.append(bbox)
            labels.append(label)
            scores.append(score)
        return bboxes, labels, scores

    def _queue_detections(self, roi_cls_locs, roi_scores, rois, roi_indices, sizes, scales,
                          bounds=None):
        """Device half of ``_to_bboxes`` for every image, queued without synchronising
        (``bounds``: the per-image row bounds of ``rois`` if the caller already knows them —
        reading ``roi_indices`` back would wait for everything queued so far)."""
        probs = F.softmax(roi_scores.detach())
        roi_cls_locs = roi_cls_locs.detach()
        if roi_cls_locs.stride(1) != 1:
            roi_cls_locs = roi_cls_locs.contiguous()
        import ctypes
        mean = (ctypes.c_double * 4)(*[float(v) for v in self.loc_normalize_mean])
        std = (ctypes.c_double * 4)(*[float(v) for v in self.loc_normalize_std])
        # RoIs are grouped by image, in order (RegionProposalNetwork): one host read gives the
        # slice bounds.  The device work of every image is queued first; the host halves run
        # afterwards while later images' kernels are still executing.
        if bounds is None:
            counts = np.bincount(roi_indices.cpu().numpy().astype(np.int64), minlength=len(sizes))
            bounds = np.concatenate([[0], np.cumsum(counts)])
        queued = []
        for index in range(len(sizes)):
            lo, hi = int(bounds[index]), int(bounds[index + 1])
            # box rows are read as one float4: a slice that starts off a 16-byte boundary is copied
            _lib.require_device(rois, roi_cls_locs)
            roi = _lib.dense(rois[lo:hi], torch.float32, '_queue_detections', 'rois', align=True)
            loc = roi_cls_locs[lo:hi]
            if loc.dtype != torch.float32:
                raise TypeError('_queue_detections: roi_cls_locs must be %s, got %s'
                                % (torch.float32, loc.dtype))
            prob = probs[lo:hi].contiguous()
            R = roi.shape[0]
            cls_bbox = torch.empty((R, self.n_class, 4), dtype=torch.float32, device=roi.device)
            if loc.stride(1) != 1 or loc.stride(0) != loc.shape[1]:
                loc = loc.contiguous()
            _lib.call('mrcnn_decode_cls_boxes', _lib.ptr(roi), _lib.ptr(loc), loc.stride(0),
                      _lib.ptr(cls_bbox), R, self.n_class, float(scales[index]), mean, std,
                      float(sizes[index][0]), float(sizes[index][1]), _lib.stream_ptr())
            queued.append(self._suppress_queue(cls_bbox, prob))
        return queued

    def _finish_detections(self, q):
        """Host half of ``_to_bboxes`` for one image (:247-260)."""
        bbox, label, score = self._suppress_finish(*q)

        bbox_int = np.round(bbox).astype(np.int32)
        bbox_sizes = ((bbox_int[:, 2] - bbox_int[:, 0]) * (bbox_int[:, 3] - bbox_int[:, 1]))
        ok = bbox_sizes > 0
        bbox, label, score = bbox[ok], label[ok], score[ok]

        if self._detections_per_im > 0:
            # literal restatement of models/mask_rcnn.py:255-260 (an argsort
            # permutation compared with a rank threshold).  The reference
            # calls np.argsort with its default (unstable) kind, so the order of EQUAL scores —
            # and with it which of two tied detections survives the cut — is unspecified there;
            # the stable kind used here is one of the orders it can produce.
            indices = np.argsort(score, kind='stable')
            ok = indices >= (len(indices) - self._detections_per_im)
            bbox, label, score = bbox[ok], label[ok], score[ok]
        return bbox, label, score

    def _roi_masks_group(self, h, bboxes, image_ids, scales):
        """Mask-head pass (:279-289) for the detections of the images ``image_ids`` (one head
        launch for the group); returns one device tensor (D_i, n_fg, M, M) per image."""
        n_fg_class, mask_size = self.n_class - 1, self.head.mask_size
        counts = [len(b) for b in bboxes]
        if sum(counts) == 0:
            return [torch.zeros((0, n_fg_class, mask_size, mask_size), device=h.device)
                    for _ in bboxes]
        rois = np.concatenate([b * np.float32(scales[i]) for b, i in zip(bboxes, image_ids)], axis=0)
        idx = np.concatenate([np.full((c,), i, dtype=np.int32) for c, i in zip(counts, image_ids)])
        with torch.no_grad():
            _, _, roi_masks = self.head(h, torch.tensor(rois, dtype=torch.float32, device=h.device),
                                        torch.tensor(idx, device=h.device), pred_bbox=False)
        bounds = np.concatenate([[0], np.cumsum(counts)])
        return [roi_masks[int(bounds[k]):int(bounds[k + 1])] for k in range(len(bboxes))]

    def _to_roi_masks(self, h, bboxes, roi_indices, scales, to_host=True):
        batch_size = h.shape[0]
        bboxes = np.concatenate(bboxes, axis=0)
        n_fg_class = self.n_class - 1
        mask_size = self.head.mask_size
        if bboxes.size == 0:
            if to_host:
                return [np.zeros((0, n_fg_class, mask_size, mask_size), dtype=np.float32)
                        for _ in range(batch_size)]
            return [torch.zeros((0, n_fg_class, mask_size, mask_size), device=h.device)
                    for _ in range(batch_size)]
        with torch.no_grad():
            scales = np.asarray(scales, dtype=np.float32)
            rois = bboxes * scales[roi_indices][:, None]
            rois = torch.tensor(rois, dtype=torch.float32, device=h.device)
            _, _, roi_masks = self.head(
                h, rois, torch.tensor(roi_indices, device=h.device), pred_bbox=False)
        if not to_host:
            idx = torch.tensor(roi_indices, device=h.device)
            return [roi_masks[idx == i] for i in range(batch_size)]
        roi_masks = roi_masks.cpu().numpy()
        return [roi_masks[roi_indices == i] for i in range(batch_size)]

    # ------------------------------------------------------------------ image I/O on device
    def prepare(self, imgs, x_flips=None, min_size=None, max_size=None):
        """models/mask_rcnn.py:152-176 + concat_examples(padding=0): a list of CHW RGB images
        (uint8 or float) -> zero-padded device batch x (N,3,H,W) channels-last, original
        sizes and scales.  The bilinear resize (cv2 INTER_LINEAR rule) and the mean
        subtraction run in one HIP kernel per image; uint8 images are uploaded as they are.
        ``x_flips`` (extension, used by datasets.MaskRCNNTransform): per-image booleans, mirror
        the resized image left-right in the same pass.  ``min_size`` / ``max_size`` (extension, used
        by the test-time augmentation views): in the place of the model's."""
        min_size = self.min_size if min_size is None else min_size
        max_size = self.max_size if max_size is None else max_size
        dev = next(self.parameters()).device
        sizes, scales, outs = [], [], []
        for img in imgs:
            _, H, W = img.shape
            scale = 1.
            if min_size:
                scale = min_size / min(H, W)
            if max_size and scale * max(H, W) > max_size:
                scale = max_size / max(H, W)
            sizes.append((H, W))
            scales.append(scale)
            outs.append((int(np.round(H * scale)), int(np.round(W * scale))))
        N = len(imgs)
        Hm, Wm = max(o[0] for o in outs), max(o[1] for o in outs)
        batch = torch.zeros((N, Hm, Wm, 3), dtype=torch.float32, device=dev)
        mean = (_lib.c_f32 * 3)(*[float(v) for v in np.asarray(self.mean).ravel()])
        for n, img in enumerate(imgs):
            is_u8 = getattr(img, 'dtype', None) == np.uint8
            host = np.ascontiguousarray(img, dtype=np.uint8 if is_u8 else np.float32)
            if dev.type == 'cuda':
                # through pinned memory, asynchronously: a pageable hipMemcpy is staged by the
                # runtime and blocks the calling thread (measured 8-12 ms for 1 MB next to a busy
                # compute stream); torch's pinned-block cache keeps the buffer alive until the
                # copy has run
                stage = torch.empty(host.shape, dtype=torch.uint8 if is_u8 else torch.float32,
                                    pin_memory=True)
                np.copyto(stage.numpy(), host)       # (plain memcpy: no OpenMP team for 1 MB)
                src = stage.to(dev, non_blocking=True)
            else:
                src = torch.as_tensor(host).to(dev)
            flip = bool(x_flips[n]) if x_flips is not None else False
            _lib.call('mrcnn_prepare_image', _lib.ptr(src), int(is_u8), 3, sizes[n][0], sizes[n][1],
                      float(scales[n]), mean, _lib.ptr(batch), Hm, Wm, outs[n][0], outs[n][1], n,
                      int(flip), _lib.stream_ptr())
        return batch.permute(0, 3, 1, 2), sizes, scales

    def _to_masks(self, bboxes, labels, scores, roi_masks, sizes):
        """sigmoid + segm_results (models/mask_rcnn.py:63-107,292-305) on the device:
        per-image (D, im_h, im_w) bool arrays."""
        masks = []
        for bbox, label, roi_mask, size in zip(bboxes, labels, roi_masks, sizes):
            D = len(bbox)
            if D == 0:
                masks.append(np.zeros((0, size[0], size[1]), dtype=bool))
                continue
            from ..functions._layout import nhwc
            _lib.require_device(roi_mask)
            logits = nhwc(roi_mask, torch.float32, '_to_masks', 'roi_masks')
            dev = logits.device
            out = torch.empty((D, size[0], size[1]), dtype=torch.uint8, device=dev)
            label_d = torch.tensor(label, dtype=torch.int32, device=dev)
            bbox_d = torch.tensor(bbox, dtype=torch.float32, device=dev)
            _lib.call('mrcnn_paste_masks', _lib.ptr(logits), _lib.ptr(label_d), _lib.ptr(bbox_d),
                      D, logits.shape[2], logits.shape[1], int(size[0]), int(size[1]),
                      _lib.ptr(out), _lib.stream_ptr())
            masks.append(out.cpu().numpy().astype(bool))
        return masks

    def predict(self, imgs):
        """Detect objects in a list of CHW RGB images (models/mask_rcnn.py:307-337):
        returns (bboxes, masks, labels, scores), per-image lists as the reference."""
        bboxes, roi_masks, labels, scores, sizes = self.predict_images(imgs, masks_to_host=False)
        masks = self._to_masks(bboxes, labels, scores, roi_masks, sizes)
        return bboxes, masks, labels, scores

    # ------------------------------------------------------------------ test-time augmentation
    def test_aug_views(self):
        """The views an image is run through, as (min_size, max_size, flip) in Detectron's order
        (core/test.py:im_detect_bbox_aug): the identity; its mirror with ``test_aug_h_flip``;
        then every extra ``test_aug_scales`` entry (with ``test_aug_max_size``, or the model's
        ``max_size`` if that is None), each followed by its mirror with ``test_aug_scale_h_flip``.
        With nothing configured that is the identity alone, and nothing is augmented.

        Every view has its own proposals, so there is one rule for merging the views' boxes and
        scores, Detectron's UNION heuristic: all candidates of all views go into the one per-class
        suppression (SCORE_HEUR / COORD_HEUR other than UNION need the same boxes in every view,
        which an RPN does not give).  Masks are computed on the final boxes in every view and
        combined by ``mask_aug_heur``.  Aspect-ratio views are not offered.

        Raises ValueError for more than 8 views, a non-positive scale or max size, an unknown
        ``mask_aug_heur``, and ``test_aug_scale_h_flip`` without ``test_aug_scales``."""
        scales = tuple(self.test_aug_scales or ())
        if self.mask_aug_heur not in _lib.MASK_AUG_HEURS:
            raise ValueError('mask_aug_heur must be one of %s, got %r'
                             % (sorted(_lib.MASK_AUG_HEURS), self.mask_aug_heur))
        if any(not s > 0 for s in scales):
            raise ValueError('test_aug_scales must be positive, got %r' % (scales,))
        if self.test_aug_max_size is not None and not self.test_aug_max_size > 0:
            raise ValueError('test_aug_max_size must be positive or None, got %r'
                             % (self.test_aug_max_size,))
        if self.test_aug_scale_h_flip and not scales:
            raise ValueError('test_aug_scale_h_flip needs test_aug_scales')
        views = [(self.min_size, self.max_size, False)]
        if self.test_aug_h_flip:
            views.append((self.min_size, self.max_size, True))
        max_size = self.max_size if self.test_aug_max_size is None else self.test_aug_max_size
        for s in scales:
            views.append((s, max_size, False))
            if self.test_aug_scale_h_flip:
                views.append((s, max_size, True))
        if len(views) > _lib.TEST_AUG_MAX_VIEWS:
            raise ValueError('at most %d test-time augmentation views (mrcnn_decode_cls_boxes_views,'
                             ' mrcnn_mask_aug_combine), got %d' % (_lib.TEST_AUG_MAX_VIEWS, len(views)))
        return views

    def predict_images(self, imgs, masks_to_host=True):
        """``prepare`` + ``predict_prepared`` for a list of CHW RGB images: returns (bboxes,
        roi_mask_logits, labels, scores, sizes), the first four as ``predict_prepared`` returns
        them.  With no test-time augmentation configured (``test_aug_views()`` is the identity)
        that is all it does.  Otherwise every view is prepared and run through the extractor, the
        RPN and the box heads; per image the views' candidates are decoded into one union in the
        image frame (mrcnn_decode_cls_boxes_views) which the usual suppression decides, Soft-NMS
        and box voting included; the mask head then runs on the final boxes in every view and the
        views' maps are combined by ``mask_aug_heur`` (mrcnn_mask_aug_combine)."""
        views = self.test_aug_views()
        if len(views) == 1:
            x, sizes, scales = self.prepare(imgs)
            return self.predict_prepared(x, scales, sizes, masks_to_host=masks_to_host) + (sizes,)
        from .. import optimizers
        from ..datasets.transforms import flip_bbox
        from ..functions import aug_merge
        optimizers.flush_all()
        was_training = self.training
        self.eval()
        try:
            n_img, n_views = len(imgs), len(views)
            flips = [flip for _, _, flip in views]
            passes = []
            with torch.no_grad():
                for min_size, max_size, flip in views:
                    x, sizes, scales = self.prepare(imgs, x_flips=[flip] * n_img,
                                                    min_size=min_size, max_size=max_size)
                    h, rois, _, bounds, locs, roi_scores = self._box_heads(x, scales)
                    if locs.stride(1) != 1:
                        locs = locs.contiguous()
                    passes.append((h, scales, rois, bounds, locs, F.softmax(roi_scores)))
            queued = []
            for i in range(n_img):
                recs, probs = [], []
                for (_, scales, rois, bounds, locs, prob), flip in zip(passes, flips):
                    lo, hi = int(bounds[i]), int(bounds[i + 1])
                    recs.append((rois[lo:hi], locs[lo:hi], scales[i], flip))
                    probs.append(prob[lo:hi])
                cls_bbox = aug_merge.decode_cls_boxes_views(
                    recs, self.n_class, self.loc_normalize_mean, self.loc_normalize_std, sizes[i])
                queued.append(self._suppress_queue(cls_bbox, torch.cat(probs, dim=0),
                                                   n_views=n_views))
            # the groups of predict_prepared: a group's boxes are made final, then its mask passes
            # (one head launch per view) and the combine of each of its images are queued
            n_groups = 2 if n_img >= 4 else 1
            per = -(-n_img // n_groups)
            bboxes, labels, scores, roi_masks = [], [], [], []
            for g0 in range(0, n_img, per):
                ids = list(range(g0, min(g0 + per, n_img)))
                for i in ids:
                    b, l, s = self._finish_detections(queued[i])
                    bboxes.append(b)
                    labels.append(l)
                    scores.append(s)
                per_view = []
                for (h, scales, _, _, _, _), flip in zip(passes, flips):
                    # the final boxes in the view's frame: mirrored about the original width, then
                    # scaled by _roi_masks_group as in the plain path
                    boxes = [flip_bbox(bboxes[i], sizes[i], x_flip=True) if flip else bboxes[i]
                             for i in ids]
                    per_view.append(self._roi_masks_group(h, boxes, ids, scales))
                for k in range(len(ids)):
                    roi_masks.append(aug_merge.mask_aug_combine([m[k] for m in per_view], flips,
                                                                self.mask_aug_heur))
            if masks_to_host:
                roi_masks = self._masks_to_host(roi_masks, h.device)
        finally:
            self.train(was_training)
        return bboxes, roi_masks, labels, scores, sizes

    def _box_heads(self, x, scales):
        """The first half of prediction on a prepared batch: extractor -> rpn.propose -> the box
        heads, one image's proposals at a time.  Returns (h, rois, roi_indices, bounds,
        roi_cls_locs, roi_scores); bounds: the per-image row bounds of rois, on the host."""
        h = self.extractor(x)
        proposals = self.rpn.propose(h, x.shape[2:], scales)
        rois, roi_indices = proposals.rois, proposals.roi_indices
        # one image's proposals at a time: keeps every activation below the 2 GiB
        # buffer-addressing limit of the conv kernels (8 x 1000 RoIs would not fit)
        # (rois are grouped by image in order and the RPN call knows their counts on the
        # host: a boolean mask per image would synchronise eight times and leave the GPU
        # idle while the host queues the next head)
        bounds = np.concatenate([[0], np.cumsum(proposals.counts)])
        locs, scs = [], []
        for i in range(x.shape[0]):
            lo, hi = int(bounds[i]), int(bounds[i + 1])
            l_i, s_i, _ = self.head(h, rois[lo:hi], roi_indices[lo:hi], pred_mask=False)
            locs.append(l_i)
            scs.append(s_i)
        return h, rois, roi_indices, bounds, torch.cat(locs, dim=0), torch.cat(scs, dim=0)

    @staticmethod
    def _masks_to_host(roi_masks, device):
        """(N x <=100 x 80 x 14 x 14 floats: ~50 MB for a batch of 8) through pinned host memory,
        all copies queued before the one synchronisation."""
        host = [torch.empty(m.shape, dtype=m.dtype, pin_memory=True) for m in roi_masks]
        for h_, m in zip(host, roi_masks):
            h_.copy_(m, non_blocking=True)
        torch.cuda.current_stream(device).synchronize()
        return [h_.numpy() for h_ in host]

    def predict_prepared(self, x, scales, sizes, masks_to_host=True, return_intermediates=False):
        """The device part of ``predict`` (:311-335) on an already prepared, zero-padded
        batch x (N,3,H,W) with per-image ``scales`` and original ``sizes`` (H,W).

        Returns (bboxes, roi_mask_logits, labels, scores): per-image lists of host arrays;
        roi_mask_logits[i] is (D_i, n_fg_class, 14, 14).  ``return_intermediates`` appends a
        dict with the head outputs the detections were computed from (``roi_cls_locs``,
        ``roi_scores``, ``rois``, ``roi_indices`` device tensors, ``feature_shape``)."""
        from .. import optimizers
        optimizers.flush_all()             # no parameter update may be pending while predicting
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad():
                h, rois, roi_indices, bounds, roi_cls_locs, roi_scores = self._box_heads(x, scales)
            # Detections: every image's device work is queued first; the host halves then run
            # group by group and each group's mask-head pass is launched as soon as its
            # boxes are final, so the GPU computes masks while the host finishes the next
            # group (rows of the head are independent: same values as one pass over all).
            # (the row bounds are already on the host: the detection kernels queue up right
            # behind the heads instead of after a read-back that drains the GPU)
            queued = self._queue_detections(roi_cls_locs, roi_scores, rois, roi_indices,
                                            sizes, scales, bounds=bounds)
            n_img = len(queued)
            n_groups = 2 if n_img >= 4 else 1
            per = -(-n_img // n_groups)
            bboxes, labels, scores, roi_masks = [], [], [], []
            for g0 in range(0, n_img, per):
                ids = list(range(g0, min(g0 + per, n_img)))
                for i in ids:
                    b, l, s = self._finish_detections(queued[i])
                    bboxes.append(b)
                    labels.append(l)
                    scores.append(s)
                roi_masks += self._roi_masks_group(h, [bboxes[i] for i in ids], ids, scales)
            if masks_to_host:
                roi_masks = self._masks_to_host(roi_masks, x.device)
        finally:
            self.train(was_training)
        if return_intermediates:
            return bboxes, roi_masks, labels, scores, dict(
                roi_cls_locs=roi_cls_locs, roi_scores=roi_scores, rois=rois,
                roi_indices=roi_indices, feature_shape=tuple(h.shape))
        return bboxes, roi_masks, labels, scores
