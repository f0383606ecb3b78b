"""InstanceSegmentationVisReport — the reference's chainer_mask_rcnn/extensions/
instance_segmentation_vis_report.py.

Per image, the ground truth and the predictions with a score of at least 0.7 are drawn onto
the image (utils.draw_instance_bboxes, labels + 1 with '__background__' prepended to the
names), the two panels are stacked, and the panels of the first rows * cols images are tiled
into one mosaic (utils.get_tile_image) that is written as a JPEG.  Everything up to the mosaic
stays on the device: ``predict_images(masks_to_host=False)`` -> packed paste
of the kept detections -> drawing in place -> tiling; the mosaic is the only large copy back to
the host.  Prediction stops once rows * cols images are drawn.
"""
import os
import os.path as osp
import shutil

import numpy as np
import torch

from ..utils import visualizations as V
from ..utils.evaluations import masks as M
from .instance_segmentation_evaluators import _batches

SCORE_THRESH = 0.7


class InstanceSegmentationVisReport(object):

    def __init__(self, iterator, target, label_names,
                 file_name='visualizations/iteration=%08d.jpg', shape=(3, 3), copy_latest=True):
        self.iterator = iterator
        self.target = target
        self.label_names = np.asarray(label_names)
        self.file_name = file_name
        self._shape = shape
        self._copy_latest = copy_latest

    def _panels(self):
        """Device (2H, W, 3) uint8 panels, ground truth above predictions, one per image."""
        target = self.target
        label_names = np.hstack((['__background__'], self.label_names))
        n_class = len(label_names)
        n_max = self._shape[0] * self._shape[1]
        vizs = []
        for batch in _batches(self.iterator):
            batch = list(batch)
            if not batch:
                continue
            bboxes, roi_masks, labels, scores, sizes = target.predict_images(
                [ex[0] for ex in batch], masks_to_host=False)
            dev = roi_masks[0].device
            for j, ex in enumerate(batch[:n_max - len(vizs)]):
                img, gt_bbox, gt_label, gt_mask = ex[:4]
                img = np.asarray(img).transpose(1, 2, 0)          # CHW -> HWC
                assert img.dtype == np.uint8
                gt_label = np.asarray(gt_label)
                H, W = sizes[j]
                img_d = torch.from_numpy(np.ascontiguousarray(img)).to(dev)
                gt_viz = img_d.clone()
                V.draw_instances_device(gt_viz, np.asarray(gt_bbox).reshape(-1, 4), gt_label + 1,
                                        n_class, masks=np.asarray(gt_mask).astype(bool),
                                        captions=label_names[gt_label + 1], bg_class=0)
                keep = np.flatnonzero(scores[j] >= SCORE_THRESH)
                p_bbox, p_label, p_score = bboxes[j][keep], labels[j][keep], scores[j][keep]
                p_masks = M.paste_packed(
                    roi_masks[j][torch.from_numpy(keep).to(dev)], p_label, p_bbox, (H, W))
                captions = ['{:s} {:.1%}'.format(l_name, p)
                            for p, l_name in zip(p_score, label_names[p_label + 1])]
                pred_viz = img_d
                V.draw_instances_device(pred_viz, p_bbox, p_label + 1, n_class, masks=p_masks,
                                        captions=captions, bg_class=0)
                vizs.append(torch.cat([gt_viz, pred_viz], 0))
            if len(vizs) >= n_max:
                break
        return vizs

    def render(self):
        """The report's mosaic as a host (H, W, 3) uint8 RGB array."""
        return V.tile_images_device(self._panels(), self._shape).cpu().numpy()

    def __call__(self, trainer):
        from PIL import Image
        viz = self.render()
        file_name = osp.join(trainer.out, self.file_name % trainer.updater.iteration)
        d = osp.dirname(file_name)
        if d:
            os.makedirs(d, exist_ok=True)
        Image.fromarray(viz).save(file_name, format='JPEG', quality=95)
        if self._copy_latest:
            shutil.copy(file_name, osp.join(d, 'latest.jpg'))
