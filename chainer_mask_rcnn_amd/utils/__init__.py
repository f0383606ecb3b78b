# flake8: noqa
from .bbox import (generate_anchor_base, enumerate_shifted_anchor, bbox_iou, bbox2loc,
                   resize_bilinear)
from .evaluations import (eval_instseg_voc, eval_instseg_coco, calc_instseg_voc_prec_rec,
                          calc_detection_voc_ap, mask_iou, eval_detection_voc,
                          eval_detection_coco, boundary_dilation, boundary_packed,
                          mask_to_boundary, boundary_counts, boundary_iou)
from .geometry import (label2instance_boxes, instance_boxes2label, mask_to_bbox, get_bbox_overlap,
                       get_mask_overlap)
from .visualizations import (draw_instance_bboxes, draw_instance_boxes, label_colormap,
                             get_tile_image)
from ._shutil import git_hash
