# flake8: noqa
from .eval_instance_segmentation_voc import eval_instseg_voc, calc_instseg_voc_prec_rec
from .eval_instance_segmentation_coco import eval_instseg_coco
from .masks import (mask_iou, boundary_dilation, boundary_packed, mask_to_boundary,
                    boundary_counts, boundary_iou)
from .matching import calc_detection_voc_ap
from .eval_detection import eval_detection_voc, eval_detection_coco
