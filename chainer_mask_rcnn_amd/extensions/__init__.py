# flake8: noqa
from .instance_segmentation_evaluators import (InstanceSegmentationVOCEvaluator,
                                               InstanceSegmentationCOCOEvaluator)
from .instance_segmentation_vis_report import InstanceSegmentationVisReport
