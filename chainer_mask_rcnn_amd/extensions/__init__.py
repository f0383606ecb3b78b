# flake8: noqa
from .instance_segmentation_evaluators import (InstanceSegmentationVOCEvaluator,
                                               InstanceSegmentationCOCOEvaluator,
                                               create_multi_node_evaluator)
from .instance_segmentation_vis_report import InstanceSegmentationVisReport
