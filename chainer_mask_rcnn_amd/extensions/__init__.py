# flake8: noqa
from .instance_segmentation_evaluators import (InstanceSegmentationVOCEvaluator,
                                               InstanceSegmentationCOCOEvaluator)
