"""Input pipeline of the train step: the reference's
``datasets/coco.py`` (annotation decoding), ``datasets/transforms.py`` and
``datasets/concat_examples.py`` (the image half on the device)."""
from .transforms import MaskRCNNTransform  # NOQA
from .transforms import resize_bbox, flip_bbox, resize_nearest, flip  # NOQA
from .transforms import draw_scale_jitter  # NOQA
from .packed_masks import PackedMasks  # NOQA
from .polygon_masks import PolygonMasks  # NOQA
from .concat_examples import concat_examples  # NOQA
from .coco import COCOInstanceSegmentationDataset  # NOQA
from .voc import VOC2012InstanceSegmentationDataset, SBDInstanceSegmentationDataset  # NOQA
from .voc import VOC2012InstanceSeg, SBDInstanceSeg  # NOQA
from .mask_rcnn import MaskRcnnDataset  # NOQA
from .indexing_dataset import IndexingDataset  # NOQA
from .scatter import scatter_dataset, SubDataset  # NOQA
from .copy_paste import CopyPasteDataset, draw_paste_selection  # NOQA
