# flake8: noqa
"""Operators — same public names as the reference's ``chainer_mask_rcnn.functions``
(/root/reference/chainer_mask_rcnn/functions/__init__.py:1-9) for the hot path."""
from .affine_channel_2d import affine_channel_2d
from .affine_channel_2d import AffineChannel2DFunction

from .roi_align_2d import roi_align_2d
from .roi_align_2d import ROIAlign2D
from .roi_align_2d import spatial_order as roi_spatial_order
from .roi_align_2d import RoiHints

from .roi_pooling_2d import roi_pooling_2d
from .roi_pooling_2d import ROIPooling2D

from .crop_and_resize import crop_and_resize
from .crop_and_resize import CropAndResize

from .conv import conv2d, deconv2x2s2, linear, stem_conv
from .stage import building_block
from .pooling import max_pooling_2d, average_pooling_2d
from .loss import (sigmoid_cross_entropy, softmax_cross_entropy, fast_rcnn_loc_loss,
                   mask_sigmoid_cross_entropy, softmax)
from .proposal_ops import non_maximum_suppression
from .proposal_ops import soft_nms
from .aug_merge import decode_cls_boxes_views, mask_aug_combine
from .gt_masks import resize_masks_nearest, upload_packed_masks
from .scale_jitter import prepare_image_crop, resize_crop_masks
from .copy_paste import copy_paste, copy_paste_meta
from .ignore_regions import union_plane, box_coverage, ignored_from_counts
from .polygons import rasterize_polygons, upsample_vertices
