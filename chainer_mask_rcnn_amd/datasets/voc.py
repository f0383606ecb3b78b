"""PASCAL VOC 2012 and SBD instance-segmentation datasets — the reference's
datasets/voc/voc.py and datasets/voc/sbd.py: same class names, constructors (plus ``root_dir``)
and example layout,

    dataset[i] -> img (H,W,3) uint8 RGB, bboxes (G,4) f32 (y1,x1,y2,x2), labels (G,) i32
                  (0-based foreground classes: the reference's ``labels -= 1``),
                  masks (G,H,W) i32 {0,1}

The label images are turned into instances on the device by ``utils.label2instance_boxes``:
the decoded PNG palette indices (or the .mat arrays) are uploaded as uint8, where 255 reads as
-1, and ``mask_by_class`` applies the reference's ``lbl_ins[np.isin(lbl_cls, [-1, 0])] = -1``
in the same pass.  There is no download here: the data must already be under ``root_dir``.
"""
import os.path as osp
import warnings

import numpy as np

from .. import utils

VOC_CLASS_NAMES = np.array([
    'aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car', 'cat', 'chair', 'cow',
    'diningtable', 'dog', 'horse', 'motorbike', 'person', 'pottedplant', 'sheep', 'sofa',
    'train', 'tvmonitor'])
VOC_CLASS_NAMES.setflags(write=0)


def read_rgb(path):
    """JPEG -> (H, W, 3) uint8 RGB whatever its colour model (as datasets/coco.py reads them)."""
    import PIL.Image
    with PIL.Image.open(path) as f:
        img = np.asarray(f if f.mode in ('L', 'RGB') else f.convert('RGB'))
    if img.ndim == 2:
        img = np.repeat(img[:, :, None], 3, axis=2)
    return img


def _as_label(a):
    """A decoded label image as uint8 (255 = -1 on the device) when it already is one, else
    int32 with the reference's ``lbl[lbl == 255] = -1``."""
    a = np.asarray(a)
    if a.dtype == np.uint8:
        return np.ascontiguousarray(a)
    a = a.astype(np.int32)
    a[a == 255] = -1
    return a


def labels_to_example(img, lbl_cls, lbl_ins):
    """(img, class label image, instance label image) -> (img, bboxes, labels, masks) of the
    reference's VOC / SBD ``get_example``."""
    labels, bboxes, masks = utils.label2instance_boxes(_as_label(lbl_ins), _as_label(lbl_cls),
                                                       return_masks=True, mask_by_class=True)
    masks = masks.astype(np.int32, copy=False)
    labels = labels.astype(np.int32, copy=False)
    labels -= 1  # background: 0 -> -1
    bboxes = bboxes.astype(np.float32, copy=False)
    return img, bboxes, labels, masks


def _read_ids(imgsets_file):
    if not osp.exists(imgsets_file):
        raise IOError('split list %s not found' % imgsets_file)
    with open(imgsets_file) as f:
        return [line.strip() for line in f if line.strip()]


class VOCInstanceSegmentationDatasetBase(object):

    class_names = VOC_CLASS_NAMES

    def __len__(self):
        return len(self.files)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self.get_example(j) for j in range(*i.indices(len(self)))]
        return self.get_example(i)


class VOC2012InstanceSegmentationDataset(VOCInstanceSegmentationDatasetBase):

    root_dir = osp.expanduser('~/data/datasets/VOC/VOCdevkit/VOC2012')

    def __init__(self, split, root_dir=None):
        if split not in ('train', 'val'):
            raise ValueError("split must be 'train' or 'val', got %r" % (split,))
        if root_dir is not None:
            self.root_dir = root_dir
        if not osp.exists(self.root_dir):
            raise IOError('%s not found; the reference downloads VOC2012 there, this build has '
                          'no download: place the VOCdevkit/VOC2012 tree there or pass root_dir'
                          % self.root_dir)
        ids = _read_ids(osp.join(self.root_dir, 'ImageSets/Segmentation/%s.txt' % split))
        self.files = [{
            'img': osp.join(self.root_dir, 'JPEGImages/%s.jpg' % did),
            'seg_class': osp.join(self.root_dir, 'SegmentationClass/%s.png' % did),
            'seg_object': osp.join(self.root_dir, 'SegmentationObject/%s.png' % did),
        } for did in ids]

    def get_example(self, i):
        import PIL.Image
        data_file = self.files[i]
        img = read_rgb(data_file['img'])
        # palette PNGs: np.asarray gives the uint8 palette indices (255 = void)
        with PIL.Image.open(data_file['seg_class']) as f:
            lbl_cls = np.asarray(f)
        with PIL.Image.open(data_file['seg_object']) as f:
            lbl_ins = np.asarray(f)
        return labels_to_example(img, lbl_cls, lbl_ins)


class SBDInstanceSegmentationDataset(VOCInstanceSegmentationDatasetBase):
    """SBD (benchmark_RELEASE/dataset).  ``imgsets_file`` defaults to the ``{split}.txt`` that
    the SBD release ships in its dataset directory; pass another list to pick other ids."""

    root_dir = osp.expanduser('~/data/datasets/VOC/benchmark_RELEASE/dataset')

    def __init__(self, split='train', root_dir=None, imgsets_file=None):
        if root_dir is not None:
            self.root_dir = root_dir
        if not osp.exists(self.root_dir):
            raise IOError('%s not found; the reference downloads SBD there, this build has no '
                          'download: place the benchmark_RELEASE/dataset tree there or pass '
                          'root_dir' % self.root_dir)
        if imgsets_file is None:
            imgsets_file = osp.join(self.root_dir, '%s.txt' % split)
        self.files = [{
            'img': osp.join(self.root_dir, 'img/%s.jpg' % did),
            'cls': osp.join(self.root_dir, 'cls/%s.mat' % did),
            'ins': osp.join(self.root_dir, 'inst/%s.mat' % did),
        } for did in _read_ids(imgsets_file)]

    def get_example(self, index):
        import scipy.io
        data_file = self.files[index]
        img = read_rgb(data_file['img'])
        lbl_cls = scipy.io.loadmat(data_file['cls'])['GTcls'][0]['Segmentation'][0]
        lbl_ins = scipy.io.loadmat(data_file['ins'])['GTinst'][0]['Segmentation'][0]
        return labels_to_example(img, lbl_cls, lbl_ins)


class VOC2012InstanceSeg(VOC2012InstanceSegmentationDataset):

    def __init__(self, *args, **kwargs):
        warnings.warn('VOC2012InstanceSeg is renamed to VOC2012InstanceSegmentationDataset.')
        super(VOC2012InstanceSeg, self).__init__(*args, **kwargs)


class SBDInstanceSeg(SBDInstanceSegmentationDataset):

    def __init__(self, *args, **kwargs):
        warnings.warn('SBDInstanceSeg is renamed to SBDInstanceSegmentationDataset.')
        super(SBDInstanceSeg, self).__init__(*args, **kwargs)
