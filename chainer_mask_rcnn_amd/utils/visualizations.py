"""Instance drawing and image mosaics — chainer_mask_rcnn/utils/visualizations.py and the
``fcn.utils`` helpers it and the visual report use.

``draw_instance_bboxes`` composites masks, boundaries, outlines and captions in one HIP launch
(``mrcnn_draw_instances``, contract in include/mrcnn_hip.h).  The host computes the
per-instance records (truncated boxes, skip flags, colour terms, outline colours, caption
rectangles), renders the captions with Pillow into one coverage atlas and uploads both in a
single copy; the masks are packed on the device (or come packed from ``paste_packed``).
``get_tile_image`` builds fcn's mosaic with ``mrcnn_tile_images``.

Documented deviations from the reference: outlines are hard-edged (cv2's LINE_AA is not
reproduced); captions use Pillow's default FreeType font at size 11 instead of cv2's Hershey
font at scale 0.4; negative box coordinates are clipped to the image where the reference's
slicing would wrap around; the mosaic's resize is bilinear instead of skimage's anti-aliased
resize.
"""
import functools
import warnings

import numpy as np
import torch

from .. import _lib
from .evaluations import masks as M

DRAW_MAX_INSTANCES = 4096          # MRCNN_DRAW_MAX_INSTANCES
TILE_MAX_CELLS = 64                # MRCNN_TILE_MAX_CELLS
_BOX_LIMIT = 1 << 30               # boxes are clipped to +-2^30 before they reach int32

# mrcnn_draw_instance (include/mrcnn_hip.h)
INSTANCE_DTYPE = np.dtype([('t', '<f8', (3,)), ('box', '<i4', (4,)), ('draw', '<i4'),
                           ('rgb', '<u4'), ('cap', '<i4', (4,)), ('cap_offset', '<i8')])
assert INSTANCE_DTYPE.itemsize == 72


class _TileCell(_lib.ctypes.Structure):
    """mrcnn_tile_cell."""
    _fields_ = [('src', _lib.c_vp), ('h', _lib.ctypes.c_int32), ('w', _lib.ctypes.c_int32),
                ('oh', _lib.ctypes.c_int32), ('ow', _lib.ctypes.c_int32),
                ('oy', _lib.ctypes.c_int32), ('ox', _lib.ctypes.c_int32)]


def label_colormap(N=256):
    """fcn.utils.labelcolormap: (N, 3) float32, ``cmap.astype(np.float32) / 255`` of the
    PASCAL colormap, whose label i spreads bits 0, 1, 2 of each 3-bit group of i onto R, G, B
    from the most significant bit down: rows 0-3 are (0, 0, 0), (128, 0, 0), (0, 128, 0),
    (128, 128, 0) times 1/255."""
    i = np.arange(N, dtype=np.int64)
    cmap = np.zeros((N, 3), np.int64)
    for j in range(8):
        for c in range(3):
            cmap[:, c] |= ((i >> (3 * j + c)) & 1) << (7 - j)
    return cmap.astype(np.float32) / 255


@functools.lru_cache(maxsize=1)
def _font():
    from PIL import ImageFont
    return ImageFont.load_default(size=11)


@functools.lru_cache(maxsize=4096)
def caption_coverage(text):
    """Pillow's coverage of ``text`` (uint8 (h, w)) and the offset (dy, dx) of its top-left
    corner from the left end of the baseline (anchor 'ls')."""
    from PIL import Image, ImageDraw
    font = _font()
    l, t, r, b = font.getbbox(text, anchor='ls')
    if r <= l or b <= t:
        return np.zeros((0, 0), np.uint8), 0, 0
    im = Image.new('L', (r - l, b - t), 0)
    ImageDraw.Draw(im).text((-l, -t), text, fill=255, font=font, anchor='ls')
    return np.asarray(im, np.uint8), t, l


def caption_layout(captions, boxes, on):
    """Per instance None or (y0, x0, coverage): the caption's text baseline starts at
    (x1, y2 - descent), the stand-in for cv2.putText at (x1, y2 - baseline)."""
    if captions is None:
        return [None] * len(boxes)
    descent = _font().getmetrics()[1]
    out = []
    for i, box in enumerate(boxes):
        if not on[i]:
            out.append(None)
            continue
        a, dy, dx = caption_coverage(str(captions[i]))
        if a.size == 0:
            out.append(None)
            continue
        out.append((int(box[2]) - descent + dy, int(box[1]) + dx, a))
    return out


def _device_of(img):
    if isinstance(img, torch.Tensor):
        _lib.require_device(img)
        return img.device
    if not torch.cuda.is_available():
        raise _lib.MrcnnHipError('draw_instance_bboxes runs on a ROCm device; none is visible '
                                 '(there is no CPU path)')
    return torch.device('cuda', torch.cuda.current_device())


def _is_packed(masks):
    return (isinstance(masks, tuple) and len(masks) == 3
            and all(isinstance(t, torch.Tensor) for t in masks)
            and masks[0].dim() == 3 and masks[1].dim() == 1 and masks[2].dim() == 2)


def _packed_masks(masks, boxes, on, H, W, dev):
    """The masks argument -> (packed, extent) device tensors of N full-frame masks."""
    N = len(boxes)
    if _is_packed(masks):
        packed, _, extent = masks
        if tuple(packed.shape) != (N, H, M.packed_words(W)) or tuple(extent.shape) != (N, 4):
            raise ValueError('packed masks of shape %s for %d instances on a %dx%d image'
                             % (tuple(packed.shape), N, H, W))
        _lib.require_device(packed, extent)
        return (_lib.dense(packed.to(dev), torch.int64, 'draw_instance_bboxes', 'masks[0] (packed)'),
                extent.to(dev, torch.int32).contiguous())
    if isinstance(masks, torch.Tensor):
        if tuple(masks.shape) != (N, H, W):
            raise ValueError('device masks must be (N, H, W) = %s, got %s'
                             % ((N, H, W), tuple(masks.shape)))
        packed, _, extent = M.pack_masks(masks, device=dev)
        return packed, extent
    if isinstance(masks, np.ndarray) and masks.ndim == 3 and masks.shape[1:] == (H, W):
        packed, _, extent = M.pack_masks(masks, device=dev)
        return packed, extent
    # a list of full-frame and box-sized masks: a box-sized mask (shape (y2-y1, x2-x1), checked
    # first as the reference does) is placed at (y1, x1) and clipped to the image
    full = np.zeros((N, H, W), np.uint8)
    for i in range(N):
        if not on[i]:
            continue
        m = np.asarray(masks[i])
        y1, x1, y2, x2 = (int(v) for v in boxes[i])
        if m.shape == (y2 - y1, x2 - x1):
            sy0, sy1, sx0, sx1 = max(y1, 0), min(y2, H), max(x1, 0), min(x2, W)
            if sy0 < sy1 and sx0 < sx1:
                full[i, sy0:sy1, sx0:sx1] = m[sy0 - y1:sy1 - y1, sx0 - x1:sx1 - x1] != 0
        elif m.shape == (H, W):
            full[i] = m != 0
        else:
            raise ValueError('mask %d of shape %s is neither (H, W) = %s nor its box\'s %s'
                             % (i, m.shape, (H, W), (y2 - y1, x2 - x1)))
    packed, _, extent = M.pack_masks(full, device=dev)
    return packed, extent


def draw_instances_device(img, boxes, labels, n_class, masks=None, captions=None, bg_class=0,
                          thickness=1, alpha=0.5, draw=None):
    """draw_instance_bboxes on a device image: img (H, W, 3) uint8 device tensor drawn IN
    PLACE (queued, not synchronised); boxes (N, 4) host array, truncated with astype(int)."""
    _lib.require_device(img)
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3 or not img.is_contiguous():
        raise TypeError('draw_instances_device: img must be a contiguous %s (H, W, 3) tensor (it is '
                        'drawn in place), got %s %s' % (torch.uint8, img.dtype, tuple(img.shape)))
    H, W = int(img.shape[0]), int(img.shape[1])
    dev = img.device
    boxes = np.clip(np.asarray(boxes).astype(int), -_BOX_LIMIT, _BOX_LIMIT).reshape(-1, 4)
    labels = np.asarray(labels)
    N = len(boxes)
    if N > DRAW_MAX_INSTANCES:
        raise ValueError('draw_instance_bboxes draws at most %d instances, got %d'
                         % (DRAW_MAX_INSTANCES, N))
    if N == 0:
        return img
    on = [bool(draw is None or draw[i]) and labels[i] != bg_class for i in range(N)]
    cmap = label_colormap(n_class)
    cmap_inst = label_colormap(N + 1)[1:]
    rec = np.zeros(N, INSTANCE_DTYPE)
    rec['box'] = boxes
    rec['draw'] = on
    # NumPy 2's float32 color_inst * alpha, widened: the reference adds it to a float64 product
    rec['t'] = ((cmap_inst * 255) * np.float32(alpha)).astype(np.float64)
    col = np.zeros((N, 3), np.uint32)
    for i in range(N):
        if on[i]:
            # cv2 receives color[::-1] while drawing on an RGB image: channel order reversed
            col[i] = np.round(cmap[labels[i]] * 255).astype(np.uint32)[::-1]
    rec['rgb'] = col[:, 0] | (col[:, 1] << 8) | (col[:, 2] << 16)
    layout = caption_layout(captions, boxes, on)
    chunks, off = [], 0
    for i, c in enumerate(layout):
        if c is not None:
            y0, x0, a = c
            rec['cap'][i] = (y0, x0, a.shape[0], a.shape[1])
            rec['cap_offset'][i] = off
            chunks.append(a.reshape(-1))
            off += a.size
    host = np.concatenate([rec.view(np.uint8)] + chunks)
    buf = torch.from_numpy(host).to(dev)
    packed = extent = None
    if masks is not None:
        packed, extent = _packed_masks(masks, boxes, on, H, W, dev)
    base = buf.data_ptr()
    _lib.call('mrcnn_draw_instances', _lib.ptr(img), H, W, _lib.ptr(packed), _lib.ptr(extent), N,
              _lib.c_vp(base), _lib.c_vp(base + rec.nbytes), off, float(alpha), int(thickness),
              _lib.stream_ptr())
    # buf, packed, extent: the caching allocator keeps their blocks for the queued kernel
    return img


def draw_instance_bboxes(img, bboxes, labels, n_class, masks=None, captions=None, bg_class=0,
                         thickness=1, alpha=0.5, draw=None):
    """The reference's draw_instance_bboxes.  img (H, W, 3) uint8: a host array gives a new
    host array (img is not modified), a device tensor a new device tensor.  masks: (N, H, W)
    full-frame masks (bool, uint8 or int32; nonzero is foreground), per-instance box-sized
    masks, or a (packed, area, extent) triple of pack_masks / paste_packed."""
    on_device = isinstance(img, torch.Tensor)
    if on_device:
        assert img.dim() == 3 and img.shape[2] == 3
        assert img.dtype == torch.uint8
    else:
        assert isinstance(img, np.ndarray)
        assert img.shape == (img.shape[0], img.shape[1], 3)
        assert img.dtype == np.uint8
    bboxes = np.asarray(bboxes)
    assert isinstance(bboxes, np.ndarray)
    assert bboxes.shape == (bboxes.shape[0], 4)
    labels = np.asarray(labels)
    assert isinstance(labels, np.ndarray)
    assert labels.shape == (labels.shape[0],)
    if draw is None:
        draw = [True] * bboxes.shape[0]
    else:
        assert len(draw) == bboxes.shape[0]
    if masks is not None:
        n_masks = masks[0].shape[0] if _is_packed(masks) else len(masks)
        assert n_masks == len(bboxes)
    if captions is not None:
        captions = np.asarray(captions)
        assert isinstance(captions, np.ndarray)
        assert captions.shape[0] == bboxes.shape[0]
    dev = _device_of(img)
    if on_device:
        out = img.contiguous().clone()
    else:
        out = torch.from_numpy(np.ascontiguousarray(img)).to(dev)
    draw_instances_device(out, bboxes, labels, n_class, masks=masks, captions=captions,
                          bg_class=bg_class, thickness=thickness, alpha=alpha, draw=draw)
    return out if on_device else out.cpu().numpy()


def draw_instance_boxes(img, boxes, instance_classes, n_class, masks=None, captions=None,
                        bg_class=0, thickness=1, draw=None):
    warnings.warn('draw_instance_boxes is deprecated, please use draw_instance_bboxes')
    return draw_instance_bboxes(img, boxes, instance_classes, n_class, masks=masks,
                                captions=captions, bg_class=bg_class, thickness=thickness,
                                draw=draw)


def tile_layout(shapes, tile_shape):
    """fcn.utils.get_tile_image's geometry: the cell (min H, min W) over all images, and per
    image in the grid (oh, ow, oy, ox): scaled by min(cellH / h, cellW / w) to (int(s*h),
    int(s*w)) and centred at ((cellH - oh) // 2, (cellW - ow) // 2)."""
    cell_h = min(int(s[0]) for s in shapes)
    cell_w = min(int(s[1]) for s in shapes)
    out = []
    for h, w in [(int(s[0]), int(s[1])) for s in shapes[:tile_shape[0] * tile_shape[1]]]:
        s = min(cell_h / h, cell_w / w)
        oh, ow = int(s * h), int(s * w)
        out.append((oh, ow, (cell_h - oh) // 2, (cell_w - ow) // 2))
    return cell_h, cell_w, out


def _tile_shape(n):
    # fcn.utils.get_tile_image's default: the squarest grid that holds n images
    x = int(np.ceil(np.sqrt(n)))
    y = int(np.ceil(n / float(x)))
    return y, x


def tile_images_device(imgs, tile_shape):
    """get_tile_image on device images: imgs a list of (h, w, 3) uint8 device tensors, returns
    the (rows * cellH, cols * cellW, 3) uint8 device mosaic (queued)."""
    rows, cols = int(tile_shape[0]), int(tile_shape[1])
    if rows * cols > TILE_MAX_CELLS:
        raise ValueError('get_tile_image: at most %d cells, got %dx%d'
                         % (TILE_MAX_CELLS, rows, cols))
    imgs = [t.contiguous() for t in imgs]
    cell_h, cell_w, cells = tile_layout([t.shape for t in imgs], (rows, cols))
    dev = imgs[0].device
    out = torch.empty((rows * cell_h, cols * cell_w, 3), dtype=torch.uint8, device=dev)
    table = (_TileCell * max(len(cells), 1))()
    for k, (oh, ow, oy, ox) in enumerate(cells):
        t = imgs[k]
        _lib.require_device(t)
        if t.dim() != 3 or t.shape[2] != 3 or t.dtype != torch.uint8 or t.device != dev:
            raise ValueError('get_tile_image expects (h, w, 3) uint8 images on one device')
        table[k] = _TileCell(_lib.addr(t, 'src'), t.shape[0], t.shape[1], oh, ow, oy, ox)
    _lib.call('mrcnn_tile_images', table, len(cells), rows, cols, cell_h, cell_w, _lib.ptr(out),
              _lib.stream_ptr())
    return out


def get_tile_image(imgs, tile_shape=None):
    """fcn.utils.get_tile_image(imgs, tile_shape) for (h, w, 3) uint8 images, row-major on
    black.  Host arrays give a host array, device tensors a device tensor."""
    if tile_shape is None:
        tile_shape = _tile_shape(len(imgs))
    on_device = isinstance(imgs[0], torch.Tensor)
    if on_device:
        return tile_images_device(list(imgs), tile_shape)
    dev = _device_of(None)
    ts = [torch.from_numpy(np.ascontiguousarray(a, np.uint8)).to(dev) for a in imgs]
    return tile_images_device(ts, tile_shape).cpu().numpy()
