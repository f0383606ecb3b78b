"""NumPy restatement of the drawing contract of utils.draw_instance_bboxes and of the mosaic of
utils.get_tile_image (include/mrcnn_hip.h, "Instance drawing and the report mosaic").

``draw`` takes full-frame boolean masks and the already rendered captions (the product's
Pillow coverage), so that both sides are compared on the same atlas."""
import numpy as np


def label_colormap(N=256):
    """fcn.utils.labelcolormap: the PASCAL bit-interleaved colormap, float32 in [0, 1]."""
    cmap = np.zeros((N, 3), np.int64)
    for i in range(N):
        c, r, g, b = i, 0, 0, 0
        for j in range(8):
            r |= ((c >> 0) & 1) << (7 - j)
            g |= ((c >> 1) & 1) << (7 - j)
            b |= ((c >> 2) & 1) << (7 - j)
            c >>= 3
        cmap[i] = (r, g, b)
    return cmap.astype(np.float32) / 255


def boundary(m):
    """find_boundaries(m, connectivity=2, mode='thick') of a 2-D mask: the 3x3 neighbourhood,
    clamped to the array (scipy's 'reflect' for a 3x3 footprint), holds both values."""
    m = np.asarray(m, bool)
    if m.size == 0:
        return m.copy()
    p = np.pad(m, 1, mode='edge')
    h, w = m.shape
    win = [p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)]
    return np.logical_or.reduce(win) & ~np.logical_and.reduce(win)


def outline(H, W, box, thickness):
    """Pixels within Chebyshev distance thickness // 2 of the 1-pixel rectangle through
    (x1, y1) and (x2, y2), clipped to the image."""
    y1, x1, y2, x2 = box
    by0, by1, bx0, bx1 = min(y1, y2), max(y1, y2), min(x1, x2), max(x1, x2)
    r = thickness // 2
    yy, xx = np.mgrid[:H, :W]
    outer = (yy >= by0 - r) & (yy <= by1 + r) & (xx >= bx0 - r) & (xx <= bx1 + r)
    inner = (yy > by0 + r) & (yy < by1 - r) & (xx > bx0 + r) & (xx < bx1 - r)
    return outer & ~inner


def draw(img, bboxes, labels, n_class, masks=None, captions=None, bg_class=0, thickness=1,
         alpha=0.5, draw=None):
    """masks: (N, H, W) boolean full-frame masks or None; captions: per instance None or
    (y0, x0, coverage (h, w) uint8)."""
    img = np.array(img, np.uint8)
    H, W = img.shape[:2]
    boxes = np.asarray(bboxes).astype(int)
    labels = np.asarray(labels)
    N = len(boxes)
    on = [(draw is None or draw[i]) and labels[i] != bg_class for i in range(N)]
    cmap = label_colormap(n_class)
    cmap_inst = label_colormap(N + 1)[1:]
    if masks is not None:
        for i in range(N):
            if not on[i]:
                continue
            y1, x1, y2, x2 = boxes[i].tolist()
            cy0, cy1, cx0, cx1 = max(y1, 0), min(y2, H), max(x1, 0), min(x2, W)
            if cy0 >= cy1 or cx0 >= cx1:
                continue
            m = np.asarray(masks[i], bool)[cy0:cy1, cx0:cx1]
            t = ((cmap_inst[i] * 255) * np.float32(alpha)).astype(np.float64)
            crop = img[cy0:cy1, cx0:cx1]
            crop[m] = (crop[m].astype(np.float64) * (1 - alpha) + t).astype(np.uint8)
            crop[boundary(m)] = 200
    for i in range(N):
        if not on[i]:
            continue
        y1, x1, y2, x2 = boxes[i].tolist()
        rgb = np.round(cmap[labels[i]] * 255).astype(np.uint8)[::-1]
        img[outline(H, W, (y1, x1, y2, x2), thickness)] = rgb
        if captions is not None and captions[i] is not None:
            y0, x0, a = captions[i]
            h, w = a.shape
            sy0, sy1, sx0, sx1 = max(y0, 0), min(y0 + h, H), max(x0, 0), min(x0 + w, W)
            if sy0 < sy1 and sx0 < sx1:
                aa = a[sy0 - y0:sy1 - y0, sx0 - x0:sx1 - x0].astype(np.int64)[..., None]
                v = img[sy0:sy1, sx0:sx1].astype(np.int64)
                img[sy0:sy1, sx0:sx1] = ((255 * aa + v * (255 - aa) + 127) // 255).astype(np.uint8)
    return img


def lin_coord(n_out, n_in):
    """The half-pixel bilinear rule of csrc/bilinear.h for one axis: (i0, i1, t float32)."""
    scale = float(n_in) / float(n_out)
    f = ((np.arange(n_out, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    lo = s < 0
    s[lo], f[lo] = 0, 0
    hi = s >= n_in - 1
    s[hi], f[hi] = n_in - 1, 0
    return s, np.minimum(s + 1, n_in - 1), f


def resize(img, oh, ow):
    h, w = img.shape[:2]
    y0, y1, ty = lin_coord(oh, h)
    x0, x1, tx = lin_coord(ow, w)
    p = img.astype(np.float32)
    one = np.float32(1)
    tx_ = tx[None, :, None]
    top = p[y0][:, x0] * (one - tx_) + p[y0][:, x1] * tx_
    bot = p[y1][:, x0] * (one - tx_) + p[y1][:, x1] * tx_
    ty_ = ty[:, None, None]
    return (top * (one - ty_) + bot * ty_).astype(np.int64).astype(np.uint8)


def tile(imgs, tile_shape):
    """fcn.utils.get_tile_image's layout with the bilinear resize."""
    rows, cols = tile_shape
    ch = min(im.shape[0] for im in imgs)
    cw = min(im.shape[1] for im in imgs)
    out = np.zeros((rows * ch, cols * cw, 3), np.uint8)
    for k, im in enumerate(imgs[:rows * cols]):
        h, w = im.shape[:2]
        s = min(ch / h, cw / w)
        oh, ow = int(s * h), int(s * w)
        if oh == 0 or ow == 0:
            continue
        oy, ox = (ch - oh) // 2, (cw - ow) // 2
        gy, gx = divmod(k, cols)
        out[gy * ch + oy:gy * ch + oy + oh, gx * cw + ox:gx * cw + ox + ow] = resize(im, oh, ow)
    return out
