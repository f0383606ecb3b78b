"""NumPy restatement of csrc/gt_masks.hip (mrcnn_mask_resize_nearest): a table lookup on the
unpacked bits, the tables clamped as the kernel clamps them.  tests/test_packed_masks_cpu.py
proves it equal to datasets.transforms.resize_nearest; tests/test_gpu_gt_masks.py compares the
kernel with both."""
import numpy as np

from chainer_mask_rcnn_amd.datasets.transforms import _nearest_index

# source (H, W) -> output (H, W): word boundaries (63 / 64 / 65), one pixel, the identity, three
# words with an odd output width, a downscale, and the shape of the train-loop test
SHAPES = [((1, 1), (5, 7)), ((7, 63), (9, 64)), ((9, 64), (13, 65)), ((11, 65), (11, 65)),
          ((37, 130), (61, 217)), ((61, 217), (23, 90)), ((96, 128), (144, 192))]


def random_masks(rng, G, H, W, fill=None):
    """(G, H, W) int32 {0,1}: random bits; with G >= 3 instance 0 is all zero and instance 1 all
    one; ``fill`` 0 / 1 makes every instance all zero / all one (the single-instance cases)."""
    m = (rng.uniform(size=(G, H, W)) > 0.5).astype(np.int32)
    if fill is not None:
        m[:] = fill
    elif G >= 3:
        m[0], m[1] = 0, 1
    return m


def tables(in_size, out_size, x_flip=False):
    """(ys, xs) int32 as functions.resize_masks_nearest builds them."""
    ys = _nearest_index(out_size[0], in_size[0])
    xs = _nearest_index(out_size[1], in_size[1])
    if x_flip:
        xs = xs[::-1]
    return ys.astype(np.int32), xs.astype(np.int32)


def resize_with_tables(packed, ys, xs):
    """out[g, y, x] = bit (g, clamp(ys[y]), clamp(xs[x])) of a PackedMasks, as uint8."""
    G, H, W = packed.shape
    bits = packed.unpack(np.uint8)
    ys = np.clip(np.asarray(ys, np.int64), 0, H - 1)
    xs = np.clip(np.asarray(xs, np.int64), 0, W - 1)
    return bits[:, ys][:, :, xs]


def resize_masks_nearest(packed, out_size, x_flip=False):
    ys, xs = tables(packed.shape[1:], out_size, x_flip)
    return resize_with_tables(packed, ys, xs)
