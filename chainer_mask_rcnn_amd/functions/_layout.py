"""Layout helpers: tensors keep the reference's logical NCHW shape and are stored
channels-last (NHWC), the layout every HIP kernel of this package reads."""
import torch


def nhwc(x, dtype=None, fn=None, arg='x'):
    """Return x (logical NCHW) backed by dense NHWC memory that starts at a multiple of 16 bytes,
    as the kernels' vector accesses read it (no copy if it already is).  ``dtype``: the element
    type the C prototype behind the caller names — float32 for the maps, int32 for an argmax map;
    any other raises TypeError naming the function ``fn`` and the argument ``arg`` (a wrong
    dtype is the caller's bug: it is never cast).  None leaves the dtype to the caller."""
    if dtype is not None and x.dtype != dtype:
        raise TypeError('%s: %s must be %s, got %s' % (fn, arg, dtype, x.dtype))
    assert x.dim() == 4
    n, c, h, w = x.shape
    want = (h * w * c, 1, w * c, c)
    if all(x.shape[i] == 1 or x.stride(i) == want[i] for i in range(4)) and x.data_ptr() % 16 == 0:
        return x
    out = torch.empty((n, h, w, c), dtype=x.dtype, device=x.device).permute(0, 3, 1, 2)
    out.copy_(x)
    return out


def empty_nhwc(shape, device, dtype=torch.float32):
    n, c, h, w = shape
    return torch.empty((n, h, w, c), dtype=dtype, device=device).permute(0, 3, 1, 2)


def zeros_nhwc(shape, device, dtype=torch.float32):
    n, c, h, w = shape
    return torch.zeros((n, h, w, c), dtype=dtype, device=device).permute(0, 3, 1, 2)
