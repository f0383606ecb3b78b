"""COCO run-length encoding (RLE) of masks on the device (format: include/mrcnn_hip.h, "COCO
RLE"; kernels: csrc/mask_rle.hip).

``encode_masks`` turns masks into ``{'size': [H, W], 'counts': str}`` — pycocotools.mask.encode
followed by the compressed string of maskApi.c — and ``decode_masks`` turns such dicts (or
uncompressed count lists) back into masks.  Masks stay on the device in the packed format of
masks.py; only the strings come back.  Each call synchronises once.

``queue_encode`` / ``fetch_encoded`` split an encode into its queued device half and its
read-back, so that a caller (the COCO evaluator) can queue several images before reading them all
back together.  The strings are read back from buffers sized by a running estimate; a call whose
strings outgrow it reads back once more with exact buffers, and the estimate grows.
"""
import numpy as np
import torch

from ... import _lib
from . import masks as M

STATUS = {1: 'a character outside 48..111', 2: 'a value that does not end (unterminated)',
          3: 'a negative run', 4: 'runs that do not sum to H * W'}

# per-mask capacity estimates of a queued encode (counts, characters); they grow with use
_per_mask = {'values': 1024, 'chars': 2048}
_PER_MASK_MAX = 1 << 16
_I31 = (1 << 31) - 1


def _pinned_to(a, dev):
    """Host array -> device tensor through pinned memory, without waiting for the copy."""
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a if a.flags.writeable else a.copy())
    return t.pin_memory().to(dev, non_blocking=True)


class _Chunk(object):
    """One mrcnn_rle_encode launch over masks [n0, n0 + N) of a job."""

    def __init__(self, packed, extent, H, W):
        self.packed, self.extent, self.H, self.W = packed, extent, H, W
        self.N = packed.shape[0]
        dev = packed.device
        self.chg_off = torch.empty((self.N * M.packed_words(W) + 1,), dtype=torch.int32, device=dev)
        self.val_off = torch.empty((self.N + 1,), dtype=torch.int32, device=dev)
        self.str_off = torch.empty((self.N + 1,), dtype=torch.int32, device=dev)

    def launch(self, cap_values, cap_chars):
        dev = self.packed.device
        self.cap_values, self.cap_chars = int(cap_values), int(cap_chars)
        self.pos = torch.empty((max(self.cap_values, 1),), dtype=torch.int32, device=dev)
        self.counts = torch.empty((max(self.cap_values, 1),), dtype=torch.int32, device=dev)
        self.chars = torch.empty((max(self.cap_chars, 1),), dtype=torch.uint8, device=dev)
        _lib.call('mrcnn_rle_encode', _lib.ptr(self.packed), _lib.ptr(self.extent), self.N,
                  self.H, self.W, _lib.ptr(self.chg_off), _lib.ptr(self.val_off),
                  _lib.ptr(self.pos), _lib.ptr(self.counts), self.cap_values,
                  _lib.ptr(self.str_off), _lib.ptr(self.chars), self.cap_chars, _lib.stream_ptr())

    def device_parts(self, uncompressed):
        parts = [self.val_off.view(torch.uint8), self.str_off.view(torch.uint8),
                 self.chars[:self.cap_chars]]
        if uncompressed:
            parts.append(self.counts[:self.cap_values].view(torch.uint8))
        return parts


class EncodeJob(object):
    """A queued encode of one packed set: ``fetch_encoded`` reads it back."""

    def __init__(self, chunks, H, W):
        self.chunks, self.H, self.W = chunks, H, W


def queue_encode(packed, area, extent, size):
    """Queue the encode of a packed set (packed (N,H,Wq), area (N,), extent (N,4)) of an image of
    ``size`` (H, W); nothing is read back."""
    H, W = int(size[0]), int(size[1])
    if packed.dim() != 3 or packed.shape[1] != H or packed.shape[2] != M.packed_words(W):
        raise ValueError('packed masks of shape %s for an image of size %s'
                         % (tuple(packed.shape), (H, W)))
    _lib.require_device(packed, extent)
    packed = _lib.dense(packed, torch.int64, 'queue_encode', 'packed')
    extent = _lib.dense(extent, torch.int32, 'queue_encode', 'extent')
    N = packed.shape[0]
    # every offset of one launch stays below 2^31 (at most 7 characters per count)
    step = max(1, _I31 // (7 * (H * W + 1)) - 1)
    chunks = []
    for n0 in range(0, N, step):
        c = _Chunk(packed[n0:n0 + step], extent[n0:n0 + step], H, W)
        c.launch(min(c.N * _per_mask['values'], _I31 // 7),
                 min(c.N * _per_mask['chars'], _I31))
        chunks.append(c)
    return EncodeJob(chunks, H, W)


def _read(chunks, uncompressed):
    """One read-back of the chunks' offsets, strings (and counts)."""
    parts = [p for c in chunks for p in c.device_parts(uncompressed)]
    if not parts:
        return []
    host = torch.cat(parts).cpu().numpy()
    out, o = [], 0
    for c in chunks:
        n = 4 * (c.N + 1)
        val_off = host[o:o + n].view(np.int32)
        o += n
        str_off = host[o:o + n].view(np.int32)
        o += n
        chars = host[o:o + c.cap_chars]
        o += c.cap_chars
        counts = None
        if uncompressed:
            counts = host[o:o + 4 * c.cap_values].view(np.int32)
            o += 4 * c.cap_values
        out.append((val_off, str_off, chars, counts))
    return out


def fetch_encoded(jobs, uncompressed=False):
    """Read queued encodes back: per job, a list of ``{'size': [H, W], 'counts': str}`` (or the
    count list with ``uncompressed``).  One read-back for all jobs, a second for the chunks whose
    strings outgrew their buffers."""
    chunks = [c for j in jobs for c in j.chunks]
    got = _read(chunks, uncompressed)
    redo = []
    for i, (c, (val_off, str_off, _, _)) in enumerate(zip(chunks, got)):
        n_val, n_chr = int(val_off[-1]), int(str_off[-1])
        if n_val > c.cap_values or n_chr > c.cap_chars:
            c.launch(n_val, min(7 * n_val, _I31) if n_val > c.cap_values else n_chr)
            redo.append(i)
        # the estimate grows to twice the mean per mask (bounded)
        _per_mask['values'] = min(_PER_MASK_MAX, max(_per_mask['values'], 2 * -(-n_val // c.N)))
        _per_mask['chars'] = min(_PER_MASK_MAX, max(_per_mask['chars'], 2 * -(-n_chr // c.N)))
    if redo:
        for i, g in zip(redo, _read([chunks[i] for i in redo], uncompressed)):
            got[i] = g
    results, k = [], 0
    for j in jobs:
        size = [j.H, j.W]
        rles = []
        for c in j.chunks:
            val_off, str_off, chars, counts = got[k]
            k += 1
            for n in range(c.N):
                if uncompressed:
                    rles.append({'size': size,
                                 'counts': counts[val_off[n]:val_off[n + 1]].tolist()})
                else:
                    rles.append({'size': size,
                                 'counts': chars[str_off[n]:str_off[n + 1]].tobytes().decode('ascii')})
        results.append(rles)
    return results


def _as_packed(masks, size):
    if isinstance(masks, (tuple, list)) and len(masks) == 3 and isinstance(masks[0], torch.Tensor):
        if size is None:
            raise ValueError('a packed (packed, area, extent) triple needs its size (H, W)')
        return masks, (int(size[0]), int(size[1]))
    if isinstance(masks, torch.Tensor):
        dev = masks.device if masks.is_cuda else M._device()
        if not masks.is_cuda:
            masks = masks.numpy()
    else:
        dev = M._device()
    if not isinstance(masks, torch.Tensor):
        a = np.asarray(masks)
        if a.ndim != 3:
            raise ValueError('encode_masks expects (N, H, W) masks, got shape %s' % (a.shape,))
        if a.dtype == np.bool_:
            a = a.view(np.uint8)
        elif a.dtype not in (np.uint8, np.int32):
            a = (a != 0).view(np.uint8)
        masks = _pinned_to(a, dev)
    if masks.dim() != 3:
        raise ValueError('encode_masks expects (N, H, W) masks, got shape %s'
                         % (tuple(masks.shape),))
    N, H, W = masks.shape
    if size is not None and (int(size[0]), int(size[1])) != (H, W):
        raise ValueError('masks of size %s, size given %s' % ((H, W), tuple(size)))
    return M.pack_masks(masks, device=dev), (H, W)


def encode_masks(masks, size=None, uncompressed=False):
    """(N, H, W) bool / uint8 / int32 masks (host array or device tensor), or a packed
    ``(packed, area, extent)`` triple with ``size`` (H, W) -> ``[{'size': [H, W], 'counts': str},
    ...]``, COCO's compressed RLE (``uncompressed``: the count lists instead)."""
    (packed, area, extent), size = _as_packed(masks, size)
    return fetch_encoded([queue_encode(packed, area, extent, size)], uncompressed)[0]


class DecodeJob(object):
    """A queued decode: ``packed`` is the (packed, area, extent) triple, ``status`` the device
    per-mask status (``check_decoded`` reads it)."""

    def __init__(self, packed, status):
        self.packed, self.status = packed, status


def _rle_size(rle, i):
    try:
        h, w = rle['size']
        return int(h), int(w)
    except (KeyError, TypeError, ValueError):
        raise ValueError('RLE entry %d: no size [H, W]' % i)


def queue_decode(rles, size=None, device=None):
    """Queue the decode of ``rles`` (dicts with ``size`` and ``counts``: a compressed str / bytes
    or a list of counts) of one image size into a packed set; nothing is read back."""
    rles = list(rles)
    sizes = {_rle_size(r, i) for i, r in enumerate(rles)}
    if size is not None:
        sizes.add((int(size[0]), int(size[1])))
    if len(sizes) > 1:
        raise ValueError('RLE entries of different sizes: %s' % sorted(sizes))
    if not sizes:
        raise ValueError('decode_masks: no entries and no size')
    H, W = sizes.pop()
    if H <= 0 or W <= 0:
        raise ValueError('RLE size %s' % ([H, W],))
    dev = torch.device(device) if device is not None else M._device()
    N, Wq = len(rles), M.packed_words(W)
    packed = torch.empty((N, H, Wq), dtype=torch.int64, device=dev)
    area = torch.empty((N,), dtype=torch.int32, device=dev)
    extent = torch.empty((N, 4), dtype=torch.int32, device=dev)
    status = torch.zeros((N,), dtype=torch.int32, device=dev)
    if N == 0:
        return DecodeJob((packed, area, extent), status)
    strs, lists = [], []
    for i, r in enumerate(rles):
        c = r.get('counts') if isinstance(r, dict) else None
        if isinstance(c, str):
            c = c.encode('utf-8')
        if isinstance(c, (bytes, bytearray)):
            strs.append((i, bytes(c)))
        elif isinstance(c, (list, tuple, np.ndarray)):
            v = np.asarray(c)
            if v.ndim != 1 or (v.size and (v.dtype.kind not in 'iu' or v.min() < -_I31
                                           or v.max() > _I31)):
                raise ValueError('RLE entry %d: counts must be a list of 32-bit integers' % i)
            lists.append((i, v.astype(np.int32)))
        else:
            raise ValueError('RLE entry %d: counts must be a compressed string or a list of '
                             'integers, got %s' % (i, type(c).__name__))
    for group, is_str in ((strs, True), (lists, False)):
        if not group:
            continue
        idx = [i for i, _ in group]
        lens = np.array([len(d) for _, d in group], np.int64)
        off = np.zeros(len(group) + 1, np.int64)
        np.cumsum(lens, out=off[1:])
        if off[-1] > _I31:
            raise ValueError('RLE entries too long for one call')
        if is_str:
            data = np.frombuffer(b''.join(d for _, d in group) or b'\0', np.uint8)
        else:
            data = np.concatenate([d for _, d in group]) if off[-1] else np.zeros(1, np.int32)
        data_d = _pinned_to(data, dev)
        off_d = _pinned_to(off.astype(np.int32), dev)
        starts = torch.empty((max(int(off[-1]), 1),), dtype=torch.int32, device=dev)
        nval = torch.empty((len(group),), dtype=torch.int32, device=dev)
        whole = len(group) == N
        outs = (packed, area, extent, status) if whole else (
            torch.empty((len(group), H, Wq), dtype=torch.int64, device=dev),
            torch.empty((len(group),), dtype=torch.int32, device=dev),
            torch.empty((len(group), 4), dtype=torch.int32, device=dev),
            torch.empty((len(group),), dtype=torch.int32, device=dev))
        _lib.call('mrcnn_rle_decode', _lib.ptr(data_d) if is_str else None,
                  None if is_str else _lib.ptr(data_d), _lib.ptr(off_d), len(group), H, W,
                  _lib.ptr(starts), _lib.ptr(nval), _lib.ptr(outs[3]), _lib.ptr(outs[0]),
                  _lib.ptr(outs[1]), _lib.ptr(outs[2]), _lib.stream_ptr())
        if not whole:                    # strings and count lists mixed: back into entry order
            ix = torch.tensor(idx, dtype=torch.int64).to(dev, non_blocking=True)
            for dst, src in zip((packed, area, extent, status), outs):
                dst.index_copy_(0, ix, src)
    return DecodeJob((packed, area, extent), status)


def check_decoded(status, names=None):
    """Raise ValueError for the first entry whose host ``status`` is not OK; ``names[i]``
    (default ``'RLE entry i'``) names entry i."""
    bad = np.flatnonzero(np.asarray(status) != 0)
    if len(bad):
        i = int(bad[0])
        name = names[i] if names is not None else 'RLE entry %d' % i
        raise ValueError('%s: malformed RLE: %s' % (name, STATUS.get(int(status[i]), 'status %d'
                                                                      % int(status[i]))))


def decode_masks(rles, packed=False, size=None):
    """COCO RLE dicts of one image size -> (N, H, W) uint8 device tensor, or with ``packed`` the
    ``(packed, area, extent)`` triple of masks.py (exact areas, extents containing every set bit).
    ``size`` gives (H, W) when ``rles`` may be empty.  A malformed entry raises ValueError naming
    it."""
    job = queue_decode(rles, size)
    p, area, extent = job.packed
    N, H = p.shape[0], p.shape[1]
    W = int(size[1]) if size is not None else _rle_size(rles[0], 0)[1]
    out = None
    if not packed:
        out = torch.empty((N, H, W), dtype=torch.uint8, device=p.device)
        if N:
            _lib.call('mrcnn_mask_unpack', _lib.ptr(p), N, H, W, _lib.ptr(out), _lib.stream_ptr())
    check_decoded(job.status.cpu().numpy())
    return job.packed if packed else out
