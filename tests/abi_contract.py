"""The contract of every tensor that crosses the C ABI of libmrcnn_hip.so, checked at the boundary.

The library takes raw pointers: ``_lib.ptr(t)`` is ``c_void_p(t.data_ptr())`` and nothing between
a Python wrapper and a kernel knows what the buffer holds.  ``include/mrcnn_hip.h`` carries typed
prototypes, so the contract can be checked generically:

* ``parse_header()`` turns the header into ``{entry: [Param(name, elem, const, pointer)]}``;
* ``Recorder`` swaps ``_lib.ptr`` for one whose pointers carry their tensor and ``_lib.call`` for
  one that checks every (entry, pointer parameter, tensor) against ``check_crossing`` — in *dry*
  mode nothing is launched (CPU tensors will do), in *live* mode the call goes on to the library;
* ``PROBES`` (second half) is the table of the smallest valid call of every Python function that
  hands a tensor to the library, and ``perturbations`` the wrong dtypes / layouts each tensor
  argument is swapped for.
"""
import collections
import contextlib
import ctypes
import os
import re

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'mrcnn_hip.h')
PACKAGE = os.path.join(ROOT, 'chainer_mask_rcnn_amd')

Param = collections.namedtuple('Param', 'name elem const pointer')

# C element type -> (kind, bytes); kind 'f' floating, 'i' integer (bool counts as 8-bit integer)
C_TYPES = {'float': ('f', 4), 'double': ('f', 8), 'int': ('i', 4), 'int32_t': ('i', 4),
           'uint32_t': ('i', 4), 'int64_t': ('i', 8), 'uint64_t': ('i', 8), 'uint8_t': ('i', 1),
           'int8_t': ('i', 1), 'char': ('i', 1), 'int16_t': ('i', 2), 'uint16_t': ('i', 2)}


def parse_header(path=HEADER):
    """``{entry: [Param]}`` for every ``mrcnn_*`` prototype.  ``elem`` is the C element type of a
    pointer to typed device data, None for ``void *``, pointers to pointers, structs and scalars."""
    text = open(path).read()
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'//[^\n]*', ' ', text)
    text = re.sub(r'^\s*#[^\n]*', ' ', text, flags=re.M)
    out = {}
    for m in re.finditer(r'\b(mrcnn_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', text):
        name, body = m.group(1), ' '.join(m.group(2).split())
        params = []
        if body and body != 'void':
            for i, decl in enumerate(body.split(',')):
                decl = decl.strip()
                pm = re.match(r'^(.*?)(\w+)$', decl)
                if pm is None:
                    raise ValueError('%s: cannot parse parameter %r' % (name, decl))
                typ, pname = pm.group(1).strip(), pm.group(2)
                stars = typ.count('*')
                words = [w for w in typ.replace('*', ' ').split() if w != 'const']
                if len(words) != 1:
                    raise ValueError('%s: cannot parse the type of %r' % (name, decl))
                elem = None
                if stars == 1 and words[0] != 'void' and words[0] in C_TYPES:
                    elem = words[0]
                elif stars == 0 and words[0] not in C_TYPES:
                    raise ValueError('%s: unknown scalar type in %r' % (name, decl))
                # const-ness of what a single pointer points to: `const T *p`
                const = stars >= 1 and typ.split('*')[0].split().count('const') > 0
                params.append(Param(pname, elem, const, stars > 0))
        out[name] = params
    return out


def scan_call_sites(package=PACKAGE):
    """``{entry: [relative file]}`` of every ``call('mrcnn_…'`` in the package source."""
    found = collections.defaultdict(list)
    for dp, _, fns in os.walk(package):
        for fn in fns:
            if fn.endswith('.py'):
                path = os.path.join(dp, fn)
                for name in re.findall(r"""call\(\s*['"](mrcnn_[a-z0-9_]+)['"]""", open(path).read()):
                    found[name].append(os.path.relpath(path, package))
    return dict(found)


def scan_named_entries(package=PACKAGE):
    """``{entry: [relative file]}`` of every quoted ``'mrcnn_…'`` name in the package outside
    ``_lib.py``: the literal call sites and the names handed on to ``_lib.call`` through a variable
    (the RoI extractors' tables, the box-IoU conventions)."""
    found = collections.defaultdict(list)
    for dp, _, fns in os.walk(package):
        for fn in fns:
            path = os.path.join(dp, fn)
            if fn.endswith('.py') and os.path.relpath(path, package) != '_lib.py':
                for name in re.findall(r"""['"](mrcnn_[a-z0-9_]+)['"]""", open(path).read()):
                    found[name].append(os.path.relpath(path, package))
    return dict(found)


# Entry points the dry sweep cannot reach and the live run of tests/test_gpu_abi_contract.py must
# see, each with its reason; only entry points called solely from models/ may stand here.  Today
# the dry sweep reaches every one.
LIVE_COVERED = {}

# Entry points no test of this contract covers, each with its reason: the collectives, and entry
# points that no Python code outside _lib.py calls.
_NO_CALLER = 'no Python caller outside _lib.py'
EXEMPT = dict(
    [(e, 'needs an RCCL world of several ranks') for e in (
        'mrcnn_allreduce_unique_id', 'mrcnn_allreduce_init', 'mrcnn_allreduce_destroy',
        'mrcnn_allreduce_info', 'mrcnn_allreduce_bucket', 'mrcnn_allreduce_wait',
        'mrcnn_allreduce_broadcast', 'mrcnn_allreduce_timing', 'mrcnn_allreduce_bucket_times')] +
    [(e, _NO_CALLER) for e in (
        'mrcnn_roi_align_fwd', 'mrcnn_roi_align_bwd', 'mrcnn_roi_align_bwd_ex', 'mrcnn_conv2d_dgrad',
        'mrcnn_sgd_momentum_wd', 'mrcnn_conv3x3_wino_fixup_count')] +
    [(e, _NO_CALLER + '; host pointers only') for e in (
        'mrcnn_device_info', 'mrcnn_conv_gemm_plan', 'mrcnn_profile_summary', 'mrcnn_set_tuning')])


# ---- the rule ---------------------------------------------------------------------------------

# operands that may be row-strided: the prototype has a leading-dimension parameter for them
ROW_STRIDED = {('mrcnn_softmax_ce', 'x'): 'ldx', ('mrcnn_softmax', 'x'): 'ldx',
               ('mrcnn_smooth_l1', 'pred'): 'ld'}

# Operands the kernels read or write with 8- / 16-byte vector accesses (float4 / uint4 casts in
# csrc/conv_gemm.hip, conv_winograd.h, elementwise.hip, roi_align.hip, roi_pool_variants.hip: the
# NHWC maps, filters and per-channel vectors, C a multiple of 4; nms.hip, soft_nms.hip,
# proposal.hip, targets.hip, test_aug.hip: (n, 4) box rows as one float4): every float pointer of
# the first group of entry points, the named parameters of the second.
ALIGNED_ENTRIES = re.compile(
    r'^mrcnn_(conv2d_|conv3x3_wino_|conv_stem_|deconv2x2s2_|filter_flip_transpose$|epilogue_bwd$|'
    r'colsum$|roi_align_|roi_pool_|crop_resize_|sparse3x3_|affine_|maxpool|avgpool_|head_tail_bwd$|'
    r'sgd_momentum_|grad_sumsq$)')
ALIGNED_PARAMS = {
    'mrcnn_decode_clip': ('anchor', 'loc', 'roi'),
    'mrcnn_nms_sorted': ('bbox',), 'mrcnn_nms_sorted_batched': ('bbox',),
    'mrcnn_soft_nms_sorted_batched': ('sorted_boxes',),
    'mrcnn_box_vote': ('sorted_boxes', 'voted_boxes'),
    'mrcnn_detect_sort': ('cls_bbox', 'sorted_boxes'),
    'mrcnn_detect_compact': ('sorted_boxes', 'bbox'),
    'mrcnn_decode_cls_boxes': ('roi', 'cls_bbox'),
    'mrcnn_decode_cls_boxes_views': ('cls_bbox',),
    'mrcnn_mask_aug_combine': ('out',),
    'mrcnn_anchor_targets_finish': ('loc',),
    'mrcnn_proposal_targets_gather': ('cand', 'sample_roi', 'gt_roi_loc'),
}


# Tensors that cross inside a host-side table (an array of pointers, or of structs that hold one):
# the wrappers take their addresses with ``_lib.addr(t, field)``.  (entry, field) -> (element type,
# const, read with vector accesses, may be row-strided: the struct carries a leading dimension).
TABLE_FIELDS = {
    ('mrcnn_observe_accumulate', 'values'): ('float', True, False, False),
    ('mrcnn_decode_cls_boxes_views', 'roi'): ('float', True, True, False),
    ('mrcnn_decode_cls_boxes_views', 'cls_loc'): ('float', True, False, True),
    ('mrcnn_mask_aug_combine', 'maps'): ('float', True, True, False),
    ('mrcnn_tile_images', 'src'): ('uint8_t', True, False, False),
    ('mrcnn_filter_flip_transpose_batched', 'w'): ('float', True, True, False),
    ('mrcnn_filter_flip_transpose_batched', 'wT'): ('float', False, True, False),
    ('mrcnn_filter_flip_transpose_batched', 'row_scale'): ('float', True, True, False),
}


def needs_alignment(entry, param):
    if entry in ALIGNED_PARAMS:
        return param.name in ALIGNED_PARAMS[entry]
    # (R, 5) RoI rows are 20 bytes: read element by element
    return bool(ALIGNED_ENTRIES.match(entry)) and param.elem == 'float' and param.name != 'rois'


def dtype_kind_width(dtype):
    if dtype == torch.bool:
        return 'i', 1
    if dtype.is_floating_point:
        return 'f', torch.finfo(dtype).bits // 8
    if dtype.is_complex:
        return 'c', 0
    return 'i', torch.iinfo(dtype).bits // 8


def nhwc_dense(t):
    """Dense NHWC memory behind a logical NCHW tensor, as functions/_layout.nhwc defines it."""
    if t.dim() != 4:
        return False
    n, c, h, w = t.shape
    want = (h * w * c, 1, w * c, c)
    return all(t.shape[i] == 1 or t.stride(i) == want[i] for i in range(4))


def layout_of(t):
    """'any' (at most one element), 'c' (contiguous), 'nhwc', 'c|nhwc' (both hold), 'rows'
    (unit inner stride, rows at a stride of at least their length), else 'strided'."""
    if t.numel() <= 1:
        return 'any'
    c, n = t.is_contiguous(), nhwc_dense(t)
    if c or n:
        return 'c|nhwc' if c and n else ('c' if c else 'nhwc')
    if t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]:
        return 'rows'
    return 'strided'


def check_crossing(entry, param, t, live=False, aligned=None, rows=None):
    """The violations (strings) of tensor ``t`` handed to pointer parameter ``param`` of ``entry``
    (``aligned`` / ``rows``: for a table field, in the place of the lists above)."""
    aligned = needs_alignment(entry, param) if aligned is None else aligned
    rows = (entry, param.name) in ROW_STRIDED if rows is None else rows
    bad = []
    if param.elem is not None:
        kind, width = C_TYPES[param.elem]
        k, w = dtype_kind_width(t.dtype)
        if k != kind:
            bad.append('wrong kind: %s for %s *' % (t.dtype, param.elem))
        elif w != width:
            bad.append('wrong width: %s for %s *' % (t.dtype, param.elem))
    lay = layout_of(t)
    if lay == 'rows' and not rows:
        bad.append('row-strided %s %s, and the prototype has no leading dimension for it'
                   % (tuple(t.shape), t.stride()))
    elif lay == 'strided':
        if t.numel() > 1 and 0 in [st for st, sz in zip(t.stride(), t.shape) if sz > 1]:
            bad.append('stride-0 (expanded) view %s %s' % (tuple(t.shape), t.stride()))
        else:
            bad.append('not dense: %s %s' % (tuple(t.shape), t.stride()))
    if aligned and t.numel() and t.data_ptr() % 16:
        bad.append('read with 16-byte vector accesses but data_ptr() %% 16 == %d' % (t.data_ptr() % 16))
    if live and not t.is_cuda:
        bad.append('a %s tensor in a launch' % t.device)
    return bad


Crossing = collections.namedtuple('Crossing', 'entry param dtype shape stride layout violations')


class TensorPtr(ctypes.c_void_p):
    """A c_void_p that remembers its tensor (ctypes takes a subclass where c_void_p is declared)."""
    tensor = None


class AbiViolation(AssertionError):
    """A live call whose tensors break the rule: it is recorded and NOT launched."""


class Recorder(object):
    """``with Recorder(dry=True) as rec: wrapper(...)``: every tensor the wrappers hand to
    ``_lib.call`` is checked; ``rec.crossings`` lists them, ``rec.violations()`` those that break
    the rule, ``rec.entries`` the entry points called.  A live recorder passes a call on to the
    library only if every tensor of it obeys the rule, and raises AbiViolation otherwise: no
    kernel ever reads a buffer the recorder has found wrong."""

    def __init__(self, dry=True, header=None, fill=None):
        self.dry = dry
        self.fill = fill or {}
        self.header = header or parse_header()
        self.crossings = []
        self.entries = []
        self._patched = []
        self._pending = []      # (field, tensor) taken with _lib.addr since the last call

    def _addr(self, t, field):
        if t is None:
            return None
        self._pending.append((field, t))
        return t.data_ptr()

    def _ptr(self, t):
        if t is None:
            return None
        p = TensorPtr(t.data_ptr())
        p.tensor = t
        return p

    def _call(self, name, *args):
        params = self.header[name]
        if len(args) != len(params):
            raise AssertionError('%s called with %d arguments, the header declares %d'
                                 % (name, len(args), len(params)))
        self.entries.append(name)
        devices, first = set(), len(self.crossings)
        pending, self._pending = self._pending, []
        for field, t in pending:
            spec = TABLE_FIELDS.get((name, field))
            if spec is None:
                raise AssertionError('%s: no table field %r is declared (TABLE_FIELDS)' % (name, field))
            elem, const, aligned, rows = spec
            bad = check_crossing(name, Param(field, elem, const, True), t, not self.dry, aligned, rows)
            devices.add(t.device)
            self.crossings.append(Crossing(name, field, t.dtype, tuple(t.shape), t.stride(),
                                           layout_of(t), tuple(bad)))
            if self.dry and not const:
                t.detach().zero_()
        for a, prm in zip(args, params):
            if not isinstance(a, TensorPtr):
                continue
            t = a.tensor
            bad = [] if prm.pointer else ['a tensor for the scalar parameter']
            bad += check_crossing(name, prm, t, live=not self.dry)
            devices.add(t.device)
            self.crossings.append(Crossing(name, prm.name, t.dtype, tuple(t.shape), t.stride(),
                                           layout_of(t), tuple(bad)))
            if self.dry and not prm.const:
                # a wrapper that reads a count back sees 0, not uninitialised memory
                t.detach().zero_()
                if (name, prm.name) in self.fill:
                    v = torch.tensor(self.fill[(name, prm.name)], dtype=t.dtype, device=t.device)
                    t.detach().reshape(-1)[:v.numel()] = v
        if not self.dry and len(devices) > 1:
            self.crossings.append(Crossing(name, '*', None, (), (), 'any',
                                           ('tensors of one call on %s' % sorted(map(str, devices)),)))
        if not self.dry:
            bad = [c for c in self.crossings[first:] if c.violations]
            if bad:
                raise AbiViolation('%s not launched:\n%s' % (name, format_crossings(bad)))
            return self._orig['call'](name, *args)

    def violations(self):
        return [c for c in self.crossings if c.violations]

    def __enter__(self):
        from chainer_mask_rcnn_amd import _lib
        self._lib = _lib
        self._orig = {k: getattr(_lib, k) for k in ('ptr', 'addr', 'call', 'stream_ptr', 'require_device')}
        _lib.ptr, _lib.addr, _lib.call = self._ptr, self._addr, self._call
        self._cuda_device = torch.cuda.device
        if self.dry:
            _lib.stream_ptr = lambda: None
            _lib.require_device = lambda *tensors: None
            if not torch.cuda.is_available():
                # on a machine without a device the dry run stands in for it with the CPU: wrappers
                # that enter `torch.cuda.device(dev)`, pick "the current device" or stage through
                # pinned memory get a no-op, the CPU, and a plain host tensor
                torch.cuda.device = lambda dev: contextlib.nullcontext()
                from chainer_mask_rcnn_amd.utils import geometry
                from chainer_mask_rcnn_amd.utils.evaluations import masks, rle
                cpu = lambda: torch.device('cpu')
                self._patched = [(masks, '_device', masks._device), (geometry, '_device', geometry._device),
                                 (rle, '_pinned_to', rle._pinned_to)]
                masks._device = geometry._device = cpu
                rle._pinned_to = lambda a, dev: torch.from_numpy(np.array(a))
        return self

    def __exit__(self, *exc):
        for k, v in self._orig.items():
            setattr(self._lib, k, v)
        torch.cuda.device = self._cuda_device
        for mod, name, value in self._patched:
            setattr(mod, name, value)
        return False


def format_crossings(crossings):
    return '\n'.join('  %s(%s): %s %s %s -> %s' % (c.entry, c.param, c.dtype, c.shape, c.stride,
                                                 '; '.join(c.violations)) for c in crossings)


# ---- perturbations ----------------------------------------------------------------------------

def _like(t, v):
    """``v`` as a leaf that requires a gradient if ``t`` does."""
    v = v.detach()
    return v.requires_grad_(True) if t.requires_grad else v


def dtype_perturbations(t):
    """[(label, tensor)]: the same values in a dtype of the same kind and another width, and in a
    dtype of the other kind."""
    kind, width = dtype_kind_width(t.dtype)
    if kind == 'f':
        others = [torch.float64 if width == 4 else torch.float32, torch.int32]
    else:
        others = [d for d in (torch.int64, torch.int16, torch.int32)
                  if dtype_kind_width(d)[1] != width][:2] + [torch.float32]
    return [('dtype:%s' % str(d)[6:], t.detach().to(d)) for d in others]


def layout_perturbations(t):
    """[(label, tensor)]: views of other memory with ``t``'s shape and dtype — every second row /
    element of a larger tensor, the transposed form, the other memory format of a 4-D map, an
    expand()ed stride-0 view, a view starting at row 1 and one starting at element 1 of a larger
    buffer.  All but the expanded view hold ``t``'s values."""
    out = []
    s = tuple(t.shape)
    if t.numel() <= 1:
        return out
    d = t.detach()
    if s[0] > 1:
        big = d.new_zeros((2 * s[0],) + s[1:])
        big[::2] = d
        out.append(('rows2', big[::2]))
    if t.dim() >= 2 and s[-1] > 1:
        big = d.new_zeros(s[:-1] + (2 * s[-1],))
        big[..., ::2] = d
        out.append(('cols2', big[..., ::2]))
    if t.dim() >= 2 and s[-1] > 1 and s[-2] > 1:
        out.append(('transposed', d.transpose(-1, -2).contiguous().transpose(-1, -2)))
    if t.dim() == 4:
        if nhwc_dense(d) and not d.is_contiguous():
            out.append(('nchw', d.contiguous()))
        elif not nhwc_dense(d):
            other = d.new_zeros((s[0], s[2], s[3], s[1])).permute(0, 3, 1, 2)
            other.copy_(d)
            out.append(('nhwc', other))
    if s[0] > 1:
        out.append(('expand', d[:1].expand(s)))
    big = d.new_zeros((s[0] + 1,) + s[1:])
    big[1:] = d
    out.append(('offset_row', big[1:]))
    flat = d.new_zeros((d.numel() + 1,))
    dense = d if layout_of(d) in ('c', 'nhwc', 'c|nhwc') else d.contiguous()
    v = torch.as_strided(flat, s, dense.stride(), 1)
    v.copy_(d)
    out.append(('offset_elem', v))
    return [(label, _like(t, v)) for label, v in out]


def dense_copy(t):
    """The same values in fresh, aligned, contiguous memory."""
    return _like(t, t.detach().clone(memory_format=torch.contiguous_format))


def flatten_outputs(out):
    """Every tensor / array of a (nested) result, in order."""
    if out is None:
        return []
    if isinstance(out, (torch.Tensor, np.ndarray)):
        return [out]
    if isinstance(out, dict):
        return [t for k in sorted(out) for t in flatten_outputs(out[k])]
    if isinstance(out, (tuple, list)):
        return [t for o in out for t in flatten_outputs(o)]
    return [np.asarray(out)] if isinstance(out, (int, float, str, bytes)) else []


def backward_of(out, grad_layout=None):
    """Back-propagate a fixed gradient through every floating output that records a graph.
    ``grad_layout``: label of the layout perturbation the gradient tensor is handed over in."""
    for o in flatten_outputs(out):
        if isinstance(o, torch.Tensor) and o.requires_grad:
            g = ((torch.arange(o.numel(), device=o.device) % 7).to(o.dtype) - 3.).reshape(o.shape)
            if grad_layout is not None:
                g = dict(layout_perturbations(g)).get(grad_layout, g)    # (a scalar has one layout)
            o.backward(g, retain_graph=True)


class Probe(object):
    """One row: ``make(dev)`` -> ``(args dict, run(args) -> result)``; ``tensors`` names the
    entries of ``args`` that are tensors handed (by the function under test) to the library."""

    def __init__(self, name, make, tensors, backward=False, cpu=True, rejects=(), dry_fill=None, reroute=()):
        self.name, self.make, self.tensors, self.backward, self.cpu = name, make, tensors, backward, cpu
        # ``reroute``: operands whose unexpected layout or dtype makes the function take its other
        # documented path instead of a copy (SparseRows: the dense backward) — a different
        # summation order, so the live comparison with the dense copy leaves them out
        self.reroute = tuple(reroute)
        # ``rejects``: further exception types the function documents for a bad argument;
        # ``dry_fill``: {(entry, parameter): values} a dry run writes where the library would have
        # (a count the wrapper reads back before its second launch)
        self.rejects, self.dry_fill = tuple(rejects), dry_fill or {}

    def run(self, dev, replace=None, grad_layout=None):
        """-> (result, args): one call, with ``replace`` = {argument: tensor} swapped in."""
        args, fn = self.make(dev)
        args.update(replace or {})

        def both():
            out = fn(args)
            if self.backward:
                backward_of(out, grad_layout)
            return out
        return _on_one_stream(both), args


PROBES = []


def probe(name, tensors, backward=False, cpu=True, rejects=(), dry_fill=None, reroute=()):
    def deco(make):
        PROBES.append(Probe(name, make, tuple(tensors), backward, cpu, rejects, dry_fill, reroute))
        return make
    return deco


# ---- the sweep --------------------------------------------------------------------------------

def _classes(layout):
    return set(layout.split('|'))


def _against_baseline(crossings, base):
    """Crossings whose memory format differs from every one the unperturbed call handed to the same
    parameter: a map that arrives NCHW where the baseline's arrived channels-last is dense, and
    wrong."""
    bad = []
    for c in crossings:
        seen = base.get((c.entry, c.param, len(c.shape)))
        if not seen or c.layout in ('any', 'rows', 'strided') or any(b == 'any' for b in seen):
            continue
        if not any(_classes(c.layout) & _classes(b) for b in seen):
            bad.append(c._replace(violations=('%s memory where the unperturbed call passes %s'
                                              % (c.layout, '/'.join(sorted(seen))),)))
    return bad


def run_recorded(p, dev, dry, replace=None, grad_layout=None):
    """-> (outcome, recorder, result): outcome 'ok', 'rejected: …' (TypeError / ValueError before
    anything crossed... or after) or 'error: …' (anything else, MrcnnHipError included)."""
    with Recorder(dry=dry, fill=p.dry_fill) as rec:
        try:
            out, _ = p.run(dev, replace, grad_layout)
            return 'ok', rec, out
        except (TypeError, ValueError) + p.rejects as e:
            return 'rejected: %s: %s' % (type(e).__name__, e), rec, None
        except Exception as e:      # noqa: the C side's MrcnnHipError, an assert, a torch error
            return 'error: %s: %s' % (type(e).__name__, e), rec, None


DENSE_FORM = re.compile(r'^[^:]+: .+ must be (torch\.\w+), got (torch\.\w+)$')


def rejection_problem(outcome, orig=None, new=None):
    """What is wrong with a 'rejected: …' outcome as the refusal of a perturbed argument, or None.
    A refusal states a contract ('… must be …' / '… expects …'): a TypeError or ValueError that
    some torch operation happened to raise on the perturbed tensor is not one.  For a dtype
    perturbation (``orig`` -> ``new``) it names the expected dtype, and in the form of
    ``_lib.dense`` / ``nhwc`` — 'function: argument must be <dtype>, got <dtype>' — both."""
    msg = outcome.split(': ', 2)[2] if outcome.count(': ') >= 2 else ''
    if not re.search(r'\bmust be\b|\bexpects\b', msg):
        return 'states no contract: %r' % msg
    if orig is None:
        return None
    m = DENSE_FORM.match(msg)
    if m:
        if (m.group(1), m.group(2)) == (str(orig), str(new)):
            return None
        return 'names %s and %s for a %s argument given as %s' % (m.group(1), m.group(2), orig, new)
    if str(orig)[6:] not in msg:
        return 'does not name the expected dtype %s: %r' % (orig, msg)
    return None


def baseline(p, dev, dry=True):
    """The unperturbed call -> (failures, {(entry, param): {layout}}, entries)."""
    outcome, rec, _ = run_recorded(p, dev, dry)
    fails = []
    if outcome != 'ok':
        fails.append('%s: the unperturbed call %s' % (p.name, outcome))
    if rec.violations():
        fails.append('%s: the unperturbed call breaks the rule:\n%s'
                     % (p.name, format_crossings(rec.violations())))
    base = collections.defaultdict(set)
    for c in rec.crossings:
        base[(c.entry, c.param, len(c.shape))].add(c.layout)
    return fails, dict(base), list(rec.entries)


def perturbed_cases(p, dev, kinds=('dtype', 'layout', 'grad')):
    """[(label, replace dict, grad_layout)] for one row."""
    args, _ = p.make(dev)
    cases = []
    for name in p.tensors:
        t = args[name]
        if 'dtype' in kinds:
            cases += [('%s=%s' % (name, lab), {name: _like(t, v) if v.is_floating_point() else v}, None)
                      for lab, v in dtype_perturbations(t)]
        if 'layout' in kinds:
            cases += [('%s=%s' % (name, lab), {name: v}, None) for lab, v in layout_perturbations(t)]
    if p.backward and 'grad' in kinds:
        cases += [('gy=%s' % lab, {}, lab) for lab in ('cols2', 'transposed', 'expand', 'offset_elem')]
    return cases


def dry_sweep(p, dev, kinds=('dtype', 'layout', 'grad')):
    """Every perturbed call of one row under the dry recorder -> (failures, entries recorded).
    A perturbed call may raise TypeError / ValueError, or proceed with every crossing obeying the
    rule; a crossing that breaks it, or any other error, is a failure."""
    fails, base, entries = baseline(p, dev, dry=True)
    if fails:
        return fails, entries
    args0, _ = p.make(dev)
    for label, replace, grad_layout in perturbed_cases(p, dev, kinds):
        outcome, rec, _ = run_recorded(p, dev, True, replace, grad_layout)
        bad = rec.violations() + _against_baseline(rec.crossings, base)
        if bad:
            fails.append('%s [%s]: reached the ABI:\n%s' % (p.name, label, format_crossings(bad)))
        elif outcome.startswith('error'):
            fails.append('%s [%s]: %s' % (p.name, label, outcome))
        elif outcome.startswith('rejected'):
            name = next(iter(replace))
            dtypes = (args0[name].dtype, replace[name].dtype) if '=dtype:' in label else (None, None)
            why = rejection_problem(outcome, *dtypes)
            if why:
                fails.append('%s [%s]: %s — %s' % (p.name, label, outcome, why))
    return fails, entries


# ---- the probe table --------------------------------------------------------------------------
# The smallest valid call of every Python function that hands a tensor to the library: maps of a
# few pixels with C a multiple of 4, a handful of boxes or RoIs.  Results that the library leaves
# undefined past a count (keep lists, sorted rows) are cut to the count by the row itself.

def _rng(seed=0):
    return np.random.RandomState(seed)


def _f(a, dev, grad=False):
    t = torch.tensor(np.asarray(a, np.float32), device=dev)
    return t.requires_grad_(True) if grad else t


def _i(a, dev, dtype=torch.int32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=dev)


def _map(shape, dev, seed=0, grad=False):
    """A float32 (N, C, H, W) map in channels-last memory."""
    from chainer_mask_rcnn_amd.functions._layout import nhwc
    t = nhwc(_f(_rng(seed).standard_normal(shape), dev))
    return t.requires_grad_(True) if grad else t


def _boxes(n, dev, seed=0, lim=40.):
    r = _rng(seed)
    b = r.uniform(0, lim, (n, 4)).astype(np.float32)
    b[:, 2:] = b[:, :2] + r.uniform(4, lim, (n, 2)).astype(np.float32)
    return _f(b, dev)


def _rois(dev):
    # (batch_index, x1, y1, x2, y2) on a 2-image, 6x7 map at scale 1/4
    return _f([[0, 1.5, 2., 20., 17.], [1, 0., 0., 27., 23.], [1, 8.2, 4.7, 9., 5.1]], dev)


def _count(t):
    return int(t.reshape(-1)[0].item())


# -- functions/loss.py
@probe('loss.sigmoid_cross_entropy', ('x', 't'), backward=True)
def _p(dev):
    from chainer_mask_rcnn_amd.functions import loss as L
    a = dict(x=_f(_rng().standard_normal((3, 5)), dev, True), t=_i(_rng().randint(-1, 2, (3, 5)), dev))
    return a, lambda a: L.sigmoid_cross_entropy(a['x'], a['t'])


@probe('loss.mask_sigmoid_cross_entropy', ('roi_masks', 'gt_roi_labels', 'gt_roi_masks'), backward=True)
def _p(dev):
    from chainer_mask_rcnn_amd.functions import loss as L
    a = dict(roi_masks=_map((3, 4, 5, 5), dev, grad=True), gt_roi_labels=_i([1, 4, 0], dev),
             gt_roi_masks=_i(_rng().randint(-1, 2, (3, 5, 5)), dev))
    return a, lambda a: L.mask_sigmoid_cross_entropy(a['roi_masks'], a['gt_roi_labels'], a['gt_roi_masks'])


@probe('loss.softmax_cross_entropy', ('x', 't'), backward=True)
def _p(dev):
    from chainer_mask_rcnn_amd.functions import loss as L
    a = dict(x=_f(_rng().standard_normal((4, 5)), dev, True), t=_i([0, 4, -1, 2], dev))
    return a, lambda a: L.softmax_cross_entropy(a['x'], a['t'])


@probe('loss.fast_rcnn_loc_loss', ('pred_loc', 'gt_loc', 'gt_label', 'cls'), backward=True)
def _p(dev):
    from chainer_mask_rcnn_amd.functions import loss as L
    a = dict(pred_loc=_f(_rng().standard_normal((4, 12)), dev, True),
             gt_loc=_f(_rng(1).standard_normal((4, 4)), dev), gt_label=_i([1, 0, -1, 2], dev),
             cls=_i([1, 0, 0, 2], dev))
    return a, lambda a: L.fast_rcnn_loc_loss(a['pred_loc'], a['gt_loc'], a['gt_label'], 3., a['cls'])


@probe('loss.softmax', ('x',))
def _p(dev):
    from chainer_mask_rcnn_amd.functions import loss as L
    return dict(x=_f(_rng().standard_normal((4, 5)), dev)), lambda a: L.softmax(a['x'])


@probe('loss.observe_accumulate', ('sums', 'v1'))
def _p(dev):
    from chainer_mask_rcnn_amd.functions import loss as L
    a = dict(sums=_f([1., 2., 3.], dev), v1=_f(0.25, dev))
    return a, lambda a: L.observe_accumulate([_f(0.5, dev), a['v1']], a['sums'])


# -- functions/proposal_ops.py
@probe('proposal_ops.decode_clip', ('anchor', 'loc'))
def _p(dev):
    from chainer_mask_rcnn_amd.functions import proposal_ops as P
    a = dict(anchor=_boxes(5, dev), loc=_f(_rng(2).standard_normal((5, 4)) * 0.1, dev))
    return a, lambda a: P.decode_clip(a['anchor'], a['loc'], (48, 64), 2.)


@probe('proposal_ops.topk_desc', ('score', 'valid'))
def _p(dev):
    from chainer_mask_rcnn_amd.functions import proposal_ops as P
    a = dict(score=_f(_rng().standard_normal(6), dev), valid=_i([1, 1, 0, 1, 1, 1], dev, torch.uint8))

    def run(a):
        order, n = P.topk_desc(a['score'], 4, a['valid'])
        return order[:_count(n)], n
    return a, run


@probe('proposal_ops.topk_desc_batched', ('score', 'valid'))
def _p(dev):
    from chainer_mask_rcnn_amd.functions import proposal_ops as P
    a = dict(score=_f(_rng().standard_normal((2, 6)), dev),
             valid=_i([[1, 1, 0, 1, 1, 1], [1, 0, 0, 0, 1, 1]], dev, torch.uint8))

    def run(a):
        order, n = P.topk_desc_batched(a['score'], 3, a['valid'])
        return [order[g, :int(n[g].item())] for g in range(2)], n
    return a, run


@probe('proposal_ops.gather_rows', ('src', 'idx', 'n_dev'))
def _p(dev):
    from chainer_mask_rcnn_amd.functions import proposal_ops as P
    a = dict(src=_boxes(5, dev), idx=_i([4, 0, 2], dev), n_dev=_i([2], dev))
    return a, lambda a: P.gather_rows(a['src'], a['idx'], a['n_dev'])


@probe('proposal_ops.nms_sorted', ('bbox', 'n_dev'))
def _p(dev):
    from chainer_mask_rcnn_amd.functions import proposal_ops as P
    a = dict(bbox=_boxes(6, dev), n_dev=_i([5], dev))

    def run(a):
        keep, n = P.nms_sorted(a['bbox'], 0.3, a['n_dev'])
        return keep[:_count(n)], n
    return a, run


@probe('proposal_ops.nms_sorted_batched', ('bbox', 'n_dev'))
def _p(dev):
    from chainer_mask_rcnn_amd.functions import proposal_ops as P
    a = dict(bbox=torch.stack([_boxes(6, dev), _boxes(6, dev, 1)]), n_dev=_i([5, 6], dev))

    def run(a):
        keep, n = P.nms_sorted_batched(a['bbox'], a['n_dev'], 0.3)
        return [keep[g, :int(n[g].item())] for g in range(2)], n
    return a, run


def _soft_nms_args(dev):
    prob = np.sort(_rng(3).uniform(0.1, 1, (2, 6)).astype(np.float32), axis=1)[:, ::-1].copy()
    return dict(bbox=torch.stack([_boxes(6, dev), _boxes(6, dev, 1)]), prob=_f(prob, dev),
                n_dev=_i([5, 6], dev))


@probe('proposal_ops.soft_nms_sorted_batched', ('bbox', 'prob', 'n_dev'))
def _p(dev):
    from chainer_mask_rcnn_amd.functions import proposal_ops as P

    def run(a):
        keep, n, soft = P.soft_nms_sorted_batched(a['bbox'], a['prob'], a['n_dev'], 'linear')
        nd = [5, 6]
        return [keep[g, :int(n[g].item())] for g in range(2)], n, [soft[g, :nd[g]] for g in range(2)]
    return _soft_nms_args(dev), run


@probe('proposal_ops.box_vote', ('bbox', 'prob', 'n_dev', 'keep', 'n_keep'))
def _p(dev):
    from chainer_mask_rcnn_amd.functions import proposal_ops as P
    a = _soft_nms_args(dev)
    a.update(keep=_i([[0, 2, 3, 0, 0, 0], [1, 4, 0, 0, 0, 0]], dev), n_keep=_i([3, 2], dev))

    def run(a):
        voted = P.box_vote(a['bbox'], a['prob'], a['n_dev'], a['keep'], a['n_keep'])
        return voted[0, [0, 2, 3]], voted[1, [1, 4]]
    return a, run


@probe('proposal_ops.non_maximum_suppression', ('bbox', 'score'))
def _p(dev):
    from chainer_mask_rcnn_amd.functions import proposal_ops as P
    a = dict(bbox=_boxes(6, dev), score=_f(_rng().uniform(0, 1, 6), dev))
    return a, lambda a: P.non_maximum_suppression(a['bbox'], 0.3, a['score'])


@probe('proposal_ops.soft_nms', ('bbox', 'score'))
def _p(dev):
    from chainer_mask_rcnn_amd.functions import proposal_ops as P
    a = dict(bbox=_boxes(6, dev), score=_f(_rng().uniform(0.1, 1, 6), dev))
    return a, lambda a: P.soft_nms(a['bbox'], a['score'])


# -- functions/target_ops.py
@probe('target_ops.bbox_iou_argmax', ('boxes_a', 'boxes_b'))
def _p(dev):
    from chainer_mask_rcnn_amd.functions import target_ops as T
    a = dict(boxes_a=_boxes(5, dev), boxes_b=_boxes(2, dev, 1))
    return a, lambda a: T.bbox_iou_argmax(a['boxes_a'], a['boxes_b'], want_matrix=True)


@probe('target_ops.anchor_labels', ('iou', 'max_iou', 'gt_max'))
def _p(dev):
    from chainer_mask_rcnn_amd.functions import target_ops as T
    iou = _rng().uniform(0, 1, (5, 2)).astype(np.float32)
    a = dict(iou=_f(iou, dev), max_iou=_f(iou.max(1), dev), gt_max=_f(iou.max(0), dev))
    return a, lambda a: T.anchor_labels(a['iou'], a['max_iou'], a['gt_max'], 0.3, 0.7)


@probe('target_ops.anchor_targets_finish',
       ('anchor_inside', 'inside_index', 'label_inside', 'argmax', 'bbox', 'disabled'))
def _p(dev):
    from chainer_mask_rcnn_amd.functions import target_ops as T
    a = dict(anchor_inside=_boxes(4, dev), inside_index=_i([0, 2, 3, 5], dev),
             label_inside=_i([1, 0, -1, 1], dev), argmax=_i([0, 1, 1, 0], dev),
             bbox=_boxes(2, dev, 1), disabled=_i([3, 0], dev))
    return a, lambda a: T.anchor_targets_finish(a['anchor_inside'], a['inside_index'], a['label_inside'],
                                                a['argmax'], a['bbox'], a['disabled'], 6)


@probe('target_ops.proposal_targets_gather', ('cand', 'bbox', 'gt_label', 'assigned', 'chosen'))
def _p(dev):
    from chainer_mask_rcnn_amd.functions import target_ops as T
    a = dict(cand=_boxes(5, dev), bbox=_boxes(2, dev, 1), gt_label=_i([3, 7], dev),
             assigned=_i([0, 1, 1, 0, 1], dev), chosen=_i([4, 1, 0], dev))
    return a, lambda a: T.proposal_targets_gather(a['cand'], a['bbox'], a['gt_label'], a['assigned'],
                                                  a['chosen'], 2, (0., 0., 0., 0.), (.1, .1, .2, .2))


@probe('target_ops.mask_targets', ('masks_u8', 'sample_roi', 'gt_index'))
def _p(dev):
    from chainer_mask_rcnn_amd.functions import target_ops as T
    a = dict(masks_u8=_i(_rng().randint(0, 2, (2, 12, 16)), dev, torch.uint8), sample_roi=_boxes(3, dev, lim=6.),
             gt_index=_i([1, 0, 0], dev))

    def run(a):
        return T.mask_targets(a['masks_u8'], a['sample_roi'], a['gt_index'], 2, 4)[:2]
    return a, run


# -- functions/pooling.py, affine_channel_2d.py
@probe('pooling.max_pooling_2d', ('x',))
def _p(dev):
    from chainer_mask_rcnn_amd.functions import pooling
    return dict(x=_map((2, 4, 5, 7), dev)), lambda a: pooling.max_pooling_2d(a['x'])


@probe('pooling.average_pooling_2d', ('x',), backward=True)
def _p(dev):
    from chainer_mask_rcnn_amd.functions import pooling
    return dict(x=_map((3, 4, 7, 7), dev, grad=True)), lambda a: pooling.average_pooling_2d(a['x'], 7)


@probe('affine_channel_2d', ('x', 'W', 'b'), backward=True)
def _p(dev):
    from chainer_mask_rcnn_amd import functions as F
    a = dict(x=_map((2, 4, 3, 5), dev, grad=True), W=_f(_rng(1).uniform(.5, 1, (1, 4, 1, 1)), dev, True),
             b=_f(_rng(2).standard_normal((1, 4, 1, 1)), dev, True))
    return a, lambda a: F.affine_channel_2d(a['x'], a['W'], a['b'])


# -- the three RoI feature extractors
def _extractor_probe(name, call):
    @probe(name, ('x', 'rois', 'order'), backward=True)
    def _p(dev):
        a = dict(x=_map((2, 4, 6, 7), dev, grad=True), rois=_rois(dev), order=_i([2, 0, 1], dev))
        return a, lambda a: call(a['x'], a['rois'], a['order'])


def _roi_align(x, rois, order):
    from chainer_mask_rcnn_amd import functions as F
    return F.roi_align_2d(x, rois, 2, 2, 0.25, order=order)


def _roi_pooling(x, rois, order):
    from chainer_mask_rcnn_amd import functions as F
    return F.roi_pooling_2d(x, rois, 2, 2, 0.25, order=order)


def _crop_and_resize(x, rois, order):
    from chainer_mask_rcnn_amd import functions as F
    return F.crop_and_resize(x, rois, 2, 2, 0.25, order=order)


_extractor_probe('roi_align_2d', _roi_align)
_extractor_probe('roi_pooling_2d', _roi_pooling)
_extractor_probe('crop_and_resize', _crop_and_resize)


# -- functions/conv.py
@probe('conv.conv2d 1x1 + bias', ('x', 'W', 'b'), backward=True)
def _p(dev):
    from chainer_mask_rcnn_amd.functions import conv
    a = dict(x=_map((2, 8, 3, 5), dev, grad=True), W=_map((4, 8, 1, 1), dev, 1, True),
             b=_f(_rng(2).standard_normal(4), dev, True))
    return a, lambda a: conv.conv2d(a['x'], a['W'], a['b'])


@probe('conv.conv2d 3x3 + affine + residual + relu', ('x', 'W', 'scale', 'shift', 'residual'), backward=True)
def _p(dev):
    from chainer_mask_rcnn_amd.functions import conv
    a = dict(x=_map((2, 4, 5, 6), dev, grad=True), W=_map((8, 4, 3, 3), dev, 1, True),
             scale=_f(_rng(2).uniform(.5, 1, 8), dev), shift=_f(_rng(3).standard_normal(8), dev),
             residual=_map((2, 8, 5, 6), dev, 4, True))
    return a, lambda a: conv.conv2d(a['x'], a['W'], None, 1, 1, a['scale'], a['shift'], a['residual'], True)


@probe('conv.linear', ('x', 'W', 'b'), backward=True)
def _p(dev):
    from chainer_mask_rcnn_amd.functions import conv
    a = dict(x=_f(_rng().standard_normal((3, 8)), dev, True), W=_f(_rng(1).standard_normal((4, 8)), dev, True),
             b=_f(_rng(2).standard_normal(4), dev, True))
    return a, lambda a: conv.linear(a['x'], a['W'], a['b'])


@probe('conv.stem_conv', ('x4', 'w784', 'b', 'scale', 'shift'))
def _p(dev):
    from chainer_mask_rcnn_amd.functions import conv
    a = dict(x4=_f(_rng().standard_normal((1, 9, 11, 4)), dev), w784=_f(_rng(1).standard_normal((4, 7, 8, 4)), dev),
             b=_f(_rng(2).standard_normal(4), dev), scale=_f(_rng(3).uniform(.5, 1, 4), dev),
             shift=_f(_rng(4).standard_normal(4), dev))
    return a, lambda a: conv.stem_conv(a['x4'], a['w784'], a['b'], a['scale'], a['shift'])


@probe('conv.deconv2x2s2', ('x', 'W', 'b'), backward=True)
def _p(dev):
    from chainer_mask_rcnn_amd.functions import conv
    a = dict(x=_map((2, 8, 3, 4), dev, grad=True), W=_map((8, 4, 2, 2), dev, 1, True),
             b=_f(_rng(2).standard_normal(4), dev, True))
    return a, lambda a: conv.deconv2x2s2(a['x'], a['W'], a['b'], relu=True)


@probe('conv.epilogue_bwd', ('gy', 'y', 'scale'))
def _p(dev):
    from chainer_mask_rcnn_amd.functions import conv
    a = dict(gy=_map((2, 4, 3, 5), dev), y=_map((2, 4, 3, 5), dev, 1), scale=_f(_rng(2).uniform(.5, 1, 4), dev))
    return a, lambda a: conv.epilogue_bwd(a['gy'], a['y'], a['scale'])


@probe('conv.conv2d 1x3 (non-square filter: the direct dgrad)', ('x', 'W'), backward=True)
def _p(dev):
    from chainer_mask_rcnn_amd.functions import conv
    a = dict(x=_map((2, 4, 3, 7), dev, grad=True), W=_map((4, 4, 1, 3), dev, 1, True))
    return a, lambda a: conv.conv2d(a['x'], a['W'], None, 1, 0)


@probe('conv.conv2d with grad_rows (row-sparse backward)', ('x', 'W', 'b', 'rows', 'lookup'), backward=True,
       reroute=('rows', 'lookup'))
def _p(dev):
    from chainer_mask_rcnn_amd.functions import conv
    rows, lookup = conv.SparseRows.host_tables([3, 7, 20], 1 * 5 * 6)
    a = dict(x=_map((1, 4, 5, 6), dev, grad=True), W=_map((8, 4, 3, 3), dev, 1, True),
             b=_f(_rng(2).standard_normal(8), dev, True), rows=_i(rows, dev), lookup=_i(lookup, dev))

    def run(a):
        hint = conv.SparseRows()
        hint.set(a['rows'], a['lookup'], 3)
        return conv.conv2d(a['x'], a['W'], a['b'], 1, 1, relu=True, grad_rows=hint)
    return a, run


@probe('conv.deconv2x2s2 (fp32 arithmetic: the K-strided form)', ('x', 'W', 'b'))
def _p(dev):
    from chainer_mask_rcnn_amd.functions import conv
    a = dict(x=_map((2, 8, 3, 4), dev), W=_map((8, 4, 2, 2), dev, 1), b=_f(_rng(2).standard_normal(4), dev))

    def run(a):
        saved = conv.DECONV_FORWARD_FORM
        conv.DECONV_FORWARD_FORM = False
        try:
            return conv.deconv2x2s2(a['x'], a['W'], a['b'])
        finally:
            conv.DECONV_FORWARD_FORM = saved
    return a, run


def _on_winograd(fn):
    """Run ``fn`` with the routing thresholds lowered so that a small 3x3 layer takes the Winograd
    route the full-size RoI head takes (functions/conv.py:uses_winograd)."""
    from chainer_mask_rcnn_amd.functions import conv
    saved = conv.WINOGRAD_MIN_CHANNELS, conv.WINOGRAD_MIN_WORK
    conv.WINOGRAD_MIN_CHANNELS, conv.WINOGRAD_MIN_WORK = 8, 1
    try:
        return fn()
    finally:
        conv.WINOGRAD_MIN_CHANNELS, conv.WINOGRAD_MIN_WORK = saved


@probe('conv.conv2d 3x3 on the Winograd route', ('x', 'W', 'scale', 'shift'), backward=True)
def _p(dev):
    from chainer_mask_rcnn_amd.functions import conv
    a = dict(x=_map((3, 8, 7, 7), dev, grad=True), W=_map((8, 8, 3, 3), dev, 1, True),
             scale=_f(_rng(3).uniform(.5, 1, 8), dev), shift=_f(_rng(4).standard_normal(8), dev))

    def run(a):
        def both():
            y = conv.conv2d(a['x'], a['W'], None, 1, 1, a['scale'], a['shift'], relu=True)
            with torch.no_grad():       # inference: the transformed filter is built once and kept
                y0 = conv.conv2d(a['x'], a['W'], None, 1, 1, a['scale'], a['shift'], relu=True)
            conv.weights_changed()      # drop the kept transform with the probe's filter
            return y, y0
        return _on_winograd(both)
    return a, run


def _stage(dev, stride):
    from chainer_mask_rcnn_amd.models.resnet_extractor import BuildingBlock
    torch.manual_seed(0)
    blk = BuildingBlock(2, 8, 4, 16, stride=stride).to(dev)
    with torch.no_grad():
        for p in blk.parameters():
            p.copy_(torch.randn(p.shape) * 0.3)
    return blk


def _on_one_stream(fn):
    """Run ``fn`` with the stage's weight gradients on the calling stream: the side stream is a
    routing choice by size (functions/conv.py:SMALL_WGRAD_MAX_PIXELS), the launches are the same."""
    from chainer_mask_rcnn_amd.functions import conv
    saved = conv.SMALL_WGRAD_MAX_PIXELS
    conv.SMALL_WGRAD_MAX_PIXELS = -1
    try:
        return fn()
    finally:
        conv.SMALL_WGRAD_MAX_PIXELS = saved


@probe('conv.building_block (a fused stage)', ('x',), backward=True)
def _p(dev):
    blk = _stage(dev, 2)
    return dict(x=_map((2, 8, 6, 7), dev, grad=True)), lambda a: blk(a['x'])


@probe('conv.building_block: its filters and affine vectors', ('W1', 's1', 'b3', 'W4'), backward=True)
def _p(dev):
    blk = _stage(dev, 2)
    x = _map((2, 8, 6, 7), dev)
    a = dict(W1=blk.a.conv1.W.detach().clone().requires_grad_(True), s1=blk.a.bn1.W.detach().clone(),
             b3=blk.a.bn3.b.detach().clone(), W4=blk.a.conv4.W.detach().clone().requires_grad_(True))

    def run(a):
        # the tensors themselves stand in the links' parameter slots, so that the weight gradients
        # arrive on the arguments
        blk.a.conv1._parameters['W'], blk.a.conv4._parameters['W'] = a['W1'], a['W4']
        blk.a.bn1._parameters['W'], blk.a.bn3._parameters['b'] = a['s1'], a['b3']
        return blk(x)
    return a, run


@probe('conv.projected_map', ('x', 'W1', 'W4'))
def _p(dev):
    from chainer_mask_rcnn_amd.functions import conv
    a = dict(x=_map((2, 8, 6, 7), dev), W1=_map((4, 8, 1, 1), dev, 1), W4=_map((16, 8, 1, 1), dev, 2))

    def run(a):
        with torch.no_grad():
            out = conv.projected_map(a['x'], a['W1'], a['W4'])
        conv.weights_changed()
        return out
    return a, run


@probe('conv.building_block with roi= and tail_rows= (the RoI head)', ('x', 'rois', 'order', 'tail_rows'),
       backward=True)
def _p(dev):
    from chainer_mask_rcnn_amd.functions import conv
    blk = _stage(dev, 2)
    a = dict(x=_map((2, 8, 6, 7), dev, grad=True), rois=_rois(dev), order=_i([2, 0, 1], dev),
             tail_rows=_i([0, 2], dev, torch.int64))

    def run(a):
        spec = conv.RoiSpec(a['rois'], 14, 14, 0.25, bin_stride=2, order=a['order'])
        return blk(a['x'], first_stride=1, roi=spec, tail_rows=a['tail_rows'])
    return a, run


# -- functions/aug_merge.py, copy_paste.py, gt_masks.py, scale_jitter.py
@probe('aug_merge.decode_cls_boxes_views', ('roi', 'loc'))
def _p(dev):
    from chainer_mask_rcnn_amd.functions import aug_merge
    a = dict(roi=_boxes(3, dev), loc=_f(_rng(1).standard_normal((3, 8)) * 0.1, dev))
    return a, lambda a: aug_merge.decode_cls_boxes_views(
        [(a['roi'], a['loc'], 1.5, False), (a['roi'], a['loc'], 0.5, True)], 2, (0., 0., 0., 0.),
        (.1, .1, .2, .2), (48, 64))


@probe('aug_merge.mask_aug_combine', ('m0', 'm1'))
def _p(dev):
    from chainer_mask_rcnn_amd.functions import aug_merge
    a = dict(m0=_map((2, 4, 6, 6), dev), m1=_map((2, 4, 6, 6), dev, 1))
    return a, lambda a: aug_merge.mask_aug_combine([a['m0'], a['m1']], [False, True])


@probe('copy_paste.copy_paste', ('img_t', 'masks_t', 'img_s', 'masks_s'))
def _p(dev):
    import chainer_mask_rcnn_amd.functions.copy_paste  # noqa: F401  (the package attribute is the function)
    import sys
    CP = sys.modules['chainer_mask_rcnn_amd.functions.copy_paste']
    S = 8
    img = lambda seed: _f(_rng(seed).standard_normal((S, S, 3)), dev).permute(2, 0, 1)
    m = lambda seed, n: _i(_rng(seed).randint(0, 2, (n, S, S)), dev, torch.uint8)
    a = dict(img_t=img(0), masks_t=m(1, 2), img_s=img(2), masks_s=m(3, 3))
    return a, lambda a: CP.copy_paste(a['img_t'], a['masks_t'], a['img_s'], a['masks_s'], [0, 2])


def _words(dev, G=2, H=5, W=70, seed=0):
    """Packed masks (G, H, ceil(W / 64)) int64 with no bit beyond column W."""
    bits = _rng(seed).randint(0, 2, (G, H, 128)).astype(np.uint8)
    bits[:, :, W:] = 0
    words = np.packbits(bits, axis=2, bitorder='little').view(np.uint64).view(np.int64)
    return torch.tensor(words[:, :, :(W + 63) // 64].copy(), device=dev)


@probe('gt_masks.resize_masks_nearest', ('words',))
def _p(dev):
    from chainer_mask_rcnn_amd.functions import gt_masks
    return dict(words=_words(dev)), lambda a: gt_masks.resize_masks_nearest((a['words'], 70), (7, 90), True)


@probe('scale_jitter.resize_crop_masks', ('words',))
def _p(dev):
    from chainer_mask_rcnn_amd.functions import scale_jitter as SJ
    return dict(words=_words(dev)), lambda a: SJ.resize_crop_masks((a['words'], 70), (8, 100), (1, 10), 6)


@probe('scale_jitter.prepare_image_crop_device', ('src',))
def _p(dev):
    from chainer_mask_rcnn_amd.functions import scale_jitter as SJ
    a = dict(src=_f(_rng().uniform(0, 255, (3, 6, 9)), dev))
    return a, lambda a: SJ.prepare_image_crop_device((122., 115., 103.), a['src'], 1.5, (9, 14), (1, 2), 8, True)


# -- utils/evaluations
def _masks(dev, n=2, H=5, W=70, seed=0):
    return _i(_rng(seed).randint(0, 2, (n, H, W)), dev, torch.uint8)


@probe('evaluations.masks.pack_masks', ('masks',))
def _p(dev):
    from chainer_mask_rcnn_amd.utils.evaluations import masks as M
    return dict(masks=_masks(dev)), lambda a: M.pack_masks(a['masks'], device=dev)


@probe('evaluations.masks.paste_packed', ('roi_mask_logits',))
def _p(dev):
    from chainer_mask_rcnn_amd.utils.evaluations import masks as M
    a = dict(roi_mask_logits=_map((2, 4, 6, 6), dev))
    return a, lambda a: M.paste_packed(a['roi_mask_logits'], np.array([1, 3], np.int32),
                                       np.array([[1, 2, 9, 30], [0, 0, 12, 70]], np.float32), (12, 70))


@probe('evaluations.masks.queue_intersections', ('pa', 'ea', 'pb', 'eb'))
def _p(dev):
    from chainer_mask_rcnn_amd.utils.evaluations import masks as M
    ext = lambda n: _i([[0, 0, 5, 70]] * n, dev)
    a = dict(pa=_words(dev, 2), ea=ext(2), pb=_words(dev, 3, seed=1), eb=ext(3))
    return a, lambda a: M.queue_intersections((a['pa'], None, a['ea']), (a['pb'], None, a['eb']), 70)


@probe('evaluations.masks.boundary_packed', ('packed', 'extent'))
def _p(dev):
    from chainer_mask_rcnn_amd.utils.evaluations import masks as M
    a = dict(packed=_words(dev), extent=_i([[0, 0, 5, 70]] * 2, dev))
    return a, lambda a: M.boundary_packed((a['packed'], None, a['extent']), (5, 70), dilation=1)[:2]


@probe('evaluations.masks.mask_to_boundary', ('masks',))
def _p(dev):
    from chainer_mask_rcnn_amd.utils.evaluations import masks as M
    return dict(masks=_masks(dev)), lambda a: M.mask_to_boundary(a['masks'], dilation=1)


@probe('evaluations.boxes.queue_box_ious voc', ('a0', 'b0'))
def _p(dev):
    from chainer_mask_rcnn_amd.utils.evaluations import boxes as B
    a = dict(a0=_boxes(3, dev), b0=_boxes(2, dev, 1))
    return a, lambda a: B.queue_box_ious([a['a0'], np.zeros((0, 4), np.float32)],
                                         [a['b0'], np.ones((1, 4), np.float32)], 'voc', device=dev)[0]


@probe('evaluations.boxes.queue_box_ious coco', ('a0', 'b0'))
def _p(dev):
    from chainer_mask_rcnn_amd.utils.evaluations import boxes as B
    a = dict(a0=_boxes(3, dev).double(), b0=_boxes(2, dev, 1).double())
    return a, lambda a: B.queue_box_ious([a['a0']], [a['b0']], 'coco', crowd_b=[np.array([0, 1])],
                                         device=dev)[0]


@probe('evaluations.rle.queue_encode', ('packed', 'extent'))
def _p(dev):
    from chainer_mask_rcnn_amd.utils.evaluations import rle
    a = dict(packed=_words(dev), extent=_i([[0, 0, 5, 70]] * 2, dev))

    def run(a):
        job = rle.queue_encode(a['packed'], None, a['extent'], (5, 70))
        return [(c.val_off, c.str_off) for c in job.chunks]
    return a, run


@probe('evaluations.rle.decode_masks', ())
def _p(dev):
    from chainer_mask_rcnn_amd.utils.evaluations import rle

    def run(a):
        job = rle.queue_decode([{'size': [5, 7], 'counts': [3, 4, 28]}, {'size': [5, 7], 'counts': '34l0'}],
                               device=dev)
        return job.packed, job.status
    return {}, run


@probe('evaluations.rle.decode_masks unpacked', ())
def _p(dev):
    from chainer_mask_rcnn_amd.utils.evaluations import rle
    return {}, lambda a: rle.decode_masks([{'size': [5, 7], 'counts': [3, 4, 28]}])


# -- utils/geometry.py, utils/visualizations.py
@probe('geometry.label_instances', ('label_instance', 'label_class'),
       dry_fill={('mrcnn_label_scan', 'meta'): [0, 1, 2, 3, 2, 2]})
def _p(dev):
    from chainer_mask_rcnn_amd.utils import geometry
    ins = np.full((6, 8), -1, np.int32)
    ins[1:3, 1:4] = 0
    ins[3:6, 4:8] = 1
    cls = np.where(ins >= 0, ins + 2, 0).astype(np.int32)
    a = dict(label_instance=_i(ins, dev), label_class=_i(cls, dev))
    return a, lambda a: geometry.label_instances(a['label_instance'], a['label_class'], return_masks=True)


@probe('geometry.instance_boxes2label', ('masks',), rejects=(AssertionError,))   # the reference's assert
def _p(dev):
    from chainer_mask_rcnn_amd.utils import geometry
    a = dict(masks=_masks(dev, 2, 5, 9).bool())
    return a, lambda a: geometry.instance_boxes2label(np.array([2, 5]), None, a['masks'], np.array([.5, .25]))


@probe('visualizations.draw_instances_device', ('img', 'masks'))
def _p(dev):
    from chainer_mask_rcnn_amd.utils import visualizations as V
    a = dict(img=_i(_rng().randint(0, 255, (12, 16, 3)), dev, torch.uint8), masks=_masks(dev, 2, 12, 16))
    return a, lambda a: V.draw_instances_device(
        a['img'].clone() if a['img'].is_contiguous() else a['img'], [[1, 2, 8, 10], [3, 3, 11, 15]], [1, 2], 3,
        masks=a['masks'])


@probe('visualizations.tile_images_device', ('i0', 'i1'))
def _p(dev):
    from chainer_mask_rcnn_amd.utils import visualizations as V
    img = lambda seed, h, w: _i(_rng(seed).randint(0, 255, (h, w, 3)), dev, torch.uint8)
    a = dict(i0=img(0, 6, 8), i1=img(1, 5, 9))
    return a, lambda a: V.tile_images_device([a['i0'], a['i1']], (1, 2))


# -- optimizers.py
def _optimizer_probe(name, hook):
    @probe(name, ())
    def _p(dev):
        from chainer_mask_rcnn_amd import optimizers

        def run(a):
            torch.manual_seed(0)
            m = torch.nn.Module()
            m.w = torch.nn.Parameter(torch.randn(3, 5, device=dev))
            m.v = torch.nn.Parameter(torch.randn(7, device=dev))
            opt = optimizers.MomentumSGD(lr=0.1).setup(m)
            opt.add_hook(optimizers.WeightDecay(1e-4))
            if hook:
                opt.add_hook(optimizers.GradientClipping(0.5))
            opt.update(lambda: (m.w * m.w).sum() + (m.v * 2).sum())
            return m.w.detach(), m.v.detach(), flatten_outputs(dict(opt.report))
        return {}, run


_optimizer_probe('optimizers.MomentumSGD.update', False)
_optimizer_probe('optimizers.MomentumSGD.update with GradientClipping', True)


# -- the detection ops of models/mask_rcnn.py (methods, probed on a stand-in for the model)
def _model_stub(dev, **kw):
    import types
    from chainer_mask_rcnn_amd.models.mask_rcnn import MaskRCNN
    ns = types.SimpleNamespace(
        n_class=3, score_thresh=0.05, nms_thresh=0.3, soft_nms=None, bbox_vote_thresh=None,
        soft_nms_thresh=0.3, soft_nms_sigma=0.5, soft_nms_min_score=0.001,
        loc_normalize_mean=(0., 0., 0., 0.), loc_normalize_std=(.1, .1, .2, .2), mean=(122., 115., 103.),
        min_size=12, max_size=20, parameters=lambda: iter([torch.zeros(1, device=dev)]))
    ns.__dict__.update(kw)
    ns._suppress_queue = lambda cls_bbox, prob, n_views=1: MaskRCNN._suppress_queue(ns, cls_bbox, prob, n_views)
    return ns, MaskRCNN


def _cut(q):
    bbox, label, score, total = q
    d = _count(total)
    return bbox[:d], label[:d], score[:d], total


def _suppress_probe(name, **kw):
    @probe(name, ('cls_bbox', 'prob'))
    def _p(dev):
        ns, MaskRCNN = _model_stub(dev, **kw)
        a = dict(cls_bbox=torch.stack([_boxes(5, dev, s) for s in range(3)], 1),
                 prob=_f(_rng().uniform(0, 1, (5, 3)), dev))
        return a, lambda a: _cut(MaskRCNN._suppress_queue(ns, a['cls_bbox'], a['prob']))


_suppress_probe('MaskRCNN._suppress_queue')
_suppress_probe('MaskRCNN._suppress_queue with soft_nms and bbox_vote', soft_nms='linear', bbox_vote_thresh=0.8)


@probe('MaskRCNN._queue_detections', ('roi_cls_locs', 'roi_scores', 'rois'))
def _p(dev):
    ns, MaskRCNN = _model_stub(dev)
    a = dict(roi_cls_locs=_f(_rng().standard_normal((5, 12)) * 0.1, dev),
             roi_scores=_f(_rng(1).standard_normal((5, 3)), dev), rois=_boxes(5, dev))
    return a, lambda a: [_cut(q) for q in MaskRCNN._queue_detections(
        ns, a['roi_cls_locs'], a['roi_scores'], a['rois'], None, [(30, 40), (24, 40)], [1., 1.5],
        bounds=[0, 3, 5])]


@probe('MaskRCNN.prepare', ())
def _p(dev):
    ns, MaskRCNN = _model_stub(dev)
    imgs = [_rng().randint(0, 255, (3, 6, 9)).astype(np.uint8), _rng(1).uniform(0, 255, (3, 8, 7)).astype(np.float32)]
    return {}, lambda a: MaskRCNN.prepare(ns, imgs)[0]


@probe('MaskRCNN._to_masks', ('roi_masks',))
def _p(dev):
    ns, MaskRCNN = _model_stub(dev)
    a = dict(roi_masks=_map((2, 2, 6, 6), dev))
    return a, lambda a: MaskRCNN._to_masks(ns, [np.array([[1, 2, 9, 30], [0, 0, 12, 40]], np.float32)],
                                           [np.array([0, 1], np.int32)], None, [a['roi_masks']], [(12, 40)])
