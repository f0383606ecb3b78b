"""Every tensor that crosses the C ABI has the element type and the dense, aligned layout the
prototype in include/mrcnn_hip.h names (tests/abi_contract.py) — checked here without a device:
the recorder launches nothing, so CPU tensors stand in for device tensors."""
import ctypes
import re

import pytest
import torch

import abi_contract as A

CPU = torch.device('cpu')
CPU_PROBES = [p for p in A.PROBES if p.cpu]


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from chainer_mask_rcnn_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(scope='module')
def header():
    return A.parse_header()


# ---- the header parser ---------------------------------------------------------------------------
def test_every_signature_parses(lib, header):
    assert sorted(header) == sorted(lib.SIGNATURES)
    for name, (_, argtypes) in lib.SIGNATURES.items():
        params = header[name]
        assert len(params) == len(argtypes), name
        for prm, at in zip(params, argtypes):
            # a pointer in the header is a pointer in the binding, a scalar a scalar
            is_ptr = at in (ctypes.c_void_p, ctypes.c_char_p) or hasattr(at, 'contents')
            assert prm.pointer == is_ptr, (name, prm)
    p = {q.name: q for q in header['mrcnn_softmax_ce']}
    assert (p['x'].elem, p['x'].const) == ('float', True)
    assert (p['t'].elem, p['t'].const) == ('int32_t', True)
    assert (p['gx'].elem, p['gx'].const) == ('float', False)
    assert p['ws'].elem is None and p['ws'].pointer and not p['ldx'].pointer
    p = {q.name: q for q in header['mrcnn_box_iou_coco']}
    assert (p['boxes_a'].elem, p['crowd_b'].elem, p['out_off'].elem) == ('double', 'uint8_t', 'int64_t')
    p = {q.name: q for q in header['mrcnn_filter_flip_transpose_batched']}
    assert p['w'].elem is None and p['w'].pointer        # a host array of device pointers
    assert {q.name: q.elem for q in header['mrcnn_rle_encode']}['chars'] == 'char'


def test_row_strided_and_aligned_lists_name_real_parameters(header):
    for (entry, prm), ld in A.ROW_STRIDED.items():
        names = [q.name for q in header[entry]]
        assert prm in names and ld in names, (entry, prm, ld)
    for entry, names in A.ALIGNED_PARAMS.items():
        for n in names:
            q = [q for q in header[entry] if q.name == n]
            assert q and q[0].elem == 'float', (entry, n)
    assert any(A.ALIGNED_ENTRIES.match(e) for e in header)


# ---- the recorder catches each kind of violation -----------------------------------------------
def _fake_wrapper(entry, *tensors):
    """A wrapper with no check of its own: hands the tensors to the leading parameters."""
    from chainer_mask_rcnn_amd import _lib
    n = len(A.parse_header()[entry])
    args = [_lib.ptr(t) if isinstance(t, torch.Tensor) else t for t in tensors]
    _lib.call(entry, *(args + [0] * (n - len(args))))


@pytest.mark.parametrize('what, entry, make, expect', [
    ('wrong width', 'mrcnn_softmax', lambda: [torch.zeros(3, 4, dtype=torch.float64)], 'wrong width'),
    ('wrong kind', 'mrcnn_gather_rows', lambda: [torch.zeros(3, 4), torch.zeros(3)], 'wrong kind'),
    ('int64 index', 'mrcnn_gather_rows', lambda: [torch.zeros(3, 4), torch.arange(3)], 'wrong width'),
    ('bool is an 8-bit integer', 'mrcnn_topk_desc', lambda: [torch.zeros(4), torch.zeros(4, dtype=torch.bool)], None),
    ('strided', 'mrcnn_sigmoid_ce', lambda: [torch.zeros(4, 6)[::2, ::2]], 'not dense'),
    ('transposed', 'mrcnn_sigmoid_ce', lambda: [torch.zeros(4, 6).t()], 'not dense'),
    ('stride-0', 'mrcnn_sigmoid_ce', lambda: [torch.zeros(1, 6).expand(4, 6)], 'stride-0'),
    ('misaligned', 'mrcnn_affine_fwd', lambda: [torch.zeros(33)[1:]], '16-byte'),
    ('aligned', 'mrcnn_affine_fwd', lambda: [torch.zeros(36)[4:]], None),
    ('row-strided with a leading dimension', 'mrcnn_softmax', lambda: [torch.zeros(4, 8)[:, :5]], None),
    ('row-strided without one', 'mrcnn_anchor_labels', lambda: [torch.zeros(4, 8)[:, :5]], 'no leading dimension'),
    ('dense NHWC', 'mrcnn_maxpool3x3s2p1_fwd', lambda: [torch.zeros(2, 3, 5, 4).permute(0, 3, 1, 2)], None),
    ('gapped NHWC', 'mrcnn_maxpool3x3s2p1_fwd', lambda: [torch.zeros(2, 3, 5, 8).permute(0, 3, 1, 2)[:, :4]],
     'not dense'),
])
def test_recorder_catches(lib, what, entry, make, expect):
    with A.Recorder(dry=True) as rec:
        _fake_wrapper(entry, *make())
    bad = [v for c in rec.violations() for v in c.violations]
    if expect is None:
        assert not bad, (what, bad)
    else:
        assert any(expect in v for v in bad), (what, bad)
    assert rec.entries == [entry]


def test_recorder_restores_the_binding_and_zero_fills_outputs(lib):
    before = (lib.ptr, lib.addr, lib.call, lib.stream_ptr, lib.require_device, torch.cuda.device)
    y = torch.ones(3, 4)
    x = torch.ones(3, 4)
    with A.Recorder(dry=True):
        assert lib.ptr(None) is None
        lib.require_device(x)                     # neutralised: CPU tensors may be used
        _fake_wrapper('mrcnn_softmax', x, 4, y)
    assert (lib.ptr, lib.addr, lib.call, lib.stream_ptr, lib.require_device, torch.cuda.device) == before
    assert float(y.sum()) == 0. and float(x.sum()) == 12.    # y is `float *`, x `const float *`
    with pytest.raises(lib.MrcnnHipError):
        lib.require_device(x)
    with pytest.raises(AssertionError, match='arguments'):
        with A.Recorder(dry=True):
            lib.call('mrcnn_softmax', lib.ptr(x))


def test_perturbations_keep_shape_and_values():
    t = torch.arange(2 * 4 * 3 * 5, dtype=torch.float32).reshape(2, 4, 3, 5)
    labels = set()
    for label, v in A.layout_perturbations(t):
        labels.add(label)
        assert v.shape == t.shape and v.dtype == t.dtype
        assert label == 'expand' or torch.equal(v, t), label
        assert A.layout_of(v) == 'strided' or label in ('nhwc', 'offset_row', 'offset_elem'), label
    assert labels == {'rows2', 'cols2', 'transposed', 'nhwc', 'expand', 'offset_row', 'offset_elem'}
    assert dict(A.layout_perturbations(t))['offset_elem'].data_ptr() % 16 == 4
    assert [l for l, _ in A.dtype_perturbations(t)] == ['dtype:float64', 'dtype:int32']
    assert [l for l, _ in A.dtype_perturbations(t.int())] == ['dtype:int64', 'dtype:int16', 'dtype:float32']
    assert [l for l, _ in A.dtype_perturbations(t.long())] == ['dtype:int16', 'dtype:int32', 'dtype:float32']


# ---- the helper the wrappers share -------------------------------------------------------------
def test_dense_names_function_argument_and_both_dtypes(lib):
    x = torch.zeros(4, 6)
    assert lib.dense(x, torch.float32, 'f', 'x') is x
    assert lib.dense(x, torch.float32, 'f', 'x', align=True) is x
    with pytest.raises(TypeError) as e:
        lib.dense(x.double(), torch.float32, 'softmax', 'x')
    for word in ('softmax', 'x', 'torch.float32', 'torch.float64'):
        assert word in str(e.value)
    for view in (x[::2], x.t(), x[:1].expand(4, 6), x[:, :5]):
        d = lib.dense(view, torch.float32, 'f', 'x')
        assert d.is_contiguous() and d.data_ptr() != view.data_ptr() and torch.equal(d, view)
    off = torch.zeros(25)[1:].view(4, 6)
    assert lib.dense(off, torch.float32, 'f', 'x') is off
    d = lib.dense(off, torch.float32, 'f', 'x', align=True)
    assert d is not off and d.data_ptr() % 16 == 0
    from chainer_mask_rcnn_amd.functions._layout import nhwc
    m = nhwc(torch.zeros(2, 4, 3, 5))
    assert nhwc(m, torch.float32, 'f') is m
    with pytest.raises(TypeError, match=r'max_pooling_2d: x must be torch.float32, got torch.float64'):
        nhwc(m.double(), torch.float32, 'max_pooling_2d')
    i = nhwc(torch.zeros(2, 4, 3, 5, dtype=torch.int32), torch.int32, 'f')     # not float-only
    assert i.dtype == torch.int32
    shifted = torch.as_strided(torch.zeros(121), m.shape, m.stride(), 1)
    assert nhwc(shifted).data_ptr() % 16 == 0


# ---- the dry sweep of the whole table ----------------------------------------------------------
@pytest.mark.parametrize('p', CPU_PROBES, ids=[p.name for p in CPU_PROBES])
def test_dry_sweep(lib, p):
    """Every perturbed call either raises TypeError / ValueError or hands over only tensors that
    obey the rule; nothing is launched."""
    fails, entries = A.dry_sweep(p, CPU)
    assert not fails, '\n'.join(fails)
    assert entries, 'the row reached no entry point'


def test_rejections_name_the_argument_and_the_dtypes(lib):
    """Where a wrapper refuses a dtype through the shared helper, the message names the function,
    the argument, the expected and the received dtype."""
    from chainer_mask_rcnn_amd.functions import loss, proposal_ops, target_ops
    cases = [
        (lambda: loss.softmax(torch.zeros(2, 3, dtype=torch.float64)), 'softmax', 'x', 'float32', 'float64'),
        (lambda: proposal_ops.gather_rows(torch.zeros(3, 4), torch.arange(3)), 'gather_rows', 'idx', 'int32', 'int64'),
        (lambda: proposal_ops.nms_sorted(torch.zeros(3, 4).double(), .5), 'nms_sorted', 'bbox', 'float32', 'float64'),
        (lambda: loss.fast_rcnn_loc_loss(torch.zeros(2, 8), torch.zeros(2, 4), torch.zeros(2, dtype=torch.int32),
                                         3., torch.zeros(2, dtype=torch.int64)),
         'fast_rcnn_loc_loss', 'cls', 'int32', 'int64'),
        (lambda: target_ops.anchor_labels(torch.zeros(3, 2).half(), torch.zeros(3), torch.zeros(2), .3, .7),
         'anchor_labels', 'iou', 'float32', 'float16'),
    ]
    with A.Recorder(dry=True) as rec:
        for call, fn, arg, want, got in cases:
            with pytest.raises(TypeError) as e:
                call()
            msg = str(e.value)
            assert msg.startswith(fn + ':') and re.search(r'\b%s\b' % arg, msg), msg
            assert 'torch.' + want in msg and 'torch.' + got in msg, msg
    assert rec.entries == []


# ---- completeness ------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def recorded(lib):
    seen = set()
    for p in CPU_PROBES:
        fails, _, entries = A.baseline(p, CPU)
        assert not fails, fails
        seen.update(entries)
    return seen


def test_every_call_site_is_covered(recorded, header):
    """The entry points the package launches = those the dry sweep records + those the live GPU run
    (tests/test_gpu_abi_contract.py) is declared to cover + the exempted collectives."""
    sites = A.scan_call_sites()
    named = A.scan_named_entries()
    assert len(sites) >= 70 and set(sites) <= set(named) <= set(header)
    launched = {e for e in named if not e.endswith('_workspace_bytes')}
    collectives = {e for e in launched if e.startswith('mrcnn_allreduce_')}
    assert not recorded & set(A.LIVE_COVERED), 'recorded without a device: take it off LIVE_COVERED'
    assert launched - collectives == recorded | set(A.LIVE_COVERED), (
        'not covered: %s; covered but never called: %s'
        % (sorted(launched - collectives - recorded - set(A.LIVE_COVERED)),
           sorted((recorded | set(A.LIVE_COVERED)) - launched)))
    assert collectives <= set(A.EXEMPT)


def test_live_list_holds_only_what_needs_the_model(header):
    """Only entry points whose every call site lies in models/ may be left to the live run."""
    sites = A.scan_call_sites()
    for entry, reason in A.LIVE_COVERED.items():
        assert entry in header and reason
        assert sites[entry] and all(f.startswith('models/') for f in sites[entry]), entry


def test_a_refusal_states_a_contract():
    ok = 'rejected: TypeError: softmax: x must be torch.float32, got torch.float64'
    assert A.rejection_problem(ok, torch.float32, torch.float64) is None
    assert A.rejection_problem(ok) is None
    assert 'names' in A.rejection_problem(ok, torch.float32, torch.int32)
    assert A.rejection_problem('rejected: TypeError: sigmoid_cross_entropy: t must be int32',
                               torch.int32, torch.int64) is None
    assert 'expected dtype' in A.rejection_problem('rejected: ValueError: bbox must be (G, n_max, 4)',
                                                   torch.float32, torch.float64)
    assert 'no contract' in A.rejection_problem(
        "rejected: ValueError: only one element tensors can be converted to Python scalars")
    assert 'no contract' in A.rejection_problem('rejected: TypeError: expected Tensor as element 0')


def test_table_fields_name_real_table_parameters(header):
    """Every declared table field belongs to an entry point with a pointer-table parameter."""
    for (entry, field), (elem, _, _, _) in A.TABLE_FIELDS.items():
        assert elem in A.C_TYPES
        assert any(q.pointer and q.elem is None and q.name not in ('stream',) for q in header[entry]) \
            or any(q.name == field for q in header[entry]), (entry, field)


def test_exemptions_are_collectives_or_have_no_caller(header):
    named = A.scan_named_entries()
    for entry, reason in A.EXEMPT.items():
        assert entry in header and reason, entry
        if entry.startswith('mrcnn_allreduce_'):
            continue
        assert entry not in named, '%s is exempt as uncalled but %s names it' % (entry, named[entry])
    # and nothing else escapes: an entry point that takes a device pointer is called (and covered
    # above), or exempt
    takes_tensors = {e for e, ps in header.items()
                     if any(q.pointer and q.name not in ('stream', 'd') for q in ps)}
    uncovered = takes_tensors - set(named) - set(A.EXEMPT)
    assert not uncovered, sorted(uncovered)
