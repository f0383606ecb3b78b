"""The packed-mask codec and counting kernels (csrc/mask_eval.hip: mask_pack, mask_intersect;
csrc/mask_rle.hip: rle_encode, rle_decode, mask_unpack) at their row, word and extent edges: the
case lists of tests/packed_mask_cases.py on the device, against that module's dense NumPy
references.  Integer kernels: every comparison is exact.

These kernels read and write through caller-sized buffers and a wrong chunk boundary faults
nothing: it gives a count that is slightly off.  So beside the values, the outputs of the direct
C-ABI calls live inside poison-filled buffers with guard bands (packed_mask_cases.Guarded), and
what a call must not write has to hold the poison afterwards.  Every library call of this module,
direct or through the wrappers, runs under the live ABI recorder of tests/abi_contract.py.
"""
import numpy as np
import pytest
import torch

import abi_contract as A
import packed_mask_cases as K
from chainer_mask_rcnn_amd import _lib
from chainer_mask_rcnn_amd.utils.evaluations import masks as M
from chainer_mask_rcnn_amd.utils.evaluations import rle as R
from oracle import np_data
from test_coco_results_cpu import np_rle_counts, np_rle_string

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def abi_checked():
    """Every tensor handed to the library is held to the header's contract; a call that breaks it
    raises instead of launching."""
    with A.Recorder(dry=False) as rec:
        yield rec
    assert not rec.violations(), A.format_crossings(rec.violations())


def _dev(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t if dtype is None else t.to(dtype)


def _u64(t):
    """A packed int64 device tensor as host uint64."""
    return t.cpu().numpy().view(np.uint64)


def _check_triple(triple, masks, what):
    """(packed, area, extent) == the reference words (pad bits zero), exact areas, tight extents."""
    packed, area, extent = triple
    assert np.array_equal(_u64(packed), K.ref_pack(masks)), '%s: packed words' % what
    assert np.array_equal(area.cpu().numpy(), K.ref_area(masks)), '%s: areas' % what
    ext = extent.cpu().numpy()
    for n, m in enumerate(masks):
        want = K.ref_extent(m)
        if want is None:
            assert ext[n, 0] >= ext[n, 1] and ext[n, 2] >= ext[n, 3], '%s: extent of empty mask %d: %s' % (what, n, ext[n])
        else:
            assert tuple(ext[n]) == want, '%s: extent of mask %d: %s, tight is %s' % (what, n, ext[n], want)


def _encode(packed, extent, H, W):
    """-> (count lists, strings) through queue_encode / fetch_encoded."""
    job = R.queue_encode(packed, None, extent, (H, W))
    counts = [r['counts'] for r in R.fetch_encoded([job], uncompressed=True)[0]]
    job = R.queue_encode(packed, None, extent, (H, W))
    return counts, [r['counts'] for r in R.fetch_encoded([job])[0]]


def _decode(entries, H, W):
    """Strings or count lists -> ((packed, area, extent), host status) through queue_decode."""
    job = R.queue_decode([{'size': [H, W], 'counts': c} for c in entries])
    return job.packed, job.status.cpu().numpy()


def _unpack_guarded(packed, N, H, W):
    g = K.Guarded(N * H * W, torch.uint8, packed.device)
    _lib.call('mrcnn_mask_unpack', _lib.ptr(packed), N, H, W, _lib.ptr(g.out), _lib.stream_ptr())
    return g


def _intersect(pa, ea, pb, eb, H, W):
    g = K.Guarded(pa.shape[0] * pb.shape[0], torch.int32, pa.device)
    _lib.call('mrcnn_mask_intersect', _lib.ptr(pa), _lib.ptr(ea), pa.shape[0], _lib.ptr(pb), _lib.ptr(eb),
              pb.shape[0], H, W, _lib.ptr(g.out), _lib.stream_ptr())
    out = g.host().reshape(pa.shape[0], pb.shape[0]).astype(np.int64)
    assert g.guards_intact(), 'mask_intersect wrote outside inter'
    return out


# ---------------------------------------------------------------------------------- section 1
@pytest.mark.parametrize('H, W', K.SHAPES, ids=['%dx%d' % s for s in K.SHAPES])
def test_shape(dev, H, W):
    """Pack (three input types), unpack, encode, decode (strings and lists) and intersect at one
    shape of the row-chunk / word grid."""
    names, masks = K.shape_masks(H, W)
    N, Wq = len(masks), K.words(W)
    counts, strings = K.ref_rle(masks)
    # pack: every input type gives the reference words, areas and tight extents
    packed = None
    for kind, a in K.pack_inputs(masks).items():
        t = _dev(a, dev)
        assert t.dtype == {'uint8': torch.uint8, 'bool': torch.bool, 'int32': torch.int32}[kind]
        packed = M.pack_masks(t)
        _check_triple(packed, masks, 'pack(%s)' % kind)
    pk, area, ext = packed
    # unpack(pack(m)) == m, nothing written outside the output
    g = _unpack_guarded(pk, N, H, W)
    assert np.array_equal(g.host().reshape(N, H, W), masks), 'unpack(pack(m))'
    assert g.guards_intact(), 'mask_unpack wrote outside its output'
    # encode: counts and strings
    got_c, got_s = _encode(pk, ext, H, W)
    for n in range(N):
        assert got_c[n] == counts[n], 'counts of %s' % names[n]
        assert got_s[n] == strings[n], 'string of %s' % names[n]
    # decode from strings and from count lists: words, areas, tight extents
    for what, entries in (('strings', strings), ('lists', counts)):
        triple, status = _decode(entries, H, W)
        assert not status.any(), 'decode(%s): status %s' % (what, status)
        _check_triple(triple, masks, 'decode(%s)' % what)
    # intersections of every pair, with the tight extents and with full ones
    want = K.ref_intersections(masks, masks)
    assert np.array_equal(_intersect(pk, ext, pk, ext, H, W), want), 'intersect, tight extents'
    full = _dev(np.tile(np.array([0, H, 0, Wq], np.int32), (N, 1)), dev)
    assert np.array_equal(_intersect(pk, full, pk, full, H, W), want), 'intersect, full extents'
    assert np.array_equal(_intersect(pk, full, pk, ext, H, W), want), 'intersect, full x tight'


# ---------------------------------------------------------------------------------- section 2
@pytest.mark.parametrize('case', K.EXTENT_CASES, ids=[c.name for c in K.EXTENT_CASES])
def test_encode_under_every_admissible_extent(dev, case):
    """Whatever extent contains the set bits — tight, full, all rows of some words, some rows of all
    words, a row or word of slack on one side, values outside the image — the counts and strings
    are those of the dense reference."""
    names, masks = K.extent_masks(case)
    counts, strings = K.ref_rle(masks)
    pk = _dev(K.ref_pack(masks).view(np.int64), dev)
    for kind, e in K.admissible_extents(case, masks):
        got_c, got_s = _encode(pk, _dev(e, dev), case.H, case.W)
        for n in range(len(masks)):
            assert got_c[n] == counts[n], 'extent %s %s: counts of %s' % (kind, e[n], names[n])
            assert got_s[n] == strings[n], 'extent %s %s: string of %s' % (kind, e[n], names[n])


@pytest.mark.parametrize('case', K.INTERSECT_CASES, ids=[c.name for c in K.INTERSECT_CASES])
def test_intersect_reads_the_clamped_overlap_and_nothing_else(dev, case):
    """Admissible extents give the dense counts; extents that cut bits off give the dense counts of
    the clamped overlap rectangle; disjoint extents give 0."""
    a, b = K.intersect_sets(case)
    pa, pb = (_dev(K.ref_pack(m).view(np.int64), dev) for m in (a, b))
    dense = K.ref_intersections(a, b)
    for name, ea, eb, kind in K.intersect_runs(case, a, b):
        got = _intersect(pa, _dev(ea, dev), pb, _dev(eb, dev), case.H, case.W)
        if kind == 'admissible':
            want = dense
        elif kind == 'cut':
            want = K.restricted_intersections(a, b, ea, eb)
        else:
            want = np.zeros_like(dense)
        assert np.array_equal(got, want), '%s (%s): %s, reference %s' % (name, kind, got.tolist(), want.tolist())


# ---------------------------------------------------------------------------------- section 3
@pytest.fixture(scope='module')
def cap_ref():
    return K.CapReference()


def _encode_capped(dev, ref, pk, ext, cap_values, cap_chars):
    """One direct mrcnn_rle_encode with the given caps; pos, counts and chars are eight elements
    longer than the reference's totals, so that every cap of the sweep lies inside the buffer."""
    H, W = K.CAP_SHAPE
    N = len(ref.masks)
    size_v, size_c = ref.V + 8, ref.C + 8
    assert cap_values <= size_v and cap_chars <= size_c
    bufs = dict(chg_off=K.Guarded(N * K.words(W) + 1, torch.int32, dev), val_off=K.Guarded(N + 1, torch.int32, dev),
                pos=K.Guarded(size_v, torch.int32, dev), counts=K.Guarded(size_v, torch.int32, dev),
                str_off=K.Guarded(N + 1, torch.int32, dev), chars=K.Guarded(size_c, torch.uint8, dev))
    _lib.call('mrcnn_rle_encode', _lib.ptr(pk), _lib.ptr(ext), N, H, W, _lib.ptr(bufs['chg_off'].out),
              _lib.ptr(bufs['val_off'].out), _lib.ptr(bufs['pos'].out), _lib.ptr(bufs['counts'].out), int(cap_values),
              _lib.ptr(bufs['str_off'].out), _lib.ptr(bufs['chars'].out), int(cap_chars), _lib.stream_ptr())
    what = 'cap_values %d, cap_chars %d' % (cap_values, cap_chars)
    for name, g in bufs.items():
        assert g.guards_intact(), '%s: the guard band of %s was written' % (what, name)
    want_so, want_counts, want_chars = ref.expected(cap_values, cap_chars, size_v, size_c)
    assert np.array_equal(bufs['val_off'].host(), ref.val_off), '%s: val_off' % what
    assert np.array_equal(bufs['str_off'].host(), want_so), '%s: str_off' % what
    got = bufs['counts'].host()
    bad = np.flatnonzero(got != want_counts)
    assert not len(bad), '%s: counts[%d] = %d, expected %d (%d is the poison)' % (
        what, bad[0], got[bad[0]], want_counts[bad[0]], K.POISON_I32)
    got = bufs['chars'].host()
    bad = np.flatnonzero(got != want_chars)
    assert not len(bad), '%s: chars[%d] = %d, expected %d (%d is the poison)' % (
        what, bad[0], got[bad[0]], want_chars[bad[0]], K.POISON_U8)
    pos = bufs['pos'].host()
    assert (pos[cap_values:] == K.POISON_I32).all(), '%s: pos written at or past the cap' % what
    # the scratch of a mask that did not fit stays untouched too: the changes of mask n start at
    # val_off[n] - n (one count more than changes per mask)
    first_unfit = next((n for n in range(N) if ref.val_off[n + 1] > cap_values), N)
    assert (pos[int(ref.val_off[first_unfit]) - first_unfit:] == K.POISON_I32).all(), \
        '%s: pos written for a mask that did not fit' % what


def test_encode_value_caps(dev, cap_ref):
    """cap_values at 0, 1, inside a mask, on every mask boundary and one either side, one short of
    the total, the total and beyond, with ample characters."""
    pk, _, ext = M.pack_masks(cap_ref.masks)
    for cap in cap_ref.value_caps():
        _encode_capped(dev, cap_ref, pk, ext, cap, cap_ref.C + 8)


def test_encode_char_caps(dev, cap_ref):
    """cap_chars at 0, inside a string, on every string boundary and one either side, one short of
    the total and the total, with exactly enough values."""
    pk, _, ext = M.pack_masks(cap_ref.masks)
    for cap in cap_ref.char_caps():
        _encode_capped(dev, cap_ref, pk, ext, cap_ref.V, cap)


@pytest.mark.parametrize('small', ['values', 'chars'])
def test_fetch_encoded_retries_with_exact_buffers(dev, cap_ref, monkeypatch, small):
    """Both retry paths of fetch_encoded, forced through the running estimate: counts that outgrow
    their buffer (one value per mask), and ample counts whose strings outgrow theirs."""
    N = len(cap_ref.masks)
    packed = M.pack_masks(cap_ref.masks)
    for uncompressed, want in ((False, cap_ref.strings), (True, cap_ref.counts)):
        # (a fetch grows the estimate: set it anew for each)
        monkeypatch.setitem(R._per_mask, 'values', 1 if small == 'values' else 1024)
        monkeypatch.setitem(R._per_mask, 'chars', 2048 if small == 'values' else 1)
        job = R.queue_encode(*packed, size=K.CAP_SHAPE)
        c = job.chunks[0]
        if small == 'values':
            assert c.cap_values == N < cap_ref.V
        else:
            assert c.cap_values >= cap_ref.V and c.cap_chars == N < cap_ref.C
        got = R.fetch_encoded([job], uncompressed)[0]
        assert c.cap_values >= cap_ref.V and c.cap_chars >= cap_ref.C          # it launched again
        assert [g['counts'] for g in got] == want
        assert all(g['size'] == list(K.CAP_SHAPE) for g in got)


# ---------------------------------------------------------------------------------- section 4
@pytest.mark.parametrize('H, W', K.CHAR_BOUNDARY_SHAPES, ids=['%dx%d' % s for s in K.CHAR_BOUNDARY_SHAPES])
def test_single_count_at_character_boundaries(dev, H, W):
    """[HW] and [HW - 1, 1] with HW on both sides of 2^4, 2^9, 2^14, 2^19 and 2^24: encode from the
    dense image, decode the string back.  One mask at a time (4096 x 4096 is 16 MB dense)."""
    for last in (0, 1):
        m = np.zeros((1, H, W), np.uint8)
        m[0, H - 1, W - 1] = last
        counts = [H * W - 1, 1] if last else [H * W]
        want = np_rle_string(counts)
        packed = M.pack_masks(_dev(m, dev))
        got_c, got_s = _encode(packed[0], packed[2], H, W)
        assert got_c == [counts] and got_s == [want]
        triple, status = _decode([want], H, W)
        assert status.tolist() == [0]
        _check_triple(triple, m, 'decode(%r)' % want)
        triple, status = _decode([counts], H, W)
        assert status.tolist() == [0]
        _check_triple(triple, m, 'decode(%s)' % counts)


def test_deltas_at_character_boundaries(dev):
    """Stored values count[3] - count[1] = +-(2^k - 1), +-2^k, +-(2^k + 1) for k = 4, 9, 14: decode
    the list, encode it back, compare with the reference string; and decode that string."""
    for name, H, W, counts in K.delta_count_lists():
        m = K.counts_to_mask(counts, H, W)[None]
        want = np_rle_string(counts)
        triple, status = _decode([counts], H, W)
        assert status.tolist() == [0], name
        _check_triple(triple, m, 'delta %s: decode(list)' % name)
        got_c, got_s = _encode(triple[0], triple[2], H, W)
        assert got_c == [counts], 'delta %s' % name
        assert got_s == [want], 'delta %s: %r, reference %r' % (name, got_s[0], want)
        triple, status = _decode([want], H, W)
        assert status.tolist() == [0], name
        _check_triple(triple, m, 'delta %s: decode(string)' % name)


def test_seven_character_values_decode(dev):
    """H * W >= 2^29 needs seven characters, which the encoder's size limit keeps it from ever
    producing: decode only.  [HW] and [HW - 1, 1] as strings at 23171 x 23171 (67 MB packed, never
    unpacked or held dense); area, extent and the non-zero words are checked on the device."""
    H, W = K.SEVEN_CHAR_SHAPE
    Wq = K.words(W)
    for counts, area, ext in (([H * W], 0, None), ([H * W - 1, 1], 1, (H - 1, H, Wq - 1, Wq))):
        s = np_rle_string(counts)
        (packed, got_area, got_ext), status = _decode([s], H, W)
        assert status.tolist() == [0]
        assert got_area.tolist() == [area]
        e = got_ext[0].tolist()
        if ext is None:
            assert e[0] >= e[1] and e[2] >= e[3]
        else:
            assert tuple(e) == ext
        assert int(torch.count_nonzero(packed)) == area
        if area:
            assert int(packed[0, H - 1, Wq - 1]) == 1 << ((W - 1) & 63)
        del packed


def _decode_abi(dev, entries, H, W):
    """One direct mrcnn_rle_decode of strings (all entries str) or count lists, every output in a
    guarded buffer.  -> {name: Guarded}."""
    is_str = isinstance(entries[0], str)
    N, Wq = len(entries), K.words(W)
    data = [np.frombuffer(e.encode('latin-1'), np.uint8) if is_str else np.asarray(e, np.int64).astype(np.int32)
            for e in entries]
    off = np.concatenate([[0], np.cumsum([len(d) for d in data])]).astype(np.int32)
    flat = np.concatenate(data + [np.zeros(1, np.uint8 if is_str else np.int32)])
    data_d, off_d = _dev(flat, dev), _dev(off, dev)
    bufs = dict(starts=K.Guarded(max(int(off[-1]), 1), torch.int32, dev), nval=K.Guarded(N, torch.int32, dev),
                status=K.Guarded(N, torch.int32, dev), packed=K.Guarded(N * H * Wq, torch.int64, dev),
                area=K.Guarded(N, torch.int32, dev), extent=K.Guarded(4 * N, torch.int32, dev))
    _lib.call('mrcnn_rle_decode', _lib.ptr(data_d) if is_str else None, None if is_str else _lib.ptr(data_d),
              _lib.ptr(off_d), N, H, W, _lib.ptr(bufs['starts'].out), _lib.ptr(bufs['nval'].out),
              _lib.ptr(bufs['status'].out), _lib.ptr(bufs['packed'].out), _lib.ptr(bufs['area'].out),
              _lib.ptr(bufs['extent'].out), _lib.stream_ptr())
    torch.cuda.synchronize()
    for name, g in bufs.items():
        assert g.guards_intact(), 'rle_decode wrote outside %s' % name
    return bufs


def _check_decoded_abi(bufs, masks, statuses, H, W, what):
    """Entries with status OK decode to ``masks[n]`` exactly; every other entry is all zero, with
    area 0 and an empty extent."""
    N, Wq = len(statuses), K.words(W)
    assert bufs['status'].host().tolist() == list(statuses), what
    packed = bufs['packed'].host().view(np.uint64).reshape(N, H, Wq)
    area, ext = bufs['area'].host(), bufs['extent'].host().reshape(N, 4)
    for n in range(N):
        if statuses[n] == K.OK:
            assert np.array_equal(packed[n], K.ref_pack(masks[n][None])[0]), '%s: words of entry %d' % (what, n)
            assert area[n] == int(masks[n].sum()), '%s: area of entry %d' % (what, n)
            want = K.ref_extent(masks[n])
            if want is not None:
                assert tuple(ext[n]) == want, '%s: extent of entry %d' % (what, n)
        else:
            assert not packed[n].any(), '%s: entry %d (status %d) left set bits' % (what, n, statuses[n])
            assert area[n] == 0, '%s: entry %d (status %d) has area %d' % (what, n, statuses[n], area[n])
        if statuses[n] != K.OK or not masks[n].any():
            assert ext[n, 0] >= ext[n, 1] and ext[n, 2] >= ext[n, 3], '%s: extent %s of entry %d' % (what, ext[n], n)


def test_noncanonical_strings(dev):
    """35 with redundant zero groups, 2, 3 and 7 characters long, decodes as the oracle's parser
    reads it; 8 groups are UNTERMINATED."""
    H, W = K.NONCANONICAL_SHAPE
    entries = list(K.NONCANONICAL_OK) + [K.NONCANONICAL_TOO_LONG]
    masks = [np_data.rle_decode({'size': [H, W], 'counts': np_data.rle_from_string(s)}) for s in entries]
    assert not np.stack(masks).any()
    bufs = _decode_abi(dev, entries, H, W)
    _check_decoded_abi(bufs, masks, [K.OK] * 3 + [K.UNTERMINATED], H, W, 'noncanonical')
    assert bufs['nval'].host()[:3].tolist() == [1, 1, 1]
    # and set bits after a long form: [0, 35] with the 35 written in seven groups
    s = '0' + K.NONCANONICAL_OK[2]
    assert np_data.rle_from_string(s) == [0, 35]
    bufs = _decode_abi(dev, [s], H, W)
    _check_decoded_abi(bufs, [np.ones((H, W), np.uint8)], [K.OK], H, W, 'noncanonical full')


def test_zero_length_runs(dev):
    """Count lists with zero-length runs (repeated run starts under the fill kernel's binary search
    and run-following loop) against the oracle's per-pixel decoder."""
    by_shape = {}
    for H, W, c in K.zero_run_lists():
        by_shape.setdefault((H, W), []).append(c)
    for (H, W), lists in by_shape.items():
        masks = [np_data.rle_decode({'size': [H, W], 'counts': list(c)}) for c in lists]
        bufs = _decode_abi(dev, lists, H, W)
        _check_decoded_abi(bufs, masks, [K.OK] * len(lists), H, W, 'zero runs %dx%d' % (H, W))
        assert bufs['nval'].host().tolist() == [len(c) for c in lists]
        # pycocotools merges the runs: encoding the result gives the canonical list
        pk = bufs['packed'].out.view(len(lists), H, K.words(W))
        got_c, _ = _encode(pk, bufs['extent'].out.view(len(lists), 4), H, W)
        assert got_c == [np_rle_counts(m).tolist() for m in masks]


@pytest.mark.parametrize('entries', [K.malformed_strings(), K.malformed_lists()], ids=['strings', 'lists'])
def test_malformed_entries_among_valid_ones(dev, entries):
    """One call that mixes valid and malformed entries: exact status per entry, every non-OK entry
    all zero with area 0 and an empty extent, valid entries exact, nothing written outside starts,
    nval, status, packed, area and extent."""
    H, W = K.MALFORMED_SHAPE
    data = [c for c, _ in entries]
    statuses = [s for _, s in entries]
    masks = [np_data.rle_decode({'size': [H, W], 'counts': np_data.rle_from_string(c) if isinstance(c, str) else c})
             if s == K.OK else np.zeros((H, W), np.uint8) for c, s in entries]
    bufs = _decode_abi(dev, data, H, W)
    _check_decoded_abi(bufs, masks, statuses, H, W, 'malformed')
    assert any(m.any() for m, s in zip(masks, statuses) if s == K.OK)
