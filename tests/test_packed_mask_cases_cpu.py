"""The conditions that make the case lists of tests/packed_mask_cases.py worth running on the
device (tests/test_gpu_packed_mask_edges.py): each list really holds the boundary it claims, and
each NumPy reference agrees with the oracle's per-pixel codec.  No GPU."""
import numpy as np

import packed_mask_cases as K
from oracle import np_data
from test_coco_results_cpu import np_rle_counts, np_rle_string


# ------------------------------------------------------------------------------ references
def test_ref_pack_is_the_documented_bit_layout():
    rng = np.random.RandomState(0)
    for H, W in ((1, 1), (3, 63), (2, 64), (3, 65), (2, 130)):
        m = rng.randint(0, 3, (2, H, W))
        p = K.ref_pack(m)
        assert p.shape == (2, H, K.words(W)) and p.dtype == np.uint64
        for n, y, x in np.ndindex(2, H, K.words(W) * 64):
            bit = (int(p[n, y, x >> 6]) >> (x & 63)) & 1
            assert bit == (1 if x < W and m[n, y, x] else 0)
    assert K.ref_extent(np.zeros((3, 3))) is None
    m = np.zeros((5, 200), np.uint8)
    m[1, 64] = m[3, 127] = 1
    assert K.ref_extent(m) == (1, 4, 1, 2)


def test_counts_to_mask_equals_the_oracle_decoder():
    for H, W, c in K.zero_run_lists():
        if H * W <= 5000:
            assert np.array_equal(K.counts_to_mask(c, H, W), np_data.rle_decode({'size': [H, W], 'counts': list(c)}))
    m = (np.random.RandomState(1).uniform(size=(9, 70)) < 0.4).astype(np.uint8)
    assert np.array_equal(K.counts_to_mask(np_rle_counts(m), 9, 70), m)


# ---------------------------------------------------------------------------------- section 1
def test_shapes_hold_the_row_chunk_and_word_boundaries():
    hs = {H for H, _ in K.SHAPES}
    assert {63, 64, 65, 127, 128, 129, 1} <= hs
    assert {1, 63, 64, 65, 128, 129} <= {W for _, W in K.SHAPES}
    wide = {(H, K.words(W)) for H, W in K.SHAPES if W > 129}
    assert {64, 65} <= {wq for _, wq in wide}
    assert {H for H, _ in wide} == {1, 3, 65}
    assert {W for _, W in K.SHAPES if W > 129} == {4096, 4097, 4160}
    # every small H meets every small W
    assert {(H, W) for H in K.SHAPE_HS for W in K.SHAPE_WS} <= set(K.SHAPES)


def test_shape_masks_hold_what_their_names_say():
    for H, W in ((129, 129), (65, 4160), (1, 1), (64, 64), (128, 65), (63, 128)):
        names, ms = K.shape_masks(H, W)
        assert len(set(names)) == len(names) == len(ms) and ms.dtype == np.uint8
        d = dict(zip(names, ms))
        assert d['empty'].sum() == 0 and d['full'].all()
        assert d['cornerHW'][H - 1, W - 1] == 1 and d['cornerHW'].sum() == 1
        assert 0.3 < d['bernoulli_0.5'].mean() < 0.7 or H * W < 64
        # the last row of every 64-row chunk and the first of the next, in one column
        for k in range(64, H, 64):
            assert d['chunk_edges_x0'][k - 1, 0] and d['chunk_edges_x0'][k, 0]
        for k in range(64, W, 64):
            assert d['word_edges_y0'][0, k - 1] and d['word_edges_y0'][0, k]
        # a run longer than a column: it crosses from (H-1, x) to (0, x+1)
        for x in K.crossing_columns(W):
            c = np_rle_counts(d['cols_%d_%d' % (x, x + 1)])
            assert c.tolist() == [x * H, 2 * H] + ([(W - x - 2) * H] if x + 2 < W else [])
        assert d['col_last'][H - 1, W - 1] == 1
    assert K.crossing_columns(129) == [63, 64, 127] and K.crossing_columns(65) == [63]


def test_pack_inputs_hold_the_named_values():
    _, ms = K.shape_masks(65, 65)
    ins = K.pack_inputs(ms)
    assert ins['uint8'].dtype == np.uint8 and ins['bool'].dtype == np.bool_ and ins['int32'].dtype == np.int32
    fg = ms != 0
    for a in ins.values():
        assert np.array_equal(a != 0, fg)
    u8 = ins['uint8'][fg]
    assert u8.min() == 2 and u8.max() == 255
    i32 = ins['int32'][fg]
    assert -1 in i32 and K.INT32_MIN in i32
    assert ((i32 & 0xff) == 0).any() and ((i32 & 0xffff) == 0).any()      # a zero low byte / half


# ---------------------------------------------------------------------------------- section 2
def _contains(extent, mask):
    t = K.ref_extent(mask)
    if t is None:
        return True
    return extent[0] <= t[0] and t[1] <= extent[1] and extent[2] <= t[2] and t[3] <= extent[3]


def test_every_extent_is_admissible_and_every_kind_is_there():
    for case in K.EXTENT_CASES:
        names, ms = K.extent_masks(case)
        H, Wq = case.H, K.words(case.W)
        ya, yb, wa, wb = case.box
        assert K.ref_extent(ms[0]) == case.box and K.ref_extent(ms[-1]) == case.box
        kinds = dict(K.admissible_extents(case, ms))
        for name, e in kinds.items():
            assert e.shape == (len(ms), 4) and e.dtype == np.int32
            assert all(_contains(e[n], ms[n]) for n in range(len(ms))), (case.name, name)
        assert kinds['tight'][0].tolist() == list(case.box)
        assert kinds['tight'][2].tolist() != list(case.box)          # really per mask
        assert kinds['full'][0].tolist() == [0, H, 0, Wq]
        assert kinds['outside_image'][0].tolist() == [-5, H + 7, -2, Wq + 3]
        for name, i, d in (('slack_row_above', 0, -1), ('slack_row_below', 1, 1),
                           ('slack_word_left', 2, -1), ('slack_word_right', 3, 1)):
            want = list(case.box)
            want[i] += d
            assert kinds[name][0].tolist() == want
    boxes = {c.name: c for c in K.EXTENT_CASES}
    c = boxes['inner_box']                                 # rows not multiples of 64, inner words
    assert c.box[0] % 64 and c.box[1] % 64 and c.box[2] > 0 and c.box[3] < K.words(c.W)
    c = boxes['all_rows_inner_words']                      # all rows with w0 > 0 and w1 < Wq
    assert c.box[:2] == (0, c.H) and c.box[2] > 0 and c.box[3] < K.words(c.W)
    _, ms = K.extent_masks(c)
    assert ms[2][c.H - 1, 64 * c.box[2]] == 1              # row H-1 of column x = 64 w0
    assert ms[3][c.H - 1, 64 * c.box[3] - 1] == 1          # bit 63 of word w1 - 1
    for name in ('whole_image_ragged', 'whole_image_word_multiple'):
        c = boxes[name]
        assert K.extent_masks(c)[1][0][c.H - 1, c.W - 1] == 1      # ends at pixel H * W - 1
    assert boxes['whole_image_word_multiple'].W % 64 == 0 and boxes['whole_image_ragged'].W % 64
    c = boxes['tall_chunks']                               # more than one row chunk, ragged ends
    assert c.box[1] - c.box[0] > 64 and (c.box[1] - c.box[0]) % 64 not in (0, 32)


def test_every_encode_branch_is_reached():
    reached = {}
    for case in K.EXTENT_CASES:
        names, ms = K.extent_masks(case)
        for kind, e in K.admissible_extents(case, ms):
            for n, m in enumerate(ms):
                for b in K.encode_branches(m, e[n]):
                    reached.setdefault(b, []).append((case.name, kind, names[n]))
    assert set(reached) == set(K.ENCODE_BRANCHES), set(K.ENCODE_BRANCHES) - set(reached)
    # the same mask under two extents takes the two sides of next_walked
    sides = {k: {(c, m) for c, _, m in reached[k]} for k in ('next_walked', 'next_not_walked')}
    assert sides['next_walked'] & sides['next_not_walked']
    # ... and of the previous word column
    assert {c for c, _, _ in reached['prev_word_outside']} & {c for c, _, _ in reached['prev_from_word_inside']}


def test_encode_branches_on_hand_made_masks():
    m = np.zeros((4, 130), np.uint8)
    m[3, 63] = m[0, 64] = 1                                # one run across the word edge
    assert K.encode_branches(m, (0, 4, 0, 3)) == {'all_rows', 'next_walked', 'prev_from_word_inside'}
    assert K.encode_branches(m, (-5, 9, -1, 9)) == {'all_rows', 'next_walked', 'prev_from_word_inside'}
    assert K.encode_branches(m[:, :64], (0, 4, 0, 1)) == {'all_rows', 'end_of_mask'}
    m[0, 64] = 0
    assert K.encode_branches(m, (0, 4, 0, 1)) == {'all_rows', 'next_not_walked'}
    assert K.encode_branches(m, (3, 4, 0, 1)) == {'some_rows', 'column_end_some_rows'}
    assert K.encode_branches(m, (0, 4, 1, 2)) == {'all_rows', 'prev_word_outside'}
    assert K.encode_branches(m, (4, 0, 3, 0)) == set()


def test_intersection_runs_cut_something_and_reach_wide_rows():
    nws = set()
    for case in K.INTERSECT_CASES:
        a, b = K.intersect_sets(case)
        dense = K.restricted_intersections(a, b, [(0, case.H, 0, K.words(case.W))] * len(a),
                                           [(0, case.H, 0, K.words(case.W))] * len(b))
        assert np.array_equal(dense, K.ref_intersections(a, b))
        assert np.array_equal(dense, (a[:, None].astype(bool) & b[None].astype(bool)).sum((2, 3)))
        kinds = {}
        for name, ea, eb, kind in K.intersect_runs(case, a, b):
            kinds[kind] = kinds.get(kind, 0) + 1
            r = K.restricted_intersections(a, b, ea, eb)
            if kind == 'admissible':
                assert all(_contains(ea[p], a[p]) for p in range(len(a))), (case.name, name)
                assert all(_contains(eb[g], b[g]) for g in range(len(b))), (case.name, name)
                assert np.array_equal(r, dense), (case.name, name)
            elif kind == 'cut':
                # a pair whose restricted count is neither 0 nor the whole count
                assert ((r != 0) & (r != dense)).any(), (case.name, name)
            else:
                assert not r.any() and dense.any(), (case.name, name)
            for p in range(len(a)):
                for g in range(len(b)):
                    ca, cb = K.clamp_extent(ea[p], case.H, K.words(case.W)), K.clamp_extent(eb[g], case.H, K.words(case.W))
                    if max(ca[0], cb[0]) < min(ca[1], cb[1]):
                        nws.add(min(ca[3], cb[3]) - max(ca[2], cb[2]))
        assert kinds['admissible'] >= 14 and kinds['cut'] >= 3 and kinds['disjoint'] == 3
    # words per row of an overlap: below, at and above the 64 of one step, and two steps wide
    assert {1, 2, 3, 63, 64, 65, 129, 130} <= nws


# ---------------------------------------------------------------------------------- section 3
def test_capacity_sweep_falls_inside_masks_on_boundaries_and_short_of_the_total():
    ref = K.CapReference()
    N = len(ref.masks)
    assert N == 6 and ref.V == sum(map(len, ref.counts)) and ref.C == sum(map(len, ref.strings))
    lens = np.diff(ref.val_off)
    assert lens.min() == 1 and lens[1] == 2 and lens.max() > 256      # [HW], [0, HW], several scan steps
    inner = set(ref.val_off[1:-1].tolist())
    vcaps = ref.value_caps()
    assert {0, 1, ref.V - 1, ref.V, ref.V + 1} <= set(vcaps) and inner <= set(vcaps)
    assert all({k - 1, k + 1} <= set(vcaps) for k in inner)
    # strictly inside a mask: some cap splits the counts of a mask with more than two counts
    assert any(ref.val_off[n] + 1 < c < ref.val_off[n + 1] - 1 for c in vcaps for n in range(N))
    assert all(any(ref.val_off[n] < c < ref.val_off[n + 1] for c in vcaps) for n in range(N) if lens[n] > 1)
    ccaps = ref.char_caps()
    assert {0, ref.C - 1, ref.C} <= set(ccaps) and set(ref.str_off.tolist()) <= set(ccaps)
    assert any(ref.str_off[n] < c < ref.str_off[n + 1] for c in ccaps for n in range(N))
    assert max(ccaps) == ref.C
    # what the reference expects at three caps
    so, cnt, ch = ref.expected(ref.V, ref.C, ref.V + 8, ref.C + 8)
    assert np.array_equal(so, ref.str_off) and (cnt[:ref.V] != K.POISON_I32).all() and (cnt[ref.V:] == K.POISON_I32).all()
    assert ch[:ref.C].tobytes().decode() == ''.join(ref.strings) and (ch[ref.C:] == K.POISON_U8).all()
    so, cnt, ch = ref.expected(int(ref.val_off[3]) + 1, ref.C, ref.V + 8, ref.C + 8)
    assert so.tolist() == ref.str_off[:4].tolist() + [int(ref.str_off[3])] * 3
    assert (cnt[ref.val_off[3]:] == K.POISON_I32).all()
    so, cnt, ch = ref.expected(ref.V, int(ref.str_off[3]) - 1, ref.V + 8, ref.C + 8)
    assert np.array_equal(so, ref.str_off) and (ch[ref.str_off[2]:] == K.POISON_U8).all()
    assert not (cnt[:ref.V] == K.POISON_I32).any()
    assert all(48 <= b <= 111 for s in ref.strings for b in s.encode())      # the poison is no character


# ---------------------------------------------------------------------------------- section 4
def test_character_count_boundaries():
    assert sorted({H * W for H, W in K.CHAR_BOUNDARY_SHAPES}) == sorted(K.CHAR_BOUNDARY_HW)
    n = [K.n_chars(v) for v in K.CHAR_BOUNDARY_HW]
    assert n == [1, 2, 2, 3, 3, 4, 4, 5, 5, 6]
    for H, W in K.CHAR_BOUNDARY_SHAPES:
        assert len(np_rle_string([H * W])) == K.n_chars(H * W)
    H, W = K.SEVEN_CHAR_SHAPE
    assert (1 << 29) <= H * W - 1 and H * W < (1 << 31)
    assert len(np_rle_string([H * W])) == 7 and len(np_rle_string([H * W - 1, 1])) == 8
    assert np_data.rle_from_string(np_rle_string([H * W - 1, 1])) == [H * W - 1, 1]


def test_delta_lists_store_the_named_deltas_on_both_sides_of_a_boundary():
    lists = K.delta_count_lists()
    assert len(lists) == 18
    stored = {}
    for name, H, W, c in lists:
        assert sum(c) == H * W and min(c) >= 1 and H == K.DELTA_H
        d = c[3] - c[1]
        assert '%+d' % d == name
        stored[d] = K.n_chars(d)
        s = np_rle_string(c)
        assert np_data.rle_from_string(s) == c
        assert np_rle_counts(K.counts_to_mask(c, H, W)).tolist() == c      # canonical: encode gives it back
    for k, chars in zip(K.DELTA_KS, (1, 2, 3)):
        for sign in (1, -1):
            assert {sign * ((1 << k) - 1), sign * (1 << k), sign * ((1 << k) + 1)} <= set(stored)
        assert (stored[(1 << k) - 1], stored[1 << k]) == (chars, chars + 1)
        assert (stored[-(1 << k)], stored[-(1 << k) - 1]) == (chars, chars + 1)


def test_noncanonical_strings_and_zero_runs():
    H, W = K.NONCANONICAL_SHAPE
    assert [len(s) for s in K.NONCANONICAL_OK] == [2, 3, 7] and K.NONCANONICAL_OK[0] == np_rle_string([H * W])
    for s in K.NONCANONICAL_OK + (K.NONCANONICAL_TOO_LONG,):
        assert np_data.rle_from_string(s) == [H * W]
    assert len(K.NONCANONICAL_TOO_LONG) == 8
    lists = K.zero_run_lists()
    for H, W, c in lists:
        assert sum(c) == H * W and min(c) >= 0 and 0 in c
    small = [c for _, _, c in lists]
    assert any(c[0] == 0 and len(c) > 1 for c in small) and any(c[-1] == 0 for c in small)
    assert any(0 in c[1:-1] for c in small)
    assert any(any(a == b == 0 for a, b in zip(c, c[1:])) for c in small)
    assert {len(c) % 2 for c in small} == {0, 1}
    # a zero-length run that starts exactly where a column starts, beyond the first column
    assert any(r == 0 and p % H == 0 and 0 < p < H * W
               for H, W, c in lists for r, p in zip(c, np.concatenate([[0], np.cumsum(c)[:-1]])))
    assert any(W > 64 for _, W, _ in lists) and any(H > 64 for H, _, _ in lists)


def test_malformed_entries_mix_every_status_with_valid_ones():
    H, W = K.MALFORMED_SHAPE
    for entries in (K.malformed_strings(), K.malformed_lists()):
        st = [s for _, s in entries]
        assert st[0] == K.OK and st[-1] == K.OK and K.OK in st[1:-1]
        assert {K.NEGATIVE, K.BAD_SUM} <= set(st)
        for c, s in entries:
            if s == K.OK:
                counts = np_data.rle_from_string(c) if isinstance(c, str) else c
                assert sum(counts) == H * W and min(counts) >= 0
    st = [s for _, s in K.malformed_strings()]
    assert st.count(K.BAD_CHAR) == 2 and st.count(K.UNTERMINATED) == 2 and st.count(K.BAD_SUM) == 3
    by = dict(K.malformed_strings())
    assert by['111K'] == K.NEGATIVE and np_data.rle_from_string('111K') == [1, 1, 1, -4]
    assert by[''] == K.BAD_SUM
    sums = [sum(c) for c, s in K.malformed_lists() if s == K.BAD_SUM and c and min(c) >= 0]
    assert any(v < H * W for v in sums) and any(v > H * W for v in sums)
    assert ([], K.BAD_SUM) in K.malformed_lists()
