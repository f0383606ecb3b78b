"""Case lists and dense NumPy references for the packed-mask kernels at their row, word and extent
edges: csrc/mask_eval.hip (mask_pack, mask_intersect) and csrc/mask_rle.hip (rle_encode,
rle_decode, mask_unpack).  Imports without a GPU; tests/test_packed_mask_cases_cpu.py holds the
conditions that make the cases worth running, tests/test_gpu_packed_mask_edges.py runs them.

Every reference is dense and knows nothing of the kernels: np.packbits for the words, the
vectorised counts / strings of tests/test_coco_results_cpu.py (pinned there to the per-pixel codec
of oracle/np_data.py), boolean sums for the intersections.  Every comparison is exact.

What the kernels do in chunks, and where the lists below put a boundary:
* walk_column (encode) and rle_fill_kernel (decode) take the rows 64 at a time: H in SHAPE_HS;
* every kernel works on 64-pixel words, the intersection walks ``nw`` words of a row and advances
  by 64 / nw rows and 64 % nw words per step: W in SHAPE_WS and WIDE_WS (Wq = 64 and 65);
* the encoder branches on the extent (all rows or not, the previous / next word column inside it
  or not): EXTENT_CASES x admissible_extents(), with encode_branches() naming what a case reaches;
* a stored value takes one more character at 2^4, 2^9, ... on either side of zero, and the parser
  gives up after seven: CHAR_BOUNDARY_SHAPES, delta_count_lists(), SEVEN_CHAR_SHAPE.
"""
import collections

import numpy as np

from oracle import np_data
from test_coco_results_cpu import np_rle_counts, np_rle_string

INT32_MIN = -(1 << 31)

# ------------------------------------------------------------------------------ references


def words(W):
    return (int(W) + 63) // 64


def ref_pack(masks):
    """(N, H, W) masks (nonzero = foreground) -> uint64 (N, H, Wq): np.packbits, little bit order,
    of rows zero-padded to a multiple of 64."""
    m = np.asarray(masks) != 0
    N, H, W = m.shape
    pad = np.zeros((N, H, words(W) * 64), bool)
    pad[:, :, :W] = m
    return np.ascontiguousarray(np.packbits(pad, axis=-1, bitorder='little')).view('<u8')


def ref_area(masks):
    return (np.asarray(masks) != 0).reshape(len(masks), -1).sum(1).astype(np.int64)


def ref_extent(mask):
    """The tight extent (y_min, y_max + 1, x_min >> 6, (x_max >> 6) + 1) of one mask, None for an
    empty one (whose extent must only be empty: lo >= hi)."""
    ys, xs = np.nonzero(np.asarray(mask))
    if not len(ys):
        return None
    return (int(ys.min()), int(ys.max()) + 1, int(xs.min()) >> 6, (int(xs.max()) >> 6) + 1)


def ref_rle(masks):
    """-> (count lists, strings) of a stack of masks."""
    counts = [np_rle_counts(m) for m in masks]
    return [c.tolist() for c in counts], [np_rle_string(c) for c in counts]


def ref_intersections(a, b):
    """(P, G) |A_p & B_g| as a float32 0/1 matrix product (exact below 2^24 pixels)."""
    fa = (np.asarray(a) != 0).reshape(len(a), -1).astype(np.float32)
    fb = (np.asarray(b) != 0).reshape(len(b), -1).astype(np.float32)
    assert fa.shape[1] < (1 << 24)
    return (fa @ fb.T).astype(np.int64)


def counts_to_mask(counts, H, W):
    """Count list -> (H, W) uint8, vectorised (np.repeat); pinned to np_data.rle_decode by the CPU
    test.  Zero-length runs are legal."""
    c = np.asarray(counts, np.int64)
    flat = np.repeat(np.arange(len(c)) & 1, c).astype(np.uint8)
    assert flat.size == H * W
    return flat.reshape(W, H).T


# ---------------------------------------------------------------------------------- section 1
SHAPE_HS = (1, 63, 64, 65, 127, 128, 129)
SHAPE_WS = (1, 63, 64, 65, 128, 129)
WIDE_WS = (4096, 4097, 4160)            # Wq = 64, 65, 65
WIDE_HS = (1, 3, 65)
SHAPES = [(H, W) for H in SHAPE_HS for W in SHAPE_WS] + [(H, W) for H in WIDE_HS for W in WIDE_WS]


def _edges(n):
    """The last index of every chunk of 64 and the first of the next, below n (n - 1 if none)."""
    e = sorted({i for k in range(64, n + 64, 64) for i in (k - 1, k) if i < n})
    return e or [n - 1]


def crossing_columns(W):
    """The x at which shape_masks() lets a run cross from (H-1, x) to (0, x+1)."""
    return sorted({x for x in (63, 64, W - 2) if 0 <= x and x + 1 < W})


def shape_masks(H, W):
    """-> (names, (N, H, W) uint8 stack) of one shape: the masks of the issue's section 1."""
    rng = np.random.RandomState(1000 * H + W)
    out = collections.OrderedDict()
    z = lambda: np.zeros((H, W), np.uint8)            # noqa: E731
    out['empty'] = z()
    out['full'] = z() + 1
    for name, (y, x) in (('corner00', (0, 0)), ('corner0W', (0, W - 1)), ('cornerH0', (H - 1, 0)),
                         ('cornerHW', (H - 1, W - 1))):
        m = z()
        m[y, x] = 1
        out[name] = m
    for x in sorted({0, W // 2, W - 1}):               # row-chunk edges down one column
        m = z()
        m[_edges(H), x] = 1
        out['chunk_edges_x%d' % x] = m
    for y in sorted({0, H // 2, H - 1}):               # word edges along one row
        m = z()
        m[y, _edges(W)] = 1
        out['word_edges_y%d' % y] = m
    for x in crossing_columns(W):                      # a run from (H-1, x) on to (0, x+1)
        m = z()
        m[:, x:x + 2] = 1
        out['cols_%d_%d' % (x, x + 1)] = m
    m = z()
    m[:, ::3] = 1                                      # runs that end where a column ends
    out['cols_every_third'] = m
    m = z()
    m[:, W - 1] = 1                                    # ends at pixel H * W - 1
    out['col_last'] = m
    m = z()
    m[sorted({0, H - 1} | set(_edges(H))), :] = 1
    out['rows_full'] = m
    out['checkerboard'] = (np.indices((H, W)).sum(0) % 2).astype(np.uint8)
    out['bernoulli_0.5'] = (rng.uniform(size=(H, W)) < 0.5).astype(np.uint8)
    out['bernoulli_0.02'] = (rng.uniform(size=(H, W)) < 0.02).astype(np.uint8)
    return list(out), np.stack(list(out.values()))


def pack_inputs(masks, seed=0):
    """{name: array}: the same foreground as three pack inputs.  uint8 with values 2..255, bool, and
    int32 with -1, INT32_MIN and values whose low byte(s) are zero: any nonzero value counts."""
    rng = np.random.RandomState(seed)
    fg = np.asarray(masks) != 0
    u8 = rng.randint(2, 256, fg.shape).astype(np.uint8)
    vals = np.array([-1, INT32_MIN, 1 << 8, 1 << 16, 1 << 24, 7], np.int64)
    i32 = vals[rng.randint(0, len(vals), fg.shape)]
    n = min(int(fg.sum()), 2)
    if n:                                              # both named values really occur
        idx = np.argwhere(fg)
        u8[tuple(idx[0])] = 255
        i32[tuple(idx[0])] = -1
        u8[tuple(idx[-1])] = 2
        i32[tuple(idx[-1])] = INT32_MIN
    return collections.OrderedDict([('uint8', u8 * fg), ('bool', fg.copy()),
                                    ('int32', (i32 * fg).astype(np.int32))])


# ---------------------------------------------------------------------------------- section 2
# A case: an image and a tight box (rows [ya, yb), words [wa, wb)) inside which its masks lie.
ExtentCase = collections.namedtuple('ExtentCase', 'name H W box')

EXTENT_CASES = [
    ExtentCase('inner_box', 70, 200, (3, 69, 1, 3)),          # partial rows, w0 > 0, w1 < Wq
    ExtentCase('all_rows_inner_words', 70, 200, (0, 70, 1, 3)),   # x = 64 w0 and bit 63 of w1 - 1 at row H-1
    ExtentCase('whole_image_ragged', 70, 200, (0, 70, 0, 4)),     # ends at pixel H * W - 1
    ExtentCase('whole_image_word_multiple', 128, 256, (0, 128, 0, 4)),   # bit 63 of the last word
    ExtentCase('tall_chunks', 200, 130, (65, 191, 0, 3)),     # rows cross two chunk boundaries
    ExtentCase('bottom_rows', 131, 130, (70, 131, 1, 3)),     # y1 == H but y0 > 0: not "all rows"
]


def box_pixels(case):
    ya, yb, wa, wb = case.box
    return ya, yb, 64 * wa, min(64 * wb, case.W)


def extent_masks(case, seed=0):
    """-> (names, (N, H, W) uint8) whose set bits lie in the case's box; the first ('rand') and the
    last ('box_full') make the box tight."""
    H, W = case.H, case.W
    ya, yb, xa, xb = box_pixels(case)
    rng = np.random.RandomState(seed + 7 * H + W)
    out = collections.OrderedDict()
    z = lambda: np.zeros((H, W), np.uint8)            # noqa: E731
    m = z()
    m[ya:yb, xa:xb] = rng.uniform(size=(yb - ya, xb - xa)) < 0.5
    m[ya, xa] = m[yb - 1, xb - 1] = m[ya, xb - 1] = m[yb - 1, xa] = 1
    out['rand'] = m
    m = z()
    m[ya:yb, xa:xb] = rng.uniform(size=(yb - ya, xb - xa)) < 0.03
    out['sparse'] = m
    m = z()
    m[yb - 1, xa] = 1                                  # the last row of column x = 64 w0
    out['bottom_of_first_column'] = m
    m = z()
    m[yb - 1, xb - 1] = 1                              # the last row of the last column (bit 63 of
    out['bottom_of_last_column'] = m                   # word w1 - 1 where the word is whole)
    m = z()
    for x in sorted({xa, xa + 1, xa + 63, min(xa + 64, xb - 1), xb - 2, xb - 1}):
        m[ya:yb, x] = 1                                # box-high columns on both sides of a word edge
    out['columns'] = m
    m = z()
    m[ya:yb, xa:xb] = 1
    out['box_full'] = m
    return list(out), np.stack(list(out.values()))


def admissible_extents(case, masks):
    """[(name, (N, 4) int32)]: every extent kind of the issue, each containing all set bits."""
    H, Wq = case.H, words(case.W)
    ya, yb, wa, wb = case.box
    N = len(masks)
    kinds = collections.OrderedDict()
    tight = [ref_extent(m) or (H, 0, Wq, 0) for m in masks]
    kinds['tight'] = np.array(tight, np.int32)

    def add(name, e):
        kinds[name] = np.tile(np.array(e, np.int32), (N, 1))
    add('box', (ya, yb, wa, wb))
    add('full', (0, H, 0, Wq))
    add('all_rows_box_words', (0, H, wa, wb))
    add('all_rows_slack_left', (0, H, max(wa - 1, 0), wb))
    add('all_rows_slack_right', (0, H, wa, min(wb + 1, Wq)))
    add('all_words_box_rows', (ya, yb, 0, Wq))
    add('slack_row_above', (ya - 1, yb, wa, wb))
    add('slack_row_below', (ya, yb + 1, wa, wb))
    add('slack_word_left', (ya, yb, wa - 1, wb))
    add('slack_word_right', (ya, yb, wa, wb + 1))
    add('outside_image', (-5, H + 7, -2, Wq + 3))
    add('outside_rows', (-5, H + 7, wa, wb))
    add('outside_words', (ya, yb, -2, Wq + 3))
    return list(kinds.items())


def clamp_extent(e, H, Wq):
    return max(int(e[0]), 0), min(int(e[1]), H), max(int(e[2]), 0), min(int(e[3]), Wq)


def encode_branches(mask, extent):
    """The branches of walk_column (csrc/mask_rle.hip) that ``extent`` makes the encode of ``mask``
    take *with an effect on the result*, as a set of names:

    all_rows / some_rows      the extent spans every row, or not;
    next_walked               a column ends set at row H-1 and the lane of the next column, inside
                              the extent, owns the change at (x+1) H: the term suppresses a duplicate;
    next_not_walked           such a column whose right neighbour lies in a word past the extent:
                              this lane must record the change itself;
    prev_from_word_inside     lane 0 takes a set bit 63 of row H-1 from the previous word column,
                              which is inside the extent;
    prev_word_outside         lane 0 of the extent's first word column (w0 > 0) starts from 0
                              without reading the word before it;
    end_of_mask               the last column ends set: H * W is no change;
    column_end_some_rows      without all rows, a column set in row y1 - 1 ends its run at x H + y1.
    """
    m = np.asarray(mask) != 0
    H, W = m.shape
    y0, y1, w0, w1 = clamp_extent(extent, H, words(W))
    out = set()
    if not (y0 < y1 and w0 < w1):
        return out
    full = y0 == 0 and y1 == H
    out.add('all_rows' if full else 'some_rows')
    xs = range(64 * w0, min(64 * w1, W))
    for x in xs:
        if full:
            if m[H - 1, x]:
                if x + 1 == W:
                    out.add('end_of_mask')
                elif ((x + 1) >> 6) < w1:
                    out.add('next_walked')
                else:
                    out.add('next_not_walked')
            if x & 63 == 0 and x > 0:
                if (x >> 6) - 1 >= w0:
                    if m[H - 1, x - 1]:
                        out.add('prev_from_word_inside')
                else:
                    out.add('prev_word_outside')
        elif m[y1 - 1, x]:
            out.add('column_end_some_rows')
    return out


ENCODE_BRANCHES = ('all_rows', 'some_rows', 'next_walked', 'next_not_walked', 'prev_from_word_inside',
                   'prev_word_outside', 'end_of_mask', 'column_end_some_rows')


# Intersections: two sets in one image, boxes that overlap in part.
IntersectCase = collections.namedtuple('IntersectCase', 'name H W box_a box_b')

INTERSECT_CASES = [
    IntersectCase('offset_boxes', 70, 200, (3, 69, 0, 3), (10, 70, 1, 4)),
    IntersectCase('chunk_rows', 200, 130, (0, 191, 0, 3), (65, 200, 0, 3)),
    IntersectCase('same_box', 128, 256, (0, 128, 0, 4), (0, 128, 0, 4)),
    # nw = 64 and 65 of the full width, 63 and 64 once a word is cut off
    IntersectCase('wide_64', 3, 4096, (0, 3, 0, 64), (0, 3, 0, 64)),
    IntersectCase('wide_65', 5, 4160, (0, 5, 0, 65), (0, 5, 0, 65)),
    IntersectCase('wide_130', 3, 8300, (0, 3, 0, 130), (0, 3, 0, 130)),
]


def intersect_sets(case):
    a = extent_masks(ExtentCase(case.name, case.H, case.W, case.box_a), seed=1)[1]
    b = extent_masks(ExtentCase(case.name, case.H, case.W, case.box_b), seed=2)[1]
    return a, b


def intersect_runs(case, a, b):
    """[(name, ext_a (P,4), ext_b (G,4), kind)], kind 'admissible' (both extents contain every set
    bit: the dense count), 'cut' (bits are cut off: the dense count restricted to the clamped
    overlap) or 'disjoint' (no overlap: zero)."""
    ca = ExtentCase(case.name, case.H, case.W, case.box_a)
    cb = ExtentCase(case.name, case.H, case.W, case.box_b)
    ka, kb = admissible_extents(ca, a), admissible_extents(cb, b)
    ta, tb = ka[0][1], kb[0][1]
    runs = []
    for (na, ea), (nb, eb) in zip(ka, kb):
        runs.append(('%s/%s' % (na, nb), ea, eb, 'admissible'))
        if na != 'tight':
            runs.append(('%s/tight' % na, ea, tb, 'admissible'))
            runs.append(('tight/%s' % nb, ta, eb, 'admissible'))
    H, Wq = case.H, words(case.W)
    oy0, oy1 = max(case.box_a[0], case.box_b[0]), min(case.box_a[1], case.box_b[1])
    ow0, ow1 = max(case.box_a[2], case.box_b[2]), min(case.box_a[3], case.box_b[3])
    dy = 1 if oy1 - oy0 < 8 else 3
    P, G = len(a), len(b)
    rep = lambda e, n: np.tile(np.array(e, np.int32), (n, 1))     # noqa: E731
    box_a, box_b = rep(case.box_a, P), rep(case.box_b, G)

    def cut(name, ea, eb):
        runs.append((name, rep(ea, P) if ea is not None else box_a,
                     rep(eb, G) if eb is not None else box_b, 'cut'))
    cut('cut_top_a', (oy0 + dy, H, 0, Wq), None)
    cut('cut_bottom_b', None, (0, oy1 - dy, 0, Wq))
    cut('cut_rows_both', (oy0 + dy, H + 7, -2, Wq + 3), (-5, oy1 - dy, -2, Wq + 3))
    if ow1 - ow0 > 1:
        cut('cut_first_word_a', (0, H, ow0 + 1, Wq), None)
        cut('cut_last_word_b', None, (0, H, 0, ow1 - 1))
        cut('cut_rows_and_words', (oy0 + dy, H, ow0 + 1, Wq), (0, H, 0, ow1))
    if ow1 - ow0 > 2:
        cut('cut_words_both', (0, H, ow0 + 1, Wq), (0, H, 0, ow1 - 1))
    ym, wm = (oy0 + oy1) // 2, (ow0 + ow1 + 1) // 2
    runs.append(('disjoint_rows', rep((0, ym, 0, Wq), P), rep((ym, H, 0, Wq), G), 'disjoint'))
    runs.append(('disjoint_words', rep((0, H, 0, wm), P), rep((0, H, wm, Wq + 3), G), 'disjoint'))
    runs.append(('disjoint_empty_a', rep((H, 0, Wq, 0), P), box_b, 'disjoint'))
    return runs


def restricted_intersections(a, b, ext_a, ext_b):
    """(P, G) |A_p & B_g| counted inside the overlap of the two extents clamped to the image."""
    a, b = np.asarray(a) != 0, np.asarray(b) != 0
    H, W = a.shape[1:]
    Wq = words(W)
    out = np.zeros((len(a), len(b)), np.int64)
    for p in range(len(a)):
        ya0, ya1, wa0, wa1 = clamp_extent(ext_a[p], H, Wq)
        for g in range(len(b)):
            yb0, yb1, wb0, wb1 = clamp_extent(ext_b[g], H, Wq)
            y0, y1, w0, w1 = max(ya0, yb0), min(ya1, yb1), max(wa0, wb0), min(wa1, wb1)
            if y0 < y1 and w0 < w1:
                out[p, g] = (a[p, y0:y1, 64 * w0:64 * w1] & b[g, y0:y1, 64 * w0:64 * w1]).sum()
    return out


# ---------------------------------------------------------------------------------- section 3
POISON_I32 = 0x5A5A5A5A
POISON_U8 = 0xA5                        # no RLE character (48..111)
POISON_I64 = 0x5A5A5A5A5A5A5A5A
GUARD = 64                              # elements in front of and behind a guarded buffer


class Guarded(object):
    """``n`` elements of an integer ``dtype`` inside a larger device buffer, GUARD elements in
    front and behind, everything prefilled with a poison value (the idea of
    gemm_edge_cases.Guarded for integer outputs).  ``out`` is the view a kernel writes."""

    def __init__(self, n, dtype, device):
        import torch
        self.poison = {torch.int32: POISON_I32, torch.uint8: POISON_U8, torch.int64: POISON_I64}[dtype]
        self.n = int(n)
        self.buf = torch.full((self.n + 2 * GUARD,), self.poison, dtype=dtype, device=device)
        self.out = self.buf[GUARD:GUARD + self.n]

    def guards_intact(self):
        b = self.buf
        return bool((b[:GUARD] == self.poison).all()) and bool((b[GUARD + self.n:] == self.poison).all())

    def host(self):
        return self.out.cpu().numpy()


CAP_SHAPE = (9, 70)


def cap_masks():
    H, W = CAP_SHAPE
    rng = np.random.RandomState(5)
    m = np.zeros((6, H, W), np.uint8)
    m[1] = 1
    m[2] = rng.uniform(size=(H, W)) < 0.5
    m[3, 4, 65] = 1
    m[4] = np.indices((H, W)).sum(0) % 2
    m[5] = rng.uniform(size=(H, W)) < 0.1
    return m


class CapReference(object):
    """Counts, strings and offsets of cap_masks(), and what a call with given caps must leave."""

    def __init__(self):
        self.masks = cap_masks()
        self.counts, self.strings = ref_rle(self.masks)
        self.val_off = np.concatenate([[0], np.cumsum([len(c) for c in self.counts])]).astype(np.int64)
        self.str_off = np.concatenate([[0], np.cumsum([len(s) for s in self.strings])]).astype(np.int64)
        self.V, self.C = int(self.val_off[-1]), int(self.str_off[-1])

    def value_caps(self):
        caps = {0, 1, self.V - 1, self.V, self.V + 1}
        for k in self.val_off:
            caps |= {int(k) - 1, int(k), int(k) + 1}
        caps |= {int(a + b) // 2 for a, b in zip(self.val_off, self.val_off[1:])}     # mid-mask
        return sorted(c for c in caps if c >= 0)

    def char_caps(self):
        caps = {0, self.C - 1, self.C}
        for k in self.str_off:
            caps |= {int(k) - 1, int(k), int(k) + 1}
        caps |= {int(a + b) // 2 for a, b in zip(self.str_off, self.str_off[1:])}     # mid-string
        return sorted(c for c in caps if 0 <= c <= self.C)

    def expected(self, cap_values, cap_chars, size_values, size_chars):
        """-> (str_off (N+1), counts (size_values), chars (size_chars)) with the poison wherever the
        call must write nothing: past a cap, and in the slots of masks that did not fit."""
        N = len(self.masks)
        fit_v = [self.val_off[n + 1] <= cap_values for n in range(N)]
        lens = [len(self.strings[n]) if fit_v[n] else 0 for n in range(N)]
        str_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        counts = np.full(size_values, POISON_I32, np.int64)
        chars = np.full(size_chars, POISON_U8, np.uint8)
        for n in range(N):
            if fit_v[n]:
                counts[self.val_off[n]:self.val_off[n + 1]] = self.counts[n]
                if str_off[n + 1] <= cap_chars:
                    chars[str_off[n]:str_off[n + 1]] = np.frombuffer(self.strings[n].encode(), np.uint8)
        return str_off, counts, chars


# ---------------------------------------------------------------------------------- section 4
# (H, W) with H * W on both sides of every character-count boundary of a stored value
CHAR_BOUNDARY_HW = (15, 16, 511, 512, (1 << 14) - 1, 1 << 14, (1 << 19) - 1, 1 << 19,
                    (1 << 24) - 1, 1 << 24)
CHAR_BOUNDARY_SHAPES = [(3, 5), (4, 4), (7, 73), (8, 64), (129, 127), (128, 128), (1, (1 << 19) - 1),
                        ((1 << 19) - 1, 1), (512, 1024), (4095, 4097), (4096, 4096)]
SEVEN_CHAR_SHAPE = (23171, 23171)       # H * W >= 2^29: seven characters, decode only


def n_chars(v):
    """Characters of one stored value (maskApi.c rleToString)."""
    return len(np_data.rle_to_string([int(v)]))


DELTA_KS = (4, 9, 14)
DELTA_H = 7


def delta_count_lists():
    """[(name, H, W, counts)]: count lists whose fourth stored value count[3] - count[1] is
    +-(2^k - 1), +-2^k, +-(2^k + 1); a last run pads H * W to a multiple of DELTA_H."""
    out = []
    for k in DELTA_KS:
        for d in ((1 << k) - 1, 1 << k, (1 << k) + 1):
            for sign in (1, -1):
                c = [1, 1, 1, 1 + d, 2] if sign > 0 else [1, d + 1, 1, 1, 2]
                c.append(DELTA_H - sum(c) % DELTA_H)
                out.append(('%+d' % (sign * d), DELTA_H, sum(c) // DELTA_H, c))
    return out


# 35 in a 5 x 7 image with redundant zero groups: 2, 3 and 7 groups decode, 8 do not end
NONCANONICAL_SHAPE = (5, 7)
NONCANONICAL_OK = ('S1', 'SQ0', 'SQPPPP0')
NONCANONICAL_TOO_LONG = 'SQPPPPP0'


def zero_run_lists():
    """[(H, W, counts)]: count lists with zero-length runs — leading, interior, consecutive,
    trailing, at column starts (repeated run starts where a lane's binary search lands), odd and
    even lengths, and random ones over more than one word column."""
    out = [(5, 7, c) for c in (
        [0, 35], [35, 0], [0, 35, 0], [3, 0, 2, 30], [3, 0, 0, 32], [3, 0, 0, 5, 27], [30, 5, 0],
        [0, 0, 0, 35], [0, 0, 35], [0, 5, 0, 0, 30], [5, 0, 0, 3, 27], [5, 0, 5, 0, 5, 0, 20],
        [10, 0, 0, 0, 0, 25], [4, 1, 0, 0, 30], [0, 0, 5, 5, 0, 0, 25, 0], [34, 0, 0, 1], [34, 1, 0])]
    rng = np.random.RandomState(11)
    for H, W in ((3, 70), (65, 66), (64, 130)):
        for _ in range(4):
            runs, left = [], H * W
            while left:
                r = int(min(left, rng.choice([0, 0, 1, 2, H - 1, H, H + 1, 3 * H, rng.randint(1, 200)])))
                if r == 0 and rng.uniform() < 0.3:      # a zero run exactly where a column starts
                    pad = (-(H * W - left)) % H
                    if 0 < pad <= left:
                        runs.append(pad)
                        left -= pad
                runs.append(r)
                left -= r
            if rng.uniform() < 0.5:
                runs.append(0)
            out.append((H, W, runs))
    return out


# Malformed input, one call per input kind, valid entries between the bad ones (5 x 7 image).
OK, BAD_CHAR, UNTERMINATED, NEGATIVE, BAD_SUM = 0, 1, 2, 3, 4
MALFORMED_SHAPE = (5, 7)


def malformed_strings():
    """[(string, status)]; the valid entries are real masks."""
    rng = np.random.RandomState(3)
    good = [np_rle_string(np_rle_counts(rng.uniform(size=MALFORMED_SHAPE) < 0.5)) for _ in range(3)]
    return [(good[0], OK), ('S1\x7f', BAD_CHAR), ('/S1', BAD_CHAR), ('S', UNTERMINATED),
            (good[1], OK), (NONCANONICAL_TOO_LONG, UNTERMINATED), ('111K', NEGATIVE), ('K', NEGATIVE),
            ('1', BAD_SUM), ('S1S1', BAD_SUM), ('', BAD_SUM), ('S1', OK), (good[2], OK)]


def malformed_lists():
    rng = np.random.RandomState(4)
    good = [np_rle_counts(rng.uniform(size=MALFORMED_SHAPE) < 0.5).tolist() for _ in range(2)]
    return [(good[0], OK), ([-5, 40], NEGATIVE), ([5, 31], BAD_SUM), ([5, 29], BAD_SUM), ([], BAD_SUM),
            ([3, 0, 2, 30], OK), ([40, -5], BAD_SUM), ([10, -1, 26], NEGATIVE), ([INT32_MIN], NEGATIVE),
            ([(1 << 31) - 1, (1 << 31) - 1], BAD_SUM), (good[1], OK)]
