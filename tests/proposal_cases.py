"""Edge inputs of the proposal / NMS / detection kernels (csrc/proposal.hip, csrc/nms.hip), shared
by tests/test_gpu_proposal.py and tests/test_gpu_inference.py (the kernels) and by
tests/test_oracle_boxes.py (the oracle alone on the same inputs: the conditions that make the
inputs worth running).  NumPy only, fixed seeds, no device work; every builder is cached and its
arrays are read-only."""
import functools

import numpy as np

from oracle import np_ref

f32 = np.float32
IMG = (256, 320)
MIN_SIZE = 16                                   # ProposalCreator's default
DECODE_SCALES = (1.0, 1.5, 1.6, 2.5)
CREATOR_PARAMS = dict(n_train_pre_nms=2112, n_train_post_nms=300,
                      n_test_pre_nms=1088, n_test_post_nms=100)
NMS_THRESHOLDS = (0.5, 0.7)
NMS_LIMITS = (0, 1, 37, 300)
SCORE_THRESH = f32(0.05)                        # MaskRCNN.score_thresh as the kernel receives it


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


def rand_boxes(rng, n, size=800.):
    cy, cx = rng.uniform(0, size, n), rng.uniform(0, size, n)
    h, w = rng.uniform(4, 300, n), rng.uniform(4, 300, n)
    b = np.stack([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2], 1)
    return np.clip(b, 0, size).astype(f32)


def dense_boxes(rng, n, n_base=20, jitter=3.):
    """Heavy overlap: jittered copies of a few boxes (tests/test_gpu_proposal.py's
    test_nms_limit_and_dense_overlap)."""
    base = rand_boxes(rng, n_base)
    return (base[rng.randint(0, n_base, n)] + rng.uniform(-jitter, jitter, (n, 4))).astype(f32)


@functools.lru_cache(None)
def anchors():
    """4800 anchors of the shipped anchor base on a 16 x 20 map (image 256 x 320)."""
    ab = np_ref.generate_anchor_base(16, (0.5, 1, 2), (2, 4, 8, 16, 32))
    a = np_ref.enumerate_shifted_anchor(ab, 16, 16, 20)
    assert a.shape == (4800, 4)
    _freeze(a)
    return a


def decode_reference(anchor, loc, img_size, scale, min_size=MIN_SIZE):
    """np_ref.ProposalCreator's arithmetic up to the validity mask: loc2bbox, clip, f32(min_size *
    scale), >=.  Returns (roi (n, 4) f32, valid (n,) bool)."""
    with np.errstate(over='ignore'):
        roi = np_ref.loc2bbox(anchor, loc)
    roi[:, 0::2] = np.clip(roi[:, 0::2], 0, img_size[0])
    roi[:, 1::2] = np.clip(roi[:, 1::2], 0, img_size[1])
    m = f32(min_size * scale)
    return roi, ((roi[:, 2] - roi[:, 0]) >= m) & ((roi[:, 3] - roi[:, 1]) >= m)


def _hand_made_rows():
    """(anchor, loc, tags) of the rows appended to the random ones in decode_cases()."""
    H, W = IMG
    up = lambda v: np.nextafter(f32(v), f32(np.inf))
    down = lambda v: np.nextafter(f32(v), f32(-np.inf))
    anchor, loc, tags = [], [], []

    def add(tag, a, l=(0, 0, 0, 0)):
        anchor.append(a); loc.append(l); tags.append(tag)

    # loc == 0 and integer anchors of side 24 = 16 * 1.5: the decoded side is the anchor's
    # (centre +- half a side, every step exact); far edge one ulp in / out, per axis.  At the
    # origin the side also survives the subtraction of the near edge bit for bit.
    for y0, x0 in ((0, 0), (32, 48), (100, 200), (232, 296)):
        add('exact', (y0, x0, y0 + 24, x0 + 24))
        add('in_h', (y0, x0, down(y0 + 24), x0 + 24))
        add('in_w', (y0, x0, y0 + 24, down(x0 + 24)))
        add('out_h', (y0, x0, up(y0 + 24), x0 + 24))
        add('out_w', (y0, x0, y0 + 24, up(x0 + 24)))
    # the same at the origin for the side f32(16 * scale) of every scale (25.6 is no integer)
    for s in DECODE_SCALES:
        m = f32(MIN_SIZE * s)
        add('exact', (0, 0, m, m))
        add('in_h', (0, 0, down(m), m)); add('in_w', (0, 0, m, down(m)))
        add('out_h', (0, 0, up(m), m)); add('out_w', (0, 0, m, up(m)))
    # min_size reached only before the clip at the image border (24 -> 16 after it)
    add('clipped', (H - 16, 100, H + 8, 124)); add('clipped', (100, W - 16, 124, W + 8))
    add('clipped', (-8, 50, 16, 74)); add('clipped', (50, -8, 74, 16))
    # exp overflows to inf (the box clips to the whole image) or underflows to a denormal / 0
    # (the box collapses onto its centre); the anchors have non-zero sides: no 0 * inf
    big = (90., -90., 800., -800.)
    for dh in big + (0.,):
        for dw in big + (0.,):
            if dh or dw:
                add('exp', (100, 150, 124, 174), (0.125, -0.25, dh, dw))
    return np.asarray(anchor, f32), np.asarray(loc, f32), np.asarray(tags)


@functools.lru_cache(None)
def decode_cases():
    """dict: anchor (n, 4), loc (n, 4) f32 — 4800 random rows (loc ~ 0.3 N(0, 1)) and the hand-made
    block behind them; n_random; tags (n,) ('' for random rows); img_size; scales."""
    rng = np.random.RandomState(101)
    a = anchors()
    loc = (0.3 * rng.standard_normal((len(a), 4))).astype(f32)
    ha, hl, ht = _hand_made_rows()
    anchor, loc = np.concatenate([a, ha]), np.concatenate([loc, hl])
    tags = np.concatenate([np.full(len(a), '', dtype=ht.dtype), ht])
    _freeze(anchor, loc, tags)
    return dict(anchor=anchor, loc=loc, tags=tags, n_random=len(a), img_size=IMG,
                scales=DECODE_SCALES)


@functools.lru_cache(None)
def creator_cases():
    """Tuple of dicts (name, loc (4800, 4), score (4800,), scale) on anchors(); scores carry ties
    (a tenth copied from entry 0, some +-0).  'all_invalid': every box below min_size;
    'few_valid': 700 rows can be valid, fewer than either n_pre_nms."""
    a = anchors()
    n = len(a)
    out = []
    for k, (name, scale) in enumerate((('scale_1.0', 1.0), ('scale_1.6', 1.6), ('scale_2.5', 2.5),
                                       ('all_invalid', 1.5), ('few_valid', 1.6))):
        rng = np.random.RandomState(200 + k)
        loc = (0.3 * rng.standard_normal((n, 4))).astype(f32)
        score = rng.standard_normal(n).astype(f32)
        score[rng.randint(0, n, n // 10)] = score[0]
        score[rng.randint(0, n, 5)] = 0.0
        score[rng.randint(0, n, 5)] = -0.0
        if name == 'all_invalid':
            loc[:, 2:] = -6                     # exp(-6) * 724 < 2 px
        elif name == 'few_valid':
            loc[rng.permutation(n)[700:], 2:] = -6
        _freeze(loc, score)
        out.append(dict(name=name, loc=loc, score=score, scale=scale))
    return tuple(out)


def nms_counts(n_max):
    return np.asarray([0, 1, 63, 64, 65, 511, 512, 513, 1024, 1025, n_max - 1, n_max], np.int32)


def stair_boxes(rng, n, d):
    """tests/test_gpu_proposal.py's test_nms_super_step_structure: box i = [i d, i d + 40]
    squares, every box overlapping its successors across chunk and super-step boundaries."""
    off = np.arange(n, dtype=np.float64) * d % 700.0
    return np.stack([off, off, off + 40.0, off + 40.0], 1).astype(f32)


@functools.lru_cache(None)
def nms_batched_cases():
    """Tuple of dicts (n_max, bbox (12, n_max, 4) f32, counts (12,) i32, kinds): 1088 rows are 17
    chunks (256-thread scan, two super-steps and a chunk), 2112 are 33 (the smallest 1024-thread
    scan, four super-steps and a chunk).  Group g's live rows are a staircase, or (g mod 3 == 1)
    half staircase and half random boxes; the step d stays below 700 / 576 so that the staircase
    wraps round only behind the chunk that follows the first super-step, and keeps and
    suppressions alternate on both sides of row 512.  The rows at and after the count are poison:
    pairwise-disjoint far-away boxes in even groups (kept, if they were live), NaN in odd ones."""
    out = []
    for n_max in (1088, 2112):
        counts = nms_counts(n_max)
        G = len(counts)
        bbox = np.empty((G, n_max, 4), f32)
        kinds = []
        for g in range(G):
            rng = np.random.RandomState(1000 * n_max + g)
            d = rng.uniform(0.6, 1.2)
            live = stair_boxes(rng, n_max, d)
            kind = 'mixed' if g % 3 == 1 else 'stair'
            if kind == 'mixed':
                live = np.where(rng.rand(n_max, 1) < 0.5, live, rand_boxes(rng, n_max)).astype(f32)
            i = np.arange(n_max, dtype=np.float64)
            if g % 2 == 0:
                poison = np.stack([5000 + 20 * i, np.full(n_max, 5000.), 5010 + 20 * i,
                                   np.full(n_max, 5010.)], 1).astype(f32)
            else:
                poison = np.full((n_max, 4), np.nan, f32)
            bbox[g] = np.where(np.arange(n_max)[:, None] < counts[g], live, poison)
            kinds.append(kind)
        _freeze(bbox, counts)
        out.append(dict(n_max=n_max, bbox=bbox, counts=counts, kinds=tuple(kinds)))
    return tuple(out)


DETECT_R = (0, 1, 255, 256, 257, 1025)
DETECT_N_CLASS = (2, 21, 81)


def detect_ids():
    """(R, n_class, variant) of every detect case; R == 1025 with 21 classes only."""
    return [(R, c, v) for R in DETECT_R for c in DETECT_N_CLASS for v in (0, 1)
            if R != 1025 or c == 21]


@functools.lru_cache(None)
def detect_case(R, n_class, variant):
    """dict: cls_bbox (R, n_class, 4) f32, prob (R, n_class) f32, n_class; full (the foreground
    class whose every RoI passes the threshold and whose boxes are near-copies of one box: NMS
    keeps one), empty (the class with no RoI above the threshold, though some exactly at it);
    at / above / below: (row, class) positions of the entries set to f32(0.05) and its two fp32
    neighbours.  Variant 0 makes the first foreground class the full one and the last the empty
    one, variant 1 swaps them; with one foreground class it is full (0) or empty (1).  prob is in
    multiples of 1 / 64 (a third of it zero), so RoIs tie inside a class; boxes are jittered
    copies of 20 boxes, so NMS removes a real share."""
    rng = np.random.RandomState(7919 * R + 31 * n_class + variant)
    cls_bbox = dense_boxes(rng, R * n_class).reshape(R, n_class, 4)
    q = rng.randint(0, 65, (R, n_class)) * (rng.rand(R, n_class) < 0.67)
    prob = (q / 64.).astype(f32)
    prob[rng.rand(R, n_class) < 0.03] = 1.0
    first, last = 1, n_class - 1
    full, empty = (first, last) if variant == 0 else (last, first)
    if first == last:
        full, empty = (first, None) if variant == 0 else (None, last)
    thr = SCORE_THRESH
    below, above = np.nextafter(thr, f32(0)), np.nextafter(thr, f32(1))
    pos = {'at': [], 'above': [], 'below': []}
    if R:
        for c in range(2, n_class - 1):                 # the ordinary classes
            rows = rng.permutation(R)[:3]
            kinds = (('at', thr), ('above', above), ('below', below))
            for r, (name, v) in zip(rows, kinds if R >= 3 else kinds[c % 3:]):
                prob[r, c] = v
                pos[name].append((int(r), c))
        if full is not None:
            prob[:, full] = (rng.randint(4, 65, R) / 64.).astype(f32)     # 1 / 16 and more
            prob[rng.permutation(R)[:1], full] = above
            one = np.asarray([100, 120, 260, 330], f32)
            cls_bbox[:, full] = one + rng.uniform(-1, 1, (R, 4)).astype(f32)
        if empty is not None:
            prob[:, empty] = rng.choice(np.asarray([0, 1 / 64., 2 / 64., 3 / 64., below, thr], f32), R)
            prob[rng.permutation(R)[:1], empty] = thr
            pos['at'] += [(int(r), empty) for r in np.where(prob[:, empty] == thr)[0]]
    _freeze(cls_bbox, prob)
    return dict(cls_bbox=cls_bbox, prob=prob, n_class=n_class, full=full, empty=empty, **pos)


def detect_cases():
    return [detect_case(*i) for i in detect_ids()]
