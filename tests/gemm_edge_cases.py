"""Degenerate and tile-edge shapes of the convolution GEMM family (csrc/conv_gemm.hip): the case
lists of tests/test_gpu_gemm_edges.py and a restatement of the host launch policy
(csrc/conv_gemm_plan.h).

Plain Python, importable without a device.  tests/test_gemm_edge_cases_cpu.py checks the lists
(coverage of the policy's branches and of the kernel instantiations, size caps), the float64
references at these geometries, and that the comparison used on the device rejects the damage each
edge is there to find.

Everything the kernels read is seeded N(0, 1) (filters scaled by 1 / sqrt(C R S)): no zeros, no
repeated rows or columns, so a dropped, duplicated or shifted K element, row, column or tap moves
the result by orders of magnitude more than the bound.

``route(entry, desc, flags, has_ws, knobs)`` restates the decision tree of csrc/conv_gemm_plan.h on
(M, N, Kc, R S, knobs), written by hand from the policy's description and not generated from the C++.
Two things hold it to the C++.  Without a device, tests/test_gemm_edge_cases_cpu.py asks the library
for its plan of the same call (mrcnn_conv_gemm_plan: the planner the entry points run, as text) and
compares the branch label and the kernel instantiation of every launch, on every call of the lists
and on a dense sweep of shapes; the plan's row ranges, grids and slab depths are checked for
consistency there.  On the device, tests/test_gpu_gemm_edges.py counts the launches the profiler
records per kind: they must equal ``Route.record``.

The Winograd route (csrc/conv_winograd.h) has a launch policy of its own, plan_wino_gemm /
plan_wino_wgrad: ``wino_plan()`` restates it (``route()`` takes its three entries too), and the lists
``wino_policy_cases()``, ``WINO_THRESHOLDS``, ``WINO_EPILOGUE_SHAPES`` and ``WINO_FIXUP_SHAPES`` are the
cases of tests/test_gpu_winograd_edges.py.
"""
import collections
import itertools
import math

import numpy as np

# ---- knobs (mrcnn_set_tuning) and their library defaults ----------------------------------------
DEFAULT_KNOBS = collections.OrderedDict([
    ('big_min_tiles', 384), ('big_split_k', -1), ('fused_tail', 512), ('tiny_split', 1),
    ('small_m_split', 0), ('split_bf16', 3), ('pw', 3), ('position_major_rows', 1)])
# not restorable through the issue's list, never changed here: read by route() at their defaults
_BIG_SPLIT_MIN_SLICES, _W8, _W8_MIN_K = 16, 1, 256

BK = 32
K_PERM_BLOCK = 128
SPLIT_WS_BYTES = 192 << 20
SLOTS_BIG, SLOTS_SMALL = 512, 1024
FWD, DGRAD, WGRAD = 'FWD', 'DGRAD', 'WGRAD'
OUT_PLAIN, OUT_STRIDED, OUT_DECONV = 'OUT_PLAIN', 'OUT_STRIDED', 'OUT_DECONV'
EPI_ACCUM = 16

FWD_LABELS = ('small/plain', 'small/tiny_split', 'small/fused_tail', 'small/main+split_leftover',
              'big/one_round_ksplit', 'big/all_rows', 'big/fused_tail', 'big/main+plain_remainder',
              'big/main+split_remainder')
WGRAD_LABELS = ('wgrad64/one_slab', 'wgrad64/split+reduce', 'wgrad128/split+reduce', 'wgrad/wperm64',
                'wgrad/wperm128', 'wgrad/no_ws')
# branches the policy has beside the label set above: the W8 launches of a plain GEMM (their smallest
# problem has 768 tiles of 256x128; the W8 kernel itself is reached through the Winograd route's batch
# of 36, 'wino/w8' below, at 22 tiles per frequency), the occupancy split behind the small_m_split knob
# (default 0 = off), and a 128x128 weight gradient that ends up with one slab
OTHER_LABELS = ('w8', 'small/m_split', 'wgrad128/one_slab')
# the Winograd route's own policy (plan_wino_gemm / plan_wino_wgrad)
WINO_LABELS = ('wino/small64', 'wino/big128', 'wino/main128+tail64', 'wino/w8',
               'wino_wgrad64/one_slab', 'wino_wgrad64/split+sum', 'wino_wgrad128/one_slab',
               'wino_wgrad128/split+sum')
WINO_XI, WINO_MAX_SPLITS = 36, 8


class Desc(collections.namedtuple('Desc', 'N H W C K R S stride pad')):
    """mrcnn_conv_desc without its derived fields."""
    __slots__ = ()

    @property
    def P(self):
        return (self.H + 2 * self.pad - self.R) // self.stride + 1

    @property
    def Q(self):
        return (self.W + 2 * self.pad - self.S) // self.stride + 1


def desc(N, C, H, W, K, R=1, S=None, stride=1, pad=0):
    return Desc(N, H, W, C, K, R, R if S is None else S, stride, pad)


Route = collections.namedtuple('Route', 'label launches record')
"""label: the branch; launches: [(profiler kind, instantiation tags)] in launch order; record:
{profiler kind: GEMM launches}, what mrcnn_profile_summary reports for the call."""


def ceil_div(a, b):
    return -(-a // b)


def kind_name(tm, mode):
    return 'conv_gemm_kernel<%d,%d,%s>' % (tm, tm, mode)


# single_buffered(): one LDS stage (and three 128x128 workgroups per CU)
def _single_buffered(tm, mode):
    if tm == 1:
        return mode == FWD
    return tm >= 2 and mode in (FWD, WGRAD)


# choose_perm(): position-major row order for many small maps under a padded filter
def choose_perm(n_img, gp, gq, R, S, stride, pad_eff, knobs):
    if not knobs['position_major_rows'] or R * S <= 1 or R * S > 16 or stride != 1 or pad_eff <= 0:
        return 0
    if gp * gq > 256 or n_img < 64:
        return 0
    return n_img


class _P(object):
    """The fields of GemmParams the policy reads."""

    def __init__(self, mode, M, N, Kc, R=1, S=1, stride=1, pad=0, gp=0, gq=0, sh=0, sw=0, ldc=None,
                 out_mode=OUT_PLAIN, stem=0, perm_n=0, has_ws=False):
        self.mode, self.M, self.N, self.Kc, self.R, self.S = mode, M, N, Kc, R, S
        self.stride, self.pad, self.gp, self.gq, self.sh, self.sw = stride, pad, gp, gq, sh, sw
        self.ldc = N if ldc is None else ldc
        self.out_mode, self.stem, self.perm_n, self.has_ws = out_mode, stem, perm_n, has_ws

    @property
    def total_slices(self):
        return self.R * self.S * ceil_div(self.Kc, BK)


# pw_plain(): PW's launch rule
def pw_plain(p):
    return (p.R == 1 and p.S == 1 and p.stride == 1 and p.pad == 0 and p.perm_n == 0 and not p.stem
            and p.gp == p.sh and p.gq == p.sw and p.out_mode == OUT_PLAIN)


# k3_plain(): K3's launch rule
def k3_plain(p):
    return (p.R == 3 and p.S == 3 and p.stride == 1 and p.pad == 1 and p.perm_n == 0 and not p.stem
            and p.out_mode == OUT_PLAIN)


# launch_kernel(): which instantiation of conv_gemm_kernel a launch of (TM, MODE) runs
def instantiation(p, tm, knobs):
    tags = [p.mode, '%dx%d' % (64 * tm, 64 * tm), p.out_mode]
    sb, pw = knobs['split_bf16'], knobs['pw']
    if p.mode == WGRAD:
        if tm == 2 and (sb & 1) and p.perm_n == 0:
            return tuple(tags + ['split', 'general'])
        if p.perm_n > 0:
            return tuple(tags + ['fp32', 'WPERM'])
        return tuple(tags + ['fp32', 'general'])
    extra = (['perm'] if p.perm_n > 0 else []) + (['stem'] if p.stem else [])
    if p.mode == FWD and (sb & (1 if tm == 2 else 2)):
        if (pw & 1) and pw_plain(p):
            return tuple(tags + ['split', 'PW'])
        if (pw & 2) and k3_plain(p):
            return tuple(tags + ['split', 'K3'])
        return tuple(tags + ['split', 'general'] + extra)
    return tuple(tags + ['fp32', 'general'] + extra)


# can_split_rows()
def can_split_rows(p):
    return (p.has_ws and p.mode != WGRAD and p.out_mode == OUT_PLAIN and not p.stem and
            p.N % 4 == 0 and p.ldc == p.N)


# fit_ws(): fewer slabs while they overflow the split-K workspace.
# The clamp is unreachable at the default knobs for every problem the entry points accept; each
# caller bounds tiles x slabs before it gets here (a 64x64 tile of a slab is 16 KiB, a 128x128 one
# 64 KiB, the workspace 192 MiB = 12288 / 3072 of them):
#   plan_gemm(), one-round rule:   T x fit <= 512 tiles of 128x128                    = 32 MiB
#   plan_gemm(), big_split_k > 0:  T < big_min_tiles = 384, <= 8 slabs: 383 x 8 x 64 KiB = 191.5 MiB
#   add_small(), tiny split:       T <= 128 tiles of 64x64, <= 16 slabs                 = 32 MiB
#   add_small(), leftover:         two slabs need < 256 leftover tiles, tiles x slabs < 512:  8 MiB
#   add_fused_tail() (64x64):      < 154 tail tiles x 16 slabs                         = 38.5 MiB
#   add_fused_tail() (128x128) and add_remainder(): two slabs need < 512 tail tiles and then
#                                  tiles x slabs < 1024 tiles                  <= 64 MiB / 16 MiB
# (reachable only with big_min_tiles raised above 384 or small_m_split >= 24).  No case is invented
# for it; route() still applies it.
def fit_ws(splits, rows, N):
    while splits > 1 and rows * N * splits * 4 > SPLIT_WS_BYTES:
        splits -= 1
    return splits


# k_splits()
def k_splits(total_slices, depth_div, target_wgs, tiles, rows, N, cap):
    return fit_ws(min(cap, total_slices // depth_div, ceil_div(target_wgs, tiles)), rows, N)


# add_split_rows(): the slab count re-derived from the slab depth (one GEMM launch + slab sum)
def _split_rows(p, tm, knobs):
    return [(kind_name(tm, p.mode), instantiation(p, tm, knobs))]


# add_fused_tail(): whole tiles and the K-split pieces of the leftover rows in ONE launch
def _fused_tail(p, tm, rows_main, knobs):
    BM = 64 * tm
    if (not knobs['fused_tail'] or not can_split_rows(p) or rows_main <= 0 or rows_main % BM != 0
            or rows_main >= p.M):
        return False
    ntn = ceil_div(p.N, BM)
    tail_tiles = ceil_div(p.M - rows_main, BM) * ntn
    target = 512 if knobs['fused_tail'] == 1 else knobs['fused_tail']
    return k_splits(p.total_slices, 4, target, tail_tiles, p.M - rows_main, p.N, 16) >= 2


# add_tiles(): a record only when the launch has blocks
def _tiles(p, tm, m_lo, m_hi, knobs):
    if ceil_div(m_hi - m_lo, 64 * tm) * ceil_div(p.N, 64 * tm) <= 0:
        return []
    return [(kind_name(tm, p.mode), instantiation(p, tm, knobs))]


# add_remainder(): the 64x64 remainder of a 128x128 launch, cut along K when it pays
def _remainder(p, rows_lo, knobs):
    left = ceil_div(p.M - rows_lo, 64) * ceil_div(p.N, 64)
    splits = k_splits(p.total_slices, 8, 512, left, p.M - rows_lo, p.N, 16)
    if not can_split_rows(p) or splits < 2:
        return 'plain', _tiles(p, 1, rows_lo, p.M, knobs)
    return 'split', _split_rows(p, 1, knobs)


# add_small(): 64x64 tiles
def _launch_small(p, knobs):
    tm, tn = ceil_div(p.M, 64), ceil_div(p.N, 64)
    T = tm * tn
    whole = (T // 256) * 256
    rem = T - whole
    total = p.total_slices
    if knobs['tiny_split'] and can_split_rows(p) and T <= 128 and total >= 32:
        if k_splits(total, 8, 512, T, p.M, p.N, 16) >= 2:
            return 'small/tiny_split', _split_rows(p, 1, knobs)
    sms = knobs['small_m_split']
    if sms > 0 and can_split_rows(p) and T < 256 * sms and total >= 16:
        if k_splits(total, 8, 256 * sms, T, p.M, p.N, 16) >= 2:
            return 'small/m_split', _split_rows(p, 1, knobs)
    can_split = (can_split_rows(p) and whole > 0 and whole <= 1024 and rem > 0 and rem < 154 and
                 total >= 8)
    rows_main = min(p.M, (whole // tn) * 64) if can_split else p.M
    left_tiles = ceil_div(p.M - rows_main, 64) * tn
    splits = 1
    if can_split and rows_main < p.M:
        splits = k_splits(total, 4, 256, left_tiles, p.M - rows_main, p.N, 16)
    if splits < 2:
        return 'small/plain', _tiles(p, 1, 0, p.M, knobs)
    if _fused_tail(p, 1, rows_main, knobs):
        return 'small/fused_tail', [(kind_name(1, p.mode), instantiation(p, 1, knobs))]
    return 'small/main+split_leftover', _tiles(p, 1, 0, rows_main, knobs) + _split_rows(p, 1, knobs)


# w8_ok(): the 256x128-tile launches (out of scope; restated so that no case takes them unnoticed)
def _w8_ok(p, knobs, batch=1):
    if (not _W8 or not (knobs['split_bf16'] & 1) or p.out_mode != OUT_PLAIN or p.stem or
            not (p.R == 1 and p.S == 1 and p.stride == 1 and p.pad == 0 and p.perm_n == 0 and
                 p.gp == p.sh and p.gq == p.sw)):
        return False
    tm, tn = ceil_div(p.M, 256), ceil_div(p.N, 128)
    return (p.N >= 128 and p.Kc >= _W8_MIN_K and tm * tn * batch >= 768 and
            (p.M % 256 == 0 or p.M >= 16 * 256))


# plan_gemm(): the forward / DGRAD policy
def _launch(p, knobs):
    tm, tn = ceil_div(p.M, 128), ceil_div(p.N, 128)
    T = tm * tn
    big_ok = p.N > 64 and p.M > 64
    total = p.total_slices
    ksplits = 1
    if knobs['big_split_k'] != 0 and big_ok and T < knobs['big_min_tiles'] and can_split_rows(p):
        if knobs['big_split_k'] > 0:
            ksplits = k_splits(total, 8, knobs['big_split_k'], T, p.M, p.N, 8)
        else:
            fit = SLOTS_BIG // T
            if 2 <= fit <= 8 and T * fit >= SLOTS_BIG * 3 // 4 and total // fit >= _BIG_SPLIT_MIN_SLICES:
                ksplits = fit_ws(fit, p.M, p.N)
    if p.mode == FWD and _w8_ok(p, knobs):
        return 'w8', [('conv_gemm_kernel<2,2,FWD,W8>', (FWD, '256x128', p.out_mode, 'split', 'W8'))]
    if ksplits >= 2:
        return 'big/one_round_ksplit', _split_rows(p, 2, knobs)
    if not big_ok or T < knobs['big_min_tiles']:
        return _launch_small(p, knobs)
    split_fwd = p.mode == FWD and (knobs['split_bf16'] & 1)
    max_per_cu = 3 if (not split_fwd and _single_buffered(2, p.mode)) else 2
    main_tiles_m, best_rem = tm, T
    for k in range(max_per_cu, 0, -1):
        slots = 256 * k
        full = T // slots
        rem = T - full * slots
        if full >= 1 and rem < best_rem:
            best_rem = rem
            main_tiles_m = (full * slots) // tn if 0 < rem < 154 else tm
    rows_main = min(p.M, main_tiles_m * 128)
    if _fused_tail(p, 2, rows_main, knobs):
        return 'big/fused_tail', [(kind_name(2, p.mode), instantiation(p, 2, knobs))]
    main = _tiles(p, 2, 0, rows_main, knobs)
    if rows_main >= p.M:
        return 'big/all_rows', main
    how, rest = _remainder(p, rows_main, knobs)
    return 'big/main+%s_remainder' % how, main + rest


# wgrad_splits(): the split count whose workgroups fill whole rounds best
def wgrad_splits(tiles, pixels, slots):
    maxs = min(64, max(1, pixels // (8 * BK)))
    best, best_u = 1, -1.
    for sp in range(1, maxs + 1):
        blocks = tiles * sp
        if blocks > 3 * slots and sp > 1:
            break
        u = blocks / float(ceil_div(blocks, slots) * slots)
        if u > best_u + 1e-9:
            best_u, best = u, sp
    return best


# plan_wgrad(): M = Kout rows, N = R S C columns, K = pixels
def _wgrad(Kout, pixels, n_img, C, P, Q, R, S, stride, pad, has_ws, knobs):
    M, N = Kout, R * S * C
    big = ceil_div(M, 128) * ceil_div(N, 128)
    small = ceil_div(M, 64) * ceil_div(N, 64)
    max_splits = min(64, max(1, pixels // (8 * BK)))
    use_big = N > 64 and M > 64 and (big * max_splits * 2 >= SLOTS_BIG or knobs['big_min_tiles'] <= 1)
    tiles = big if use_big else small
    perm_n = 0
    if C % (128 if use_big else 64) == 0 and n_img >= BK:
        perm_n = choose_perm(n_img, P, Q, R, S, stride, pad, knobs)
    k_extent = ceil_div(n_img, BK) * BK * P * Q if perm_n else pixels
    split_kernel = (knobs['split_bf16'] & 1) and perm_n == 0
    slots_big = 768 if (not split_kernel and _single_buffered(2, WGRAD)) else SLOTS_BIG
    splits = wgrad_splits(tiles, pixels, slots_big if use_big else SLOTS_SMALL)
    if not has_ws:
        splits = 1
    split_len = ceil_div(ceil_div(k_extent, splits), BK) * BK
    splits = ceil_div(k_extent, split_len)
    tm = 2 if use_big else 1
    p = _P(WGRAD, M, N, pixels, R, S, stride, pad, perm_n=perm_n, has_ws=has_ws)
    if not has_ws:
        label = 'wgrad/no_ws'
    elif perm_n:
        label = 'wgrad/wperm%d' % (64 * tm)
    else:
        label = 'wgrad%d/%s' % (64 * tm, 'split+reduce' if splits > 1 else 'one_slab')
    return label, [(kind_name(tm, WGRAD), instantiation(p, tm, knobs))]


# ---- the Winograd route: 36 per-frequency GEMMs per launch (blockIdx.z), three planes when split ------
W8_KIND = 'conv_gemm_kernel<2,2,FWD,W8>'
WinoLaunch = collections.namedtuple('WinoLaunch', 'kind tags rows grid slab')
"""rows: (m_lo, m_hi); grid: (x, y) with the batch of 36 in z; slab: K slices' worth of tiles per slab
(weight gradient), else 0."""
WinoPlan = collections.namedtuple('WinoPlan', 'label M N k launches slabs')


def wino_tiles(d):
    return d.N * ceil_div(d.H, 4) * ceil_div(d.W, 4)


def _wino_p(mode, M, N, Kc):
    return _P(mode, M, N, Kc, gp=1, gq=1, sh=1, sw=1)


# plan_wino_gemm(): forward (rows = tiles, columns = K, depth = C) and data gradient (columns = C, depth = K)
def wino_gemm_plan(T, N, Kc, knobs):
    p = _wino_p(FWD, T, N, Kc)
    big = T > 64 and N > 64
    rem = T % 128

    def launch(tm, lo, hi):
        return WinoLaunch(kind_name(tm, FWD), instantiation(p, tm, knobs), (lo, hi),
                          (ceil_div(hi - lo, 64 * tm) * ceil_div(N, 64 * tm), 1), 0)
    if big and _w8_ok(p, knobs, WINO_XI):
        return WinoPlan('wino/w8', T, N, ceil_div(Kc, BK), [WinoLaunch(
            W8_KIND, (FWD, '256x128', OUT_PLAIN, 'split', 'W8'), (0, T), (ceil_div(T, 256) * ceil_div(N, 128), 1), 0)], 0)
    if big and 0 < rem <= 64 and T >= 256:
        return WinoPlan('wino/main128+tail64', T, N, ceil_div(Kc, BK), [launch(2, 0, T - rem), launch(1, T - rem, T)], 0)
    if big:
        return WinoPlan('wino/big128', T, N, ceil_div(Kc, BK), [launch(2, 0, T)], 0)
    return WinoPlan('wino/small64', T, N, ceil_div(Kc, BK), [launch(1, 0, T)], 0)


# plan_wino_wgrad(): K rows, C columns, summed over the T tiles in at most WINO_MAX_SPLITS slabs
def wino_wgrad_plan(T, K, C, knobs):
    p = _wino_p(WGRAD, K, C, T)
    big = K > 64 and C > 64
    tm = 2 if big else 1
    tiles = ceil_div(K, 64 * tm) * ceil_div(C, 64 * tm)
    # (768 slots for the 128x128 tiles whatever the arithmetic: single_buffered(2, WGRAD))
    slots = (768 if _single_buffered(2, WGRAD) else SLOTS_BIG) if big else SLOTS_SMALL
    splits = min(WINO_MAX_SPLITS, wgrad_splits(tiles * WINO_XI, T, slots))
    split_len = ceil_div(ceil_div(T, splits), BK) * BK
    splits = ceil_div(T, split_len)
    label = 'wino_wgrad%d/%s' % (64 * tm, 'split+sum' if splits > 1 else 'one_slab')
    return WinoPlan(label, K, C, T, [WinoLaunch(kind_name(tm, WGRAD), instantiation(p, tm, knobs), (0, K),
                                                (tiles, splits), split_len)], splits)


WINO_ENTRIES = ('conv3x3_wino_fwd', 'conv3x3_wino_dgrad', 'conv3x3_wino_wgrad')


def wino_plan(entry, d, knobs=None):
    """The WinoPlan of one call of a WINO_ENTRIES name."""
    kn = dict(DEFAULT_KNOBS)
    kn.update(knobs or {})
    T = wino_tiles(d)
    if entry == 'conv3x3_wino_fwd':
        return wino_gemm_plan(T, d.K, d.C, kn)
    if entry == 'conv3x3_wino_dgrad':
        return wino_gemm_plan(T, d.C, d.K, kn)
    if entry == 'conv3x3_wino_wgrad':
        return wino_wgrad_plan(T, d.K, d.C, kn)
    raise ValueError(entry)


def wino_rejects(d):
    """wino_check(): why the Winograd entry points refuse ``d`` (None: accepted)."""
    if (d.R, d.S, d.stride, d.pad) != (3, 3, 1, 1):
        return 'the Winograd path serves 3x3 / stride 1 / pad 1 only'
    if d.C % 4 or d.K % 4:
        return 'channel'
    if d.N * d.H * d.W * d.C >= 2 ** 31 - 1 or d.N * d.P * d.Q * d.K >= 2 ** 31 - 1:
        return 'tensor exceeds 2^31 elements'
    if wino_tiles(d) * max(d.C, d.K) >= 1 << 29:
        return 'one frequency plane exceeds 2 GiB'
    return None


ENTRIES = ('conv2d_fwd', 'conv_stem_fwd', 'conv2d_dgrad', 'conv2d_dgrad_ex', 'conv2d_dgrad_wt',
           'conv2d_wgrad', 'conv2d_wgrad_ex', 'deconv2x2s2_fwd', 'deconv2x2s2_fwd_wt',
           'deconv2x2s2_dgrad', 'deconv2x2s2_wgrad')


def gemm_problem(entry, d, has_ws, knobs):
    """The GemmParams each entry point of conv_gemm.hip builds from its descriptor (forward / DGRAD
    entries; the deconvolution descriptors carry the INPUT map (N, H, W, C) and K output channels)."""
    if entry == 'conv2d_fwd':                       # mrcnn_conv2d_fwd
        perm = choose_perm(d.N, d.P, d.Q, d.R, d.S, d.stride, d.pad, knobs)
        M = ceil_div(d.N, K_PERM_BLOCK) * K_PERM_BLOCK * d.P * d.Q if perm else d.N * d.P * d.Q
        return _P(FWD, M, d.K, d.C, d.R, d.S, d.stride, d.pad, d.P, d.Q, d.H, d.W, perm_n=perm,
                  has_ws=has_ws)
    if entry == 'conv_stem_fwd':                    # mrcnn_conv_stem_fwd: no workspace argument
        P, Q = (d.H + 6 - 7) // 2 + 1, (d.W + 6 - 7) // 2 + 1
        return _P(FWD, d.N * P * Q, d.K, 32, 7, 1, 2, 3, P, Q, d.H, d.W, stem=1, has_ws=False)
    if entry in ('conv2d_dgrad', 'conv2d_dgrad_ex'):    # mrcnn_conv2d_dgrad_ex (dgrad: ws = NULL)
        ws = has_ws and entry == 'conv2d_dgrad_ex'
        if d.stride == 1:
            return _P(DGRAD, d.N * d.H * d.W, d.C, d.K, d.R, d.S, 1, d.pad, d.H, d.W, d.P, d.Q,
                      has_ws=ws)
        return _P(DGRAD, d.N * d.P * d.Q, d.C, d.K, d.R, d.S, d.stride, d.pad, d.P, d.Q, d.P, d.Q,
                  out_mode=OUT_STRIDED, has_ws=ws)
    if entry == 'conv2d_dgrad_wt':                  # mrcnn_conv2d_dgrad_wt
        if d.stride > 1:                            # (the strided branch never sets split_ws)
            return _P(FWD, d.N * d.P * d.Q, d.C, d.K, 1, 1, 1, 0, d.P, d.Q, d.P, d.Q,
                      out_mode=OUT_STRIDED, has_ws=False)
        pad = d.R - 1 - d.pad
        perm = choose_perm(d.N, d.H, d.W, d.R, d.S, 1, pad, knobs)
        M = ceil_div(d.N, K_PERM_BLOCK) * K_PERM_BLOCK * d.H * d.W if perm else d.N * d.H * d.W
        return _P(FWD, M, d.C, d.K, d.R, d.S, 1, pad, d.H, d.W, d.P, d.Q, perm_n=perm, has_ws=has_ws)
    if entry == 'deconv2x2s2_fwd':                  # mrcnn_deconv2x2s2_fwd: K-strided form
        return _P(DGRAD, d.N * d.H * d.W, 4 * d.K, d.C, 1, 1, 1, 0, d.H, d.W, d.H, d.W, ldc=d.K,
                  out_mode=OUT_DECONV, has_ws=False)
    if entry == 'deconv2x2s2_fwd_wt':               # mrcnn_deconv2x2s2_fwd_wt: forward form
        return _P(FWD, d.N * d.H * d.W, 4 * d.K, d.C, 1, 1, 1, 0, d.H, d.W, d.H, d.W, ldc=d.K,
                  out_mode=OUT_DECONV, has_ws=False)
    if entry == 'deconv2x2s2_dgrad':                # mrcnn_deconv2x2s2_dgrad = conv2d_fwd 2x2 / 2
        return _P(FWD, d.N * d.H * d.W, d.C, d.K, 2, 2, 2, 0, d.H, d.W, 2 * d.H, 2 * d.W,
                  has_ws=False)
    raise ValueError(entry)


def route(entry, d, flags=0, has_ws=True, knobs=None):
    """The branch, the launches and the profiler record of one call of ``entry`` (an ENTRIES or
    WINO_ENTRIES name)
    with descriptor ``d`` under ``knobs`` (DEFAULT_KNOBS updated by the dict given).  ``flags`` (the
    MRCNN_EPI_* bits) do not steer the policy; they are accepted so that a call site states them."""
    kn = dict(DEFAULT_KNOBS)
    kn.update(knobs or {})
    if entry in WINO_ENTRIES:
        # one profiler record per GEMM scope: the main128+tail64 pair is ONE record of the 128x128 kind
        w = wino_plan(entry, d, kn)
        return Route(w.label, [(l.kind, l.tags) for l in w.launches], {w.launches[0].kind: 1})
    if entry in ('conv2d_wgrad', 'conv2d_wgrad_ex'):        # mrcnn_conv2d_wgrad_ex
        label, launches = _wgrad(d.K, d.N * d.P * d.Q, d.N, d.C, d.P, d.Q, d.R, d.S, d.stride, d.pad,
                                 has_ws, kn)
    elif entry == 'deconv2x2s2_wgrad':                      # mrcnn_deconv2x2s2_wgrad
        label, launches = _wgrad(d.C, d.N * d.H * d.W, d.N, d.K, d.H, d.W, 2, 2, 2, 0, has_ws, kn)
    else:
        label, launches = _launch(gemm_problem(entry, d, has_ws, kn), kn)
    return Route(label, launches, dict(collections.Counter(k for k, _ in launches)))


def moved_bytes(entry, d):
    """Bytes of the operands and the output of one call (fp32)."""
    if entry.startswith('deconv'):
        return 4 * (d.N * d.H * d.W * d.C + 4 * d.C * d.K + 4 * d.N * d.H * d.W * d.K)
    if entry == 'conv_stem_fwd':
        P, Q = (d.H - 1) // 2 + 1, (d.W - 1) // 2 + 1
        return 4 * (d.N * d.H * d.W * 4 + d.K * 7 * 8 * 4 + d.N * P * Q * d.K)
    return 4 * (d.N * d.H * d.W * d.C + d.K * d.R * d.S * d.C + d.N * d.P * d.Q * d.K)


# ---- operands -----------------------------------------------------------------------------------

def seed_of(*key):
    return (hash(tuple(int(k) for k in key)) & 0x7fffffff) % 1000003 + 1


def operands(d, seed=None):
    """x (N,C,H,W), w (K,C,R,S) / sqrt(C R S), gy (N,K,P,Q), fp32 NCHW / KCRS, seeded N(0,1)."""
    rng = np.random.RandomState(seed_of(*d) if seed is None else seed)
    x = rng.standard_normal((d.N, d.C, d.H, d.W)).astype(np.float32)
    w = (rng.standard_normal((d.K, d.C, d.R, d.S)) / math.sqrt(d.C * d.R * d.S)).astype(np.float32)
    gy = rng.standard_normal((d.N, d.K, d.P, d.Q)).astype(np.float32)
    return x, w, gy


# ---- the case lists -----------------------------------------------------------------------------
# Tile-boundary grid, pointwise: F.conv2d on (1, Cin, 1, M) with a 1x1 filter
PW_M = (1, 63, 64, 65, 128, 129, 200)
PW_COUT = (4, 60, 64, 68, 128, 132)
PW_CIN = (4, 28, 32, 36, 64, 100)


def pw_desc(M, Cout, Cin):
    return desc(1, Cin, 1, M, Cout)


def pw_id(M, Cout, Cin):
    return 'pw rows%d(%s) cols%d(%s) depth%d(%s)' % (M, _edge(M, (64, 128)), Cout, _edge(Cout, (64, 128)),
                                                     Cin, _edge(Cin, (32, 64)))


def _edge(v, bounds):
    for b in bounds:
        if v == b:
            return 'at %d' % b
        if v == b - 1 or v == b + 1:
            return '%d%+d' % (b, v - b)
    below = [b for b in bounds if v < b]
    return 'below %d' % below[0] if below and v < bounds[0] else 'off-tile'


PW_GRID = [(pw_id(*c), c) for c in itertools.product(PW_M, PW_COUT, PW_CIN)]
PW_BIG_GRID = [(i, c) for i, c in PW_GRID if c[0] > 64 and c[1] > 64]       # 128x128 tiles (big_min_tiles = 1)
PW_DIAGONAL = [(pw_id(*c), c) for c in ((1, 4, 4), (63, 60, 28), (64, 64, 32), (65, 68, 36),
                                        (128, 128, 64), (129, 132, 100), (200, 132, 100))]

# Small maps under real filters: (what, R, S, pad, H, W)
SMALL_MAP_GEOMS = [
    ('3x3p1 on 1x1: every tap but the centre reads padding', 3, 3, 1, 1, 1),
    ('3x3p1 on 1x2', 3, 3, 1, 1, 2),
    ('3x3p1 on 2x2: filter larger than the map', 3, 3, 1, 2, 2),
    ('3x3p1 on 3x3', 3, 3, 1, 3, 3),
    ('3x3p1 on 1x9: one row', 3, 3, 1, 1, 9),
    ('3x3p1 on 7x7', 3, 3, 1, 7, 7),
    ('3x3p0 on 3x3: one output pixel', 3, 3, 0, 3, 3),
    ('3x3p0 on 4x5', 3, 3, 0, 4, 5),
    ('1x3p0 on 2x5: non-square filter, the K-strided dgrad_ex route', 1, 3, 0, 2, 5),
]
SMALL_MAP_N = (1, 3, 63, 64, 65, 128, 129)       # 64: choose_perm's threshold; 128: kPermBlock
SMALL_MAP_CK = ((4, 4), (36, 40), (64, 128), (128, 64))


def small_map_cases(geom):
    what, R, S, pad, H, W = geom
    return [('%s, %d images, C%d K%d' % (what, N, C, K), desc(N, C, H, W, K, R, S, 1, pad))
            for N in SMALL_MAP_N for C, K in SMALL_MAP_CK]


# choose_perm's position threshold: 256 positions take the position-major order, 272 do not
PERM_POSITIONS = [('3x3p1 16x16 = 256 positions at 64 images: position-major', desc(64, 36, 16, 16, 40, 3, 3, 1, 1)),
                  ('3x3p1 16x17 = 272 positions at 64 images: natural order', desc(64, 36, 16, 17, 40, 3, 3, 1, 1))]

# Strided 1x1
STRIDED_MAPS = ((1, 1), (2, 2), (3, 3), (5, 4), (7, 7), (13, 10))
STRIDED_NCK = ((1, 4, 4), (3, 36, 40), (2, 64, 132))
STRIDED = [('1x1 stride 2 on %dx%d%s, %d images, C%d K%d' % (H, W, ' (odd map)' if (H | W) & 1 else '', N, C, K),
            desc(N, C, H, W, K, 1, 1, 2, 0)) for H, W in STRIDED_MAPS for N, C, K in STRIDED_NCK]

# K-strided entry points, direct: the fused pieces of the data-gradient epilogue
DGRAD_VARIANTS = ('plain', 'accum', 'res_g', 'res_g+res_y', 'out_mask_y', 'out_scale', 'all')
DGRAD_DIRECT = ([('dgrad ' + pw_id(M, K, C), desc(1, C, 1, M, K))
                 for M in (1, 63, 65, 129) for C in (4, 68, 132) for K in (4, 36, 100)] +
                [('dgrad %s, %d images, C%d K%d' % (g[0], N, C, K), desc(N, C, g[4], g[5], K, 3, 3, 1, 1))
                 for g in SMALL_MAP_GEOMS[:4] + SMALL_MAP_GEOMS[5:6] for N in (1, 3, 65)
                 for C, K in ((4, 4), (36, 40))])
# 64 rows x 64 columns x 1024 deep: one tile, 32 K slices -> tiny_split in DGRAD mode, the fused
# pieces applied by splitk_epilogue_kernel
DGRAD_TINY_SPLIT = ('dgrad 64 rows x 64 cols x 1024 deep: small/tiny_split, epilogue in the slab sum',
                    desc(1, 64, 1, 64, 1024))

# Deconvolution 2x2 / 2: (N, H, W) by pixel count
DECONV_PIXELS = {1: (1, 1, 1), 49: (1, 7, 7), 65: (1, 5, 13), 196: (4, 7, 7)}
DECONV = [('deconv 4K=%d (%s) C%d %d pixels' % (4 * K, 'whole tiles' if 4 * K % 64 == 0 else
                                                 'a column group straddles a tile', C, px),
           desc(n, C, h, w, K, 2, 2, 2, 0))
          for K in (4, 20, 36, 64) for C in (4, 36, 64) for px, (n, h, w) in sorted(DECONV_PIXELS.items())]

# Linear
LINEAR = [('linear rows%d in%d out%d' % (R, Cin, Cout), (R, Cin, Cout))
          for R in (1, 2, 64, 65) for Cin in (4, 100, 2048) for Cout in (4, 84, 408)]

# Stem 7x7 / 2 / pad 3
STEM = [('stem %dx%d image%s, %d images, K%d, %s' % (H, W, ' smaller than the filter' if min(H, W) < 7 else '',
                                                     N, K, 'affine' if aff else 'bias only'),
         (N, H, W, K, aff))
        for H, W in ((1, 1), (3, 5), (7, 7), (8, 9), (14, 13)) for N in (1, 3) for K in (4, 64)
        for aff in (True, False)]


def stem_desc(N, H, W, K):
    return Desc(N, H, W, 3, K, 7, 7, 2, 3)


# Weight gradient by pixel count: (1, C, 1, pixels) 1x1, so R S C = C
WGRAD_PIXELS = (1, 31, 32, 33, 255, 256, 257, 511, 512, 513)
WGRAD_KOUT = (4, 60, 68, 132)
WGRAD_RSC = (60, 68, 124, 132)
WGRAD_BY_PIXELS = [('wgrad %d pixels (%s) Kout%d RSC%d' % (px, 'fewer than 8 slices: one slab' if px < 256
                                                           else 'splits allowed', Ko, C),
                    desc(1, C, 1, px, Ko)) for px in WGRAD_PIXELS for Ko in WGRAD_KOUT for C in WGRAD_RSC]
# the WPERM gate: position-major pixel order needs C % 64 (64x64 tiles) / C % 128 (128x128 tiles, here
# under big_min_tiles = 1), >= 64 images (choose_perm; plan_wgrad()'s own N >= 32 is implied) and <= 256 positions
WGRAD_WPERM = [
    ('wperm64: C%64 == 0, 64 images', desc(64, 64, 2, 2, 4, 3, 3, 1, 1), {}, 'wgrad/wperm64'),
    ('no wperm: C=96, C%64 != 0', desc(64, 96, 2, 2, 4, 3, 3, 1, 1), {}, 'wgrad64/one_slab'),
    ('no wperm: 63 images', desc(63, 64, 2, 2, 4, 3, 3, 1, 1), {}, 'wgrad64/one_slab'),
    ('wperm64 ragged: 129 images, 7x7', desc(129, 64, 7, 7, 60, 3, 3, 1, 1), {}, 'wgrad/wperm64'),
    ('wperm128: C%128 == 0 on 128x128 tiles', desc(64, 128, 2, 2, 132, 3, 3, 1, 1), {'big_min_tiles': 1},
     'wgrad/wperm128'),
    ('no wperm on 128x128 tiles: C=192, C%128 != 0', desc(64, 192, 4, 4, 132, 3, 3, 1, 1),
     {'big_min_tiles': 1}, 'wgrad128/split+reduce'),
    ('wgrad128 by the fill rule: 68 x 4608 x 2048 pixels', desc(8, 512, 16, 16, 68, 3, 3, 1, 1), {},
     'wgrad128/split+reduce'),
]

# Winograd at tiny maps: (N, C, H, W, K)
WINOGRAD = [(1, 4, 1, 1, 4), (1, 36, 3, 3, 40), (2, 64, 4, 4, 64), (3, 32, 5, 4, 48), (65, 64, 2, 7, 64)]


# ---- policy branches with ragged last tiles -------------------------------------------------------
def _policy_desc(entry, rows, cols, depth, rs):
    """rows x cols x depth as a (1, ., 1, rows) map: 1x1, or 3x3 / pad 1 on a single row of pixels."""
    R = 3 if rs == 9 else 1
    pad = 1 if rs == 9 else 0
    if entry == 'conv2d_fwd':
        return desc(1, depth, 1, rows, cols, R, R, 1, pad)
    return desc(1, cols, 1, rows, depth, R, R, 1, pad)       # data gradient: columns = C, depth = K


def smallest_problem(label, entry, cols, rs, knobs):
    """The problem with the fewest bytes moved that route() sends to ``label``: over the depths
    32 .. 4096 the smallest row count that leaves a partial last tile."""
    kn = dict(DEFAULT_KNOBS)
    kn.update(knobs)
    best = None
    for depth in (32, 64, 128, 256, 512, 1024, 2048, 4096):
        # the policy reads the row count through ceil(rows / 64) and ceil(rows / 128) only, so the
        # smallest ragged row count of every tile row, 64 k + 1, is enough
        for rows in range(1, 70000, 64):
            d = _policy_desc(entry, rows, cols, depth, rs)
            if moved_bytes(entry, d) >= (best[0] if best is not None else 256 << 20):
                break
            if route(entry, d, 0, True, kn).label == label:
                best = (moved_bytes(entry, d), d)
                break
    return None if best is None else best[1]


def _policy_knobs(label):
    kn = {}
    if label.startswith('big') and label != 'big/one_round_ksplit':
        kn['big_min_tiles'] = 1
    if label in ('small/main+split_leftover', 'big/main+split_remainder'):
        kn['fused_tail'] = 0
    return kn


# why a policy case may move more than 16 MiB
POLICY_SIZE_REASON = {
    'big/fused_tail': '256 tiles of 128x128 before the remainder, 8 slices',
    'big/main+plain_remainder': '256 tiles of 128x128 before the remainder',
    'big/main+split_remainder': '256 tiles of 128x128 before the remainder, 16 slices',
    # not a remainder branch, but no 1x1 problem of 132 columns reaches it below 48 MiB: T tiles cut
    # into fit slabs need T fit >= 384 and depth >= 512 fit, the rows are 64 T, so the input alone is
    # 64 T x 512 fit x 4 bytes >= 48 MiB (the 3x3 case of the same branch moves 10 MiB)
    'big/one_round_ksplit': '>= 384 workgroups of >= 16 slices, 1x1',
}
_POLICY_CACHE = []


def policy_cases():
    """[(id, entry, desc, knobs, label)]: per forward / DGRAD label, the smallest ragged problem that
    reaches it with a column count of 4 mod 64 (68 on 64x64 tiles, 132 on 128x128 tiles), 1x1, in the
    forward form (run on both arithmetics) and in the K-strided DGRAD mode; one 3x3 each for
    small/fused_tail and big/one_round_ksplit."""
    if _POLICY_CACHE:
        return _POLICY_CACHE
    for label in FWD_LABELS:
        cols = 132 if label.startswith('big') else 68
        kn = _policy_knobs(label)
        for entry in ('conv2d_fwd', 'conv2d_dgrad_ex'):
            for rs in (1, 9) if label in ('small/fused_tail', 'big/one_round_ksplit') else (1,):
                d = smallest_problem(label, entry, cols, rs, kn)
                if d is None:
                    continue
                rows, depth = d.W, (d.C if entry == 'conv2d_fwd' else d.K)
                forced = ' (size forced by %s: %s)' % (label, POLICY_SIZE_REASON[label]) \
                    if moved_bytes(entry, d) > (16 << 20) else ''
                _POLICY_CACHE.append(('%s %s %s: %d rows x %d cols x %d deep%s' % (
                    label, entry, '3x3' if rs == 9 else '1x1', rows, cols, depth, forced), entry, d, kn, label))
    return _POLICY_CACHE


# ---- every GEMM call of the lists -------------------------------------------------------------------
def uses_transposed_dgrad(d):
    """functions/_conv_launch.py:_uses_transposed_dgrad."""
    if d.stride == 1:
        return d.R == d.S
    return d.R == 1 and d.S == 1 and d.pad == 0


def conv2d_calls(d):
    """The GEMM entry points F.conv2d's forward and backward issue for descriptor ``d``."""
    return ['conv2d_fwd', 'conv2d_dgrad_wt' if uses_transposed_dgrad(d) else 'conv2d_dgrad_ex', 'conv2d_wgrad']


def all_calls():
    """(family, id, entry, desc, has_ws, knobs) of every GEMM call the device test makes, on the default
    arithmetic and on fp32 where the family runs both."""
    both = ({}, {'split_bf16': 0})
    for i, c in PW_GRID + PW_DIAGONAL:
        for e in conv2d_calls(pw_desc(*c)):
            yield 'pointwise', i, e, pw_desc(*c), True, {}
    for i, c in PW_BIG_GRID:
        for kn in both:
            for e in conv2d_calls(pw_desc(*c)):
                yield 'pointwise 128x128', i, e, pw_desc(*c), True, dict(kn, big_min_tiles=1)
    for g in SMALL_MAP_GEOMS:
        for i, d in small_map_cases(g):
            for pm in (1, 0):
                for e in conv2d_calls(d):
                    yield 'small maps', i, e, d, True, {'position_major_rows': pm}
    for i, d in PERM_POSITIONS:
        for e in conv2d_calls(d):
            yield 'small maps', i, e, d, True, {}
    for i, d in STRIDED:
        for e in ('conv2d_fwd', 'conv2d_dgrad_wt', 'conv2d_dgrad_ex'):
            yield 'strided 1x1', i, e, d, True, {}
    for i, d in DGRAD_DIRECT + [DGRAD_TINY_SPLIT]:
        for ws in (True, False):
            yield 'dgrad direct', i, 'conv2d_dgrad_ex', d, ws, {}
        yield 'dgrad direct', i, 'conv2d_dgrad', d, False, {}
    for i, d in DECONV:
        for e in ('deconv2x2s2_fwd', 'deconv2x2s2_fwd_wt', 'deconv2x2s2_dgrad', 'deconv2x2s2_wgrad'):
            yield 'deconv', i, e, d, e == 'deconv2x2s2_wgrad', {}
    for i, (R, Cin, Cout) in LINEAR:
        for e in conv2d_calls(desc(R, Cin, 1, 1, Cout)):
            yield 'linear', i, e, desc(R, Cin, 1, 1, Cout), True, {}
    for i, (N, H, W, K, aff) in STEM:
        yield 'stem', i, 'conv_stem_fwd', stem_desc(N, H, W, K), False, {}
    for i, d in WGRAD_BY_PIXELS:
        for ws in (True, False):
            yield 'wgrad by pixels', i, 'conv2d_wgrad_ex', d, ws, {}
    for i, d, kn, _ in WGRAD_WPERM:
        yield 'wgrad wperm', i, 'conv2d_wgrad_ex', d, True, kn
    for i, e, d, kn, _ in policy_cases():
        for arith in (both if e == 'conv2d_fwd' else ({},)):
            yield 'policy', i, e, d, True, dict(kn, **arith)


# ---- the Winograd route: policy branches, thresholds, epilogue shapes ----------------------------
def wino_desc(N, C, H, W, K):
    return desc(N, C, H, W, K, 3, 3, 1, 1)


def wino_moved_bytes(d):
    """Bytes of x, y / gy and gx of one case (fp32); the filter is small beside them."""
    return 4 * d.N * d.H * d.W * (d.C + d.K)


def _wino_policy_desc(entry, rows, cols, depth):
    """rows maps of 4x4 (one tile each, every row and column of the transforms read)."""
    if entry == 'conv3x3_wino_fwd':
        return wino_desc(rows, depth, 4, 4, cols)              # columns = K, depth = C
    if entry == 'conv3x3_wino_dgrad':
        return wino_desc(rows, cols, 4, 4, depth)              # columns = C, depth = K
    return wino_desc(depth, cols, 4, 4, rows)                  # weight gradient: rows = K, depth = tiles


def wino_smallest_problem(label, entry):
    """The 4x4-map problem with the fewest bytes moved that reaches ``label`` with a partial last tile
    in the rows and a column count of 4 mod 64."""
    best = None
    if entry == 'conv3x3_wino_wgrad':
        rows, cols = (132, 132) if '128' in label else (36, 68)
        for tiles in range(1, 5000):
            if tiles % BK == 0:
                continue
            d = _wino_policy_desc(entry, rows, cols, tiles)
            if wino_plan(entry, d).label == label:
                return d
        return None
    cols = 68 if label == 'wino/small64' else 132
    for depth in (32, 64, 128, 256, 512):
        for rows in range(1, 5000):
            if rows % 64 == 0:
                continue
            d = _wino_policy_desc(entry, rows, cols, depth)
            if best is not None and wino_moved_bytes(d) >= best[0]:
                break
            if wino_plan(entry, d).label == label:
                best = (wino_moved_bytes(d), d)
                break
    return None if best is None else best[1]


# why a Winograd case may move more than 16 MiB: the W8 branch needs 22 tiles of 256x128 per frequency,
# 256 channels deep (w8_min_k), i.e. >= 2816 maps (whole row tiles) or >= 4096 (a ragged last one)
WINO_SIZE_REASON = 'size forced by wino/w8: >= 22 tiles of 256x128 per frequency at >= 256 channels'
_WINO_POLICY_CACHE = []


def wino_policy_cases():
    """[(id, entry, desc, label)]: per WINO_LABELS entry (forward and data gradient each for the four
    GEMM branches, the weight gradient for its four) the smallest ragged 4x4-map problem that reaches it."""
    if _WINO_POLICY_CACHE:
        return _WINO_POLICY_CACHE
    for label in WINO_LABELS:
        for entry in (WINO_ENTRIES[2:] if label.startswith('wino_wgrad') else WINO_ENTRIES[:2]):
            d = wino_smallest_problem(label, entry)
            if d is None:
                continue
            forced = ' (%s)' % WINO_SIZE_REASON if wino_moved_bytes(d) > (16 << 20) else ''
            _WINO_POLICY_CACHE.append(('%s %s: %d maps of 4x4, C%d K%d%s' % (
                label, entry[len('conv3x3_'):], d.N, d.C, d.K, forced), entry, d, label))
    return _WINO_POLICY_CACHE


# Both sides of every comparison of the two plans: ((N, C, H, W, K), forward label, data-gradient label,
# (weight-gradient tile, slabs, slab depth, depth of the last slab)).  Labels without their 'wino/' prefix.
WINO_THRESHOLDS = [
    ((64, 68, 4, 4, 68), 'small64', 'small64', (128, 1, 64, 64)),            # T > 64: below
    ((65, 68, 4, 4, 68), 'big128', 'big128', (128, 1, 96, 65)),              # ... above
    ((65, 64, 4, 4, 68), 'big128', 'small64', (64, 1, 96, 65)),              # columns > 64: 64 / 68, by C
    ((65, 68, 4, 4, 64), 'small64', 'big128', (64, 1, 96, 65)),              # ... by K
    ((192, 68, 4, 4, 132), 'big128', 'big128', (128, 1, 192, 192)),          # rem = 64 but T < 256: one launch
    ((256, 68, 4, 4, 68), 'big128', 'big128', (128, 1, 256, 256)),           # rem = 0
    ((257, 68, 4, 4, 68), 'main128+tail64', 'main128+tail64', (128, 1, 288, 257)),   # rem = 1
    ((320, 68, 4, 4, 68), 'main128+tail64', 'main128+tail64', (128, 1, 320, 320)),   # rem = 64
    ((321, 68, 4, 4, 68), 'big128', 'big128', (128, 1, 352, 321)),           # rem = 65
    ((47, 68, 5, 9, 132), 'main128+tail64', 'main128+tail64', (128, 1, 288, 282)),   # ragged 2x3-tile maps
    ((511, 64, 4, 4, 64), 'small64', 'small64', (64, 1, 512, 511)),          # fewer than 2 x 8 K slices
    ((512, 64, 4, 4, 64), 'small64', 'small64', (64, 2, 256, 256)),          # two whole slabs
    ((513, 64, 4, 4, 64), 'small64', 'small64', (64, 2, 288, 225)),          # a short last slab
    ((700, 132, 4, 4, 132), 'main128+tail64', 'main128+tail64', (128, 2, 352, 348)),
    ((2050, 64, 3, 3, 64), 'small64', 'small64', (64, 8, 288, 34)),          # the cap of 8 slabs, 64x64 tiles
    ((2049, 132, 2, 2, 68), 'main128+tail64', 'main128+tail64', (128, 8, 288, 33)),  # ... 128x128 tiles
    # W8: 3 column tiles with 4 ragged columns, depth 260 = 8 slices + 4
    ((2816, 260, 4, 4, 260), 'w8', 'w8', (128, 7, 416, 320)),
    ((4100, 260, 2, 2, 260), 'w8', 'w8', (128, 7, 608, 452)),                # T >= 4096: a ragged last row tile
    ((4095, 260, 2, 2, 260), 'big128', 'big128', (128, 7, 608, 447)),        # T % 256 != 0 below 4096
    ((2816, 252, 4, 4, 260), 'big128', 'w8', (128, 7, 416, 320)),            # depth 252 < w8_min_k, forward only
    ((2816, 256, 4, 4, 128), 'big128', 'big128', (128, 8, 352, 352)),        # only 11 x 36 tiles
]

# Epilogue shapes: a one-pixel map, maps smaller than a tile in one axis only (2x7, 5x4), 7x7 (2x2 tiles,
# ragged both ways), 5x9; channels of 4 and 36 / 40; 64x64 tiles, 128x128 tiles, and the main128+tail64 pair
WINO_EPILOGUE_SHAPES = [(1, 4, 1, 1, 4), (3, 36, 2, 7, 40), (5, 40, 5, 4, 36), (33, 68, 7, 7, 132),
                        (47, 68, 5, 9, 132)]
# ... and the W8 kernel in front of the output transform: 704 maps of 7x7 = 2816 tiles, forward on W8 (the
# data gradient, 132 deep, on 128x128 tiles); 54 MiB moved, the size the W8 branch forces
WINO_EPILOGUE_W8 = (704, 260, 7, 7, 132)

# Fix-up values (EXACT_SIGNS with every output inside the bound): C in {4, 36, 256, 260}, maps 1x1, 2x7, 7x7
WINO_FIXUP_SHAPES = [(3, 4, 1, 1, 8), (2, 36, 2, 7, 40), (2, 256, 7, 7, 8), (3, 260, 2, 7, 12), (5, 4, 7, 7, 4)]
WINO_FIXUP_OVERFLOW = (2050, 8, 3, 3, 4)          # fix_cap = (8 x 36 x 4 x 8 - 4) / 2 = 4606 of 73 800 outputs


def wino_fix_cap(d):
    """Entries of the fix list behind the forward's buffers: [count (16 B) | (pixel, channel) pairs] in the
    8 x 36 K C floats the weight gradient's slabs use."""
    return min(1 << 20, (8 * WINO_XI * d.K * d.C - 4) // 2)


def wino_fixup_epilogue(d, kind):
    """(flags name, scale, shift) fp32 arrays (or None) of the EXACT_SIGNS cases.  'affine0': mixed-sign
    scale, zero shift, so that every output stays inside a bound of 2 |A^T||M||A| |scale|.  'bias' /
    'affine': a shift of at most 0.03, which is below 0.1 x the rms of the pre-activation on every shape of
    WINO_FIXUP_SHAPES (a 1x1 map sees one tap of nine: rms 1 / 3)."""
    rng = np.random.RandomState(seed_of(*d) + 11)
    sign = np.where(np.arange(d.K) % 2 == 0, 1., -1.)
    scale = (rng.uniform(.5, 1.5, d.K) * sign).astype(np.float32)
    shift = rng.uniform(-.03, .03, d.K).astype(np.float32)
    shift[shift == 0] = .01
    if kind == 'affine0':
        return scale, np.zeros(d.K, np.float32)
    if kind == 'bias':
        return None, shift
    if kind == 'affine':
        return scale, shift
    raise ValueError(kind)


def is_w8_case(d):
    return any(wino_plan(e, d).label == 'wino/w8' for e in WINO_ENTRIES[:2])


def wino_cases():
    """[(family, id, desc)] of every Winograd case of the device test."""
    out = [('policy', i, d) for i, _, d, _ in wino_policy_cases()]
    out += [('threshold', 'winograd threshold %s' % (c,), wino_desc(*c)) for c, _, _, _ in WINO_THRESHOLDS]
    out += [('epilogue', 'winograd epilogue %s' % (c,), wino_desc(*c)) for c in WINO_EPILOGUE_SHAPES + [WINO_EPILOGUE_W8]]
    out += [('tiny maps', 'winograd %s' % (c,), wino_desc(*c)) for c in WINOGRAD]
    return out


def wino_calls():
    """(family, id, entry, desc, knobs) of every Winograd GEMM call of the device test: the W8 cases on the
    default arithmetic, the others on the split and the fp32 one."""
    for fam, i, d in wino_cases():
        for kn in ({},) if is_w8_case(d) else ({}, {'split_bf16': 0}):
            for e in WINO_ENTRIES:
                yield fam, i, e, d, kn


WINO_REJECTED = [
    ('1x1 filter', desc(2, 8, 7, 7, 8, 1, 1, 1, 0), 'Winograd'),
    ('3x3 / stride 2', desc(2, 8, 7, 7, 8, 3, 3, 2, 1), 'Winograd'),
    ('3x3 / pad 0', desc(2, 8, 7, 7, 8, 3, 3, 1, 0), 'Winograd'),
    ('C = 6', wino_desc(2, 6, 7, 7, 8), 'multiples of 4'),
    ('K = 6', wino_desc(2, 8, 7, 7, 6), 'multiples of 4'),
    ('a frequency plane of 2^29 floats: 2^20 maps of 1x1, C = 512', wino_desc(1 << 20, 512, 1, 1, 8), 'frequency plane'),
    ('2^20 maps of 4x4, C = 512: the tensor itself is over 2^31 elements', wino_desc(1 << 20, 512, 4, 4, 8), '2^31'),
]


# ---- rejected by design -------------------------------------------------------------------------
REJECTED = [
    ('C not a multiple of 4', 'conv2d_fwd', desc(1, 6, 3, 3, 8, 1)),
    ('K not a multiple of 4', 'conv2d_fwd', desc(1, 8, 3, 3, 6, 1)),
    ('C not a multiple of 4 (data gradient)', 'conv2d_dgrad_ex', desc(1, 6, 3, 3, 8, 1)),
    ('K not a multiple of 4 (weight gradient)', 'conv2d_wgrad', desc(1, 8, 3, 3, 6, 1)),
    ('3x3 / stride 2 data gradient', 'conv2d_dgrad_ex', desc(1, 8, 5, 5, 8, 3, 3, 2, 1)),
    ('3x3 / stride 2 data gradient, transposed filter', 'conv2d_dgrad_wt', desc(1, 8, 5, 5, 8, 3, 3, 2, 1)),
    ('res_g with stride 2', 'conv2d_dgrad_ex+res_g', desc(1, 8, 4, 4, 8, 1, 1, 2, 0)),
    ('res_g with stride 2, transposed filter', 'conv2d_dgrad_wt+res_g', desc(1, 8, 4, 4, 8, 1, 1, 2, 0)),
]


# ---- the comparison used on the device ------------------------------------------------------------
GUARD = 64                       # floats on each side of a guarded output: 256 bytes
NAN_BITS = 0x7fc0dead             # a quiet NaN with a payload


class Guarded(object):
    """An output of ``n`` floats inside a larger buffer: GUARD floats in front and behind, everything
    prefilled with one NaN bit pattern.  ``out`` is the view a kernel writes; ``check()`` returns what
    is wrong: a guard word that changed, or (``defined``: bool mask or None for all) a prefill NaN
    left where the operation defines a value."""

    def __init__(self, n, device):
        import torch
        self.n = int(n)
        self.buf = torch.full((self.n + 2 * GUARD,), NAN_BITS, dtype=torch.int32, device=device)
        self.out = self.buf[GUARD:GUARD + self.n].view(torch.float32)

    def check(self, defined=None):
        import torch
        bits = self.buf
        front, back = bits[:GUARD], bits[GUARD + self.n:]
        if not (bool((front == NAN_BITS).all()) and bool((back == NAN_BITS).all())):
            bad = torch.nonzero(torch.cat([front, back]) != NAN_BITS).flatten()
            return 'guard band written at guard word %d' % int(bad[0])
        left = bits[GUARD:GUARD + self.n] == NAN_BITS
        if defined is not None:
            left = left & defined.reshape(-1)
        if bool(left.any()):
            return 'element %d never written' % int(torch.nonzero(left).flatten()[0])
        return None


def dgrad_flags_operands(variant, d, rng):
    """(flags, res_g, res_y, out_mask_y, out_scale, prev) NCHW fp32 arrays (or None) of a DGRAD_VARIANTS
    name; ``prev``: the seeded finite prefill of gx under ACCUM."""
    shape = (d.N, d.C, d.H, d.W)
    want = lambda *names: variant == 'all' or variant in names      # noqa: E731
    res_g = rng.standard_normal(shape).astype(np.float32) if want('res_g', 'res_g+res_y') else None
    res_y = rng.standard_normal(shape).astype(np.float32) if want('res_g+res_y') else None
    mask = rng.standard_normal(shape).astype(np.float32) if want('out_mask_y') else None
    scale = rng.uniform(0.5, 1.5, d.C).astype(np.float32) if want('out_scale') else None
    prev = rng.standard_normal(shape).astype(np.float32) if want('accum') else None
    return (EPI_ACCUM if prev is not None else 0), res_g, res_y, mask, scale, prev
