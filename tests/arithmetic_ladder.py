"""The reduced arithmetics of the convolution GEMMs ('split_bf16x2', 'bf16x1': functions.conv.
set_gemm_arithmetic, the "split_planes" knob, NP in csrc/conv_gemm_kernel.h): what
tests/test_arithmetic_ladder_cpu.py and tests/test_gpu_arithmetic_ladder.py share — the rounding
maps, the error bounds, the cases (taken from tests/gemm_edge_cases.py) with their seeded operands,
the float64 references, and a float64 model of the three product sets.  Importable without a device.

The planes.  u = 2^-8 is bf16's unit roundoff.  split3 (test_split_arithmetic_cpu.split3, the
kernel's) gives a = hi + mid + lo with hi = bf16(a), mid = bf16(a - hi), and, writing lo := a - hi - mid
for the exact remainder (the kernel's third plane is bf16 of it),
    |a - hi| = |mid + lo| <= u |a|,   |lo| <= u^2 |a|,
hence |hi| <= (1 + u) |a| and |mid| <= |mid + lo| + |lo| <= (u + u^2) |a|.
r1(a) = hi, r2(a) = hi + mid (exact in fp32: 8 + 8 bits at most 9 binary places apart).

BOUNDS, per product a b (then summed over the reduction: S = sum |a||b|, float64).
One plane keeps hi hi:   a b - ah bh = (a - ah) b + ah (b - bh), so
    |a b - ah bh| <= u |a||b| + (1 + u) u |a||b| = (2u + u^2) |a||b|.                    C1
Two planes keep hi hi + hi mid + mid hi and drop SIX products:
    |am bm| <= (u + u^2)^2          |ah bl|, |al bh| <= (1 + u) u^2   each
    |am bl|, |al bm| <= (u + u^2) u^2  each          |al bl| <= u^4          (times |a||b|)
    sum = (u^2 + 2u^3 + u^4) + (2u^2 + 2u^3) + (2u^3 + 2u^4) + u^4 = 3u^2 + 6u^3 + 4u^4.  C2
The kernels add fp32 accumulation on top; for that the tests grant T3 = 1e-5 max|ref|, what
tests/test_gpu_split_bf16.py (test_error_against_float64_is_at_the_fp32_kernels_level) grants the
three-plane kernel, which accumulates the same way.

TIES (statement 2 of the tests).  "'split_bf16x2' on (x, w) equals 'split_bf16x3' on (r2(x), w) for a
bf16-exact w" needs the kernel to split r2(x) back into (hi, mid, 0).  It does unless mid is exactly
half an ulp of hi — bf16(hi + mid) is then a tie, and round-to-even moves hi by one ulp for every
second such element: (hi + ulp, -mid, 0) is the same number, but its products are accumulated from
other parts, so the fp32 roundings differ.  About one element in 2^10 is affected.  ``tie_free``
replaces those elements by their hi (a bf16 value: mid = 0), which makes the premise true and leaves
every other element as seeded.
"""
import collections
import math

import numpy as np
import torch
import torch.nn.functional as TF

import gemm_edge_cases as G
from test_split_arithmetic_cpu import bf16_round, split3

U = 2.0 ** -8
C1 = 2 * U + U ** 2
C2 = 3 * U ** 2 + 6 * U ** 3 + 4 * U ** 4
T3 = 1e-5                                   # of max|ref|
NAMES = ('fp32', 'split_bf16x3', 'split_bf16x2', 'bf16x1')
BOUND = {'bf16x1': C1, 'split_bf16x2': C2}
PLANES = {'split_bf16x3': 3, 'split_bf16x2': 2, 'bf16x1': 1}


def r1(a):
    """Round-to-nearest-even bf16 of fp32 ``a``, as fp32 (torch's conversion: test_split_arithmetic_cpu.bf16_round,
    which the CPU test holds it to, is the bit-level statement but slow on the 50 M elements of the W8 case)."""
    a = np.ascontiguousarray(a, np.float32)
    return torch.from_numpy(a).to(torch.bfloat16).to(torch.float32).numpy()


def hi_mid(a):
    a = np.asarray(a, np.float32)
    hi = r1(a)
    return hi, r1(a - hi)


def r2(a):
    hi, mid = hi_mid(a)
    return hi + mid


def tie_free(a):
    """``a`` with the elements whose r2 does not split back into (hi, mid, 0) replaced by their hi."""
    a = np.asarray(a, np.float32)
    hi, mid = hi_mid(a)
    return np.where(r1(hi + mid) == hi, a, hi)


# ---- cases ------------------------------------------------------------------------------------------
# kind: 'conv' F.conv2d (+ bias) forward and, with ``backward``, both gradients; 'deconv' F.deconv2x2s2
# (+ bias) forward and gradients; 'stem' F.stem_conv (+ bias) forward.  knobs: mrcnn_set_tuning.
Case = collections.namedtuple('Case', 'id kind d knobs backward')

BIG = {'big_min_tiles': 1}
# the RoI head's 1x1 1024 -> 512 on 1024 RoIs of 7x7: the W8 launch of tests/test_gpu_conv.py's bit-identity test
W8_DESC = G.desc(1024, 1024, 7, 7, 512)
# the 128x128 weight gradient with a K-split workspace (G.WGRAD_WPERM, "by the fill rule")
WGRAD128_WS = [c for c in G.WGRAD_WPERM if c[3] == 'wgrad128/split+reduce' and not c[2]][0]
_CASES = []


def cases():
    if _CASES:
        return _CASES
    add = lambda *a: _CASES.append(Case(*a))         # noqa: E731
    # the three geometry instantiations on 64x64 tiles and on forced 128x128 tiles, ragged in rows, columns, depth
    add('64x64 PW', 'conv', G.pw_desc(65, 68, 36), {}, True)
    add('64x64 K3', 'conv', G.desc(3, 36, 7, 7, 40, 3, 3, 1, 1), {}, True)
    add('64x64 general (3x3 pad 0)', 'conv', G.desc(3, 36, 4, 5, 40, 3, 3, 1, 0), {}, True)
    add('64x64 general, position-major rows', 'conv', G.desc(65, 36, 3, 3, 40, 3, 3, 1, 1), {}, True)
    add('128x128 PW', 'conv', G.pw_desc(129, 132, 100), BIG, True)
    add('128x128 K3', 'conv', G.desc(2, 36, 9, 11, 132, 3, 3, 1, 1), BIG, True)
    add('128x128 general (3x3 pad 0)', 'conv', G.desc(3, 36, 10, 12, 132, 3, 3, 1, 0), BIG, True)
    # strided 1x1 (forward general, data gradient scattered), stem, forward-form deconvolution
    add('strided 1x1', 'conv', G.desc(2, 64, 5, 4, 132, 1, 1, 2, 0), {}, True)
    add('stem', 'stem', G.stem_desc(1, 14, 13, 64), {}, False)
    add('deconvolution, forward form', 'deconv', G.desc(1, 36, 5, 13, 20, 2, 2, 2, 0), {}, True)
    # every forward branch of the launch policy, at its smallest ragged problem (forward only)
    for cid, entry, d, kn, label in G.policy_cases():
        if entry == 'conv2d_fwd':
            add('policy ' + cid, 'conv', d, kn, False)
    add('W8', 'conv', W8_DESC, {}, False)
    add('128x128 weight gradient, K-split workspace', 'conv', WGRAD128_WS[1], {}, True)
    return _CASES


def operands(case):
    """x, w, gy (None without a backward), b: seeded fp32 arrays, NCHW / KCRS (deconv: w (C, K, 2, 2))."""
    d = case.d
    rng = np.random.RandomState(G.seed_of(*d) + 7)
    b = rng.standard_normal(d.K).astype(np.float32)
    if case.kind == 'conv':
        x, w, gy = G.operands(d)
    elif case.kind == 'stem':
        x = rng.uniform(-120, 130, (d.N, 3, d.H, d.W)).astype(np.float32)
        w = (rng.standard_normal((d.K, 3, 7, 7)) / 12.).astype(np.float32)
        gy = None
    else:
        x = rng.standard_normal((d.N, d.C, d.H, d.W)).astype(np.float32)
        w = (rng.standard_normal((d.C, d.K, 2, 2)) / math.sqrt(d.C)).astype(np.float32)
        gy = rng.standard_normal((d.N, d.K, 2 * d.H, 2 * d.W)).astype(np.float32)
    return x, w, (gy if case.backward else None), b


def split_outputs(case):
    """Which of y / gx / gw come from a split-operand launch (the others run fp32 MFMA under every arithmetic)."""
    d = case.d
    if case.kind == 'stem':
        entries = {'y': 'conv_stem_fwd'}
    elif case.kind == 'deconv':
        entries = {'y': 'deconv2x2s2_fwd_wt', 'gx': 'deconv2x2s2_dgrad', 'gw': 'deconv2x2s2_wgrad'}
    else:
        fwd, dgrad, wgrad = G.conv2d_calls(d)
        entries = {'y': fwd, 'gx': dgrad, 'gw': wgrad}
    if not case.backward:
        entries = {'y': entries['y']}
    out = {}
    for name, entry in entries.items():
        launches = G.route(entry, d, 0, True, case.knobs).launches
        out[name] = all('split' in tags for _, tags in launches)
    return out


# ---- float64 -----------------------------------------------------------------------------------------

def bilinear(case, x, w, gy):
    """{'y', 'gx', 'gw'} of the case's operation WITHOUT its bias, in float64 (torch, CPU): every one is
    bilinear in its two operands (x, w), (gy, w), (x, gy)."""
    d = case.d
    t = lambda a, g: torch.tensor(np.asarray(a, np.float64), requires_grad=g)     # noqa: E731
    xt, wt = t(x, case.backward), t(w, case.backward)
    with torch.enable_grad():
        if case.kind == 'deconv':
            y = TF.conv_transpose2d(xt, wt, stride=2)
        elif case.kind == 'stem':
            y = TF.conv2d(xt, wt, stride=2, padding=3)
        else:
            y = TF.conv2d(xt, wt, stride=d.stride, padding=d.pad)
        out = {'y': y.detach().numpy()}
        if case.backward:
            y.backward(torch.tensor(np.asarray(gy, np.float64)))
            out['gx'], out['gw'] = xt.grad.numpy(), wt.grad.numpy()
    return out


def reference(case, x, w, gy):
    """(ref, S): the float64 results and, per element, the sum over the reduction of |a||b|."""
    ab = lambda a: None if a is None else np.abs(np.asarray(a, np.float64))      # noqa: E731
    return bilinear(case, x, w, gy), bilinear(case, ab(x), ab(w), ab(gy))


def model(case, planes, x, w, gy):
    """The product set of ``planes`` planes evaluated in float64 (no accumulation rounding): one plane
    hi hi; two planes (hi + mid)(hi + mid) - mid mid; three planes all nine minus mid lo, lo mid, lo lo."""
    parts = [None if a is None else [p.astype(np.float64) for p in split3(a)] for a in (x, w, gy)]
    pick = lambda f: [None if p is None else f(p) for p in parts]                 # noqa: E731
    if planes == 1:
        return bilinear(case, *pick(lambda p: p[0]))
    full = bilinear(case, *pick(lambda p: p[0] + p[1] + (p[2] if planes == 3 else 0)))
    drop = bilinear(case, *pick(lambda p: p[1]))                 # mid mid
    if planes == 2:
        return {k: full[k] - drop[k] for k in full}
    ml = bilinear(case, *pick(lambda p: p[1] + p[2]))            # (mid + lo)(mid + lo) = mid mid + the three dropped
    return {k: full[k] - (ml[k] - drop[k]) for k in full}
