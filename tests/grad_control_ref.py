"""float64 reference of the step's control word (include/mrcnn_hip.h: mrcnn_grad_sumsq,
mrcnn_grad_control): the exact sum of squares of an fp32 gradient and, from it, the norm of the
averaged gradient, chainer's clipping factor, the skip flag and the reported norm."""
import math

import numpy as np

CTL_NORM, CTL_FACTOR, CTL_SKIPPED, CTL_NORM_REPORTED = 0, 1, 2, 3


def exact_sumsq(g):
    """sum g[i]^2 of fp32 values, correctly rounded: the product of two fp32 values is exact in
    float64 and math.fsum adds without intermediate rounding.  inf for an infinity, NaN for a NaN."""
    g = np.asarray(g, dtype=np.float32).astype(np.float64).ravel()
    if np.isnan(g).any():
        return float('nan')
    if np.isinf(g).any():
        return float('inf')
    return math.fsum((g * g).tolist())


def control_word(sumsq, grad_scale, clip, skip_nonfinite):
    """dict(norm: float64, clipping: bool, factor: float64 (grad_scale itself when not clipping),
    skipped: 0. / 1., norm_reported: float64) for the float64 ``sumsq``; ``grad_scale`` and
    ``clip`` are taken as the float32 values the entry point receives."""
    gs = float(np.float32(grad_scale))
    clip = float(np.float32(clip))
    finite = math.isfinite(sumsq)
    norm = (math.sqrt(sumsq) if not math.isnan(sumsq) else float('nan')) * gs
    clipping = clip > 0 and norm > clip          # False for a NaN norm
    factor = gs * clip / norm if clipping else gs
    return dict(norm=norm, clipping=clipping, factor=factor,
                skipped=1. if (skip_nonfinite and not finite) else 0.,
                norm_reported=norm if finite else 0.)


def ulp32(x):
    """Spacing of float32 at ``x``."""
    return float(np.spacing(np.abs(np.float32(x))))
