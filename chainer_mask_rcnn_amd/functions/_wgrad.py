"""Who owns a parameter's gradient, and when the launch that writes it is issued.

A gradient is written in place into the parameter's arena slot (optimizers.ParamArena) when the
slot can be claimed, else into a fresh tensor that autograd accumulates.  The launch of a weight
gradient runs at once on the compute stream, at once on the weight-gradient side stream, or is
held back in a ``DeferQueue`` for the next step's proposal window.  The launches themselves are
functions/_conv_launch.py.
"""
import torch

from .. import _lib
from ..streams import join_wgrad_stream
from ._layout import empty_nhwc
from ._conv_launch import _colsum, _launch_wgrad, wino_wgrad_into


def _direct_grad(p):
    """Claim the right to WRITE ``p``'s gradient in place: true for an arena-backed parameter
    (optimizers.ParamArena) whose arena view is intact and that has not received a gradient yet
    in this step.  Otherwise the caller returns a fresh tensor and autograd accumulates it."""
    arena = getattr(p, '_arena', None)
    if arena is None:
        return False
    if arena.claim(p):
        return True
    join_wgrad_stream(p.device)      # an earlier in-place write may still be queued there
    return False


def _grad_target(p):
    """The gradient-ownership rule in one place: ``(buffer, result)`` for parameter ``p`` — the
    buffer the producing kernel writes (not adds) p's gradient into and what the autograd node
    returns for p: ``(p.grad, None)`` when the arena slot could be claimed, else the same fresh
    tensor twice (autograd accumulates it)."""
    if _direct_grad(p):
        return p.grad, None
    g = empty_nhwc(tuple(p.shape), p.device) if p.dim() == 4 else \
        torch.empty(tuple(p.shape), dtype=torch.float32, device=p.device)
    return g, g


def _bias_grad(b, g, M):
    """Bias gradient = column sum of the (M, len(b)) gradient ``g``; returns what autograd gets."""
    gb, result = _grad_target(b)
    _colsum(_lib.ptr(g), M, b.shape[0], gb, g.device)
    return result


# ---- weight gradients deferred into the next step's proposal window --------------------------
# Between the RPN convolution and the RoI head of a train step the GPU is nearly idle: the
# proposal kernels (top-k, NMS scan: two workgroups) run, then the host samples the RoIs
# (~2 ms together).  The RoI head's weights are not read before that window has passed, so the
# weight gradients of some head layers — and the SGD update of exactly those parameters — can be
# held back at the end of a step and run INSIDE the next step's window on a second stream, where
# they cost nothing (optimizers.MomentumSGD.defer_weight_gradients; same gradients, same update,
# applied before the parameter is read again: results are bit-identical).
class WgradJob(object):
    """One weight gradient: ``gW`` = backward-filter of descriptor ``d`` from the input ``x`` and
    the output gradient ``g`` (rows scaled by ``row_scale`` if given).  ``wino``: on the Winograd
    route, from the raw input ``x`` or the forward's kept transform ``v`` (the other is None)."""

    def __init__(self, d, x, g, gW, row_scale=None, wino=False, v=None):
        self.d, self.x, self.g, self.gW = d, x, g, gW
        self.row_scale, self.wino, self.v = row_scale, wino, v

    def launch(self):
        """On the current stream (``_lib.workspace`` keys the scratch on it: two streams never
        share a buffer)."""
        if self.wino:
            wino_wgrad_into(self.d, self.x, self.v, self.g, self.gW, self.row_scale)
        else:
            _launch_wgrad(self.d, self.x, self.g, self.gW, self.row_scale)

    def tensors(self):
        """The operands a held-back job keeps alive."""
        return [t for t in (self.x, self.g, self.gW, self.row_scale, self.v) if t is not None]


class DeferQueue(object):
    """``jobs``: one ``WgradJob`` per held-back weight gradient of the parameters ``params``.
    MomentumSGD.update hangs one on the parameter arena (``ParamArena.defer``) around backward."""

    def __init__(self, params):
        self.ids = set(id(p) for p in params)
        self.jobs = []

    def grad_ptrs(self):
        """Addresses of the gradient buffers the held-back jobs will write."""
        return set(j.gW.data_ptr() for j in self.jobs)


def run_deferred_wgrads(jobs):
    """Launch the held-back weight gradients on the current stream (the caller selects it)."""
    for job in jobs:
        job.launch()


def _wgrad(d, x, g, W, side=None, row_scale=None, wino=False, v=None):
    """Weight gradient of parameter ``W``; returns the tensor autograd should see for W (None when
    written in place or held back in the defer queue).  ``wino`` / ``v``: see ``WgradJob``.  With
    ``side`` (a stream) the launch is queued there, ordered after everything queued so far on the
    current stream; only arena-backed (direct) gradients may use it."""
    gW, result = _grad_target(W)
    job = WgradJob(d, x, g, gW, row_scale, wino, v)
    direct = result is None
    # (direct: the arena slot was claimed, so the arena exists and answers the rest of the question)
    defer = W._arena.defer if direct else None
    if defer is not None and id(W) in defer.ids:
        defer.jobs.append(job)
    elif direct and side is not None:
        # The weight-gradient side stream (streams.wgrad_stream): dgrad and wgrad of a convolution
        # are independent given the incoming gradient, so the wgrad launches of a bottleneck go to
        # a second HIP stream, where their workgroups fill the CUs that the tail round of the
        # concurrently running dgrad leaves idle (and vice versa): with 128x128 tiles and 512
        # resident workgroups a single kernel wastes up to a round at its end.
        side.wait_stream(torch.cuda.current_stream(g.device))
        for t in (x, g):
            t.record_stream(side)
        with torch.cuda.stream(side):
            job.launch()
    else:
        job.launch()
    return result
