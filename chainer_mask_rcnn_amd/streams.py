"""The HIP streams of a train step, one set per device for the whole process.

The step uses exactly FOUR streams, because a GPU has four hardware queues by default
(GPU_MAX_HW_QUEUES = 4):

  compute        torch's current stream: everything not named below;
  copy           ``copy_stream``: host-to-device uploads (the step's targets, the input pipeline's
                 next batch and its prepare kernels);
  weight grads   ``wgrad_stream``: weight gradients of the backbone's small-M layers, beside the
                 next data gradient (functions/conv.py: SMALL_WGRAD_MAX_PIXELS);
  deferred work  ``defer_stream``: the weight gradients and SGD slices the optimizer held back into
                 the next step's proposal window (optimizers.MomentumSGD.launch_pending) — and,
                 between two windows, the frozen-prefix prefetch of the NEXT batch
                 (models/resnet_extractor.py: prefetch_frozen), which borrows this stream instead
                 of opening one of its own.

Do not add a fifth: it shares a hardware queue with one of the four and serialises work that was
meant to overlap.  Which streams end up on one queue depends on the order they were created in,
and the proposal chain then queues behind the deferred weight gradients — measured +2.4 ms per
step under data parallelism, +6 ms with 5..8 queues (profiles/HISTORY.md 7a).  Input pipelines
upload on ``copy_stream`` rather than create their own.

For the same reason every stream is created LAZILY, at its first use, never together with the
others: creating them earlier or in another order changes the queue assignment.
"""
import torch


_streams = {}         # (str(device), 'copy' | 'wgrad' | 'defer') -> torch.cuda.Stream


def _get(device, kind):
    key = (str(device), kind)
    if key not in _streams:
        _streams[key] = torch.cuda.Stream(device=device)
    return _streams[key]


def copy_stream(device):
    """The host-to-device copy stream of ``device``."""
    return _get(device, 'copy')


def wgrad_stream(device):
    """The weight-gradient side stream of ``device``."""
    return _get(device, 'wgrad')


def defer_stream(device):
    """The deferred-work stream of ``device``."""
    return _get(device, 'defer')


def wgrad_stream_if_used(device):
    """The weight-gradient side stream of ``device`` if one has been created, else None."""
    return _streams.get((str(device), 'wgrad'))


def join_wgrad_stream(device=None):
    """Make the current stream wait for every weight gradient queued on the side stream
    (call before reading gradients: optimizer step, all-reduce)."""
    for (dev, kind), st in _streams.items():
        if kind == 'wgrad' and (device is None or dev == str(device)):
            torch.cuda.current_stream(st.device).wait_stream(st)
