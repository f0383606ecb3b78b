"""Data-parallel gradient exchange over RCCL / xGMI (one process per GPU).

Replaces ChainerMN's 'hierarchical' communicator + multi-node optimizer
(/root/reference/examples/train_common.py:97-103,178): gradients are
averaged across ranks before the optimizer step and rank-0 parameters are broadcast once.

MI355X-first design
* The gradient arena of ``optimizers.ParamArena`` is laid out in the order backward produces
  gradients (mask head, FCs, res5.b2, res5.b1, res5.a, RPN, res4 ..., res3 ...), so every
  bucket is ONE contiguous slice.  Buckets are cut at layer-block boundaries, ~16 MB each
  (xGMI is point-to-point, 7 links per GPU: tens-of-MB messages keep each ring segment
  bandwidth-bound instead of latency-bound).
* A bucket's all-reduce is queued as soon as every gradient in it has been queued by
  backward — polled from hooks inside the fused stage nodes (after every bottleneck), at the
  RoI head's entry and at the stage boundaries — on the library's own high-priority HIP stream
  (``mrcnn_allreduce_bucket``, include/mrcnn_hip.h), ordered by events after the compute stream
  and the weight-gradient side stream.  The first collective therefore starts under res5's
  backward; the compute stream waits only right before the SGD launch, which also applies the
  1/world scale.
* ``torch.distributed`` is the control plane only (rendezvous, the 128-byte RCCL unique id,
  max-over-ranks of the timings): the data path is RCCL behind the C ABI.  ``TorchDistExchange``
  (gloo on CPU, used by the multi-process CPU tests) implements the same interface.
"""
import ctypes
import os
import sys

import torch
import torch.distributed as dist


# ---------------------------------------------------------------------------------------------
# Exchanges: who moves the bytes
# ---------------------------------------------------------------------------------------------
class TorchDistExchange(object):
    """All-reduce / broadcast through a torch.distributed process group (gloo on CPU)."""

    name = 'torch.distributed'

    def __init__(self, group=None):
        if not dist.is_initialized():
            raise RuntimeError('torch.distributed is not initialised')
        self.group = group
        self.world_size = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        self._works = []
        self.name = 'torch.distributed/%s' % dist.get_backend(group)

    def broadcast(self, tensor, src=0):
        dist.broadcast(tensor, src=src, group=self.group)

    def allreduce_async(self, tensor, bucket_id=0):
        if tensor.is_cuda:
            # weight gradients queued on the side stream must be ordered before the collective
            from .streams import join_wgrad_stream
            join_wgrad_stream(tensor.device)
        self._works.append(dist.all_reduce(tensor, op=dist.ReduceOp.SUM, group=self.group,
                                           async_op=True))

    def wait_all(self):
        for w in self._works:
            w.wait()
        self._works = []

    def barrier(self):
        dist.barrier(group=self.group)

    def timing(self, enable):
        pass

    def bucket_times(self, n_buckets):
        return None

    def describe(self):
        d = dict(library=self.name, ranks=self.world_size)
        if getattr(self, 'fallback', None):
            d['fallback'] = self.fallback
        return d


class RcclExchange(object):
    """RCCL communicator behind the C ABI (``mrcnn_allreduce_*``).  The unique id travels
    through the c10d store of the already initialised process group (any backend)."""

    name = 'rccl-c-abi'
    _counter = 0

    def __init__(self, device=None):
        from . import _lib
        self._lib = _lib
        lib = _lib.load()
        if not dist.is_initialized():
            raise RuntimeError('torch.distributed (control plane) is not initialised')
        self.rank, self.world_size = dist.get_rank(), dist.get_world_size()
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else device
        key = 'mrcnn_rccl_unique_id_%d' % RcclExchange._counter
        RcclExchange._counter += 1
        store = dist.distributed_c10d._get_default_store()
        buf = ctypes.create_string_buffer(128)
        if self.rank == 0:
            _lib.check(lib.mrcnn_allreduce_unique_id(buf), 'mrcnn_allreduce_unique_id')
            store.set(key, buf.raw)
        else:
            buf.raw = bytes(store.get(key))[:128]
        handle = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(lib.mrcnn_allreduce_init(buf, self.rank, self.world_size,
                                                ctypes.byref(handle)), 'mrcnn_allreduce_init')
        self.handle = handle
        r, w, v = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        where = ctypes.create_string_buffer(256)
        _lib.check(lib.mrcnn_allreduce_info(handle, ctypes.byref(r), ctypes.byref(w),
                                            ctypes.byref(v), where, 256), 'mrcnn_allreduce_info')
        self.rccl_version, self.library = v.value, where.value.decode()
        assert (r.value, w.value) == (self.rank, self.world_size)

    def _compute_stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _side_stream(self):
        from .streams import wgrad_stream_if_used
        st = wgrad_stream_if_used(self.device)
        return ctypes.c_void_p(st.cuda_stream) if st is not None else None

    def broadcast(self, tensor, src=0):
        assert tensor.is_cuda and tensor.is_contiguous()
        self._lib.call('mrcnn_allreduce_broadcast', self.handle, self._lib.ptr(tensor),
                       tensor.numel() * tensor.element_size(), int(src), self._compute_stream())

    def allreduce_async(self, tensor, bucket_id=0):
        assert tensor.is_cuda and tensor.dtype == torch.float32 and tensor.is_contiguous()
        self._lib.call('mrcnn_allreduce_bucket', self.handle, self._lib.ptr(tensor),
                       tensor.numel(), int(bucket_id), self._compute_stream(), self._side_stream())

    def wait_all(self):
        self._lib.call('mrcnn_allreduce_wait', self.handle, self._compute_stream())

    def barrier(self):
        """All ranks have reached this point AND their queued device work is done."""
        t = torch.zeros(4, dtype=torch.float32, device=self.device)
        self.allreduce_async(t, -2)
        self.wait_all()
        torch.cuda.synchronize(self.device)

    def timing(self, enable):
        self._lib.call('mrcnn_allreduce_timing', self.handle, 1 if enable else 0)

    def bucket_times(self, n_buckets):
        """[(total_ms, total_bytes, launches)] per bucket id (device must be synchronised)."""
        out = []
        for b in range(n_buckets):
            ms, by, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
            self._lib.call('mrcnn_allreduce_bucket_times', self.handle, b, ctypes.byref(ms),
                           ctypes.byref(by), ctypes.byref(n))
            out.append((ms.value, by.value, n.value))
        return out

    def describe(self):
        return dict(library='RCCL via libmrcnn_hip.so mrcnn_allreduce_* (%s)' % self.library,
                    rccl_version=self.rccl_version, ranks=self.world_size)

    def close(self):
        if self.handle is not None:
            self._lib.load().mrcnn_allreduce_destroy(self.handle)
            self.handle = None


def default_exchange(group=None):
    """RCCL behind the C ABI on a ROCm device, torch.distributed (gloo) on CPU.

    If creating the C-ABI communicator fails on ANY rank, every rank learns it through the control
    plane (so no rank is left waiting in a collective) and every rank RAISES: the gradient exchange
    of this build is `mrcnn_allreduce_*` and nothing else.  Setting
    ``MRCNN_ALLOW_TORCH_RCCL_FALLBACK=1`` opts into torch.distributed's own RCCL binding instead
    (still RCCL over xGMI; reported on stderr and in ``describe()['fallback']``) — a debugging aid,
    never selected silently."""
    if not (torch.cuda.is_available() and group is None):
        return TorchDistExchange(group)
    import os
    import sys
    if rehearsal():
        ex = TorchDistExchange(group)
        ex.fallback = 'MRCNN_DP_REHEARSAL=1: gloo on device tensors, ranks sharing one GPU (launch-path rehearsal)'
        return ex
    ex, err = None, ''
    try:
        ex = RcclExchange()
    except Exception as e:                      # noqa: BLE001 — reported below, never silent
        err = '%s: %s' % (type(e).__name__, e)
    ok = torch.tensor([1 if ex is not None else 0], dtype=torch.int32)
    if dist.get_world_size() > 1:
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)           # CPU tensor: gloo
    if int(ok.item()) == 1:
        return ex
    if ex is not None:
        ex.close()
    why = err or 'the C-ABI communicator failed on a peer rank'
    if os.environ.get('MRCNN_ALLOW_TORCH_RCCL_FALLBACK') != '1':
        from . import _lib
        raise _lib.MrcnnHipError(
            'mrcnn_allreduce_init failed on at least one rank (%s).  The data-parallel gradient '
            'exchange runs through libmrcnn_hip.so only; set MRCNN_ALLOW_TORCH_RCCL_FALLBACK=1 to '
            "use torch.distributed's RCCL binding instead." % why)
    sys.stderr.write('[chainer_mask_rcnn_amd.parallel] mrcnn_allreduce_init failed on at least one '
                     'rank (%s); MRCNN_ALLOW_TORCH_RCCL_FALLBACK=1: using torch.distributed nccl '
                     '(RCCL)\n' % why)
    fb = TorchDistExchange(None)
    fb.fallback = why
    return fb


# ---------------------------------------------------------------------------------------------
# Buckets: what is exchanged when
# ---------------------------------------------------------------------------------------------
class GradBuckets(object):
    """Contiguous slices of a flat gradient buffer, all-reduced independently and in order."""

    def __init__(self, flat, bounds, group=None, exchange=None):
        self.flat = flat
        self.bounds = list(bounds)          # [(start, end), ...] in backward order
        self.exchange = exchange if exchange is not None else TorchDistExchange(group)
        self.launched = [False] * len(self.bounds)
        self.next = 0                       # first bucket not yet launched by poll()

    def launch(self, i):
        if self.launched[i]:
            return
        self.launched[i] = True
        s, e = self.bounds[i]
        if e > s:
            self.exchange.allreduce_async(self.flat[s:e], i)

    def poll(self, ready):
        """Launch, in order, every leading bucket for which ``ready(i)`` holds."""
        while self.next < len(self.bounds) and (self.launched[self.next] or ready(self.next)):
            self.launch(self.next)
            self.next += 1

    def wait_all(self):
        for i in range(len(self.bounds)):
            self.launch(i)                  # anything not yet issued
        self.exchange.wait_all()
        self.launched = [False] * len(self.bounds)
        self.next = 0


def plan_buckets(arena, units, bucket_bytes):
    """Cut the arena into buckets at unit boundaries.  ``units``: per arena parameter an
    opaque unit key (consecutive parameters with the same key are never separated).  Returns
    [(first_param, last_param)] with every bucket except possibly the last >= bucket_bytes."""
    n = len(arena.params)
    groups, start = [], 0
    for i in range(1, n + 1):
        if i == n or units[i] != units[i - 1]:
            groups.append((start, i - 1))
            start = i
    buckets, first = [], None
    for g_first, g_last in groups:
        if first is None:
            first = g_first
        lo, hi = arena.slice_bounds(first, g_last)
        if (hi - lo) * 4 >= bucket_bytes:
            buckets.append((first, g_last))
            first = None
    if first is not None:
        if buckets and (arena.slice_bounds(first, n - 1)[1] - arena.slice_bounds(first, n - 1)[0]) * 4 \
                < bucket_bytes // 4:
            buckets[-1] = (buckets[-1][0], n - 1)      # tiny tail: fold into the previous bucket
        else:
            buckets.append((first, n - 1))
    return buckets


class _ArenaRange(object):
    """View of the parameters [first, last] of an arena with plan_buckets' interface."""

    def __init__(self, arena, first, last):
        self.arena, self.first = arena, first
        self.params = arena.params[first:last + 1]

    def slice_bounds(self, a, b):
        return self.arena.slice_bounds(self.first + a, self.first + b)


class DataParallelGradSync(object):
    """Hooks a MomentumSGD to an exchange: rank-0 broadcast at attach, bucketed all-reduce
    of the gradient arena overlapped with backward, 1/world scale handed to the SGD launch."""

    def __init__(self, optimizer, group=None, exchange=None, bucket_bytes=16 << 20):
        self.exchange = exchange if exchange is not None else default_exchange(group)
        self.world_size = self.exchange.world_size
        self.optimizer = optimizer
        self.bucket_bytes = int(bucket_bytes)
        self.buckets = None
        self.bucket_params = []
        optimizer.grad_sync = self

    # -- setup -----------------------------------------------------------------
    def attach(self, optimizer):
        arena = optimizer.arena
        target = optimizer.target
        # bcast_data: EVERY parameter and buffer of the model from rank 0 (the arena holds the
        # trainable ones; the frozen stem / res2 / AffineChannel2D parameters live outside it)
        self.exchange.broadcast(arena.values, src=0)
        in_arena = set(id(p) for p in arena.params)
        with torch.no_grad():
            for t in list(target.parameters()) + list(target.buffers()):
                if id(t) in in_arena:
                    continue
                if t.is_contiguous():
                    self.exchange.broadcast(t.data, src=0)
                else:                                   # channels-last filter views
                    flat = t.data.clone(memory_format=torch.contiguous_format)
                    self.exchange.broadcast(flat, src=0)
                    t.data.copy_(flat)
        from .functions import conv
        conv.weights_changed()      # the broadcast wrote parameters behind torch's version counters
        # units: a bottleneck block, or a leaf layer, by MODULE IDENTITY (no name matching)
        owner = {}
        from .models.resnet_extractor import Bottleneck
        for m in target.modules():
            if isinstance(m, Bottleneck):
                for p in m.parameters():
                    owner[id(p)] = id(m)
        for m in target.modules():
            for p in m.parameters(recurse=False):
                owner.setdefault(id(p), id(m))
        units = [owner.get(id(p), id(p)) for p in arena.params]
        # parameters whose weight gradients the optimizer holds back into the next step's
        # proposal window (optimizers.defer_weight_gradients) are reduced there, on their own:
        # the in-backward buckets are planned over the remaining runs of the arena
        held = set(id(p) for p in getattr(optimizer, 'deferred_params', []))
        self.bucket_params = []
        i, n = 0, len(arena.params)
        while i < n:
            if id(arena.params[i]) in held:
                i += 1
                continue
            j = i
            while j + 1 < n and id(arena.params[j + 1]) not in held:
                j += 1
            sub = _ArenaRange(arena, i, j)
            self.bucket_params += [(i + a, i + b) for a, b in plan_buckets(sub, units[i:j + 1],
                                                                           self.bucket_bytes)]
            i = j + 1
        bounds = [arena.slice_bounds(a, b) for a, b in self.bucket_params]
        self.buckets = GradBuckets(arena.grads, bounds, exchange=self.exchange)
        # poll points inside backward (duck-typed: a MaskRCNNTrainChain around a MaskRCNNResNet)
        if hasattr(target, 'features_grad_hook'):
            target.features_grad_hook = self._tensor_hook
        from .models.resnet_extractor import BuildingBlock, ResNetExtractorBase
        for m in target.modules():
            if isinstance(m, BuildingBlock):
                m.grad_poll = self.poll
            if isinstance(m, ResNetExtractorBase):
                for key in m.functions:
                    m.stage_hooks[key] = self._tensor_hook

    # -- per step ----------------------------------------------------------------
    def begin_backward(self):
        pass

    def _bucket_ready(self, i):
        arena = self.optimizer.arena
        a, b = self.bucket_params[i]
        epoch = arena.epoch
        for p in arena.params[a:b + 1]:
            if p._grad_epoch != epoch:
                return False
        return True

    def poll(self):
        """Queue the all-reduce of every leading bucket whose gradients have all been queued
        (a parameter counts once its FIRST gradient of the step is queued: parameters shared
        between layers must not be used with overlapping buckets)."""
        if self.buckets is not None:
            self.buckets.poll(self._bucket_ready)

    def _tensor_hook(self, grad):
        self.poll()
        return grad

    def stage_hook(self, stage_index=None):
        return self._tensor_hook

    supports_deferred = True

    def reduce_deferred(self, flat_slices):
        """All-reduce the gradient slices of held-back parameters on the CURRENT stream (the
        optimizer's defer stream, after their weight-gradient kernels) and make it wait."""
        for k, t in enumerate(flat_slices):
            self.exchange.allreduce_async(t, 1000 + k)
        self.exchange.wait_all()

    def finish(self):
        """Wait for every bucket; returns the scale (1/world) to apply to the sums."""
        self.buckets.wait_all()
        return 1.0 / self.world_size

    def describe(self):
        d = self.exchange.describe()
        arena = self.optimizer.arena
        if arena is not None and self.buckets is not None:
            d['buckets_mb'] = [round((e - s) * 4 / 2 ** 20, 1) for s, e in self.buckets.bounds]
        return d


def rehearsal():
    """``MRCNN_DP_REHEARSAL=1``: run the N-rank launch path on a box with FEWER GPUs than ranks — every
    rank on device 0, the process group on gloo only, gradients through ``TorchDistExchange`` (gloo
    moves device tensors through the host).  It exists to exercise everything around the RCCL calls
    (rendezvous, rank-0 broadcast, bucket polling inside a real backward, deferred reductions, the
    benchmark's fences and max-over-ranks) where RCCL itself cannot run (it refuses two ranks on one
    device); never a measurement."""
    return os.environ.get('MRCNN_DP_REHEARSAL') == '1'


def init_from_env(backend=None):
    """One process per GPU, rendezvous from RANK / WORLD_SIZE / MASTER_* / LOCAL_RANK.
    The process group is the CONTROL plane (gloo; plus torch's nccl binding for device tensors
    so that RCCL stays available as a library fallback); gradients travel through
    ``RcclExchange``."""
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', str(rank)))
    if rehearsal():
        # A leaked MRCNN_DP_REHEARSAL=1 on a real multi-GPU node would put every rank on device 0 and
        # move the gradients through the host without an error: refuse where one GPU per rank exists.
        n_dev = torch.cuda.device_count() if torch.cuda.is_available() else 0
        if world > 1 and n_dev >= world:
            raise RuntimeError(
                'MRCNN_DP_REHEARSAL=1 with WORLD_SIZE=%d on a node with %d visible GPUs: the rehearsal '
                'mode (every rank on device 0, gradients over gloo) is for boxes with FEWER GPUs than '
                'ranks; unset it to run one rank per GPU over RCCL' % (world, n_dev))
        if rank == 0:
            sys.stderr.write('[chainer_mask_rcnn_amd] MRCNN_DP_REHEARSAL=1: %d rank(s) share device 0 and '
                             'exchange gradients over gloo through the host — a launch-path rehearsal, '
                             'never a measurement\n' % world)
        local, backend = 0, 'gloo'
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29500')
        if os.environ['MASTER_ADDR'] in ('127.0.0.1', 'localhost'):
            # single node: bootstrap sockets on loopback (the container's hostname may not
            # resolve); the gradient traffic itself goes over xGMI
            os.environ.setdefault('GLOO_SOCKET_IFNAME', 'lo')
            os.environ.setdefault('NCCL_SOCKET_IFNAME', 'lo')
        if backend is None:
            backend = 'cpu:gloo,cuda:nccl' if torch.cuda.is_available() else 'gloo'
        if 'nccl' in backend:
            torch.cuda.set_device(local)
        dist.init_process_group(backend, rank=rank, world_size=world)
    return rank, world, local


# ---------------------------------------------------------------------------------------------
# Control-plane objects: host data between ranks at log / evaluation boundaries
# ---------------------------------------------------------------------------------------------
def all_gather_bytes(payload, group=None):
    """Every rank's ``payload`` (bytes), in rank order, over the process group's CPU backend
    (gloo): the sizes first, then the payloads padded to the largest as uint8 CPU tensors.  CPU
    tensors never take torch's nccl binding on a ``cpu:gloo,cuda:nccl`` group."""
    world = dist.get_world_size(group)
    size = torch.tensor([len(payload)], dtype=torch.int64)
    sizes = [torch.zeros(1, dtype=torch.int64) for _ in range(world)]
    dist.all_gather(sizes, size, group=group)
    sizes = [int(s.item()) for s in sizes]
    buf = torch.zeros(max(sizes), dtype=torch.uint8)
    if payload:
        buf[:len(payload)] = torch.frombuffer(bytearray(payload), dtype=torch.uint8)
    bufs = [torch.zeros(max(sizes), dtype=torch.uint8) for _ in range(world)]
    dist.all_gather(bufs, buf, group=group)
    return [bytes(b[:n].numpy().tobytes()) for b, n in zip(bufs, sizes)]


def all_gather_object_cpu(obj, group=None):
    """``[obj of rank 0, obj of rank 1, ...]`` on every rank (pickled, all_gather_bytes)."""
    import pickle
    return [pickle.loads(b) for b in all_gather_bytes(pickle.dumps(obj, protocol=4), group)]


def broadcast_object_cpu(obj, src=0, group=None):
    """Rank ``src``'s ``obj`` on every rank (pickled, as uint8 CPU tensors over gloo)."""
    import pickle
    payload = pickle.dumps(obj, protocol=4) if dist.get_rank(group) == src else b''
    size = torch.tensor([len(payload)], dtype=torch.int64)
    dist.broadcast(size, src=src, group=group)
    buf = torch.zeros(int(size.item()), dtype=torch.uint8)
    if payload:
        buf[:] = torch.frombuffer(bytearray(payload), dtype=torch.uint8)
    dist.broadcast(buf, src=src, group=group)
    return pickle.loads(buf.numpy().tobytes())
