"""Training driver of the HIP path: the contract of chainer.training (Trainer, triggers, the
extensions examples/train_common.py:251-372 registers) restated on top of tools/train_loop.py's
TrainLoop, plus the datasets examples/custom_dataset/train.py adds.

chainer's training classes are third-party (not in the reference repository); what is restated
here is their behaviour as train_common.py relies on it (chainer >= 4):

* ``Trainer(loop, stop_trigger, out)`` runs ``loop.step()`` until the stop trigger fires; after
  each update the extensions whose trigger fires run, by priority (writer 300, reader 100,
  snapshot -100) and then in registration order.  The update's reported values are in
  ``trainer.observation`` as ``main/<key>`` (the chain's ``report``: device scalars), together
  with what the writer extensions of that iteration add (``validation/main/*``, ``lr``).
* ``IntervalTrigger``: fires when ``previous // period != current // period`` (iteration or
  fractional epoch); ``ManualScheduleTrigger``: when ``previous < p <= current`` for a point p;
  ``MaxValueTrigger``: at each interval, the mean of the key's observations since the last one
  is compared with the best so far (the first comparison fires; then only a strictly greater
  value).
* Summaries (LogReport, PlotReport) average each key over the iterations of their window as
  ``reporter.Summary`` does: ``_x += value`` from 0, then ``_x / n``.  For the device scalars the
  running float32 sum stays on the device (functions.loss.observe_accumulate, one launch per
  iteration and summary); it is read back only when the window closes.

Evaluation and the visual report run between two updates without changing training: the
deferred parameter updates are flushed first, the input worker's pending batch is left alone
(waited for, not taken), the extractor's frozen-prefix prefetch of the next batch is kept, the
Python / NumPy random states are restored and the model is back in ``train()`` mode afterwards.
"""
import json
import numbers
import os
import os.path as osp
import random
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PRIORITY_WRITER = 300
PRIORITY_READER = 100
PRIORITY_SNAPSHOT = -100


# ---- datasets --------------------------------------------------------------------------------
class ConcatenatedDataset(object):
    """chainer.datasets.ConcatenatedDataset(*datasets): the examples of each dataset in turn."""

    def __init__(self, *datasets):
        self._datasets = datasets

    def __len__(self):
        return sum(len(d) for d in self._datasets)

    def __getitem__(self, i):
        if i < 0:
            raise IndexError
        for dataset in self._datasets:
            if i < len(dataset):
                return dataset[i]
            i -= len(dataset)
        raise IndexError

    get_example = __getitem__


class VOCLikeDataset(object):
    """examples/custom_dataset/train.py's VOCLikeDataset: ``JPEGImages/<id>.jpg`` with
    ``SegmentationClass/<id>.npy`` and ``SegmentationObject/<id>.npy`` label images (instance 0
    is ignored).  The ids are the sorted file stems of JPEGImages: the reference takes
    ``os.listdir``'s order, which depends on the file system."""

    def __init__(self, root_dir):
        import chainer_mask_rcnn_amd as cmr
        self.class_names = cmr.datasets.VOC2012InstanceSeg.class_names
        self._root_dir = root_dir
        img_dir = osp.join(root_dir, 'JPEGImages')
        self._ids = [osp.splitext(f)[0] for f in sorted(os.listdir(img_dir))]

    def __len__(self):
        return len(self._ids)

    def get_example(self, i):
        import chainer_mask_rcnn_amd as cmr
        from chainer_mask_rcnn_amd.datasets.voc import read_rgb
        id_ = self._ids[i]
        img = read_rgb(osp.join(self._root_dir, 'JPEGImages', id_ + '.jpg'))
        cls = np.load(osp.join(self._root_dir, 'SegmentationClass', id_ + '.npy'))
        ins = np.load(osp.join(self._root_dir, 'SegmentationObject', id_ + '.npy'))
        ins[ins == 0] = -1  # instance id 0 should be ignored.
        assert img.shape[:2] == cls.shape == ins.shape
        labels, bboxes, masks = cmr.utils.label2instance_boxes(
            label_instance=ins, label_class=cls, return_masks=True)
        masks = masks.astype(np.int32, copy=False)
        labels = labels.astype(np.int32, copy=False)
        labels -= 1  # background: 0 -> -1
        bboxes = bboxes.astype(np.float32, copy=False)
        return img, bboxes, labels, masks

    __getitem__ = get_example


# ---- triggers --------------------------------------------------------------------------------
class IntervalTrigger(object):

    def __init__(self, period, unit):
        if unit not in ('epoch', 'iteration'):
            raise ValueError('unit must be epoch or iteration, got %r' % (unit,))
        self.period, self.unit = period, unit
        self._previous_iteration = 0
        self._previous_epoch_detail = 0.

    def __call__(self, trainer):
        updater = trainer.updater
        if self.unit == 'epoch':
            fire = self._previous_epoch_detail // self.period != updater.epoch_detail // self.period
        else:
            fire = self._previous_iteration // self.period != updater.iteration // self.period
        self._previous_iteration = updater.iteration
        self._previous_epoch_detail = updater.epoch_detail
        return fire


class ManualScheduleTrigger(object):

    def __init__(self, points, unit):
        if unit not in ('epoch', 'iteration'):
            raise ValueError('unit must be epoch or iteration, got %r' % (unit,))
        self.points = points if isinstance(points, (list, tuple)) else [points]
        self.unit = unit
        self._previous = 0.

    def __call__(self, trainer):
        updater = trainer.updater
        current = updater.epoch_detail if self.unit == 'epoch' else updater.iteration
        fire = any(self._previous < p <= current for p in self.points)
        self._previous = current
        return fire


def get_trigger(trigger):
    if trigger is None:
        return IntervalTrigger(1, 'iteration')
    if callable(trigger):
        return trigger
    return IntervalTrigger(*trigger)


class MaxValueTrigger(object):
    """chainer.training.triggers.MaxValueTrigger(key, trigger)."""

    def __init__(self, key, trigger=(1, 'epoch')):
        self._key = key
        self._interval_trigger = get_trigger(trigger)
        self._best_value = None
        self._summary = DictSummary()

    def __call__(self, trainer):
        if self._key in trainer.observation:
            self._summary.add({self._key: trainer.observation[self._key]})
        if not self._interval_trigger(trainer):
            return False
        stats = self._summary.compute_mean()
        self._summary = DictSummary()
        if self._key not in stats:
            return False
        value = float(stats[self._key])
        if self._best_value is None or value > self._best_value:
            self._best_value = value
            return True
        return False


# ---- summaries -------------------------------------------------------------------------------
class DeviceSums(object):
    """Float32 running sums of device scalars (the same keys every iteration), accumulated on
    the device by one kernel launch per ``add`` and read back by ``read_and_reset`` only."""

    def __init__(self, keys, device):
        from chainer_mask_rcnn_amd.functions import loss
        if len(keys) > loss.MAX_OBSERVED:
            raise ValueError('at most %d device scalars per summary' % loss.MAX_OBSERVED)
        self.keys = tuple(keys)
        self.sums = torch.zeros(len(keys), dtype=torch.float32, device=device)
        self.count = 0

    def add(self, values):
        from chainer_mask_rcnn_amd.functions import loss
        loss.observe_accumulate([values[k] for k in self.keys], self.sums)
        self.count += 1

    def read_and_reset(self):
        host = self.sums.cpu().numpy().copy()     # the one D2H copy of the window
        self.sums.zero_()
        n, self.count = self.count, 0
        return host, n


def _is_device_scalar(v):
    return isinstance(v, torch.Tensor) and v.is_cuda and v.numel() == 1


class DictSummary(object):
    """chainer.reporter.DictSummary: per-key mean over what was added.  Device scalars are
    summed on the device (DeviceSums); numbers on the host as ``_x += value`` from 0."""

    def __init__(self):
        self._host = {}        # key -> [_x, _n]
        self._dev = None

    def add(self, d):
        dev = {}
        for k, v in d.items():
            if _is_device_scalar(v):
                dev[k] = v
            elif isinstance(v, (numbers.Number, np.ndarray, np.generic)) and not isinstance(v, bool):
                s = self._host.setdefault(k, [0, 0])
                s[0] += v
                s[1] += 1
        if dev:
            if self._dev is None:
                self._dev = DeviceSums(sorted(dev), next(iter(dev.values())).device)
            elif set(dev) != set(self._dev.keys):
                raise ValueError('device observations changed keys: %s -> %s'
                                 % (sorted(self._dev.keys), sorted(dev)))
            self._dev.add(dev)

    def compute_mean(self, gather=None):
        """``gather`` (data parallel): a collective returning every rank's ``(sums, n)`` in rank
        order; the device means are then over all ranks (rank_order_mean).  Host numbers stay
        this rank's own."""
        out = {k: x / n for k, (x, n) in self._host.items()}
        if self._dev is not None and self._dev.count:
            sums, n = self._dev.read_and_reset()
            if gather is None:
                for k, s in zip(self._dev.keys, sums):
                    out[k] = np.float32(s) / np.float32(n)    # float32 _x / _n (Summary.compute_mean)
            else:
                per_rank = gather((self._dev.keys, sums, n))
                if any(keys != self._dev.keys or m != n for keys, _, m in per_rank):
                    raise RuntimeError('ranks closed a summary window over different keys or '
                                       'iteration counts: %s' % [(k, m) for k, _, m in per_rank])
                means = rank_order_mean([s for _, s, _ in per_rank], n)
                out.update(zip(self._dev.keys, means))
        self._host = {}
        return out


def rank_order_mean(sums_by_rank, n):
    """Mean over ranks and over a window of ``n`` iterations from each rank's float32 window sums:
    the sums added in rank order in float32, divided by float32(n * world).  Deterministic, and
    the same on every rank."""
    total = np.array(sums_by_rank[0], dtype=np.float32)
    for s in sums_by_rank[1:]:
        total = (total + np.asarray(s, dtype=np.float32)).astype(np.float32)
    return total / np.float32(n * len(sums_by_rank))


# ---- trainer ---------------------------------------------------------------------------------
class Updater(object):
    """StandardUpdater's counters over a TrainLoop.  The loop's iterator runs one batch ahead
    when it prefetches, so the position is that of the reference's SerialIterator after
    ``iteration`` batches: epoch = floor(i*B / N), current_position = i*B mod N."""

    def __init__(self, loop):
        self.loop = loop
        self.batch_size = loop.iterator.batch_size
        self.n = len(loop.iterator.dataset)
        self.previous_epoch_detail = None

    @property
    def iteration(self):
        return self.loop.iteration

    @property
    def epoch(self):
        return self.iteration * self.batch_size // self.n

    @property
    def epoch_detail(self):
        return self.epoch + (self.iteration * self.batch_size % self.n) / self.n

    def get_optimizer(self, name='main'):
        return self.loop.optimizer

    def update(self):
        self.previous_epoch_detail = self.epoch_detail
        return self.loop.step()


class _Entry(object):
    def __init__(self, extension, trigger, priority, name, order):
        self.extension, self.trigger, self.priority, self.name, self.order = \
            extension, trigger, priority, name, order


class Trainer(object):

    def __init__(self, loop, stop_trigger, out='result'):
        # out=None: a data-parallel rank other than 0, which writes nothing
        self.loop = loop
        self.updater = Updater(loop)
        self.stop_trigger = get_trigger(stop_trigger)
        self.out = out
        self.observation = {}
        self._entries = []
        self._start = None
        self._done = False

    @property
    def iteration(self):
        return self.updater.iteration

    @property
    def epoch(self):
        return self.updater.epoch

    @property
    def epoch_detail(self):
        return self.updater.epoch_detail

    @property
    def elapsed_time(self):
        return 0. if self._start is None else time.time() - self._start

    def extend(self, extension, name=None, trigger=None, priority=None):
        if trigger is None:
            trigger = getattr(extension, 'trigger', (1, 'iteration'))
        if priority is None:
            priority = getattr(extension, 'priority', PRIORITY_READER)
        name = name or getattr(extension, 'name', None) or type(extension).__name__
        self._entries.append(_Entry(extension, get_trigger(trigger), priority, name,
                                    len(self._entries)))

    def ordered_entries(self):
        return sorted(self._entries, key=lambda e: (-e.priority, e.order))

    def get_extension(self, name):
        for e in self._entries:
            if e.name == name:
                return e.extension
        raise ValueError('extension %s not found' % name)

    def run(self):
        if self._done:
            raise RuntimeError('cannot run training loop multiple times')
        if self.out is not None:
            os.makedirs(self.out, exist_ok=True)
        entries = self.ordered_entries()
        for e in entries:
            init = getattr(e.extension, 'initialize', None)
            if init is not None:
                init(self)
        self._start = time.time()
        chain = self.loop.chain
        try:
            while not self.stop_trigger(self):
                self.observation = {}
                self.updater.update()
                self.observation.update(('main/' + k, v) for k, v in chain.report.items())
                # the optimizer's device scalars (grad_norm, skipped) beside the chain's, if any
                opt_report = getattr(getattr(self.loop, 'optimizer', None), 'report', None) or {}
                self.observation.update(('main/' + k, v) for k, v in opt_report.items())
                for e in entries:
                    if e.trigger(self):
                        e.extension(self)
        finally:
            for e in entries:
                fin = getattr(e.extension, 'finalize', None)
                if fin is not None:
                    fin()
        self._done = True


# ---- extensions ------------------------------------------------------------------------------
class between_steps(object):
    """``with between_steps(trainer): ...`` — run inference between two updates without
    changing training (see the module docstring)."""

    def __init__(self, trainer):
        self.trainer = trainer

    def __enter__(self):
        loop = self.trainer.loop
        loop.optimizer.flush()               # deferred weight gradients / SGD slices land now
        loop.settle()                        # the worker is idle: its batch stays pending
        ext = loop.chain.mask_rcnn.extractor
        self._prefetched = getattr(ext, '_prefetched', None)
        self._random = random.getstate()
        self._np_random = np.random.get_state()
        return self

    def __exit__(self, *exc):
        loop = self.trainer.loop
        random.setstate(self._random)
        np.random.set_state(self._np_random)
        ext = loop.chain.mask_rcnn.extractor
        if hasattr(ext, '_prefetched'):
            ext._prefetched = self._prefetched
        loop.chain.train()
        return False


class Evaluator(object):
    """The package's VOC / COCO evaluator as a trainer extension: its observation
    (``validation/main/*``) joins the iteration's observation."""

    priority = PRIORITY_WRITER
    trigger = (1, 'epoch')
    name = 'validation'

    def __init__(self, evaluator):
        self.evaluator = evaluator

    def __call__(self, trainer):
        with between_steps(trainer):
            result = self.evaluator.evaluate()
        trainer.observation.update(result)
        return result


class VisReport(object):
    """extensions.InstanceSegmentationVisReport between two updates."""

    priority = PRIORITY_READER
    trigger = (1, 'epoch')

    def __init__(self, report):
        self.report = report

    def __call__(self, trainer):
        with between_steps(trainer):
            self.report(trainer)


class observe_lr(object):
    """chainer.training.extensions.observe_lr(): ``lr`` of the optimizer into the observation."""

    priority = PRIORITY_WRITER
    name = 'observe_lr'

    def __call__(self, trainer):
        opt = trainer.updater.get_optimizer('main')
        # the rate the SGD launch got: the schedule's value times the warm-up factor (1.0: the same)
        trainer.observation['lr'] = opt.lr * getattr(opt, 'lr_scale', 1.0)


class LinearWarmup(object):
    """Detectron's linear warm-up: update number i (0-based) runs at ``lr * (factor + (1 - factor)
    * i / iters)`` for i < iters and at exactly ``lr`` afterwards.  It sets the optimizer's
    ``lr_scale`` for the next update and leaves ``lr`` to the schedule, so ExponentialShift
    composes; register it for every iteration."""

    priority = PRIORITY_READER
    trigger = (1, 'iteration')

    def __init__(self, iters, factor=1. / 3.):
        iters = int(iters)
        if iters < 0 or not 0. <= factor <= 1.:
            raise ValueError('LinearWarmup: iters >= 0 and 0 <= factor <= 1, got %r, %r'
                             % (iters, factor))
        self.iters, self.factor = iters, float(factor)

    def scale(self, i):
        if i >= self.iters:
            return 1.0
        return self.factor + (1. - self.factor) * i / self.iters

    def initialize(self, trainer):
        self(trainer)

    def __call__(self, trainer):
        trainer.updater.get_optimizer('main').lr_scale = self.scale(trainer.updater.iteration)


class StopWhenEverythingSkipped(object):
    """With optimizers.SkipNonFiniteUpdate: a run whose every update of a log window was skipped
    has diverged and would skip for ever, so it ends with an error.  Runs at the log trigger,
    after the LogReport, on its newest entry."""

    priority = PRIORITY_READER

    def __init__(self, log_report='LogReport', key='main/skipped'):
        self._log_report, self._key = log_report, key
        self._seen = 0

    def __call__(self, trainer):
        log = trainer.get_extension(self._log_report).log
        if len(log) == self._seen:
            return
        self._seen = len(log)
        entry = log[-1]
        if entry.get(self._key) == 1.0:
            raise RuntimeError(
                'every update up to iteration %d of the last log window was skipped for '
                'non-finite gradients (%s = 1): training has diverged'
                % (entry.get('iteration', trainer.updater.iteration), self._key))


class ExponentialShift(object):
    """chainer.training.extensions.ExponentialShift(attr, rate): at its t-th call the
    optimizer's ``attr`` becomes ``init * rate ** t`` (used by the next update)."""

    priority = PRIORITY_READER

    def __init__(self, attr, rate, init=None):
        self._attr, self._rate, self._init = attr, rate, init
        self._t = 0

    def initialize(self, trainer):
        opt = trainer.updater.get_optimizer('main')
        if self._init is None:
            self._init = getattr(opt, self._attr)
        setattr(opt, self._attr, self._init * self._rate ** self._t)

    def __call__(self, trainer):
        self._t += 1
        setattr(trainer.updater.get_optimizer('main'), self._attr,
                self._init * (self._rate ** self._t))


def _atomic_write(path, write):
    d = osp.dirname(path) or '.'
    fd, tmp = tempfile.mkstemp(prefix=osp.basename(path), dir=d)
    os.close(fd)
    try:
        write(tmp)
        shutil.move(tmp, path)
    finally:
        if osp.exists(tmp):
            os.remove(tmp)


class LogReport(object):
    """chainer.training.extensions.LogReport(trigger): every trigger, the float means of every
    key observed since the last entry plus epoch, iteration and elapsed_time; the whole list is
    written as JSON (indent 4) to ``out/log`` through a temporary file and a rename."""

    priority = PRIORITY_READER
    name = 'LogReport'

    def __init__(self, trigger=(1, 'epoch'), log_name='log', gather=None):
        # gather: see DictSummary.compute_mean (log_name=None: the window is closed, not written)
        self._trigger = get_trigger(trigger)
        self._log_name = log_name
        self._gather = gather
        self._summary = DictSummary()
        self.log = []

    def __call__(self, trainer):
        self._summary.add(trainer.observation)
        if not self._trigger(trainer):
            return
        stats = {k: float(v) for k, v in self._summary.compute_mean(self._gather).items()}
        stats['epoch'] = trainer.updater.epoch
        stats['iteration'] = trainer.updater.iteration
        stats['elapsed_time'] = trainer.elapsed_time
        self.log.append(stats)
        self._summary = DictSummary()
        if self._log_name is not None:
            def write(tmp):
                with open(tmp, 'w') as f:
                    json.dump(self.log, f, indent=4)
            _atomic_write(osp.join(trainer.out, self._log_name), write)


class PrintReport(object):
    """chainer.training.extensions.PrintReport(entries): the LogReport's new entries as rows."""

    priority = PRIORITY_READER

    def __init__(self, entries, log_report='LogReport', out=sys.stdout):
        self._entries = entries
        self._log_report = log_report
        self._out = out
        self._log_len = 0
        widths = [max(10, len(e)) for e in entries]
        self._header = '  '.join(('{:%d}' % w).format(e) for e, w in zip(entries, widths)) + '\n'
        self._widths = widths

    def __call__(self, trainer):
        out = self._out
        if self._header:
            out.write(self._header)
            self._header = None
        log = trainer.get_extension(self._log_report).log
        for line in log[self._log_len:]:
            cells = []
            for e, w in zip(self._entries, self._widths):
                if e in line:
                    v = line[e]
                    cells.append(('{:<%dg}' % w).format(v) if isinstance(v, float)
                                 else ('{:<%d}' % w).format(v))
                else:
                    cells.append(' ' * w)
            out.write('  '.join(cells) + '\n')
        out.flush()
        self._log_len = len(log)


class PlotReport(object):
    """chainer.training.extensions.PlotReport(y_keys, 'iteration', trigger, file_name): the
    mean of each key over every trigger window, plotted against the iteration with matplotlib."""

    priority = PRIORITY_READER

    def __init__(self, y_keys, file_name='plot.png', trigger=(1, 'epoch'), x_key='iteration',
                 gather=None, write=True):
        # gather: see DictSummary.compute_mean; write=False: the windows are closed, not plotted
        self._gather, self._write = gather, write
        self._y_keys = list(y_keys)
        self._file_name = file_name
        self._trigger = get_trigger(trigger)
        self._x_key = x_key
        self._summary = DictSummary()
        self._data = {k: [] for k in self._y_keys}

    def __call__(self, trainer):
        self._summary.add({k: trainer.observation[k] for k in self._y_keys
                           if k in trainer.observation})
        if not self._trigger(trainer):
            return
        stats = self._summary.compute_mean(self._gather)
        self._summary = DictSummary()
        x = getattr(trainer.updater, self._x_key)
        for k in self._y_keys:
            if k in stats:
                self._data[k].append((x, float(stats[k])))
        if not self._write:
            return
        import matplotlib
        matplotlib.use('Agg')
        import matplotlib.pyplot as plt
        fig = plt.figure()
        ax = fig.add_subplot(111)
        ax.set_xlabel(self._x_key)
        ax.grid()
        for k in self._y_keys:
            xy = np.asarray(self._data[k])
            if len(xy):
                ax.plot(xy[:, 0], xy[:, 1], marker='x', label=k)
        if ax.has_data():
            ax.legend(bbox_to_anchor=(1.05, 1), loc='upper left', borderaxespad=0.)
        _atomic_write(osp.join(trainer.out, self._file_name),
                      lambda tmp: fig.savefig(tmp, format='png', bbox_inches='tight'))
        plt.close(fig)


class snapshot_object(object):
    """chainer.training.extensions.snapshot_object(target, filename): serializers.save_npz of
    ``target`` to ``out/filename`` (through a temporary file; the save flushes deferred
    parameter updates)."""

    priority = PRIORITY_SNAPSHOT

    def __init__(self, target, filename):
        self.target, self.filename = target, filename

    def __call__(self, trainer):
        from chainer_mask_rcnn_amd import serializers

        def write(tmp):
            with open(tmp, 'wb') as f:
                serializers.save_npz(f, self.target)
        _atomic_write(osp.join(trainer.out, self.filename.format(trainer)), write)


class ParamsReport(object):
    """fcn.extensions.ParamsReport(params): ``params`` as ``out/params.yaml`` before training."""

    priority = PRIORITY_READER

    def __init__(self, params, file_name='params.yaml'):
        self._params, self._file_name = params, file_name

    def initialize(self, trainer):
        import yaml
        os.makedirs(trainer.out, exist_ok=True)
        with open(osp.join(trainer.out, self._file_name), 'w') as f:
            yaml.safe_dump(_plain(self._params), f, default_flow_style=False)

    def __call__(self, trainer):
        pass


class RankZeroOnly(object):
    """A rank-0-only extension that reads the parameters (snapshot, visual report) under data
    parallelism.  Reading them flushes pending deferred updates, which launches the deferred
    gradients' all-reduce (a collective): on rank 0 alone that would hang the job, so it raises
    instead.  The all-rank evaluator flushes first at the same trigger."""

    def __init__(self, extension):
        self.extension = extension
        for attr in ('trigger', 'priority', 'name'):
            if hasattr(extension, attr):
                setattr(self, attr, getattr(extension, attr))
        self.name = getattr(extension, 'name', None) or type(extension).__name__
        if hasattr(extension, 'initialize'):
            self.initialize = extension.initialize
        if hasattr(extension, 'finalize'):
            self.finalize = extension.finalize

    def __call__(self, trainer):
        opt = trainer.updater.get_optimizer('main')
        if getattr(opt, 'has_pending', lambda: False)():
            raise RuntimeError('rank-0-only extension %s found deferred parameter updates pending: '
                               'flushing them here would all-reduce on rank 0 alone; flush on every '
                               'rank first (an all-rank extension at the same trigger)' % self.name)
        return self.extension(trainer)


def _plain(v):
    """YAML-safe copy (tuples -> lists, NumPy scalars -> Python numbers)."""
    if isinstance(v, dict):
        return {str(k): _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple, np.ndarray)):
        return [_plain(x) for x in v]
    if isinstance(v, np.generic):
        return v.item()
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return str(v)


LOG_KEYS = ['main/loss', 'main/roi_loc_loss', 'main/roi_cls_loss', 'main/roi_mask_loss',
            'main/rpn_loc_loss', 'main/rpn_cls_loss']
# the optimizer's report with a gradient-norm hook (optimizers.py).  6 + 2 device scalars per
# summary: exactly MRCNN_MAX_OBSERVED (DeviceSums), so a further one needs a larger bound there
GRAD_KEYS = ['main/grad_norm', 'main/skipped']


def extend_reference_set(trainer, model, evaluator=None, vis_iterator=None, class_names=None,
                         step_size=None, params=None, eval_interval=(1, 'epoch'),
                         log_interval=(20, 'iteration'), plot_interval=(0.1, 'epoch'),
                         print_interval=(20, 'iteration'), plot=True, print_out=sys.stdout,
                         rank=0, gather=None, eval_bbox=False, warmup=None, grad_report=False,
                         eval_boundary=False):
    """The extensions of examples/train_common.py:251-372 (without dump_graph / ProgressBar)
    with the same triggers and priorities; ``model``: the MaskRCNN (``chain.mask_rcnn``).
    ``eval_bbox``: the evaluator also reports ``validation/main/bbox/map``, which then joins the
    printed report (the best snapshot and accuracy.png stay on ``validation/main/map``);
    ``eval_boundary``: likewise for ``validation/main/boundary/map`` (Boundary AP).
    ``warmup``: a LinearWarmup, run every iteration on every rank.  ``grad_report``: the optimizer
    has a gradient-norm hook: ``main/grad_norm`` and ``main/skipped`` join the printed report and
    StopWhenEverythingSkipped ends a run whose whole log window was skipped.

    Data parallel (``gather``: the control-plane all-gather, see DictSummary.compute_mean): the lr
    shift, the evaluator (a multi-node one), observe_lr and the summaries of LogReport and the
    loss PlotReport run on every rank, the loss means over all ranks; the snapshot, params.yaml,
    the visual report, PrintReport and the files of the reports on rank 0 only (the snapshot and
    the visual report, which read the parameters, behind RankZeroOnly)."""
    import chainer_mask_rcnn_amd as cmr
    parallel = gather is not None
    lead = rank == 0

    def extend_lead(extension, reads_params=False, **kw):
        if lead:
            trainer.extend(RankZeroOnly(extension) if parallel and reads_params else extension, **kw)
    if step_size is not None:
        trainer.extend(ExponentialShift('lr', 0.1),
                       trigger=ManualScheduleTrigger(step_size, 'epoch'))
    if warmup is not None:
        trainer.extend(warmup, trigger=(1, 'iteration'))
    if evaluator is not None:
        trainer.extend(Evaluator(evaluator), trigger=eval_interval)
        extend_lead(snapshot_object(model, 'snapshot_model.npz'), reads_params=True,
                    trigger=MaxValueTrigger('validation/main/map', eval_interval))
    if params is not None:
        extend_lead(ParamsReport(params))
    if vis_iterator is not None:
        extend_lead(VisReport(cmr.extensions.InstanceSegmentationVisReport(
            vis_iterator, model, label_names=class_names)), reads_params=True,
                    trigger=eval_interval)
    trainer.extend(observe_lr(), trigger=log_interval)
    trainer.extend(LogReport(trigger=log_interval, log_name='log' if lead else None,
                             gather=gather))
    if grad_report:
        trainer.extend(StopWhenEverythingSkipped(), trigger=log_interval)
    if print_out is not None:
        extend_lead(PrintReport(['iteration', 'epoch', 'elapsed_time', 'lr'] + LOG_KEYS[:1]
                                + LOG_KEYS[1:] + (GRAD_KEYS if grad_report else [])
                                + ['validation/main/map']
                                + (['validation/main/bbox/map'] if eval_bbox else [])
                                + (['validation/main/boundary/map'] if eval_boundary else []),
                                out=print_out),
                    trigger=print_interval)
    if plot:
        trainer.extend(PlotReport(LOG_KEYS, file_name='loss.png', trigger=plot_interval,
                                  gather=gather, write=lead), trigger=plot_interval)
        extend_lead(PlotReport(['validation/main/map'], file_name='accuracy.png',
                               trigger=plot_interval), trigger=eval_interval)
    return trainer
